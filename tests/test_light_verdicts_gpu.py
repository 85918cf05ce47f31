"""Light verdicts of a resting view (rt_scene_set_light_verdicts): the second launch in a row of
bit-identical inputs writes, per tile, which lights added nothing and which were all clear; later launches consume that.
Every frame must be the same bits as without the table and as the brute-force kernel's.

The library takes at most RT_MAX_LIGHTS = 8 lights, which is also the number of lights a word holds: a ninth light
is refused by rt_scene_set_lights, so the "lights beyond 8" cap cannot be reached; the test renders the 8-light scene
and asserts the refusal."""
import ctypes as C

import numpy as np
import pytest

import verdict_runs as R
from scenes import Inputs, Scn, mixed_scene

pytestmark = pytest.mark.gpu

W, H = 160, 90


def frame(sc, w=W, h=H, **kw):
    import torch
    out = sc.render(w, h, **kw)
    torch.cuda.synchronize()
    return out["rgba"].cpu().numpy().view(np.uint32), out["packed"].cpu().numpy().view(np.uint32)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def inputs(rt, gpu):
    return {n: Inputs(rt, n) for n in (1024, 256)}


def references(inp, w=W, h=H, **kw):
    """The frame with the switch off and the brute-force frame, from a scene of its own."""
    return R.switched_off(inp, w, h, **kw)[0]


LAYOUTS = {
    "tile8": dict(),
    "tile16": dict(tile=16),
    "tile32": dict(tile=32),
    "tile64": dict(tile=64),
    "band": dict(y0=16, y1=72),
    "interleave": dict(interleave=(2, 1, 16)),
}


@pytest.mark.parametrize("n", [1024, 256])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_record_and_use(inputs, n, layout):
    kw = LAYOUTS[layout]
    off = references(inputs[n], **kw)
    sc = inputs[n].scene()
    states = []
    for k in range(5):
        f = frame(sc, **kw)
        assert same(f, off), (layout, n, k)
        info = sc.light_verdicts()
        states.append(info["state"])
        if k == 1:   # the launch that wrote: every tile of the launch has its word, and all three codes occur
            tile = kw.get("tile", 8)
            assert info["tiles_x"] == (W + tile - 1) // tile
            assert info["unwritten"] == 0
            assert info["nothing"] > 0 and info["clear"] > 0
    assert states == [0, 1, 2, 2, 2]


def test_switch(inputs):
    sc = inputs[256].scene()
    off = references(inputs[256])
    sc.set_light_verdicts(0)
    for _ in range(3):
        assert same(frame(sc), off)
        assert sc.light_verdicts()["state"] == 0
    sc.set_light_verdicts(1)
    assert [(same(frame(sc), off), sc.light_verdicts()["state"]) for _ in range(3)] == [(True, 0), (True, 1), (True, 2)]


def test_invalidation(rt, inputs):
    """Each change between launches of a warmed-up scene: the next frames equal a fresh scene's and the brute-force one."""
    inp = Inputs(rt, 1024)
    sc = inp.scene()
    state = dict(w=W, h=H, kw=dict())

    def settle(tag):
        fresh = inp.scene()
        fresh.set_light_verdicts(0)
        want = frame(fresh, state["w"], state["h"], **state["kw"])
        assert same(want, frame(fresh, state["w"], state["h"], cull=False, **state["kw"])), tag
        seen = []
        for k in range(3):   # nothing, write, read -- all under the new inputs
            assert same(frame(sc, state["w"], state["h"], **state["kw"]), want), (tag, k)
            seen.append(sc.light_verdicts()["state"])
        return seen

    assert settle("start") == [0, 1, 2]
    # one light's position
    inp.lights = R.copy_lights(rt, inp.lights, 3)
    inp.lights[0].pos.x = 14.0
    sc.set_lights(inp.lights, 3)
    assert settle("light position") == [0, 1, 2]
    # one light's colour, non-finite
    inp.lights[1].b = float("inf")
    sc.set_lights(inp.lights, 3)
    assert settle("light colour inf") == [0, 1, 2]
    inp.lights[1].b = 1.0
    sc.set_lights(inp.lights, 3)
    assert settle("light colour back") == [0, 1, 2]
    # one texel inf
    inp.tex = [p.copy() for p in inp.tex]
    inp.tex[1][inp.tex[1].shape[0] // 2, inp.tex[1].shape[1] // 3] = np.inf
    sc.set_texture(inp.tex)
    assert settle("texel inf") == [0, 1, 2]
    # camera origin, yaw
    cam0 = inp.cam
    inp.cam = rt.Camera(rt.Vec3(4.5, 3, 10), rt.Vec3(0, 0, 1), 0.0, 180.0, -20.0)
    state["kw"] = dict(cam=inp.cam)
    assert settle("origin") == [0, 1, 2]
    cam1 = inp.cam
    inp.cam = rt.Camera(rt.Vec3(4.5, 3, 10), rt.Vec3(0, 0, 1), 0.0, 171.0, -20.0)
    state["kw"] = dict(cam=inp.cam)
    assert settle("yaw") == [0, 1, 2]
    # back to an earlier view. The yaw view was the scene's third: its view lists went into a fresh buffer, which bumps
    # the scene's generation of buffers, so the earlier view's table no longer matches and is written anew
    # (test_slots_are_reused_and_evicted returns to layouts whose tables do survive)
    inp.cam = cam1
    state["kw"] = dict(cam=inp.cam)
    assert settle("origin again") == [0, 1, 2]
    # the sphere list
    inp.spheres = rt.generate_spheres(1024, 7)
    sc.set_spheres(inp.spheres, 1024)
    assert settle("spheres") == [0, 1, 2]
    # the frame size, shrinking and growing
    state.update(w=96, h=54)
    assert settle("shrink") == [0, 1, 2]
    state.update(w=W, h=H)
    assert settle("grow") == [0, 1, 2]   # (new ray tables: a new generation)
    # rows, tile shape, interleave -- five layouts and views by now: the four slots evict each other
    for tag, extra in (("rows", dict(y0=8, y1=80)), ("tile", dict(tile=32)), ("interleave", dict(interleave=(2, 0, 16)))):
        state["kw"] = dict(cam=inp.cam, **extra)
        assert settle(tag) == [0, 1, 2]
    inp.cam = cam0
    state["kw"] = dict()
    assert settle("first view again") == [0, 1, 2]   # (never seen with this sphere list)


def test_slots_are_reused_and_evicted(inputs):
    """Five layouts of one view share the scene's four tables: a layout whose table is still there reads it at once,
    the least recently used one has lost it and writes it anew, which in turn evicts the next oldest."""
    inp = inputs[1024]
    sc = inp.scene()
    layouts = [dict(), dict(tile=16), dict(tile=32), dict(y0=8, y1=80), dict(y0=16, y1=64)]
    want = [references(inp, **kw) for kw in layouts]

    def visit(i):
        seen = []
        for _ in range(3):
            assert same(frame(sc, **layouts[i]), want[i]), i
            info = sc.light_verdicts()
            seen.append((info["state"], info["slot"]))
        return [s for s, _ in seen], seen[-1][1]

    slots = []
    for i in range(5):
        states, slot = visit(i)
        assert states == [0, 1, 2], i
        slots.append(slot)
    assert sorted(slots[:4]) == [0, 1, 2, 3] and slots[4] == slots[0]   # the fifth took the first one's
    assert visit(4) == ([2, 2, 2], slots[4])                            # still there: read at once
    assert visit(3) == ([2, 2, 2], slots[3])
    states, slot = visit(0)                                             # evicted by the fifth: written anew ...
    assert states == [0, 1, 2] and slot == slots[1]                     # ... into the least recently used, the second's
    assert visit(2) == ([2, 2, 2], slots[2])
    assert visit(1)[0] == [0, 1, 2]


def test_rt_multi_takes_no_verdicts(rt, inputs):
    """rt_multi renders its devices' shares through scenes of its own, which never record or read a table."""
    import torch
    lib = rt.load_library()
    inp = inputs[1024]
    off = references(inp)
    fp = C.POINTER(C.c_float)
    ptr = lambda a: a.ctypes.data_as(fp)
    for shares in (1, 2):
        m = C.c_void_p()
        devs = (C.c_int * shares)(*([0] * shares))
        assert lib.rt_multi_create_ex(devs, shares, 2, C.byref(m)) == 0, lib.rt_last_error()
        try:
            assert lib.rt_multi_set_spheres(m, inp.spheres, inp.n) == 0
            assert lib.rt_multi_set_texture(m, ptr(inp.tex[0]), ptr(inp.tex[1]), ptr(inp.tex[2]), inp.tex[0].shape[1], inp.tex[0].shape[0]) == 0
            assert lib.rt_multi_set_sky(m, C.byref(inp.sky_box), ptr(inp.sky[0]), ptr(inp.sky[1]), ptr(inp.sky[2]), inp.sky[0].shape[1],
                                        inp.sky[0].shape[0]) == 0
            assert lib.rt_multi_set_lights(m, inp.lights, 3) == 0
            tmp = rt.Scene()
            fd = tmp.frame_desc(W, H)
            for k in range(4):
                out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
                assert lib.rt_multi_render(m, C.byref(fd), out.data_ptr()) == 0, lib.rt_last_error()
                assert lib.rt_multi_sync(m) == 0
                torch.cuda.synchronize()
                assert np.array_equal(out.cpu().numpy().view(np.uint32), off[1]), (shares, k)
                for i in range(shares):
                    info = rt.LightVerdictsInfo()
                    assert lib.rt_debug_light_verdicts(lib.rt_multi_scene(m, i, None), C.byref(info), None, 0) == 0
                    assert info.state == 0 and info.slot == -1, (shares, k, i)
            tmp.close()
        finally:
            lib.rt_multi_destroy(m)


def test_more_groups_than_a_word_holds(rt, gpu):
    g = rt.generate_spheres(4096, 3)
    tiny = Scn(rt, [(g[i].orgin.x, g[i].orgin.y, g[i].orgin.z, 0.12) for i in range(4096)])
    sc = tiny.scene()
    import torch
    ids = sc.render(W, H, aov=("id",))["aov"]["id"].cpu().numpy()
    torch.cuda.synchronize()
    most = 0
    for ty in range(0, H - 7, 8):
        for tx in range(0, W, 8):
            t = ids[ty:ty + 8, tx:tx + 8].reshape(-1, 2)
            most = max(most, len({int(i) for k, i in t if k >= 0}))
    assert most > 4, most   # distinct spheres of distinct centres: one group each
    ref = tiny.scene()
    ref.set_light_verdicts(0)
    off = frame(ref)
    assert same(off, frame(ref, cull=False))
    for k in range(4):
        assert same(frame(sc), off), k
    assert sc.light_verdicts()["state"] == 2


def test_eight_lights_fill_the_word_and_a_ninth_is_refused(rt, gpu):
    pos = [(20, 20, 20), (0, 20, -20), (0, 20, 0), (-20, 15, 5), (10, 25, -5), (25, 8, 0), (-5, 30, 12), (3, 18, 25), (8, 9, 10)]
    lights = [(p, 20, 0.2 + 0.1 * (i % 3), 0.1 * (i % 4), 0.15 * (i % 5)) for i, p in enumerate(pos)]
    inp = Inputs(rt, 256)
    nine = Scn(rt, [], lights=lights)
    sc0 = inp.scene()
    assert sc0.lib.rt_scene_set_lights(sc0.handle, nine.lights, 9) != 0   # RT_MAX_LIGHTS = 8
    inp.lights, inp.n_lights = Scn(rt, [], lights=lights[:8]).lights, 8
    off = references(inp)
    sc = inp.scene()
    for k in range(4):
        assert same(frame(sc), off), k
    words = sc.light_verdicts(want_words=True)["words"]
    assert ((words >> np.uint64(14)) & np.uint64(3)).any()   # the eighth light has verdicts of its own


def test_two_frames_in_flight(inputs):
    import torch
    off = references(inputs[1024])
    sc = inputs[1024].scene()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for k in range(8):
        with torch.cuda.stream(streams[k % 2]):
            outs.append(sc.render(W, H, stream=streams[k % 2]))
    torch.cuda.synchronize()
    assert sc.light_verdicts()["state"] == 2
    for k, o in enumerate(outs):
        assert np.array_equal(o["rgba"].cpu().numpy().view(np.uint32), off[0]), k
        assert np.array_equal(o["packed"].cpu().numpy().view(np.uint32), off[1]), k


def test_meaning_of_nothing(rt, inputs):
    """A tile whose groups all carry code 1 for a light: the light's colour does not reach its pixels."""
    inp = inputs[1024]
    sc = inp.scene()
    full = frame(sc)
    frame(sc)
    words = sc.light_verdicts(want_words=True)["words"]
    assert words.shape == ((H + 7) // 8, (W + 7) // 8)
    import torch
    ids = sc.render(W, H, aov=("id",))["aov"]["id"].cpu().numpy()
    torch.cuda.synchronize()
    checked = 0
    for li in range(3):
        dark = Inputs(rt, 1024)
        dark.lights = R.copy_lights(rt, inp.lights, 3)
        dark.lights[li].r = dark.lights[li].g = dark.lights[li].b = 0.0
        d = frame(dark.scene())
        for ty in range(words.shape[0]):
            for tx in range(words.shape[1]):
                t = ids[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
                hit = t[..., 0] >= 0
                if not hit.any():
                    continue
                groups = len({int(i) for i in t[..., 1][hit]})   # spheres of distinct centres
                codes = [(int(words[ty, tx]) >> (16 * g + 2 * li)) & 3 for g in range(min(groups, 4))]
                if groups <= 4 and all(c == 1 for c in codes):
                    sl = (slice(ty * 8, ty * 8 + 8), slice(tx * 8, tx * 8 + 8))
                    assert np.array_equal(d[0][sl], full[0][sl]) and np.array_equal(d[1][sl], full[1][sl]), (li, ty, tx)
                    checked += 1
    assert checked > 50, checked


def test_tile_order_resorts(inputs):
    off = references(inputs[1024])
    sc = inputs[1024].scene()
    sc.set_tile_order(1)
    for k in range(9):   # the order is sorted again before launches 1, 2, 4 and 8 of an unchanged view
        assert same(frame(sc), off), k
    assert sc.light_verdicts()["state"] == 2


def test_launches_out_of_scope(rt, inputs):
    """Stats, G-buffer, multi-sample, cube / plane and mesh launches: the same frames, and no table."""
    import meshes
    import torch

    def run(make, **kw):
        res = []
        for mode in (0, 1):
            sc = make()
            sc.set_light_verdicts(mode)
            fs = [frame(sc, **kw) for _ in range(3)]
            assert sc.light_verdicts()["state"] == 0, kw
            assert same(fs[0], fs[1]) and same(fs[0], fs[2])
            res.append(fs[0])
        assert same(res[0], res[1]), kw

    run(inputs[256].scene, want_stats=True)
    run(inputs[256].scene, aov=("depth", "id"))
    run(inputs[256].scene, w=96, h=54, spp=4)

    def mixed():
        inp = mixed_scene(rt)
        sc = inp.scene()
        sc.set_planes(inp.planes, inp.n_planes)
        sc.set_cubes(inp.cubes, inp.n_cubes)
        return sc
    run(mixed)

    def with_mesh():
        sc = Inputs(rt, 64).scene()
        sc.set_mesh(rt.mesh_from_obj_text(meshes.uv_sphere_obj()))
        return sc
    run(with_mesh)
    torch.cuda.synchronize()
