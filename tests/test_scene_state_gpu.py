"""A long-lived scene against fresh ones. rt_scene keeps about a dozen caches between calls (eye cones, light columns,
occluder lists, raygen tables, RtFrameAux, the sphere table, tile orders, the sphere BVH, materials, frame graphs), each
reused while a hand-written key says it is current. Here one scene goes through sequences of changes -- targeted
transitions first, then seeded random walks (tests/scene_walk.py) -- and every output (rgba bits, packed, every rt_hit
field, occlusion, reflect queue lengths) is compared with a fresh scene built from the current state alone. A few
checkpoints compare with the oracle or the reflection composers directly, so that the check is not circular.

The caches that came later are covered by tests/test_scene_state2_gpu.py with this file's helpers and the second
vocabulary of tests/scene_walk.py: the reflect scope with the plane and cube material tables, the supersampling scratch
and its per-group events, the view-list slots and their switch (also under a recorded graph), G-buffer outputs, the
denoisers' shared scratch, temporal accumulation's raygen table, temporal_motion's host copies, guided upsampling and
the wrapper's host mirrors of the material tables (Scene.upsample_select). The six walks of this file stay as they
were, op for op (their digests are pinned in tests/test_scene_walk_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import scene_walk as sw
from scene_walk import State

pytestmark = pytest.mark.gpu


def _u32(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def _frame(rt, scene, w, h, cam=0, aspect=None, spp=1, cull=1, band=(0, 0), depth=0, stream=None):
    """Enqueue a frame (no wait): {'packed', 'rgba'} tensors."""
    c = sw.camera(rt, cam) if isinstance(cam, int) else cam
    return scene.render(w, h, y0=band[0], y1=band[1], cam=c, aspect=aspect, spp=spp, cull=bool(cull),
                        reflect_depth=depth, stream=stream)


def _fresh_frame(rt, state, w, h, stats=False, **kw):
    """The frame (and with `stats` the reflect queue lengths) of a fresh scene built from `state`."""
    import torch
    s = sw.fresh_scene(rt, state)
    try:
        out = _frame(rt, s, w, h, **kw)
        torch.cuda.synchronize()
        res = (_u32(out["packed"]), _u32(out["rgba"]))
        if stats:
            res = res + (s.reflect_stats()["queue"],)
        return res
    finally:
        s.close()


def _same(got, want, where):
    import torch
    torch.cuda.synchronize()
    g = (_u32(got["packed"]), _u32(got["rgba"])) if isinstance(got, dict) else got
    assert np.array_equal(g[0], want[0]), "packed differs: %s" % where
    assert np.array_equal(g[1], want[1]), "rgba differs: %s" % where


def _render_check(rt, scene, state, w, h, where, **kw):
    got = _frame(rt, scene, w, h, **kw)
    want = _fresh_frame(rt, state, w, h, **kw)
    _same(got, want, where)
    return want


def _lights(rt, lights):
    return sw.light_array(rt, lights), len(lights)


def _set(rt, scene, state, op):
    sw.apply_to_scene(rt, scene, op, state)
    return sw.apply(state, op)


def _oracle_check(rt, oracle, state, got, w, h, cam=0, aspect=None, where=""):
    rgba, packed, _ = sw.oracle_frame(oracle, rt, state, sw.camera(rt, cam), w, h, aspect=aspect)
    assert np.array_equal(got[0], packed), "packed differs from the oracle: %s" % where
    assert np.array_equal(got[1], np.ascontiguousarray(rgba, dtype=np.float32).view(np.uint32)), \
        "rgba differs from the oracle: %s" % where


# ------------------------------------------------------------------------------------------------ graphs and lights
class _Graph:
    """One frame graph over `scene` (`spp` samples in one kernel node, no host copy), replayed on its own stream."""

    def __init__(self, rt, scene, w, h, cam=0, spp=1):
        import torch
        self.lib, self.rt, self.w, self.h, self.spp = rt.load_library(), rt, w, h, spp
        self.pk = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        self.rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        self.stream = torch.cuda.Stream()
        self.cam = cam
        fd = scene.frame_desc(w, h, pixels=self.pk.data_ptr(), rgba=self.rgba.data_ptr(), cam=sw.camera(rt, cam))
        self.g = self.lib.rt_graph_capture(scene.handle, C.byref(fd), spp, None, self.stream.cuda_stream)
        assert self.g, self.lib.rt_last_error()

    def set_camera(self, cam):
        self.cam = cam
        assert self.lib.rt_graph_set_camera(self.g, C.byref(sw.camera(self.rt, cam))) == 0, self.lib.rt_last_error()

    def replay(self):
        import torch
        self.pk.zero_()
        self.rgba.zero_()
        torch.cuda.synchronize()
        assert self.lib.rt_graph_launch(self.g, self.stream.cuda_stream) == 0, self.lib.rt_last_error()
        self.stream.synchronize()
        return _u32(self.pk), _u32(self.rgba)

    def want(self, state):
        return _fresh_frame(self.rt, state, self.w, self.h, cam=self.cam, spp=self.spp)

    def destroy(self):
        self.lib.rt_graph_destroy(self.g)


def _light_change(kind):
    L = [list(l) for l in sw.DEFAULT_LIGHTS]
    if kind == "moved":
        L[0][0:3] = [25.0, 18.0, 12.0]
    elif kind == "count":
        L.append([-10.0, 22.0, 5.0, 10.0, 0.5, 0.5, 0.2])
    else:                                   # only size and colour
        L[1][3] = 6.0
        L[1][4:7] = [0.3, 0.8, 0.1]
    return tuple(tuple(l) for l in L)


@pytest.mark.parametrize("kind", ["moved", "count", "colour"])
def test_graph_replay_right_after_set_lights(rt, oracle, gpu, kind):
    """A replay directly after rt_scene_set_lights (no render in between) renders the new lights; so does a replay
    after rt_graph_set_camera following set_lights; setting the same lights again changes nothing."""
    w, h = 96, 54
    st = State(spheres=(1024, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    g = _Graph(rt, scene, w, h)
    try:
        old = g.replay()
        assert np.array_equal(old[0], g.want(st)[0])
        st = _set(rt, scene, st, {"op": "lights", "lights": _light_change(kind)})
        got = g.replay()
        want = g.want(st)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "replay after set_lights (%s)" % kind
        assert not np.array_equal(got[0], old[0])
        if kind == "moved":   # the checkpoint: the oracle with the new lights
            _oracle_check(rt, oracle, st, got, w, h, where="graph replay after set_lights")
        # set_lights, then a camera move of the graph, then the replay
        st = _set(rt, scene, st, {"op": "lights", "lights": sw.DEFAULT_LIGHTS})
        g.set_camera(3)
        got = g.replay()
        want = g.want(st)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "set_camera after set_lights"
        # the same lights again (what the drop-in boundary does every frame): the replay is unchanged
        st = _set(rt, scene, st, {"op": "lights", "lights": sw.DEFAULT_LIGHTS})
        again = g.replay()
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    finally:
        g.destroy()
        scene.close()


def _axis_bits(p):
    p = np.float32(p)
    ln = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2], dtype=np.float32)
    return (p / ln).astype(np.float32).view(np.uint32)


@pytest.mark.parametrize("n", [1024, 9000])   # 9000: above the occluder lists, the shadow rays walk the column tables
def test_light_moved_along_its_axis_and_through_the_origin(rt, oracle, gpu, n):
    """pos * 2 keeps the normalised axis (the column tables' key) bit for bit and moves the light (the occluder lists'
    key): the frame equals a fresh scene's (and the oracle's). Then the light at the origin (no axis), back, and to
    another axis."""
    w, h = 96, 54
    st = State(spheres=(n, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    try:
        first = _render_check(rt, scene, st, w, h, "start")
        L = [list(l) for l in st.lights]
        p0 = list(L[0][0:3])
        L[0][0:3] = [v * 2.0 for v in p0]
        assert np.array_equal(_axis_bits(p0), _axis_bits(L[0][0:3]))
        st = _set(rt, scene, st, {"op": "lights", "lights": tuple(tuple(l) for l in L)})
        got = _render_check(rt, scene, st, w, h, "light 0 at pos * 2")
        assert not np.array_equal(got[0], first[0])
        if n <= 1024:
            _oracle_check(rt, oracle, st, got, w, h, where="light 0 at pos * 2")
        for cull in (1, 0):
            _render_check(rt, scene, st, w, h, "light 0 at pos * 2, cull %d" % cull, cull=cull, cam=2)
        L[0][0:3] = [0.0, 0.0, 0.0]
        st = _set(rt, scene, st, {"op": "lights", "lights": tuple(tuple(l) for l in L)})
        _render_check(rt, scene, st, w, h, "light 0 at the origin")
        _render_check(rt, scene, st, w, h, "light 0 at the origin, camera 1", cam=1)
        L[0][0:3] = p0
        st = _set(rt, scene, st, {"op": "lights", "lights": tuple(tuple(l) for l in L)})
        back = _render_check(rt, scene, st, w, h, "light 0 back")
        assert np.array_equal(back[0], first[0]) and np.array_equal(back[1], first[1])
        for k, pos in enumerate(([-15.0, 25.0, 8.0], [5.0, 30.0, -12.0])):   # other axes, the same count
            L[k][0:3] = pos
            st = _set(rt, scene, st, {"op": "lights", "lights": tuple(tuple(l) for l in L)})
            _render_check(rt, scene, st, w, h, "light %d on another axis" % k)
            _render_check(rt, scene, st, w, h, "light %d on another axis, camera 5" % k, cam=5)
    finally:
        scene.close()


# ------------------------------------------------------------------------------------------------ sphere table
def test_sphere_counts_cross_the_thresholds(rt, oracle, gpu):
    """One scene through 0, 63, 64, 65 (eye cones and light columns from 64 on), 8191 .. 8193 (occluder lists up to
    8192, device-built eye cones up to 8192) and above, up and down; the same list set twice."""
    w, h = 64, 36
    st = State(spheres=(65, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    try:
        got = _render_check(rt, scene, st, w, h, "65 spheres")
        _oracle_check(rt, oracle, st, got, w, h, where="65 spheres")
        for n, seed in ((64, 2), (63, 3), (0, 1), (64, 4), (65, 5), (8191, 1), (8192, 2), (8193, 3), (9000, 4),
                        (8192, 5), (8191, 6), (1024, 7), (65, 8), (64, 9), (1024, 7)):
            for rep in range(2 if n in (64, 8193) else 1):        # the same list again: the h_prev shortcut
                st = _set(rt, scene, st, {"op": "spheres", "spheres": (n, seed, 0.0)})
                where = "%d spheres (seed %d, set %d times)" % (n, seed, rep + 1)
                _render_check(rt, scene, st, w, h, where)
                _render_check(rt, scene, st, w, h, where + ", cull 0, camera 2", cull=0, cam=2)
    finally:
        scene.close()


def test_eye_cone_slots_cycle_on_two_streams(rt, oracle, gpu):
    """Five ray origins cycled A B C D E A B ... over three cone slots, frames alternating between two streams and
    compared only after all of them are enqueued; a same-count sphere change between two visits to A."""
    import torch
    w, h = 96, 54
    st = State(spheres=(1024, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    try:
        for phase in range(2):
            seq = [0, 1, 2, 3, 4, 0, 2, 1, 0]
            outs = []
            for i, cam in enumerate(seq):
                streams[i & 1].wait_stream(torch.cuda.current_stream())
                outs.append(_frame(rt, scene, w, h, cam=cam, stream=streams[i & 1]))
            torch.cuda.synchronize()
            for cam, out in zip(seq, outs):
                want = _fresh_frame(rt, st, w, h, cam=cam)
                _same(out, want, "phase %d camera %d" % (phase, cam))
                if phase == 1 and cam == 4:
                    _oracle_check(rt, oracle, st, want, w, h, cam=4, where="camera 4 after the sphere move")
            st = _set(rt, scene, st, {"op": "spheres", "spheres": (1024, 1, 0.5)})   # same count, moved
    finally:
        scene.close()


def test_raygen_tables_follow_aspect_and_samples(rt, oracle, gpu):
    """The same width and height with another aspect; spp 1 -> 4 -> 1; rt_scene_primary_rays in between."""
    import torch
    w, h = 96, 54
    st = State(spheres=(256, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    try:
        for aspect in (None, 0.75, 1.25, None, 0.75):
            for spp in (1, 4, 1):
                got = _render_check(rt, scene, st, w, h, "aspect %s spp %d" % (aspect, spp), aspect=aspect, spp=spp)
                if aspect == 0.75 and spp == 1:
                    _oracle_check(rt, oracle, st, got, w, h, aspect=0.75, where="aspect 0.75")
                rays = scene.primary_rays(w, h, cam=sw.camera(rt, 1), aspect=aspect)
                fresh = sw.fresh_scene(rt, st)
                want = fresh.primary_rays(w, h, cam=sw.camera(rt, 1), aspect=aspect)
                torch.cuda.synchronize()
                assert np.array_equal(_u32(rays), _u32(want)), "primary rays, aspect %s" % aspect
                fresh.close()
    finally:
        scene.close()


def test_tile_order_slots_evict(rt, gpu):
    """Five layouts (sizes, bands, samples) cycled twice over four tile-order slots: every frame equals a fresh one."""
    st = State(spheres=(1024, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    layouts = [dict(w=64, h=36), dict(w=96, h=54), dict(w=96, h=54, band=(10, 40)), dict(w=128, h=72, spp=2),
               dict(w=64, h=36, band=(5, 20), cull=0)]
    try:
        for rnd in range(2):
            for i, lay in enumerate(layouts):
                lay = dict(lay)
                w, h = lay.pop("w"), lay.pop("h")
                for cam in (0, 1):
                    _render_check(rt, scene, st, w, h, "round %d layout %d camera %d" % (rnd, i, cam), cam=cam, **lay)
    finally:
        scene.close()


# ------------------------------------------------------------------------------------------------ materials
def test_materials_through_sphere_changes(rt, oracle, gpu):
    """Glass, then the spheres moved at the same count (materials kept, BVH rebuilt); new mirrors through the new entry;
    the old entry (no glass); another count (no materials); the old count again (none come back). Reflective frames and
    their queue lengths equal a fresh scene's; checkpoints against the glass composer."""
    from test_refract_cpu import glass_composer_for
    from scenes import Inputs
    w, h, n = 64, 36, 256
    st = State(spheres=(n, 1, 0.0))
    scene = sw.fresh_scene(rt, st)

    def check(where, depth=3, cull=1, cam=0):
        got = _frame(rt, scene, w, h, cam=cam, depth=depth, cull=cull)
        want = _fresh_frame(rt, st, w, h, stats=depth > 0, cam=cam, depth=depth, cull=cull)
        _same(got, want, where)
        if depth:
            assert scene.reflect_stats()["queue"] == want[2], where
        return want

    try:
        plain = check("no materials", depth=0)
        st = _set(rt, scene, st, {"op": "materials", "mats": ("ex", 5)})
        want = check("glass")
        k, tau, ior = sw.material_arrays("ex", 5, n)
        inp = Inputs(rt, n)
        comp = glass_composer_for(oracle, rt, inp)
        rgba, packed = comp.render(w, h, k, 3, tau=tau, ior=ior)
        assert np.array_equal(want[0], packed) and np.array_equal(want[1], rgba.view(np.uint32)), "glass composer"
        st = _set(rt, scene, st, {"op": "spheres", "spheres": (n, 1, 0.75)})       # same count: kept, BVH rebuilt
        check("glass, spheres moved")
        check("glass, spheres moved, cull 0", cull=0)
        st = _set(rt, scene, st, {"op": "materials", "mats": ("ex", 6)})          # new k at the same length
        check("other mirrors and glass")
        st = _set(rt, scene, st, {"op": "materials", "mats": ("k", 6)})           # the old entry clears the glass
        check("old entry: mirrors only")
        st = _set(rt, scene, st, {"op": "materials", "mats": ("ex", 5)})
        check("glass again", cam=1)
        st = _set(rt, scene, st, {"op": "spheres", "spheres": (n + 1, 2, 0.0)})   # another count: cleared
        assert st.mats is None
        refl = check("new count: no materials")
        assert np.array_equal(refl[0], _fresh_frame(rt, st, w, h)[0])
        st = _set(rt, scene, st, {"op": "spheres", "spheres": (n, 1, 0.0)})       # back: none come back
        back = check("old count again")
        assert np.array_equal(back[0], plain[0]) and np.array_equal(back[1], plain[1])
    finally:
        scene.close()


# ------------------------------------------------------------------------------------------------ queries
def _random_rays(seed, m=2048):
    rng = np.random.default_rng(seed)
    O = rng.uniform(-15, 15, (m, 3)).astype(np.float32)
    O[: m // 2] = np.float32([4.0, 3.0, 9.0]) + rng.normal(0, 1, (m // 2, 3)).astype(np.float32)
    D = rng.normal(0, 1, (m, 3)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True).astype(np.float32)
    return np.concatenate([O, D], axis=1).astype(np.float32)


def _query_outputs(scene, rays, modes, cull):
    return {m: scene.trace_rays(rays, m, cull=bool(cull)) for m in modes}


def _query_check(rt, scene, state, rays, where, modes=("nearest", "occluded", "shade"), cull=1):
    """Queries on the long-lived scene first (directly after whatever came before), then on a fresh scene."""
    import torch
    got = _query_outputs(scene, rays, modes, cull)
    fresh = sw.fresh_scene(rt, state)
    try:
        want = _query_outputs(fresh, rays, modes, cull)
        torch.cuda.synchronize()
    finally:
        fresh.close()
    for m in modes:
        if m == "nearest":
            a = np.stack([_u32(got[m][f].reshape(len(rays), -1)) for f in ("t", "kind", "index")], 1)
            for f in ("uv", "txy", "normal", "new_org"):
                assert np.array_equal(_u32(got[m][f]), _u32(want[m][f])), "%s: nearest %s" % (where, f)
            b = np.stack([_u32(want[m][f].reshape(len(rays), -1)) for f in ("t", "kind", "index")], 1)
            assert np.array_equal(a, b), "%s: nearest t/kind/index" % where
        else:
            for f in got[m]:
                assert np.array_equal(_u32(got[m][f]), _u32(want[m][f])), "%s: %s %s" % (where, m, f)
    return want


def test_queries_directly_after_changes(rt, oracle, gpu):
    """NEAREST, OCCLUDED and SHADE issued right after set_spheres, set_lights and set_texture (no render in between)
    equal a fresh scene's; a reflective frame right after a query rebuilt the BVH."""
    import torch
    w, h = 64, 36
    st = State(spheres=(1024, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    rand = torch.from_numpy(_random_rays(5)).cuda()
    try:
        prim = sw.fresh_scene(rt, st)
        rays = prim.primary_rays(w, h, cam=sw.camera(rt, 0)).reshape(-1, 6)
        torch.cuda.synchronize()
        prim.close()
        _render_check(rt, scene, st, w, h, "start")
        changes = [{"op": "spheres", "spheres": (1024, 1, 0.5)}, {"op": "lights", "lights": _light_change("moved")},
                   {"op": "texture", "texture": 1}, {"op": "spheres", "spheres": (300, 2, 0.0)},
                   {"op": "lights", "lights": _light_change("count")}, {"op": "spheres", "spheres": (300, 3, 0.0)}]
        for i, op in enumerate(changes):
            st = _set(rt, scene, st, op)
            for cull in (1, 0):
                want = _query_check(rt, scene, st, rays, "after %s, primary rays, cull %d" % (op["op"], cull), cull=cull)
                _query_check(rt, scene, st, rand, "after %s, random rays, cull %d" % (op["op"], cull), cull=cull)
            if i == 1:   # the checkpoint: SHADE of the frame's primary rays is the oracle's frame
                _, packed, _ = sw.oracle_frame(oracle, rt, st, sw.camera(rt, 0), w, h)
                assert np.array_equal(_u32(want["shade"]["packed"]).reshape(h, w), packed)
        # a query rebuilds the BVH after a same-count move; the reflective frame that follows reads it
        st = _set(rt, scene, st, {"op": "materials", "mats": ("ex", 2)})
        _render_check(rt, scene, st, w, h, "reflective before the move", depth=2)
        st = _set(rt, scene, st, {"op": "spheres", "spheres": (300, 3, -0.5)})
        _query_check(rt, scene, st, rand, "nearest after the move", modes=("nearest",))
        _render_check(rt, scene, st, w, h, "reflective after the query", depth=2)
    finally:
        scene.close()


# ------------------------------------------------------------------------------------------------ several GPUs
def test_multi_one_share_follows_changes(rt, gpu):
    """rt_multi_create(1): lights, spheres and resolution change between frames; every rt_multi_render equals the
    frame of a fresh single scene."""
    import torch
    lib = rt.load_library()
    m = lib.rt_multi_create(1)
    assert m, lib.rt_last_error()
    fp = C.POINTER(C.c_float)
    ptr = lambda a: a.ctypes.data_as(fp)
    st = State(spheres=(256, 1, 0.0))
    try:
        assert lib.rt_multi_set_spheres(m, sw.sphere_array(rt, st.spheres), st.n) == 0
        tex = sw.texture_planes(rt, 0)
        assert lib.rt_multi_set_texture(m, ptr(tex[0]), ptr(tex[1]), ptr(tex[2]), tex[0].shape[1], tex[0].shape[0]) == 0
        box, sky = sw.sky(rt)
        assert lib.rt_multi_set_sky(m, C.byref(box), ptr(sky[0]), ptr(sky[1]), ptr(sky[2]), sky[0].shape[1],
                                    sky[0].shape[0]) == 0
        assert lib.rt_multi_set_lights(m, *_lights(rt, st.lights)) == 0
        steps = [None, ("lights", _light_change("moved")), ("size", (128, 64)), ("spheres", (1024, 2, 0.0)),
                 ("lights", _light_change("colour")), ("size", (96, 48)), ("spheres", (1024, 2, 0.5)),
                 ("lights", _light_change("count")), ("size", (160, 96))]
        w, h = 96, 48
        sc = rt.Scene()
        for i, change in enumerate(steps):
            if change and change[0] == "lights":
                st = sw.apply(st, {"op": "lights", "lights": change[1]})
                assert lib.rt_multi_set_lights(m, *_lights(rt, st.lights)) == 0
            elif change and change[0] == "spheres":
                st = sw.apply(st, {"op": "spheres", "spheres": change[1]})
                assert lib.rt_multi_set_spheres(m, sw.sphere_array(rt, st.spheres), st.n) == 0
            elif change:
                w, h = change[1]
            fd = sc.frame_desc(w, h, cam=sw.camera(rt, i % 3))
            out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            assert lib.rt_multi_render(m, C.byref(fd), out.data_ptr()) == 0, lib.rt_last_error()
            assert lib.rt_multi_sync(m) == 0
            torch.cuda.synchronize()
            want = _fresh_frame(rt, st, w, h, cam=i % 3)
            assert np.array_equal(_u32(out), want[0]), "step %d (%s)" % (i, change)
        sc.close()
    finally:
        lib.rt_multi_destroy(m)


# ------------------------------------------------------------------------------------------------ random walks
def _walk_render(rt, scene, state, op, streams, pending, where):
    import torch
    w, h = op["size"]
    kw = dict(cam=op["cam"], aspect=op["aspect"], spp=op["spp"], cull=op["cull"], band=op["band"], depth=op["depth"])
    want = _fresh_frame(rt, state, w, h, stats=op["depth"] > 0, **kw)
    st = streams[op["stream"]]
    st.wait_stream(torch.cuda.current_stream())   # (the output tensors come from the current stream's pool)
    got = _frame(rt, scene, w, h, stream=st, **kw)
    if op["defer"]:                              # compared after the next step has run
        pending.append((where, got, want))
        return
    _same(got, want, where)
    if op["depth"]:
        assert scene.reflect_stats()["queue"] == want[2], where + ": reflect queues"


def _walk_query(rt, scene, state, op, where):
    import torch
    w, h = op["size"]
    if op["rays"] == "primary":
        rays = scene.primary_rays(w, h, cam=sw.camera(rt, op["cam"]), aspect=op["aspect"])
        fresh = sw.fresh_scene(rt, state)
        want = fresh.primary_rays(w, h, cam=sw.camera(rt, op["cam"]), aspect=op["aspect"])
        torch.cuda.synchronize()
        fresh.close()
        assert np.array_equal(_u32(rays), _u32(want)), where + ": primary rays"
        rays = rays.reshape(-1, 6)
    else:
        rays = torch.from_numpy(_random_rays(op["ray_seed"], 1024)).cuda()
    _query_check(rt, scene, state, rays, where, modes=op["modes"], cull=op["cull"])


@pytest.mark.parametrize("seed", sw.WALK_SEEDS)
def test_random_walk(rt, gpu, seed):
    """One scene through a seeded walk of sw.WALK_STEPS steps (tests/scene_walk.py); every output equals a fresh
    scene's. Some frames go to a second stream and are compared only after the next step (often a change) ran."""
    import torch
    ops = sw.generate(seed, sw.WALK_STEPS)
    st = State()
    scene = sw.fresh_scene(rt, st)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    gf = sw.GRAPH_FRAME
    g = _Graph(rt, scene, gf["w"], gf["h"], spp=gf["spp"])
    pending = []
    try:
        for i, op in enumerate(ops):
            where = "seed %d step %d %s" % (seed, i, op)
            ready, pending = pending, []
            k = op["op"]
            if k in sw.MUTATIONS:
                sw.apply_to_scene(rt, scene, op, st)
                st = sw.apply(st, op)
            elif k == "render":
                _walk_render(rt, scene, st, op, streams, pending, where)
            elif k == "query":
                _walk_query(rt, scene, st, op, where)
            else:
                if op["cam"] is not None:
                    g.set_camera(op["cam"])
                got = g.replay()
                want = g.want(st)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), where + ": graph replay"
            torch.cuda.synchronize()
            for w_, got, want in ready:
                _same(got, want, w_ + " (checked after step %d)" % i)
        for w_, got, want in pending:
            _same(got, want, w_)
    finally:
        torch.cuda.synchronize()
        g.destroy()
        scene.close()
