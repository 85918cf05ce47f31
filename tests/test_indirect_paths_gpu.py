"""The diffuse paths of rt_scene_indirect_paths on the device, bit for bit: bounces = 1 against
rt_scene_indirect; both variants, with the BVH and with the whole lists, against the numpy restatement
(tests/indirect_paths_ref.py) fed by the composed reference (query_ref.CastRef) and by the device's own NEAREST and
SHADE; the exact ladder of throughputs; monotone and prefix-stable sums; the corner one bounce leaves dark; whole
queues, tails and chosen wave patterns at the second compaction (tests/indirect_paths_guides.py); every output
element; a long-lived scene against fresh ones; the refusals; the pipeline."""
from types import SimpleNamespace

import numpy as np
import pytest

import indirect_guides as IG
import indirect_paths_guides as PG
import indirect_paths_ref as R
import meshes
import postpass as P
import query_ref as Q
import test_indirect_gpu as G1
from scenes import Inputs, Scn, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
POISON = P.SENTINEL
DEAD_COLOURS = np.array([[0x7fc12345, 0x7f800000, 0xff800000, 0xffc00001],
                         [0x7f812345, 0x43960000, 0xc0a00000, 0x7fffffff]], dtype=np.uint32).view(np.float32)


class Memo:
    """A callable that keeps what it returned for a ray set: the bounces of one scene share their first rays."""

    def __init__(self, fn):
        self.fn, self.seen = fn, {}

    def __call__(self, O, D):
        k = (O.tobytes(), D.tobytes())
        if k not in self.seen:
            self.seen[k] = self.fn(O, D)
        return self.seen[k]


def _memo(pair):
    return Memo(pair[0]), Memo(pair[1])


def _paths(sc, inp, frame, **kw):
    return sc.indirect_paths(frame, cam=inp.cam, aspect=inp.aspect, want_packed=True, **kw)


def _reference(sc, inp, frame, w, h, callables, colour=True, modulate=True, **kw):
    g = G1._np(frame)
    O, D = G1._primary(sc, inp, w, h)
    return R.indirect_paths(w, g["depth"], g["normal"], g["id"], O, D, callables[0], callables[1], inp.tex,
                            albedo=g["albedo"] if modulate else None, rgba_in=g["rgba"] if colour else None,
                            details=True, **kw)


def _term(sc, inp, frame, **kw):
    return sc.indirect_paths(frame, cam=inp.cam, aspect=inp.aspect, colour=None, modulate=False, **kw)["rgba"].cpu().numpy().reshape(-1, 4)[:, :3]


# ----------------------------------------------------------------------------- one bounce is rt_scene_indirect
def test_one_bounce_is_rt_scene_indirect(rt, gpu):
    import torch
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    sc.set_indirect_timing(True)
    frame = G1._frame(sc, inp, w, h)
    for variant in (0, 1):
        for cull in (True, False):
            a = G1._call(sc, inp, frame, rays=3, cull=cull, variant=variant)
            ta, ca = sc.indirect_times(), sc.indirect_counts()
            b = _paths(sc, inp, frame, bounces=1, rays=3, cull=cull, variant=variant)
            tb, cb = sc.indirect_times(), sc.indirect_counts()
            torch.cuda.synchronize()
            G1._same_outputs(a, b, (variant, cull))
            assert len(ta) == len(tb) == (3 if variant == 0 else 1) and ca == cb
            assert sc.indirect_path_counts() == [] and len(sc.indirect_paths_times()) == len(tb)


# ----------------------------------------------------------------------------- against the independent reference
@pytest.mark.parametrize("case", ["view", "inside", "kinds", "groups"])
def test_both_variants_equal_the_composed_reference(rt, oracle, gpu, case):
    """64 spheres at 32 x 20; a camera inside a large sphere at 24 x 16, for negative t at every bounce; planes, cubes,
    spheres and a mesh with smooth normals at 32 x 20; five rays, for a second group and the running sum."""
    import torch
    mesh = None
    if case in ("view", "groups"):
        inp, w, h = Inputs(rt, 64), 32, 20
        kw = dict(rays=2, ray_base=5, seed=9, strength=0.75) if case == "view" else dict(rays=5, seed=1)
    elif case == "inside":
        inp, w, h = Scn(rt, [(0, 0, 0, 30.0), (2, 1, 6, 1.0), (-3, 0, 5, 1.5)], cam=P.cam(rt, 0, 0, 0, 180, 0)), 24, 16
        kw = dict(rays=2, ray_base=1, seed=3, strength=1.5)
    else:
        inp, mesh, w, h = mixed_scene(rt), meshes.uv_sphere_obj(), 32, 20
        kw = dict(rays=2)
    sc = P.scene(rt, inp, mesh) if mesh is not None else inp.scene()
    frame = G1._frame(sc, inp, w, h)
    calls = _memo(R.castref_callables(Q.CastRef(oracle, inp, mesh_text=mesh)))
    for bounces in (2, 3, 4):
        rgba, packed, det = _reference(sc, inp, frame, w, h, calls, bounces=bounces, **kw)
        hits = np.concatenate(det["hits"])
        assert (hits >= 2).any()                                        # paths that go on
        if case != "inside":
            assert (hits == 0).any()                                    # and gather rays that miss
        if case == "groups":
            assert len(det["counts"]) == 2
        for variant in (0, 1):
            for cull in (True, False):
                out = _paths(sc, inp, frame, bounces=bounces, cull=cull, variant=variant, **kw)
                torch.cuda.synchronize()
                G1._same(out, rgba, packed, (case, bounces, variant, cull))
                if variant == 0:
                    assert sc.indirect_path_counts() == det["counts"], (case, bounces, cull)
                    assert sc.indirect_counts() == []
                else:
                    assert sc.indirect_path_counts() == []


def test_both_variants_equal_the_restatement_over_the_device_casts(rt, gpu):
    import torch
    inp, w, h = Inputs(rt, 256), 160, 90
    sc = inp.scene()
    frame = G1._frame(sc, inp, w, h)
    rgba, packed, det = _reference(sc, inp, frame, w, h, R.device_callables(sc), bounces=3, rays=4, seed=2)
    assert det["live"].sum() > 1000 and (~det["live"]).sum() > 1000 and det["counts"][0][2] > 100
    for variant in (0, 1):
        out = _paths(sc, inp, frame, bounces=3, rays=4, seed=2, variant=variant)
        torch.cuda.synchronize()
        G1._same(out, rgba, packed, variant)
    out = _paths(sc, inp, frame, bounces=3, rays=4, seed=2)
    assert sc.indirect_path_counts() == det["counts"]


# ----------------------------------------------------------------------------- hand-made guides
def _upload(g):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(g, k))).cuda() for k in ("depth", "normal", "id", "albedo", "rgba_in")}


def _run(rt, sc, inp, g, *, bounces, rays=1, variant=0, cull=1, albedo=True, rgba_in=True, in_place=False, entry="paths",
         strength=0.75, seed=PG.SEED, ray_base=PG.RAY_BASE):
    """One call over the guides `g` with poisoned outputs: the bits of rgba_out [m, 4] and of pixels [m]."""
    import torch
    w, h = g.width, g.height
    dev = _upload(g)
    out = dev["rgba_in"].clone() if in_place else torch.full((h * w, 4), POISON, dtype=torch.int32, device="cuda")
    packed = torch.full((h * w,), POISON, dtype=torch.int32, device="cuda")
    src = out if in_place else dev["rgba_in"]
    d = sc.indirect_desc(w, h, cam=inp.cam, aspect=IG.view_aspect(rt, w, h), depth=dev["depth"].data_ptr(),
                         normal=dev["normal"].data_ptr(), id=dev["id"].data_ptr(),
                         albedo=dev["albedo"].data_ptr() if albedo else 0, rgba_in=src.data_ptr() if rgba_in else 0,
                         rgba_out=out.data_ptr(), pixels=packed.data_ptr(), rays=rays, ray_base=ray_base, seed=seed,
                         strength=strength, cull=cull, variant=variant)
    rc = sc.indirect_paths_raw(d, sc.indirect_paths_opts(bounces)) if entry == "paths" else sc.indirect_raw(d)
    assert rc == 0, rt.load_library().rt_last_error()
    torch.cuda.synchronize()
    return P.tensor_bits(out).reshape(-1, 4), P.tensor_bits(packed).reshape(-1)


def _view(rt, sc, inp, w, h):
    r = sc.primary_rays(w, h, cam=inp.cam, aspect=IG.view_aspect(rt, w, h)).reshape(-1, 6).cpu().numpy()
    return np.ascontiguousarray(r[:, :3]), np.ascontiguousarray(r[:, 3:])


def _want(rt, sc, inp, g, calls, *, bounces, rays=1, albedo=True, rgba_in=True, strength=0.75, seed=PG.SEED,
          ray_base=PG.RAY_BASE):
    O, Dir = _view(rt, sc, inp, g.width, g.height)
    rgba, packed, det = R.indirect_paths(g.width, g.depth, g.normal, g.id, O, Dir, calls[0], calls[1], inp.tex,
                                         bounces=bounces, rays=rays, ray_base=ray_base, seed=seed, strength=strength,
                                         albedo=g.albedo if albedo else None, rgba_in=g.rgba_in if rgba_in else None,
                                         details=True)
    return P.bits(rgba), packed, det


def _same_bits(got, want, what):
    (rgba, packed), (wr, wp) = got, want[:2]
    assert not (rgba == POISON).any() and not (packed == POISON).any(), what
    bad = (rgba != wr).any(axis=1)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8], rgba[bad][:2], wr[bad][:2])
    assert np.array_equal(packed, wp), what


@pytest.fixture(scope="module")
def world(rt, oracle, gpu):
    inp = PG.scene_inputs(rt)
    sc = inp.scene()
    yield SimpleNamespace(rt=rt, inp=inp, sc=sc, calls=_memo(R.castref_callables(Q.CastRef(oracle, inp))))
    sc.close()


@pytest.mark.parametrize("w,h,name", PG.cases())
def test_wave_patterns_at_the_second_compaction(world, w, h, name):
    """Every mask of indirect_paths_guides at 1, 4 and 5 rays and three bounces: the exact count per (group, bounce) and
    all bits against the restatement over the composed reference, for both variants."""
    W = world
    g = PG.masked(w, h, name)
    for k, p in enumerate(np.nonzero(g.kinds == PG.DEAD)[0][:len(DEAD_COLOURS)]):
        g.rgba_in[p] = DEAD_COLOURS[k]                                  # NaN payloads that dead pixels carry through
    for rays in (PG.RAYS if w * h <= 256 else (1, 5)):
        want = _want(W.rt, W.sc, W.inp, g, W.calls, bounces=PG.BOUNCES, rays=rays)
        assert want[2]["counts"] == PG.counts(g.kinds, rays, PG.BOUNCES)
        for variant in (0, 1):
            got = _run(W.rt, W.sc, W.inp, g, bounces=PG.BOUNCES, rays=rays, variant=variant)
            _same_bits(got, want, (name, rays, variant))
            if variant == 0:
                assert W.sc.indirect_path_counts() == PG.counts(g.kinds, rays, PG.BOUNCES), (name, rays)
        dead = g.kinds == PG.DEAD
        assert np.array_equal(got[0][dead], P.bits(g.rgba_in)[dead])


def test_outputs_in_place_optional_inputs_and_stale_scratch(world):
    W = world
    g = PG.masked(50, 30, "mixed")
    full = PG.guides(50, 30, np.full(1500, PG.CONT, dtype=np.int8))
    want = _want(W.rt, W.sc, W.inp, g, W.calls, bounces=3, rays=5)
    for variant in (0, 1):
        # an all-hit call at more rays, then a one-bounce call, leave their queues, slab, sum and counters behind
        _run(W.rt, W.sc, W.inp, full, bounces=4, rays=8, variant=variant)
        _run(W.rt, W.sc, W.inp, full, bounces=1, rays=8, variant=variant, entry="indirect")
        _same_bits(_run(W.rt, W.sc, W.inp, g, bounces=3, rays=5, variant=variant), want, ("stale", variant))
        got = _run(W.rt, W.sc, W.inp, g, bounces=3, rays=5, variant=variant, in_place=True)
        _same_bits(got, want, ("in place", variant))
    bare = _want(W.rt, W.sc, W.inp, g, W.calls, bounces=3, rays=5, albedo=False, rgba_in=False)
    for variant in (0, 1):
        _same_bits(_run(W.rt, W.sc, W.inp, g, bounces=3, rays=5, variant=variant, albedo=False, rgba_in=False), bare,
                   ("bare", variant))


# ----------------------------------------------------------------------------- exact values
def test_ladder(rt, gpu):
    """A constant sky s, a constant texture 0.5, lights of colour 0: every live pixel is exactly s * 0.5^k, k the hits of
    its path by the restatement, or exactly 0 where the budget ended it."""
    inp = PG.ladder_inputs(rt)
    sc = inp.scene()
    w, h = 50, 30
    g = PG.masked(w, h, "mixed")
    calls = _memo(R.device_callables(sc))
    for bounces in (1, 2, 3, 4):
        kw = dict(bounces=bounces, rays=1, albedo=False, rgba_in=False, strength=1.0, seed=5, ray_base=0)
        _, _, det = _want(rt, sc, inp, g, calls, **kw)
        for variant in (0, 1):
            rgba, _ = _run(rt, sc, inp, g, variant=variant, **kw)
            ks = PG.ladder_check(rgba.view(np.float32)[:, :3], det, bounces)
            assert ks == ({0, 1} if bounces == 1 else {0, 1, bounces})
    sc.close()


def test_monotone_and_prefix_stable(rt, gpu):
    """Non-negative lights, sky and texture: more bounces never darken a pixel; and a pixel all of whose paths ended
    before bounce 2 has the same bits under 2, 3 and 4 bounces."""
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    frame = G1._frame(sc, inp, w, h)
    _, _, det = _reference(sc, inp, frame, w, h, R.device_callables(sc), colour=False, modulate=False, bounces=4, rays=2,
                           seed=4)
    for variant in (0, 1):
        t = {b: _term(sc, inp, frame, bounces=b, rays=2, seed=4, variant=variant) for b in (1, 2, 3, 4)}
        assert (t[4] >= t[3]).all() and (t[3] >= t[2]).all() and (t[2] >= t[1]).all()
        assert (t[3] > t[1]).any()
        short = det["idx"][np.max(np.stack(det["hits"]), axis=0) <= 1]
        assert len(short) > 50
        assert np.array_equal(P.bits(t[2][short]), P.bits(t[3][short])) and np.array_equal(P.bits(t[2][short]), P.bits(t[4][short]))


def test_it_lights_what_one_bounce_leaves_dark(rt, gpu):
    """The construction tests/test_indirect_paths_cpu.py holds against the restatement: black under one bounce, lit
    under three wherever a path met the sphere and then the plane."""
    inp = PG.corner_inputs(rt)
    sc = inp.scene()
    g = PG.corner_guides()
    kw = dict(rays=PG.CORNER["rays"], seed=PG.CORNER["seed"], albedo=False, rgba_in=False, strength=1.0, ray_base=0)
    _, _, det = _want(rt, sc, inp, g, R.device_callables(sc), bounces=3, **kw)
    lit = PG.corner_lit(det)
    assert lit.sum() >= g.width * g.height // 2
    for variant in (0, 1):
        one = _run(rt, sc, inp, g, bounces=1, variant=variant, **kw)[0].view(np.float32)
        three = _run(rt, sc, inp, g, bounces=3, variant=variant, **kw)[0].view(np.float32)
        assert not one[:, :3].any()
        assert (three[lit, :3] > 0).all() and not three[~lit, :3].any()
    sc.close()


# ----------------------------------------------------------------------------- whole queues and tails
def test_whole_queues(rt, gpu):
    """A closed room at 1 024 x 520: every gather ray and every continuation hits, 532 480 entries at every bounce --
    more than one trip of the 2 048 x 256 grid."""
    import torch
    w, h = 1024, 520
    room = G1._box(rt, closed=True)
    sc = room.scene()
    frame = G1._frame(sc, room, w, h)
    a = _paths(sc, room, frame, bounces=3, variant=0)
    counts = sc.indirect_path_counts()
    b = _paths(sc, room, frame, bounces=3, variant=1)
    torch.cuda.synchronize()
    G1._same_outputs(a, b, "room")
    assert counts == [[w * h] * 3] and w * h > 2048 * 256


@pytest.mark.parametrize("w,h", [(1, 1), (3, 1), (1, 70), (70, 1), (64, 4)])
def test_tails_and_empty_queues(rt, gpu, w, h):
    import torch
    room = G1._box(rt, closed=True)
    room.aspect = IG.view_aspect(rt, w, h)
    sc = room.scene()
    frame = G1._frame(sc, room, w, h)
    for rays in (1, 5):
        a = _paths(sc, room, frame, bounces=3, rays=rays, variant=0)
        assert sc.indirect_path_counts() == [[min(4, rays - j0) * w * h] * 3 for j0 in range(0, rays, 4)]
        b = _paths(sc, room, frame, bounces=3, rays=rays, variant=1)
        torch.cuda.synchronize()
        G1._same_outputs(a, b, (w, h, rays))
        # two bounces: the first shade pass runs straight into the last, no middle pass
        a = _paths(sc, room, frame, bounces=2, rays=rays, variant=0)
        assert sc.indirect_path_counts() == [[min(4, rays - j0) * w * h] * 2 for j0 in range(0, rays, 4)]
        b = _paths(sc, room, frame, bounces=2, rays=rays, variant=1)
        torch.cuda.synchronize()
        G1._same_outputs(a, b, (w, h, rays, 2))
        # one bounce: the only shade pass is first and last at once; both entries, both variants
        a = _paths(sc, room, frame, bounces=1, rays=rays, variant=0)
        assert sc.indirect_counts() == [min(4, rays - j0) * w * h for j0 in range(0, rays, 4)]
        assert sc.indirect_path_counts() == []
        b = _paths(sc, room, frame, bounces=1, rays=rays, variant=1)
        c = G1._call(sc, room, frame, rays=rays, variant=0)
        assert sc.indirect_counts() == [min(4, rays - j0) * w * h for j0 in range(0, rays, 4)]
        assert sc.indirect_path_counts() == []
        d = G1._call(sc, room, frame, rays=rays, variant=1)
        torch.cuda.synchronize()
        for other, what in ((b, "variants"), (c, "entries"), (d, "entries and variants")):
            G1._same_outputs(a, other, (w, h, rays, 1, what))
    # a sky-only view: nothing is cast at any bounce, the output is the input
    inp = Inputs(rt, 8)
    sky = inp.scene()
    sky.set_spheres(inp.spheres, 0)
    sky.set_indirect_timing(True)
    frame = G1._frame(sky, inp, w, h)
    for variant, passes in ((0, 5), (1, 1)):
        out = _paths(sky, inp, frame, bounces=3, variant=variant)
        assert len(sky.indirect_paths_times()) == passes
        assert np.array_equal(P.tensor_bits(out["rgba"]), P.tensor_bits(frame["rgba"]))
        if variant == 0:
            assert sky.indirect_path_counts() == [[0, 0, 0]]
    for bounces in (2, 1):
        for variant, passes in ((0, 2 + bounces), (1, 1)):
            outs = [_paths(sky, inp, frame, bounces=bounces, variant=variant)]
            assert len(sky.indirect_paths_times()) == passes
            if variant == 0:
                assert sky.indirect_path_counts() == ([[0, 0]] if bounces == 2 else [])
                assert sky.indirect_counts() == ([] if bounces == 2 else [0])
            if bounces == 1:
                outs.append(G1._call(sky, inp, frame, variant=variant))
                assert len(sky.indirect_times()) == passes
                if variant == 0:
                    assert sky.indirect_counts() == [0] and sky.indirect_path_counts() == []
            for out in outs:
                assert np.array_equal(P.tensor_bits(out["rgba"]), P.tensor_bits(frame["rgba"]))


def test_every_output_element_is_written(rt, gpu):
    import torch
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    frame = G1._frame(sc, inp, w, h)
    want = _paths(sc, inp, frame, bounces=3, rays=5, seed=3, variant=1)
    o3 = sc.indirect_paths_opts(3)
    for variant in (0, 1):
        for rgba_in in (True, False):
            out, packed = G1._poisoned(w, h)
            assert sc.indirect_paths_raw(G1._raw(sc, inp, frame, out, packed, rgba_in=rgba_in, rays=5, seed=3, variant=variant), o3) == 0
            torch.cuda.synchronize()
            assert not (out == POISON).any() and not (packed == POISON).any(), (variant, rgba_in)
            if rgba_in:
                assert np.array_equal(P.tensor_bits(out), P.tensor_bits(want["rgba"]))
                assert np.array_equal(P.tensor_bits(packed), P.tensor_bits(want["packed"]))
        buf = frame["rgba"].clone()                                     # in place: rgba_out is rgba_in itself
        _, packed = G1._poisoned(w, h)
        d = G1._raw(sc, inp, frame, buf, packed, rays=5, seed=3, variant=variant)
        d.rgba_in = buf.data_ptr()
        assert sc.indirect_paths_raw(d, o3) == 0
        torch.cuda.synchronize()
        assert np.array_equal(P.tensor_bits(buf), P.tensor_bits(want["rgba"]))


# ----------------------------------------------------------------------------- state
def test_a_long_lived_scene_equals_fresh_scenes(rt, gpu):
    import torch
    inp = Inputs(rt, 64)
    sc = inp.scene()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    step = [0]

    def check(what, w=50, h=30, bounces=None, **kw):
        st = streams[step[0] % 2]
        step[0] += 1
        frame = G1._frame(sc, inp, w, h, stream=st)
        fresh = inp.scene()
        f2 = G1._frame(fresh, inp, w, h)
        if bounces is None:
            got = sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, want_packed=True, stream=st, **kw)
            want = G1._call(fresh, inp, f2, **kw)
        else:
            got = sc.indirect_paths(frame, cam=inp.cam, aspect=inp.aspect, want_packed=True, stream=st, bounces=bounces, **kw)
            want = _paths(fresh, inp, f2, bounces=bounces, **kw)
        torch.cuda.synchronize()
        G1._same_outputs(got, want, what)
        assert (got["rgba"][..., :3] != frame["rgba"][..., :3]).any(), what
        fresh.close()

    check("paths first", bounces=2, rays=2)
    check("one bounce after paths", rays=2)
    check("three bounces", bounces=3, rays=2)
    P.move_spheres(inp, {3: (0.5, 0.2, -0.3), 10: (-0.4, 0.1, 0.2)})
    sc.set_spheres(inp.spheres, inp.n)                                  # the shared BVH goes stale
    check("after set_spheres", bounces=4, rays=3)
    check("paths at one bounce", bounces=1, rays=4)
    check("a larger size, across the group limit", w=120, h=70, bounces=3, rays=5)   # every scratch buffer grows
    check("one bounce at the larger size", w=120, h=70, rays=9)
    check("a smaller size", bounces=2, rays=4)
    P.move_spheres(inp, {5: (0.1, -0.2, 0.3)})
    sc.set_spheres(inp.spheres, inp.n)
    check("whole lists, the yardstick", bounces=3, rays=2, cull=False, variant=1)
    check("the yardstick across groups", bounces=2, rays=6, variant=1)
    check("one bounce again", rays=16)
    check("four bounces, sixteen rays", bounces=4, rays=16)


# ----------------------------------------------------------------------------- refusals
def test_refusals_on_the_device_write_nothing(rt, gpu):
    import torch
    lib = rt.load_library()
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    frame = G1._frame(sc, inp, w, h)
    out, packed = G1._poisoned(w, h)
    ok = dict(rays=2)
    o = sc.indirect_paths_opts(3)
    for b in (0, 5):
        assert sc.indirect_paths_raw(G1._raw(sc, inp, frame, out, packed, **ok), sc.indirect_paths_opts(b)) == 1
        assert "bounces" in lib.rt_last_error().decode()
    for kw, text in ((dict(rays=0), "rays"), (dict(rays=17), "rays"), (dict(ray_base=-1), "ray_base"), (dict(cull=2), "cull"),
                     (dict(variant=2), "variant"), (dict(strength=-1.0), "strength"), (dict(aspect=0.0), "aspect")):
        assert sc.indirect_paths_raw(G1._raw(sc, inp, frame, out, packed, **{**ok, **kw}), o) == 1, kw
        theirs = lib.rt_last_error().decode()
        assert sc.indirect_raw(G1._raw(sc, inp, frame, out, packed, **{**ok, **kw})) == 1
        assert text in theirs and theirs.replace("rt_scene_indirect_paths:", "rt_scene_indirect:") == lib.rt_last_error().decode()
    d = G1._raw(sc, inp, frame, out, packed, **ok)
    d.normal += 8
    assert sc.indirect_paths_raw(d, o) == 1 and "aligned" in lib.rt_last_error().decode()
    d = G1._raw(sc, inp, frame, out, packed, **ok)
    d.rgba_out = frame["aov"]["normal"].data_ptr()
    assert sc.indirect_paths_raw(d, o) == 1 and "overlaps" in lib.rt_last_error().decode()
    bare = rt.Scene()
    assert bare.indirect_paths_raw(G1._raw(bare, inp, frame, out, packed, **ok), o) == 1 and "sky" in lib.rt_last_error().decode()
    bare.close()
    s = torch.cuda.Stream()                                             # a capturing stream
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = sc.indirect_paths_raw(G1._raw(sc, inp, frame, out, packed, **ok), o, s.cuda_stream)
    assert rc == 2 and "captured" in lib.rt_last_error().decode()
    torch.cuda.synchronize()
    assert (out == POISON).all() and (packed == POISON).all()
    assert sc.indirect_paths_raw(G1._raw(sc, inp, frame, out, packed, **ok), o) == 0    # and the scene still works
    torch.cuda.synchronize()
    assert not (out == POISON).any()


# ----------------------------------------------------------------------------- the pipeline
def test_pipeline_half_resolution_upsample_temporal_denoise(rt, gpu):
    import torch
    inp = Inputs(rt, 256)
    sc = inp.scene()
    W, H = 160, 90
    hi = G1._frame(sc, inp, W, H)
    lo = G1._frame(sc, inp, W // 2, H // 2)
    sky = (hi["aov"]["id"][..., 0] < 0).cpu().numpy()
    history = one = None
    for k in range(4):
        ind = sc.indirect_paths(lo, cam=inp.cam, aspect=inp.aspect, bounces=3, rays=1, ray_base=k)
        assert tuple(ind["rgba"].shape) == (H // 2, W // 2, 4)
        up = sc.upsample(hi, lo, colour=ind["rgba"], base=True, demodulate=True)
        history = sc.temporal(hi, history, cam=inp.cam, aspect=inp.aspect, colour=up["rgba"])
        i1 = sc.indirect(lo, cam=inp.cam, aspect=inp.aspect, rays=1, ray_base=k)
        one = sc.temporal(hi, one, cam=inp.cam, aspect=inp.aspect,
                          colour=sc.upsample(hi, lo, colour=i1["rgba"], base=True, demodulate=True)["rgba"])
        torch.cuda.synchronize()
        for t in (ind["rgba"], up["rgba"], history["rgba"]):
            assert not torch.isnan(t).any()
        assert np.array_equal(P.tensor_bits(up["rgba"])[sky], P.tensor_bits(hi["rgba"])[sky])
    assert float(history["rgba"][..., 3].max()) == 4.0
    out = sc.denoise({"rgba": history["rgba"], "aov": hi["aov"]})
    torch.cuda.synchronize()
    assert tuple(out["rgba"].shape) == (H, W, 4) and not torch.isnan(out["rgba"]).any()
    assert np.array_equal(P.tensor_bits(out["rgba"])[sky][:, :3], P.tensor_bits(hi["rgba"])[sky][:, :3])
    # three bounces carry more light than one
    assert float(history["rgba"][..., :3].sum()) > float(one["rgba"][..., :3].sum()) > float(hi["rgba"][..., :3].sum())
