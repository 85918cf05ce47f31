"""Emissive surfaces (rt_scene_set_emission) on the device, bit for bit on rgba and the packed words, both
variants, with the BVH and with the whole lists: against the wrapped restatement (tests/indirect_emit_ref.py) over the
composed reference (query_ref.CastRef) and over the device's own NEAREST and SHADE; the dyadic furnace; no table is
the pass as it was; an emitter lights a room; the wave patterns of tests/indirect_paths_guides.py and small sizes;
poisoned outputs, dead pixels and a long-lived scene against fresh ones; the capture refusal; Scene.emission_term."""
from types import SimpleNamespace

import numpy as np
import pytest

import indirect_emit_ref as E
import indirect_guides as IG
import indirect_paths_guides as PG
import indirect_paths_ref as R
import meshes
import postpass as P
import query_ref as Q
import test_indirect_gpu as G1
import test_indirect_paths_gpu as G2
from scenes import Inputs, Scn, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
NAN_FILL = 0x7fc12345           # a quiet NaN with a payload, as an int32
VARIANTS = [(variant, cull) for variant in (0, 1) for cull in (True, False)]


def _colours(n, every, seed=11):
    """[n, 3]: every `every`-th primitive emits a colour of its own, the others nothing."""
    e = np.zeros((n, 3), dtype=np.float32)
    k = np.arange(0, n, every)
    e[k] = (f32(0.125) + np.random.default_rng(seed).random((len(k), 3), dtype=np.float32) * f32(2)).astype(np.float32)
    return e


def _set_tables(sc, tabs):
    for name in ("sphere", "plane", "cube"):
        sc.set_emission(name, tabs.get(name))


def _call(sc, inp, frame, bounces, entry="paths", **kw):
    """indirect_paths, or -- bounces == 1 and entry "indirect" -- indirect."""
    if entry == "indirect":
        assert bounces == 1
        return G1._call(sc, inp, frame, **kw)
    return G2._paths(sc, inp, frame, bounces=bounces, **kw)


def _counts(sc, bounces):
    """The last variant-0 call's queue lengths as [group][bounce], whichever entry's counters hold them."""
    return sc.indirect_path_counts() if bounces > 1 else [[c] for c in sc.indirect_counts()]


# ----------------------------------------------------------------------------- against the composed reference
@pytest.mark.parametrize("case", ["view", "groups", "kinds", "inside"])
def test_both_variants_equal_the_restatement_over_the_composed_reference(rt, oracle, gpu, case):
    """64 spheres at 32 x 20, every fourth emissive, at one to four bounces; the same scene at five rays (a second group)
    with ray_base, seed and strength; planes, cubes, spheres and a mesh with one emissive plane, one emissive cube and
    two emissive spheres (a gather hit on a triangle takes nothing); a camera inside a large emissive sphere."""
    import torch
    mesh = None
    if case in ("view", "groups"):
        inp, w, h = Inputs(rt, 64), 32, 20
        tabs = dict(sphere=_colours(64, 4))
        kw = dict(rays=2) if case == "view" else dict(rays=5, ray_base=5, seed=9, strength=0.75)
    elif case == "kinds":
        inp, mesh, w, h = mixed_scene(rt), meshes.uv_sphere_obj(), 32, 20
        sph = np.zeros((inp.n, 3), dtype=np.float32)
        sph[3], sph[inp.n - 1] = (0.5, 1.25, 0.25), (2.0, 0.125, 0.75)
        cube = np.zeros((inp.n_cubes, 3), dtype=np.float32)
        cube[inp.n_cubes - 1] = (0.75, 0.5, 1.5)
        tabs, kw = dict(sphere=sph, plane=[[0.25, 0.5, 1.0], [0, 0, 0]], cube=cube), dict(rays=2)
    else:
        inp, w, h = Scn(rt, [(0, 0, 0, 30.0), (2, 1, 6, 1.0), (-3, 0, 5, 1.5)], cam=P.cam(rt, 0, 0, 0, 180, 0)), 24, 16
        tabs, kw = dict(sphere=[[0.25, 0.5, 1.0], [0, 0, 0], [0, 0, 0]]), dict(rays=2, ray_base=1, seed=3, strength=1.5)
    sc = P.scene(rt, inp, mesh)
    bare = P.scene(rt, inp, mesh)                                       # the same scene without tables
    _set_tables(sc, tabs)
    frame = G1._frame(sc, inp, w, h)
    inner = G2._memo(R.castref_callables(Q.CastRef(oracle, inp, mesh_text=mesh)))
    calls = E.emissive(inner[0], inner[1], E.tables(**tabs))
    for bounces in (1, 2, 3, 4):
        rgba, packed, det = G2._reference(sc, inp, frame, w, h, calls, bounces=bounces, **kw)
        dark = G2._reference(sc, inp, frame, w, h, inner, bounces=bounces, **kw)
        assert (P.bits(rgba) != P.bits(dark[0])).any() and det["counts"] == dark[2]["counts"]
        if case == "inside":
            assert (G1._np(frame)["depth"].reshape(-1)[det["live"]] < 0).any()
        for variant, cull in VARIANTS:
            for entry in (("paths", "indirect") if bounces == 1 else ("paths",)):
                out = _call(sc, inp, frame, bounces, entry, cull=cull, variant=variant, **kw)
                torch.cuda.synchronize()
                G1._same(out, rgba, packed, (case, bounces, variant, cull, entry))
                if variant == 0:                                        # emission changes no path
                    assert _counts(sc, bounces) == det["counts"], (case, bounces, cull, entry)
                    _call(bare, inp, frame, bounces, entry, cull=cull, variant=0, **kw)
                    assert _counts(bare, bounces) == det["counts"]
    sc.close()
    bare.close()


def test_both_variants_equal_the_restatement_over_the_device_casts(rt, gpu):
    import torch
    inp, w, h = Inputs(rt, 256), 160, 90
    sc = inp.scene()
    tab = _colours(256, 8)
    sc.set_emission("sphere", tab)
    frame = G1._frame(sc, inp, w, h)
    inner = E.device_callables(sc)
    calls = E.emissive(inner[0], inner[1], E.tables(sphere=tab))
    rgba, packed, det = G2._reference(sc, inp, frame, w, h, calls, bounces=3, rays=4, seed=2)
    assert det["live"].sum() > 1000 and (~det["live"]).sum() > 1000 and det["counts"][0][2] > 100
    first = inner[0](det["start"][det["idx"]], det["G"][0])
    assert (tab[first["index"][first["kind"] == E.SPHERE]] > 0).any()   # gather rays that meet an emitter
    for variant in (0, 1):
        out = G2._paths(sc, inp, frame, bounces=3, rays=4, seed=2, variant=variant)
        torch.cuda.synchronize()
        G1._same(out, rgba, packed, variant)
    G2._paths(sc, inp, frame, bounces=3, rays=4, seed=2)
    assert sc.indirect_path_counts() == det["counts"]
    sc.close()


# ----------------------------------------------------------------------------- exact values
def test_the_dyadic_furnace(rt, gpu):
    """A closed furnace whose every surface emits E = (0.25, 0.5, 1.0) under a constant texture 0.5 and lights of
    colour 0: every gather path hits at every bounce, every hit is E, the throughput halves per bounce, and every live
    pixel is exactly E * (2 - 2^(1 - B)) -- E, 1.5 E, 1.75 E, 1.875 E, all exact in binary32, as are the sum of four rays
    and its mean. No tolerance.
    The furnace is the closed room of test_indirect_gpu._box, six emissive planes and an emissive sphere, not the
    inside of one sphere: castRay reports a sphere met from inside by its negative near root, the point behind the ray,
    whose outward normal sends the gather rays out of the sphere -- 625 of 960 hit anything in the composed reference,
    and the rest see the sky. (That case is held bit for bit against the reference above, "inside".)"""
    import torch
    tex = [np.full((8, 8), 0.5, dtype=np.float32)] * 3
    inp = G1._box(rt, closed=True, tex=tex, lights=[((20, 20, 20), 20, 0.0, 0.0, 0.0)])
    sc = inp.scene()
    emit = np.array([0.25, 0.5, 1.0], dtype=np.float32)
    sc.set_emission("sphere", emit[None])
    sc.set_emission("plane", np.repeat(emit[None], inp.n_planes, axis=0))
    w, h = 50, 30
    frame = G1._frame(sc, inp, w, h)
    assert (frame["aov"]["id"][..., 0] > 0).all()
    for bounces, factor in ((1, 1.0), (2, 1.5), (3, 1.75), (4, 1.875)):
        want = np.tile(np.append(emit * f32(factor), f32(1)).astype(np.float32), (w * h, 1))
        for variant, cull in VARIANTS:
            for entry in (("paths", "indirect") if bounces == 1 else ("paths",)):
                out = _call(sc, inp, frame, bounces, entry, colour=None, modulate=False, strength=1.0, rays=4,
                            cull=cull, variant=variant)
                torch.cuda.synchronize()
                got = P.tensor_bits(out["rgba"]).reshape(-1, 4)
                assert np.array_equal(got, P.bits(want)), (bounces, variant, cull, entry, out["rgba"].reshape(-1, 4)[0])
                if variant == 0:
                    assert _counts(sc, bounces) == [[4 * w * h] * bounces]
    sc.close()


# ----------------------------------------------------------------------------- no table is the pass as it was
def test_no_table_is_the_pass_without_emission(rt, gpu):
    """Tables on all three kinds, a call that uploads them, then all three cleared: both entries give the bits, the
    queue lengths and the number of timed launches of a scene that never had a table; an all-zero table gives the same
    bits through the other instantiations."""
    import torch
    inp, w, h = mixed_scene(rt), 50, 30
    fresh, sc = P.scene(rt, inp), P.scene(rt, inp)
    for s in (fresh, sc):
        s.set_indirect_timing(True)
    frame = G1._frame(fresh, inp, w, h)
    _set_tables(sc, dict(sphere=_colours(inp.n, 8), plane=_colours(inp.n_planes, 1), cube=_colours(inp.n_cubes, 2)))
    lit = G2._paths(sc, inp, frame, bounces=2, rays=2)
    _set_tables(sc, {})
    assert sc.emission == {}
    for variant, cull in VARIANTS:
        for bounces, entry in ((1, "indirect"), (1, "paths"), (3, "paths")):
            kw = dict(rays=5, seed=4, cull=cull, variant=variant)
            a = _call(fresh, inp, frame, bounces, entry, **kw)
            ta, ca = fresh.indirect_paths_times(), _counts(fresh, bounces)
            b = _call(sc, inp, frame, bounces, entry, **kw)
            tb, cb = sc.indirect_paths_times(), _counts(sc, bounces)
            torch.cuda.synchronize()
            G1._same_outputs(a, b, (variant, cull, bounces, entry))
            assert len(ta) == len(tb) == (2 * (2 + bounces) if variant == 0 else 1) and ca == cb
    torch.cuda.synchronize()
    assert (P.tensor_bits(lit["rgba"]) != P.tensor_bits(G2._paths(fresh, inp, frame, bounces=2, rays=2)["rgba"])).any()
    fresh.close()
    sc.close()
    inp = Inputs(rt, 64)
    fresh, zero = inp.scene(), inp.scene()
    zero.set_emission("sphere", np.zeros((64, 3)))
    frame = G1._frame(fresh, inp, w, h)
    for variant, cull in VARIANTS:
        for bounces in (1, 3):
            kw = dict(rays=5, seed=4, cull=cull, variant=variant)
            a, b = _call(fresh, inp, frame, bounces, **kw), _call(zero, inp, frame, bounces, **kw)
            torch.cuda.synchronize()
            G1._same_outputs(a, b, ("zero", variant, cull, bounces))
            if variant == 0:
                assert _counts(fresh, bounces) == _counts(zero, bounces)
    fresh.close()
    zero.close()


# ----------------------------------------------------------------------------- an emitter lights a room
def room_inputs(rt):
    """Lights of colour 0 and a black sky; a closed room whose floor is plane 0 (y = -2), a sphere on the floor and a
    tall cube beside it that hides the whole sphere from a stretch of floor on its far side. Light reaches that floor
    by the walls and the ceiling alone: at the second bounce."""
    sky = [np.zeros((8, 16), dtype=np.float32)] * 3
    tex = [np.full((8, 8), 0.5, dtype=np.float32)] * 3
    pl = [(0, -2, 0, 0, 1, 0), (0, 8, 0, 0, -1, 0), (10, 0, 0, -1, 0, 0), (-10, 0, 0, 1, 0, 0), (0, 0, -8, 0, 0, 1),
          (0, 0, 14, 0, 0, -1)]
    return Scn(rt, [(-2.5, 0.5, 0, 1.6)], planes=pl, cubes=[(1, -2, -4, 2, 6, 4)], cam=P.cam(rt, 0, 5, 12, 180, 30), sky=sky,
               tex=tex, lights=[((20, 20, 20), 20, 0.0, 0.0, 0.0)])


def test_an_emitter_lights_a_room(rt, gpu):
    import torch
    inp, w, h = room_inputs(rt), 64, 36
    sc = inp.scene()
    frame = G1._frame(sc, inp, w, h)
    ids = frame["aov"]["id"].cpu().numpy().reshape(-1, 2)
    floor = (ids[:, 0] == E.PLANE) & (ids[:, 1] == 0)
    kw = dict(colour=None, rays=16, seed=6)
    for variant in (0, 1):                                              # without the table: exactly 0 everywhere
        for bounces in (1, 3):
            assert not G2._paths(sc, inp, frame, bounces=bounces, variant=variant, **kw)["rgba"][..., :3].any()
    tab = np.array([[4.0, 2.0, 1.0]], dtype=np.float32)
    sc.set_emission("sphere", tab)
    # the restatement names the pixels: floor pixels with a gather ray that meets the emitter, and floor pixels none of
    # whose 16 rays does
    inner = E.device_callables(sc)
    calls = E.emissive(inner[0], inner[1], E.tables(sphere=tab))
    one = G2._reference(sc, inp, frame, w, h, calls, colour=False, bounces=1, rays=16, seed=6)
    three = G2._reference(sc, inp, frame, w, h, calls, colour=False, bounces=3, rays=16, seed=6)
    idx = one[2]["idx"]
    sees = np.zeros(w * h, dtype=bool)
    sees[idx] = np.any([c.any(axis=1) for c in one[2]["colours"]], axis=0)
    below, hidden = floor & sees, floor & ~sees
    later = hidden & three[0][:, :3].any(axis=1)                        # a later hit of some path is the emitter
    assert below.sum() >= 100 and hidden.sum() >= 100 and later.sum() >= 100
    for variant in (0, 1):
        t1 = G2._paths(sc, inp, frame, bounces=1, variant=variant, **kw)["rgba"].cpu().numpy().reshape(-1, 4)[:, :3]
        t3 = G2._paths(sc, inp, frame, bounces=3, variant=variant, **kw)["rgba"].cpu().numpy().reshape(-1, 4)[:, :3]
        torch.cuda.synchronize()
        assert (t1[below] > 0).all()
        assert not t1[hidden].any()
        assert (t3[later] > 0).all() and (t3[below] >= t1[below]).all()
    sc.close()


# ----------------------------------------------------------------------------- hand-made guides
PLANE_TABLE = np.array([[0.25, 0.5, 1.0], [0, 0, 0], [0, 0, 0]], dtype=np.float32)     # plane 0 (A) emits


def _strip(npx):
    """70 pixels of every type in turn, a continuing path in the last."""
    t = np.array([PG.CONT, PG.STOP, PG.MISS, PG.DEAD] * ((npx + 3) // 4), dtype=np.int8)[:npx]
    t[npx - 1] = PG.CONT
    return t


def _run(rt, sc, inp, g, *, bounces, rays=1, variant=0, cull=1, in_place=False, entry="paths", stream=None):
    """test_indirect_paths_gpu._run with outputs pre-filled with NaN: the bits of rgba_out [m, 4] and of pixels [m]."""
    import torch
    w, h = g.width, g.height
    dev = G2._upload(g)
    out = dev["rgba_in"].clone() if in_place else torch.full((h * w, 4), NAN_FILL, dtype=torch.int32, device="cuda")
    packed = torch.full((h * w,), NAN_FILL, dtype=torch.int32, device="cuda")
    src = out if in_place else dev["rgba_in"]
    d = sc.indirect_desc(w, h, cam=inp.cam, aspect=IG.view_aspect(rt, w, h), depth=dev["depth"].data_ptr(),
                         normal=dev["normal"].data_ptr(), id=dev["id"].data_ptr(), albedo=dev["albedo"].data_ptr(),
                         rgba_in=src.data_ptr(), rgba_out=out.data_ptr(), pixels=packed.data_ptr(), rays=rays,
                         ray_base=PG.RAY_BASE, seed=PG.SEED, strength=0.75, cull=cull, variant=variant)
    rc = sc.indirect_paths_raw(d, sc.indirect_paths_opts(bounces)) if entry == "paths" else sc.indirect_raw(d)
    assert rc == 0, rt.load_library().rt_last_error()
    torch.cuda.synchronize()
    return P.tensor_bits(out).reshape(-1, 4), P.tensor_bits(packed).reshape(-1)


def _same_bits(got, want, what):
    (rgba, packed), (wr, wp) = got, want[:2]
    bad = (rgba != wr).any(axis=1)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8], rgba[bad][:2], wr[bad][:2])
    assert np.array_equal(packed, wp), what


@pytest.fixture(scope="module")
def world(rt, oracle, gpu):
    inp = PG.scene_inputs(rt)
    sc = inp.scene()
    sc.set_emission("plane", PLANE_TABLE)
    inner = G2._memo(R.castref_callables(Q.CastRef(oracle, inp)))
    yield SimpleNamespace(rt=rt, inp=inp, sc=sc, calls=E.emissive(inner[0], inner[1], E.tables(plane=PLANE_TABLE)))
    sc.close()


@pytest.mark.parametrize("w,h,name", PG.cases() + [(1, 70, "strip"), (70, 1, "strip")])
def test_wave_patterns_and_small_sizes(world, w, h, name):
    """Every mask of indirect_paths_guides (the only continuing lane 0 or 63, alternating lanes, tail waves, queues of
    1, 63, 65, 66 and 128 entries) and two strips, plane 0 emissive, at 1, 4 and 5 rays and one to three bounces: all
    bits against the restatement over the composed reference and the exact count per (group, bounce); outputs that held
    NaN are fully overwritten, and dead pixels carry rgba_in's bits, NaN payloads included."""
    W = world
    g = PG.guides(w, h, _strip(w * h)) if name == "strip" else PG.masked(w, h, name)
    for k, p in enumerate(np.nonzero(g.kinds == PG.DEAD)[0][:len(G2.DEAD_COLOURS)]):
        g.rgba_in[p] = G2.DEAD_COLOURS[k]
    dead = g.kinds == PG.DEAD
    for rays in (PG.RAYS if w * h <= 256 else (1, 5)):
        for bounces in (3, 2, 1):
            want = G2._want(W.rt, W.sc, W.inp, g, W.calls, bounces=bounces, rays=rays)
            if name != "strip":
                assert want[2]["counts"] == PG.counts(g.kinds, rays, bounces)
            stop = g.kinds == PG.STOP                                   # a STOP pixel's gather rays meet plane 0
            for variant in (0, 1):
                got = _run(W.rt, W.sc, W.inp, g, bounces=bounces, rays=rays, variant=variant)
                _same_bits(got, want, (name, rays, bounces, variant))
                if variant == 0:
                    assert _counts(W.sc, bounces) == want[2]["counts"], (name, rays, bounces)
                assert np.array_equal(got[0][dead], P.bits(g.rgba_in)[dead])
            if bounces == 1 and stop.any():                             # and the table shows in them
                W.sc.set_emission("plane", None)
                off = _run(W.rt, W.sc, W.inp, g, bounces=1, rays=rays)
                W.sc.set_emission("plane", PLANE_TABLE)
                assert (off[0][stop, :3] != got[0][stop, :3]).any(axis=1).all()
                assert np.array_equal(off[0][~stop], got[0][~stop])


def test_outputs_in_place_and_the_one_bounce_entry(world):
    W = world
    g = PG.masked(50, 30, "mixed")
    for bounces, entry in ((3, "paths"), (1, "indirect")):
        want = G2._want(W.rt, W.sc, W.inp, g, W.calls, bounces=bounces, rays=5)
        for variant in (0, 1):
            for cull in (1, 0):
                for in_place in (False, True):
                    got = _run(W.rt, W.sc, W.inp, g, bounces=bounces, rays=5, variant=variant, cull=cull,
                               in_place=in_place, entry=entry)
                    _same_bits(got, want, (entry, variant, cull, in_place))


# ----------------------------------------------------------------------------- state
def test_a_long_lived_scene_equals_fresh_scenes(rt, gpu):
    """Ten steps and more on two streams: tables set, changed and cleared per kind, both entries in turn, one to four
    bounces, rays across the group limit, two sizes, a sphere list set again with the same count (the table stays) and
    with another (the table is cleared) -- every output against a fresh scene built from the current state."""
    import torch
    inp = mixed_scene(rt)
    sc = P.scene(rt, inp)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cur, step = {}, [0]

    def put(kind, tab):
        sc.set_emission(kind, tab)
        cur[kind] = tab

    def check(what, w=50, h=30, bounces=None, **kw):
        st = streams[step[0] % 2]
        step[0] += 1
        frame = G1._frame(sc, inp, w, h, stream=st)
        fresh = P.scene(rt, inp)
        _set_tables(fresh, cur)
        f2 = G1._frame(fresh, inp, w, h)
        if bounces is None:
            got = sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, want_packed=True, stream=st, **kw)
            want = G1._call(fresh, inp, f2, **kw)
        else:
            got = sc.indirect_paths(frame, cam=inp.cam, aspect=inp.aspect, want_packed=True, stream=st, bounces=bounces, **kw)
            want = G2._paths(fresh, inp, f2, bounces=bounces, **kw)
        torch.cuda.synchronize()
        G1._same_outputs(got, want, what)
        assert set(sc.emission) == {E.KINDS[k] for k, v in cur.items() if v is not None}, what
        fresh.close()
        return got

    put("sphere", _colours(inp.n, 8, seed=1))
    a = check("a sphere table", rays=2)
    put("sphere", _colours(inp.n, 8, seed=2))
    b = check("another sphere table", rays=2)
    assert (P.tensor_bits(a["rgba"]) != P.tensor_bits(b["rgba"])).any()
    put("plane", _colours(inp.n_planes, 1))
    put("cube", _colours(inp.n_cubes, 2))
    check("all three kinds, across the group limit, a larger size", w=120, h=70, bounces=3, rays=5)
    put("sphere", None)
    check("the sphere table cleared", rays=3)
    put("sphere", _colours(inp.n, 4, seed=3))
    P.move_spheres(inp, {3: (0.5, 0.2, -0.3), 10: (-0.4, 0.1, 0.2)})
    sc.set_spheres(inp.spheres, inp.n)                                  # the same count: the table stays
    check("after set_spheres with the same count", bounces=4, rays=2)
    inp.n = 150
    sc.set_spheres(inp.spheres, inp.n)                                  # another count: the table is cleared
    cur["sphere"] = None
    with pytest.raises(rt.RtError, match="200 colours for 150 spheres"):
        sc.set_emission("sphere", _colours(200, 4))
    check("after set_spheres with another count", bounces=2, rays=4)
    put("plane", None)
    check("the plane table cleared", rays=9)
    put("cube", None)
    c = check("no table at all", bounces=3, rays=2)
    put("cube", _colours(inp.n_cubes, 1, seed=4))
    d = check("the yardstick over the whole lists", bounces=3, rays=2, cull=False, variant=1)
    assert (P.tensor_bits(c["rgba"]) != P.tensor_bits(d["rgba"])).any()
    put("sphere", _colours(inp.n, 8, seed=5))
    check("a table for the shorter list, sixteen rays", rays=16)
    check("four bounces at the larger size", w=120, h=70, bounces=4, rays=6)
    sc.close()


def test_a_capturing_stream_is_refused_with_nothing_written(rt, gpu):
    import torch
    lib = rt.load_library()
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    sc.set_emission("sphere", _colours(64, 4))
    frame = G1._frame(sc, inp, w, h)
    out, packed = G1._poisoned(w, h)
    o = sc.indirect_paths_opts(3)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = sc.indirect_paths_raw(G1._raw(sc, inp, frame, out, packed, rays=2), o, s.cuda_stream)
        rc1 = sc.indirect_raw(G1._raw(sc, inp, frame, out, packed, rays=2), s.cuda_stream)
    assert rc == 2 and rc1 == 2 and "captured" in lib.rt_last_error().decode()
    torch.cuda.synchronize()
    assert (out == G1.POISON).all() and (packed == G1.POISON).all()
    assert sc.indirect_paths_raw(G1._raw(sc, inp, frame, out, packed, rays=2), o) == 0      # and the scene still works
    torch.cuda.synchronize()
    assert not (out == G1.POISON).any()
    want = G2._paths(sc, inp, frame, bounces=3, rays=2)
    assert np.array_equal(P.tensor_bits(out).reshape(-1), P.tensor_bits(want["rgba"]).reshape(-1))
    sc.close()


# ----------------------------------------------------------------------------- what the primary ray sees
def test_emission_term_of_a_rendered_frame(rt, gpu):
    import torch
    inp, mesh, w, h = mixed_scene(rt), meshes.uv_sphere_obj(), 160, 90
    sc = P.scene(rt, inp, mesh)
    tabs = dict(sphere=_colours(inp.n, 2), plane=_colours(inp.n_planes, 1))     # the cubes have no table
    _set_tables(sc, tabs)
    frame = G1._frame(sc, inp, w, h)
    term = sc.emission_term(frame)
    assert term.dtype == torch.float32 and tuple(term.shape) == (h, w, 4) and term.device == frame["aov"]["id"].device
    ids = frame["aov"]["id"].cpu().numpy()
    assert {0, 1, 2, 3} <= set(ids[..., 0].reshape(-1).tolist())          # (kind -1: the CPU test)
    want = E.term_lookup(E.tables(**tabs), ids)
    assert np.array_equal(P.tensor_bits(term), P.bits(want))
    assert want[ids[..., 0] == E.SPHERE].any() and want[ids[..., 0] == E.PLANE].any()
    assert not want[(ids[..., 0] <= 0) | (ids[..., 0] == E.CUBE)].any() and not want[..., 3].any()
    out = frame["rgba"] + term                                          # the pipeline's last line
    assert np.array_equal(P.tensor_bits(out[..., 3]), P.tensor_bits(frame["rgba"][..., 3]))
    sc.close()
