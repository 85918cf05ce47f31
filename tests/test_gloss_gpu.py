"""Glossy reflections on the device (rt_scene_set_roughness, rt_scene_set_gloss_seed): parity with the
composed reference of tests/gloss_ref.py for one sample and many, the whole scene, glass, bands and seeds; the identities
with the mirror frame; a long-lived scene against fresh ones; the refusals. Every comparison is bit for bit: rgba with
its .w, the packed words and the queue lengths. The conditions a case is chosen for -- perturbed continuations, the
halved fourth draw, a rejected R' -- are asserted from the reference's trace before the device frame is looked at."""
import ctypes as C
import functools

import numpy as np
import pytest

import gloss_ref as G
from scenes import Inputs, Scn
from test_gloss_cpu import check_count_rules, check_table_rules

pytestmark = pytest.mark.gpu

W1, H1, N1, D1 = 96, 54, 256, 3
W2, H2, D2 = 50, 30, 2                    # 1 500 pixels, a multiple of neither 64 nor 256
K_TABLE = (0.0, 0.25, 0.5, 1.0)
RHO_TABLE = (0.0, 0.05, 0.3, 1.0)


def _k(n):
    return np.array([K_TABLE[i % 4] for i in range(n)], dtype=np.float32)


def _rho(n):
    """Every pair of K_TABLE x RHO_TABLE occurs."""
    return np.array([RHO_TABLE[(i // 4) % 4] for i in range(n)], dtype=np.float32)


def _render(scene, w, h, **kw):
    """(packed, rgba, queue) of a frame into fresh buffers."""
    import torch
    out = scene.render(w, h, **kw)
    torch.cuda.synchronize()
    queue = scene.reflect_stats()["queue"] if kw.get("reflect_depth", 0) > 0 else None
    return out["packed"].cpu().numpy().view(np.uint32), out["rgba"].cpu().numpy(), queue


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _check(got, ref, what=""):
    """A device frame (packed, rgba, queue) against a reference (rgba, packed, queue)."""
    bad = int((got[1].view(np.uint32) != ref[0].view(np.uint32)).any(axis=2).sum())
    assert bad == 0, (what, "rgba", bad)
    assert np.array_equal(got[0], ref[1]), (what, "packed")
    assert got[2] == list(ref[2]), (what, got[2], ref[2])


def _queue(trace, depth):
    return ([t["index"].shape[0] for t in trace[1:]] + [0] * depth)[:depth]


def _enough(trace, what=""):
    assert G.count(trace) >= 50, (what, G.count(trace))


def _mirrors(rt, rho=None, seed=None):
    sc = Inputs(rt, N1).scene()
    sc.set_materials(_k(N1))
    if rho is not None:
        sc.set_roughness("sphere", rho)
    if seed is not None:
        sc.set_gloss_seed(seed)
    return sc


# ----------------------------------------------------------------------------- the shared references
@functools.lru_cache(maxsize=None)
def _ref_one(rt, oracle, seed=0, y0=0, y1=H1):
    """The one-sample glossy frame of the mirrors: ((rgba, packed, queue), gloss trace)."""
    comp = G.gloss_composer_for(oracle, rt, Inputs(rt, N1)).set_gloss(sphere=_rho(N1), seed=seed)
    rgba, packed = comp.render(W1, H1, _k(N1), D1, y0=y0, y1=y1)
    return (rgba, packed, _queue(comp.trace, D1)), comp.gloss_trace


@functools.lru_cache(maxsize=None)
def _ref_many(rt, oracle, spp):
    comp = G.gloss_composer_for(oracle, rt, Inputs(rt, N1)).set_gloss(sphere=_rho(N1), seed=3)
    ref = G.GlossSampleRef(rt, comp).render(W2, H2, D2, spp=spp, k=_k(N1))
    return (ref["rgba"], ref["packed"], ref["queue"]), [t for s in ref["samples"] for t in s["gloss"]]


@functools.lru_cache(maxsize=None)
def _scene_case(rt, oracle):
    """The staged scene of tests/test_reflect_scene_gpu.py with a rough mirror floor (rho = 1: the camera looks along it,
    so that many R' dip below it), a rough mirror slab and a slightly rough mirror sphere."""
    from test_reflect_scene_gpu import MIRROR, _stage
    inp, mesh, mats = _stage(rt, oracle)
    rough = {"sphere": np.zeros(inp.n, dtype=np.float32), "plane": np.array([1.0], dtype=np.float32),
             "cube": np.array([0.3, 0.5], dtype=np.float32)}           # (cube 1 has k = 0: its roughness is idle)
    rough["sphere"][MIRROR] = 0.1
    return inp, mesh, mats, rough


@functools.lru_cache(maxsize=None)
def _ref_scene(rt, oracle):
    W, H, depth = 64, 48, 3
    inp, mesh, mats, rough = _scene_case(rt, oracle)
    comp = G.GlossSceneComposer(oracle, rt, inp, mesh).set_gloss(seed=11, **rough)
    return comp.render(W, H, depth, **mats), comp.gloss_trace, comp.trace


def _glass_mats(n):
    tau = np.array([0.8 if i % 4 == 2 else 0.0 for i in range(n)], dtype=np.float32)
    ior = np.where(tau > 0, 1.5, 0.0).astype(np.float32)
    k = np.where(tau > 0, 0.0, _k(n)).astype(np.float32)
    return k, tau, ior


@functools.lru_cache(maxsize=None)
def _ref_glass(rt, oracle):
    W, H, n, depth = 64, 36, 128, 3
    k, tau, ior = _glass_mats(n)
    rho = np.full(n, 0.3, dtype=np.float32)                               # the glass spheres included
    comp = G.gloss_composer_for(oracle, rt, Inputs(rt, n), glass=True).set_gloss(sphere=rho, seed=5)
    rgba, packed = comp.render(W, H, k, depth, tau=tau, ior=ior)
    queue = ([t["pix"].shape[0] for t in comp.trace[1:]] + [0] * depth)[:depth]
    return (rgba, packed, queue), comp.gloss_trace, comp.trace


# ----------------------------------------------------------------------------- 1. one sample
def test_one_sample_against_the_reference(rt, oracle, gpu):
    ref, trace = _ref_one(rt, oracle)
    _enough(trace)
    assert {float(r) for t in trace for r in t["rho"]} == {float(np.float32(v)) for v in RHO_TABLE}
    assert {t["b"] for t in trace if (t["what"] != 0).any()} == {0, 1, 2}     # the primary hit and both bounces that go on
    assert ref[2][2] > 0
    sc = _mirrors(rt, _rho(N1))
    _check(_render(sc, W1, H1, reflect_depth=D1), ref, "culled")
    _check(_render(sc, W1, H1, reflect_depth=D1, cull=False), ref, "whole list")
    sc.set_reflect_samples("many")                                           # one sample under MANY: s = 0 as well
    _check(_render(sc, W1, H1, reflect_depth=D1), ref, "many")


# ----------------------------------------------------------------------------- 2. many samples
def test_five_samples_cross_the_group_boundary(rt, oracle, gpu):
    ref, trace = _ref_many(rt, oracle, 5)
    _enough(trace)
    sc = _mirrors(rt, _rho(N1), seed=3)
    sc.set_reflect_samples("many")
    _check(_render(sc, W2, H2, reflect_depth=D2, spp=5), ref, "culled")
    _check(_render(sc, W2, H2, reflect_depth=D2, spp=5, cull=False), ref, "whole list")


def test_three_samples_in_one_call_equal_one_by_one(rt, oracle, gpu):
    import torch
    ref, trace = _ref_many(rt, oracle, 3)
    _enough(trace)
    sc = _mirrors(rt, _rho(N1), seed=3)
    sc.set_reflect_samples("many")
    single = _render(sc, W2, H2, reflect_depth=D2, spp=3)
    _check(single, ref, "single")
    packed = torch.full((H2, W2), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rgba = torch.full((H2, W2, 4), 3.0, dtype=torch.float32, device="cuda")
    queue = [0] * D2
    for k in range(3):
        fd = sc.frame_desc(W2, H2, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=D2, spp=1, sample_base=k,
                           sample_total=3, accumulate=k > 0, resolve=0 if k == 2 else -1)
        sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        queue = [a + b for a, b in zip(queue, sc.reflect_stats()["queue"])]
    prog = (packed.cpu().numpy().view(np.uint32), rgba.cpu().numpy(), queue)
    assert _same(prog, single) and prog[2] == single[2]
    # and the samples differ from one another in their draws: sample 1 alone is not sample 0 alone
    a = _render(sc, W2, H2, reflect_depth=D2, spp=1, sample_base=0, sample_total=3, resolve=-1)
    b = _render(sc, W2, H2, reflect_depth=D2, spp=1, sample_base=1, sample_total=3, resolve=-1)
    assert not np.array_equal(a[1], b[1])


# ----------------------------------------------------------------------------- 3. the whole scene
def test_whole_scene_against_the_reference(rt, oracle, gpu):
    from reflect_scene_ref import CUBE, PLANE, SPHERE
    from test_reflect_scene_gpu import _scene
    ref, trace, walk = _ref_scene(rt, oracle)
    _enough(trace)
    assert G.count(trace, G.REJECTED) >= 5                                   # R' below the grazing floor
    by_rho = {float(r) for t in trace for r in t["rho"][t["what"] != 0]}
    assert by_rho == {float(np.float32(0.1)), float(np.float32(0.3)), 1.0}   # the sphere, the slab and the floor
    inp, mesh, mats, rough = _scene_case(rt, oracle)
    sc = _scene(rt, inp, mesh, mats)
    for kind, v in rough.items():
        sc.set_roughness(kind, v)
    sc.set_gloss_seed(11)
    _check(_render(sc, 64, 48, reflect_depth=3), ref, "culled")
    _check(_render(sc, 64, 48, reflect_depth=3, cull=False), ref, "whole list")


# ----------------------------------------------------------------------------- 4. glass
def test_a_rough_mirror_behind_glass(rt, oracle, gpu):
    ref, trace, walk = _ref_glass(rt, oracle)
    _enough(trace)
    # rays that passed through a glass sphere (rule 4) at bounce b - 1 and were perturbed at a mirror at bounce b
    seen = 0
    for t in trace:
        if t["b"] == 0:
            continue
        before = walk[t["b"] - 1]
        through = before["pix"][before["rule"] == 4]
        seen += int(np.isin(t["pix"][(t["what"] & G.PERTURBED) != 0], through).sum())
    assert seen >= 10, seen
    W, H, n, depth = 64, 36, 128, 3
    k, tau, ior = _glass_mats(n)
    sc = Inputs(rt, n).scene()
    sc.set_materials_ex(k, tau, ior)
    sc.set_roughness("sphere", np.full(n, 0.3, dtype=np.float32))
    sc.set_gloss_seed(5)
    got = _render(sc, W, H, reflect_depth=depth)
    _check(got, ref, "culled")
    _check(_render(sc, W, H, reflect_depth=depth, cull=False), ref, "whole list")
    # roughness on the glass spheres themselves changes nothing
    sc.set_roughness("sphere", np.where(tau > 0, 0.0, 0.3).astype(np.float32))
    assert _same(_render(sc, W, H, reflect_depth=depth), got)
    sc.set_roughness("sphere", np.where(tau > 0, 1.0, 0.3).astype(np.float32))
    assert _same(_render(sc, W, H, reflect_depth=depth), got)


# ----------------------------------------------------------------------------- 5. bands
def test_bands_equal_the_full_frame(rt, oracle, gpu):
    """The key takes the row of the full frame: a band that counted its rows from y0 would draw row 27 as row 0."""
    ref, trace = _ref_one(rt, oracle)
    lower = np.concatenate([t["pix"][(t["what"] & G.PERTURBED) != 0] for t in trace]) >= 27 * W1
    assert int(lower.sum()) >= 50                                            # perturbed pixels in the second band
    sc = _mirrors(rt, _rho(N1))
    full = _render(sc, W1, H1, reflect_depth=D1)
    _check(full, ref)
    queue = [0] * D1
    for y0, y1 in ((0, 27), (27, 54)):
        band = _render(sc, W1, H1, reflect_depth=D1, y0=y0, y1=y1)
        assert _same(band, (full[0][y0:y1], full[1][y0:y1])), (y0, y1)
        queue = [a + b for a, b in zip(queue, band[2])]
    assert queue == full[2]
    band_ref, _ = _ref_one(rt, oracle, 0, 27, 54)                            # the reference agrees about the band
    assert np.array_equal(band_ref[0].view(np.uint32), ref[0][27:54].view(np.uint32))
    sc.set_reflect_samples("many")
    full = _render(sc, W1, H1, reflect_depth=D1, spp=2)
    for y0, y1 in ((0, 27), (27, 54)):
        assert _same(_render(sc, W1, H1, reflect_depth=D1, spp=2, y0=y0, y1=y1), (full[0][y0:y1], full[1][y0:y1])), (y0, y1)


# ----------------------------------------------------------------------------- 6. the seed
def test_a_seed_changes_the_perturbed_pixels_only(rt, oracle, gpu):
    ref0, trace0 = _ref_one(rt, oracle)
    ref7, trace7 = _ref_one(rt, oracle, 7)
    _enough(trace7)
    touched = G.perturbed_pixels(trace0, W1 * H1).reshape(H1, W1)
    assert np.array_equal(touched, G.perturbed_pixels(trace7, W1 * H1).reshape(H1, W1))   # the first perturbed hit is the same
    assert 50 <= int(touched.sum()) < W1 * H1 - 50
    sc = _mirrors(rt, _rho(N1))
    a = _render(sc, W1, H1, reflect_depth=D1)
    sc.set_gloss_seed(7)
    b = _render(sc, W1, H1, reflect_depth=D1)
    _check(a, ref0, "seed 0")
    _check(b, ref7, "seed 7")
    changed = (a[1].view(np.uint32) != b[1].view(np.uint32)).any(axis=2)
    assert int(changed.sum()) >= 50
    assert not (changed & ~touched).any()
    sc.set_gloss_seed(0)
    assert _same(_render(sc, W1, H1, reflect_depth=D1), a)


# ----------------------------------------------------------------------------- 7. identities
def test_identities_with_the_mirror_frame(rt, oracle, gpu):
    _, trace = _ref_one(rt, oracle)
    _enough(trace)
    sc = _mirrors(rt)
    mirror = _render(sc, W1, H1, reflect_depth=D1)
    assert mirror[2][0] > 0
    sc.set_gloss_seed(9)                                                     # a seed alone draws nothing
    assert _same(_render(sc, W1, H1, reflect_depth=D1), mirror)
    sc.set_roughness("sphere", np.zeros(N1, dtype=np.float32))               # an all-zero table is no table
    assert _same(_render(sc, W1, H1, reflect_depth=D1), mirror)
    sc.set_roughness("sphere", np.where(_k(N1) == 0, 0.7, 0.0))              # roughness where nothing is reflected
    assert _same(_render(sc, W1, H1, reflect_depth=D1), mirror)
    sc.set_roughness("sphere", _rho(N1))
    glossy = _render(sc, W1, H1, reflect_depth=D1)
    assert not _same(glossy, mirror) and glossy[2][0] == mirror[2][0]
    plain = _render(sc, W1, H1)                                              # depth 0 reads no table
    sc.set_roughness("sphere", None)
    assert _same(_render(sc, W1, H1, reflect_depth=D1), mirror)
    assert _same(_render(sc, W1, H1), plain)
    sc.set_roughness("sphere", _rho(N1))                                     # and set again it is the glossy frame again
    assert _same(_render(sc, W1, H1, reflect_depth=D1), glossy)


def test_the_halved_draw_and_the_rejection_happen(rt, oracle):
    """Across the file's references (asserted from their traces alone)."""
    traces = [_ref_one(rt, oracle)[1], _ref_many(rt, oracle, 5)[1], _ref_scene(rt, oracle)[1], _ref_glass(rt, oracle)[1]]
    assert sum(G.count(t, G.HALVED) for t in traces) >= 5
    assert sum(G.count(t, G.REJECTED) for t in traces) >= 5
    for t in traces:
        _enough(t)


# ----------------------------------------------------------------------------- 8. a long-lived scene
def _state_scn(rt, n_s, n_p, n_c):
    """In front of the default camera (at (4, 3, 10), looking down along -z): spheres of radius 0.72 over a floor, a back
    and a side wall, cubes in the foreground."""
    spheres = [(1.0 + 2.0 * (i % 4), 0.75 + 1.6 * (i // 4), 0.5 - 1.0 * (i % 3), 0.85) for i in range(n_s)]
    planes = [(0, 0, 0, 0, 1, 0), (0, 0, -6, 0, 0, 1), (-2, 0, 0, 1, 0, 0)][:n_p]
    cubes = [(0.5 + 3.5 * i, 0, 3.0, 2.0 + 3.5 * i, 1.0, 4.5) for i in range(n_c)]
    return Scn(rt, spheres, planes=planes, cubes=cubes)


def test_a_long_lived_scene_against_fresh_ones(rt, gpu):
    """Set, change and clear the three tables and the seed, with the counts of all three lists changing in between, on
    two streams; after every step the long-lived scene renders what a scene built from scratch renders."""
    import torch
    W, H, depth = 48, 27, 3
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    st = {"n": {"sphere": 8, "plane": 2, "cube": 2}, "rough": {"sphere": None, "plane": None, "cube": None}, "seed": 0}
    k_of = lambda n: np.array([(1.0, 0.5, 0.0)[i % 3] for i in range(n)], dtype=np.float32)
    rho_of = lambda n, a: np.array([(a, 0.0, 1.0, 0.3)[i % 4] for i in range(n)], dtype=np.float32)

    def apply_lists(sc, scn, fresh):
        if fresh or sc.n_spheres != scn.n:
            sc.set_spheres(scn.spheres, scn.n)
        if fresh or sc.n_planes != scn.n_planes:
            sc.set_planes(scn.planes, scn.n_planes)
        if fresh or sc.n_cubes != scn.n_cubes:
            sc.set_cubes(scn.cubes, scn.n_cubes)

    def materials(sc):
        sc.set_materials(k_of(st["n"]["sphere"]))
        sc.set_plane_materials(k_of(st["n"]["plane"]))
        sc.set_cube_materials(k_of(st["n"]["cube"]))

    def build():
        scn = _state_scn(rt, st["n"]["sphere"], st["n"]["plane"], st["n"]["cube"])
        sc = scn.scene()
        sc.set_reflect_scope("scene")
        materials(sc)
        for kind, v in st["rough"].items():
            sc.set_roughness(kind, v)
        sc.set_gloss_seed(st["seed"])
        return sc

    live = build()

    def rough(kind, a):
        def step():
            st["rough"][kind] = None if a is None else rho_of(st["n"][kind], a)
            live.set_roughness(kind, st["rough"][kind])
        return step

    def seed(v):
        def step():
            st["seed"] = v
            live.set_gloss_seed(v)
        return step

    def count(kind, n, same=False):
        def step():
            st["n"][kind] = n
            if not same:
                st["rough"][kind] = None                  # a new count clears the kind's table (and its materials)
            scn = _state_scn(rt, st["n"]["sphere"], st["n"]["plane"], st["n"]["cube"])
            {"sphere": lambda: live.set_spheres(scn.spheres, scn.n), "plane": lambda: live.set_planes(scn.planes, scn.n_planes),
             "cube": lambda: live.set_cubes(scn.cubes, scn.n_cubes)}[kind]()
            materials(live)
        return step

    steps = [("nothing set", lambda: None), ("sphere table", rough("sphere", 0.2)), ("seed", seed(5)),
             ("plane table", rough("plane", 1.0)), ("cube table", rough("cube", 0.4)),
             ("spheres, same count", count("sphere", 8, same=True)), ("sphere table changed", rough("sphere", 0.6)),
             ("sphere count", count("sphere", 11)), ("sphere table again", rough("sphere", 0.2)),
             ("planes, same count", count("plane", 2, same=True)), ("plane count", count("plane", 3)),
             ("plane table again", rough("plane", 0.5)), ("cube count", count("cube", 1)), ("seed back", seed(0)),
             ("cube table again", rough("cube", 1.0)), ("cubes, same count", count("cube", 1, same=True)),
             ("sphere table cleared", rough("sphere", None)), ("plane table cleared", rough("plane", None)),
             ("cube table cleared", rough("cube", None)), ("all three", lambda: [rough(k, 0.3)() for k in st["rough"]]),
             ("sphere count back", count("sphere", 8))]
    differ = 0
    prev = None
    for i, (name, step) in enumerate(steps):
        step()
        with torch.cuda.stream(streams[i % 2]):
            got = _render(live, W, H, reflect_depth=depth, stream=streams[i % 2])
            want = _render(build(), W, H, reflect_depth=depth, stream=streams[(i + 1) % 2])
        assert got[2] == want[2] and got[2][0] > 0, name
        assert _same(got, want), name
        differ += prev is not None and not _same(got, prev)
        prev = got
    assert differ >= 8, differ                             # the steps are visible: 16 of them are meant to change the frame


# ----------------------------------------------------------------------------- 9. the table rules, with lists that exist
@pytest.mark.parametrize("kind", ["sphere", "plane", "cube"])
def test_table_rules_on_a_device(rt, gpu, kind):
    sc = _state_scn(rt, 8, 2, 2).scene()
    n = {"sphere": 8, "plane": 2, "cube": 2}[kind]
    check_table_rules(rt, sc, kind, n)
    check_count_rules(rt, sc, kind)


# ----------------------------------------------------------------------------- 10. refusals
def _refused(sc, lib, w, h, code=2, **kw):
    import torch
    packed = torch.full((h, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rgba = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), **kw)
    rc = lib.rt_scene_render(sc.handle, C.byref(fd), None)
    torch.cuda.synchronize()
    return rc == code and bool((packed == 0x5a5a5a5a).all()) and bool((rgba == 3.0).all())


def test_refusals_write_nothing(rt, gpu):
    """What a reflective frame refuses, it refuses with roughness set as well, and writes nothing."""
    import torch
    lib = rt.load_library()
    w, h = 64, 64
    sc = Inputs(rt, 64).scene()
    sc.set_materials([0.5] * 64)
    sc.set_roughness("sphere", [0.4] * 64)
    sc.set_gloss_seed(2)
    assert not _refused(sc, lib, w, h, reflect_depth=2)                       # the frame itself renders
    for kw in (dict(spp=4), dict(accumulate=True), dict(sample_base=1, sample_total=4)):   # the default sampling mode
        assert _refused(sc, lib, w, h, reflect_depth=2, **kw), kw
    sc.set_reflect_samples("many")
    for kw in (dict(interleave=(2, 0, 16)), dict(table_lds=True), dict(profile=True)):
        assert _refused(sc, lib, w, h, reflect_depth=2, spp=4, **kw), kw
    assert _refused(sc, lib, w, h, code=1, reflect_depth=2, spp=17)
    packed = torch.full((h, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rgba = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=2)
    assert not lib.rt_graph_capture(sc.handle, C.byref(fd), 1, None, None)
    assert b"reflect" in lib.rt_last_error()
    dev = (C.c_int * 1)(0)
    m = C.c_void_p()
    assert lib.rt_multi_create_ex(dev, 1, 2, C.byref(m)) == 0, lib.rt_last_error()
    try:
        assert lib.rt_multi_render(m, C.byref(fd), packed.data_ptr()) == 2
        assert lib.rt_multi_sync(m) == 0
        torch.cuda.synchronize()
        assert bool((packed == 0x5a5a5a5a).all()) and bool((rgba == 3.0).all())
    finally:
        lib.rt_multi_destroy(m)
    # a plane in the scene under the spheres-only scope, with a plane table set
    scn = _state_scn(rt, 8, 1, 0)
    sp = scn.scene()
    sp.set_materials([0.5] * 8)
    sp.set_roughness("plane", [1.0])
    sp.set_roughness("sphere", [0.4] * 8)
    assert _refused(sp, lib, w, h, reflect_depth=2)
    sp.set_reflect_scope("scene")
    assert not _refused(sp, lib, w, h, reflect_depth=2)
    # a refused table changes nothing: the frame after it is the frame before it
    before = _render(sc, w, h, reflect_depth=2)
    with pytest.raises(rt.RtError):
        sc.set_roughness("sphere", [0.9] * 63 + [1.5])
    with pytest.raises(rt.RtError):
        sc.set_roughness("sphere", [0.9] * 63)
    assert _same(_render(sc, w, h, reflect_depth=2), before)
