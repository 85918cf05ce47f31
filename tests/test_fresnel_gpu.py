"""Fresnel glass on the device (rt_scene_set_glass_model): parity with the composed reference of
tests/fresnel_ref.py for one sample and many, frosted glass, the whole scene, bands and seeds; the identities with the
plain model; a long-lived scene against fresh ones; the refusals. Every comparison is bit for bit: rgba with its .w, the
packed words and the queue lengths. The conditions a case is chosen for -- reflect and transmit choices at every
bounce, perturbed exits and perturbed glass reflections -- are asserted from the reference's trace before the device
frame is looked at."""
import ctypes as C
import functools

import numpy as np
import pytest

import fresnel_ref as FR
import gloss_ref as G
from scenes import Inputs
from test_fresnel_cpu import K_TABLE, check_model_rules, glass_mats

pytestmark = pytest.mark.gpu

W1, H1, N1, D1 = 96, 54, 256, 3
W2, H2, D2 = 50, 30, 2                    # 1 500 pixels, a multiple of neither 64 nor 256
SEED = 1


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
    return ([t["pix"].shape[0] for t in trace[1:]] + [0] * depth)[:depth]


def _glass(rt, n=N1, model="fresnel", rho=None, seed=None):
    sc = Inputs(rt, n).scene()
    sc.set_materials_ex(*glass_mats(n))
    sc.set_glass_model(model)
    if rho is not None:
        sc.set_roughness("sphere", rho)
    if seed is not None:
        sc.set_gloss_seed(seed)
    return sc


# ----------------------------------------------------------------------------- the shared references
@functools.lru_cache(maxsize=None)
def _ref_base(rt, oracle, seed=SEED, rho=0.0, y0=0, y1=H1, model=FR.FRESNEL):
    """The base scene's frame: ((rgba, packed, queue), Fresnel trace, gloss trace)."""
    k, tau, ior = glass_mats(N1)
    table = np.full(N1, rho, dtype=np.float32) if rho > 0 else None
    comp = FR.fresnel_composer_for(oracle, rt, Inputs(rt, N1)).set_gloss(sphere=table, seed=seed).set_glass_model(model)
    rgba, packed = comp.render(W1, H1, k, D1, y0=y0, y1=y1, tau=tau, ior=ior)
    return (rgba, packed, _queue(comp.trace, D1)), comp.fresnel_trace, comp.gloss_trace


@functools.lru_cache(maxsize=None)
def _ref_many(rt, oracle, spp):
    k, tau, ior = glass_mats(N1)
    comp = FR.fresnel_composer_for(oracle, rt, Inputs(rt, N1)).set_gloss(seed=3).set_glass_model()
    ref = FR.FresnelSampleRef(rt, comp).render(W2, H2, D2, spp=spp, k=k, tau=tau, ior=ior)
    return (ref["rgba"], ref["packed"], ref["queue"]), [s["fresnel"] for s in ref["samples"]]


def _enough(trace, what=""):
    """The conditions of the base scene: reflect choices at every bounce that continues, and many transmit choices."""
    assert FR.count(trace, FR.REFLECTED) >= 30, (what, FR.count(trace, FR.REFLECTED))
    for b in range(D1):
        assert FR.count(trace, FR.REFLECTED, b=b) >= 3, (what, b, FR.count(trace, FR.REFLECTED, b=b))
    assert FR.count(trace, FR.THROUGH) >= 200, (what, FR.count(trace, FR.THROUGH))


# ----------------------------------------------------------------------------- 1. the base scene
def test_base_scene_against_the_reference(rt, oracle, gpu):
    ref, trace, _ = _ref_base(rt, oracle)
    _enough(trace)
    k, tau, ior = glass_mats(N1)
    hit_iors = {float(v) for v in ior[tau > 0]}
    assert hit_iors == {1.5, float(np.float32(2.4))}
    assert ref[2][2] > 0
    sc = _glass(rt, seed=SEED)
    _check(_render(sc, W1, H1, reflect_depth=D1), ref, "culled")
    _check(_render(sc, W1, H1, reflect_depth=D1, cull=False), ref, "whole list")
    sc.set_reflect_samples("many")                                           # one sample under MANY: s = 0 as well
    _check(_render(sc, W1, H1, reflect_depth=D1), ref, "many")


# ----------------------------------------------------------------------------- 2. frosted glass
def test_frosted_glass(rt, oracle, gpu):
    ref, trace, gloss = _ref_base(rt, oracle, SEED, 0.3)
    _enough(trace, "frosted")
    assert FR.count_perturbed(trace, FR.THROUGH) >= 20, FR.count_perturbed(trace, FR.THROUGH)          # step 5
    assert FR.count_perturbed(trace, FR.REFLECTED) >= 20, FR.count_perturbed(trace, FR.REFLECTED)      # step 4
    assert G.count(gloss) >= 50                                              # and the mirrors are rough as well
    sc = _glass(rt, rho=np.full(N1, 0.3, dtype=np.float32), seed=SEED)
    got = _render(sc, W1, H1, reflect_depth=D1)
    _check(got, ref, "culled")
    _check(_render(sc, W1, H1, reflect_depth=D1, cull=False), ref, "whole list")
    clear = _ref_base(rt, oracle)[0]
    assert not np.array_equal(ref[0].view(np.uint32), clear[0].view(np.uint32))


# ----------------------------------------------------------------------------- 3. samples
def _enough_many(traces, what=""):
    refl = sum(FR.count(t, FR.REFLECTED, depth=D2) for t in traces)
    thru = sum(FR.count(t, FR.THROUGH, depth=D2) for t in traces)
    assert refl >= 30 and thru >= 200, (what, refl, thru)
    assert all(FR.count(t, FR.REFLECTED, depth=D2) >= 3 for t in traces), what      # in every sample


def test_five_samples_cross_the_group_boundary(rt, oracle, gpu):
    ref, traces = _ref_many(rt, oracle, 5)
    _enough_many(traces)
    # the samples draw differently: some pixel is reflected in one sample and not in another
    r = np.stack([FR.reflected_pixels(t, W2 * H2, depth=D2) for t in traces])
    assert int((r.any(axis=0) & ~r.all(axis=0)).sum()) >= 10
    sc = _glass(rt, seed=3)
    sc.set_reflect_samples("many")
    _check(_render(sc, W2, H2, reflect_depth=D2, spp=5), ref, "culled")
    _check(_render(sc, W2, H2, reflect_depth=D2, spp=5, cull=False), ref, "whole list")


def test_three_samples_in_one_call_equal_one_by_one(rt, oracle, gpu):
    import torch
    ref, traces = _ref_many(rt, oracle, 3)
    _enough_many(traces)
    sc = _glass(rt, seed=3)
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


# ----------------------------------------------------------------------------- 4. the whole scene
@functools.lru_cache(maxsize=None)
def _ref_scene(rt, oracle):
    from test_reflect_scene_gpu import GLASS, _stage
    W, H, depth = 64, 48, 3
    inp, mesh, mats = _stage(rt, oracle)
    rough = np.zeros(inp.n, dtype=np.float32)
    rough[GLASS] = 0.2                                                       # the staged glass sphere, frosted
    comp = FR.FresnelSceneComposer(oracle, rt, inp, mesh).set_gloss(seed=11, sphere=rough).set_glass_model()
    return comp.render(W, H, depth, **mats), comp.fresnel_trace, rough


def test_whole_scene_against_the_reference(rt, oracle, gpu):
    from test_reflect_scene_gpu import _scene, _stage
    ref, trace, rough = _ref_scene(rt, oracle)
    assert FR.count(trace, FR.REFLECTED, depth=3) >= 10 and FR.count(trace, FR.THROUGH, depth=3) >= 50
    assert FR.count_perturbed(trace, FR.THROUGH, depth=3) >= 20
    inp, mesh, mats = _stage(rt, oracle)
    sc = _scene(rt, inp, mesh, mats)
    sc.set_glass_model("fresnel")
    sc.set_roughness("sphere", rough)
    sc.set_gloss_seed(11)
    _check(_render(sc, 64, 48, reflect_depth=3), ref, "culled")
    _check(_render(sc, 64, 48, reflect_depth=3, cull=False), ref, "whole list")
    sc.set_glass_model("plain")                                              # and the plain model is another frame
    assert not np.array_equal(_render(sc, 64, 48, reflect_depth=3)[1].view(np.uint32), ref[0].view(np.uint32))


# ----------------------------------------------------------------------------- 5. bands
def test_bands_equal_the_full_frame(rt, oracle, gpu):
    """The key takes the row of the full frame: a band that counted its rows from y0 would draw row 27 as row 0."""
    ref, trace, _ = _ref_base(rt, oracle)
    lower = np.concatenate([t["pix"][t["choice"] == FR.REFLECTED] for t in trace]) >= 27 * W1
    assert int(lower.sum()) >= 10                                            # reflect choices in the second band
    sc = _glass(rt, seed=SEED)
    full = _render(sc, W1, H1, reflect_depth=D1)
    _check(full, ref)
    queue = [0] * D1
    for y0, y1 in ((0, 27), (27, 54)):
        band = _render(sc, W1, H1, reflect_depth=D1, y0=y0, y1=y1)
        assert _same(band, (full[0][y0:y1], full[1][y0:y1])), (y0, y1)
        queue = [a + b for a, b in zip(queue, band[2])]
    assert queue == full[2]
    band_ref, _, _ = _ref_base(rt, oracle, SEED, 0.0, 27, 54)                # the reference agrees about the band
    assert np.array_equal(band_ref[0].view(np.uint32), ref[0][27:54].view(np.uint32))


# ----------------------------------------------------------------------------- 6. the seed
def test_a_seed_changes_only_pixels_with_a_draw(rt, oracle, gpu):
    ref_a, trace_a, _ = _ref_base(rt, oracle)
    ref_b, trace_b, _ = _ref_base(rt, oracle, 7)
    drawn = FR.drawn_pixels(trace_a, W1 * H1).reshape(H1, W1)
    assert np.array_equal(drawn, FR.drawn_pixels(trace_b, W1 * H1).reshape(H1, W1))   # the first draw is at the same hit
    assert 200 <= int(drawn.sum()) < W1 * H1 - 200
    sc = _glass(rt, seed=SEED)
    a = _render(sc, W1, H1, reflect_depth=D1)
    sc.set_gloss_seed(7)
    b = _render(sc, W1, H1, reflect_depth=D1)
    _check(a, ref_a, "seed a")
    _check(b, ref_b, "seed b")
    changed = (a[1].view(np.uint32) != b[1].view(np.uint32)).any(axis=2)
    assert int(changed.sum()) >= 30
    assert not (changed & ~drawn).any()
    sc.set_gloss_seed(SEED)
    assert _same(_render(sc, W1, H1, reflect_depth=D1), a)


# ----------------------------------------------------------------------------- 7. identities
def test_identities_with_the_plain_model(rt, oracle, gpu):
    plain_ref, trace, _ = _ref_base(rt, oracle, SEED, 0.0, 0, H1, FR.PLAIN)  # the glass composer as it was
    assert trace == []
    k, tau, ior = glass_mats(N1)
    sc = _glass(rt, model="plain", seed=SEED)
    plain = _render(sc, W1, H1, reflect_depth=D1)
    _check(plain, plain_ref, "plain")
    sc.set_roughness("sphere", np.where(tau > 0, 0.5, 0.0).astype(np.float32))   # roughness on the glass: no effect
    assert _same(_render(sc, W1, H1, reflect_depth=D1), plain)
    flat = _render(sc, W1, H1)                                               # depth 0
    sc.set_glass_model("fresnel")
    assert _same(_render(sc, W1, H1), flat)                                  # any model at depth 0
    frosted = _render(sc, W1, H1, reflect_depth=D1)
    assert not _same(frosted, plain)
    sc.set_roughness("sphere", None)
    fres = _render(sc, W1, H1, reflect_depth=D1)
    _check(fres, _ref_base(rt, oracle)[0], "fresnel")
    assert not _same(fres, plain) and not _same(fres, frosted) and fres[2][0] == plain[2][0]
    sc.set_glass_model("plain")
    assert _same(_render(sc, W1, H1, reflect_depth=D1), plain)
    # a scene without glass: the model changes nothing, with and without rough mirrors
    mir = Inputs(rt, N1).scene()
    kk = np.array([K_TABLE[i % 4] for i in range(N1)], dtype=np.float32)
    mir.set_materials(kk)
    for rho in (None, np.full(N1, 0.3, dtype=np.float32)):
        mir.set_roughness("sphere", rho)
        mir.set_glass_model("plain")
        a = _render(mir, W1, H1, reflect_depth=D1)
        mir.set_glass_model("fresnel")
        assert _same(_render(mir, W1, H1, reflect_depth=D1), a) and a[2][0] > 0
    mir.set_materials_ex(kk, np.zeros(N1), np.zeros(N1))                     # the extended entry with tau = 0 everywhere
    assert _same(_render(mir, W1, H1, reflect_depth=D1), a)


# ----------------------------------------------------------------------------- 8. a long-lived scene
def test_a_long_lived_scene_against_fresh_ones(rt, gpu):
    """Model, roughness, seed, materials and the sphere list change on one scene, on two streams; after every step it
    renders what a scene built from scratch renders. The model survives set_spheres and set_materials*."""
    import torch
    W, H, depth = 48, 27, 3
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    st = {"n": 64, "model": "plain", "rho": None, "seed": 0, "mats": "glass"}

    def mats(n):
        k, tau, ior = glass_mats(n)
        if st["mats"] == "dense":                                            # another index on every glass sphere
            ior = np.where(tau > 0, 1.33, 0.0).astype(np.float32)
        if st["mats"] == "mirrors":
            return np.where(tau > 0, 0.5, k).astype(np.float32), None, None
        return k, tau, ior

    def set_mats(sc):
        k, tau, ior = mats(st["n"])
        if tau is None:
            sc.set_materials(k)
        else:
            sc.set_materials_ex(k, tau, ior)

    def build():
        sc = Inputs(rt, st["n"]).scene()
        set_mats(sc)
        sc.set_glass_model(st["model"])
        sc.set_roughness("sphere", st["rho"])
        sc.set_gloss_seed(st["seed"])
        return sc

    live = build()

    def model(m):
        def step():
            st["model"] = m
            live.set_glass_model(m)
        return step

    def rough(a):
        def step():
            st["rho"] = None if a is None else np.array([(a, 0.0, a, 0.3)[i % 4] for i in range(st["n"])], dtype=np.float32)
            live.set_roughness("sphere", st["rho"])
        return step

    def seed(v):
        def step():
            st["seed"] = v
            live.set_gloss_seed(v)
        return step

    def materials(which):
        def step():
            st["mats"] = which
            set_mats(live)
        return step

    def spheres(n):
        def step():
            if n != st["n"]:
                st["rho"] = None                           # a new count clears the tables, not the model or the seed
            st["n"] = n
            inp = Inputs(rt, n)
            live.set_spheres(inp.spheres, n)
            set_mats(live)
        return step

    def bad_model():
        with pytest.raises(rt.RtError):
            live.set_glass_model(2)                        # refused: nothing changes

    steps = [("nothing set", lambda: None), ("fresnel", model("fresnel")), ("seed", seed(5)), ("frosted", rough(0.3)),
             ("a refused model", bad_model), ("spheres, same count", spheres(64)), ("another index", materials("dense")),
             ("plain", model("plain")), ("fresnel again", model("fresnel")), ("sphere count", spheres(80)),
             ("frosted again", rough(0.15)), ("mirrors only", materials("mirrors")), ("glass back", materials("glass")),
             ("seed back", seed(0)), ("roughness cleared", rough(None)), ("sphere count back", spheres(64)),
             ("plain at last", model("plain"))]
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
    assert differ >= 10, differ                            # the steps are visible: 14 of them are meant to change the frame


def test_model_rules_on_a_device(rt, gpu):
    sc = _glass(rt, 64)
    check_model_rules(rt, sc)


# ----------------------------------------------------------------------------- 9. refusals
def _refused(sc, lib, w, h, code=2, **kw):
    import torch
    packed = torch.full((h, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rgba = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), **kw)
    rc = lib.rt_scene_render(sc.handle, C.byref(fd), None)
    torch.cuda.synchronize()
    return rc == code and bool((packed == 0x5a5a5a5a).all()) and bool((rgba == 3.0).all())


def test_refusals_write_nothing(rt, gpu):
    """What a reflective frame refuses, it refuses under the Fresnel model as well, and writes nothing."""
    import torch
    lib = rt.load_library()
    w, h, n = 64, 64, 64
    sc = _glass(rt, n, rho=np.full(n, 0.2, dtype=np.float32), seed=2)
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
    # a mirror that is glass as well stays refused, and the refusal changes nothing
    before = _render(sc, w, h, reflect_depth=2)
    k, tau, ior = glass_mats(n)
    with pytest.raises(rt.RtError):
        sc.set_materials_ex(np.where(tau > 0, 0.5, k), tau, ior)
    # a bad model value: refused, and the frame after it is the frame before it
    assert lib.rt_scene_set_glass_model(sc.handle, 2) == 1
    assert _same(_render(sc, w, h, reflect_depth=2), before)
    # a plane in the scene under the spheres-only scope
    from test_gloss_gpu import _state_scn
    sp = _state_scn(rt, 8, 1, 0).scene()
    sp.set_materials_ex([0.0] * 8, [0.5] * 8, [1.5] * 8)
    sp.set_glass_model("fresnel")
    assert _refused(sp, lib, w, h, reflect_depth=2)
    sp.set_reflect_scope("scene")
    assert not _refused(sp, lib, w, h, reflect_depth=2)
