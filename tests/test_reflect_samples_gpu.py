"""Supersampled reflective frames on the device (rt_scene_set_reflect_samples(RT_REFLECT_SAMPLES_MANY)):
parity with the composed reference of tests/reflect_samples_ref.py over mirrors, glass and the whole scene, odd shapes
and group boundaries, sample ranges and progression, the plain frame, bands, the switch with its refusals and the life
cycle of the scratch. Everything is bit for bit: rgba with its .w, the packed words and the queue lengths. The conditions
a case is chosen for are asserted from the reference, never from the device."""
import ctypes as C
import functools

import numpy as np
import pytest

from reflect_samples_ref import SampleRef, ends_differ, kinds_differ, queued_disagree
from reflect_scene_ref import SceneComposer
from scenes import Inputs
from test_reflect_cpu import composer_for
from test_refract_cpu import glass_composer_for

pytestmark = pytest.mark.gpu


def _k_by_index(n, table=(0.0, 0.25, 0.5, 1.0)):
    return np.array([table[i % 4] for i in range(n)], dtype=np.float32)


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
    """A device frame (packed, rgba, queue) against a reference dict."""
    bad = int((got[1].view(np.uint32) != ref["rgba"].view(np.uint32)).any(axis=2).sum())
    assert bad == 0, (what, "rgba", bad)
    assert np.array_equal(got[0], ref["packed"]), (what, "packed")
    assert got[2] == ref["queue"], (what, got[2], ref["queue"])


def _many(scene):
    scene.set_reflect_samples("many")
    return scene


# ----------------------------------------------------------------------------- the shared references
W1, H1, N1, D1 = 96, 54, 256, 3          # case 1: mirrors
W2, H2, N2, D2 = 50, 30, 48, 2           # case 2: 1 500 pixels, a multiple of neither 64 nor 256


@functools.lru_cache(maxsize=None)
def _ref1(rt, oracle):
    inp = Inputs(rt, N1)
    return SampleRef(rt, composer_for(oracle, rt, inp)).render(W1, H1, D1, spp=4, k=_k_by_index(N1))


@functools.lru_cache(maxsize=None)
def _ref2(rt, oracle, spp, base=0, total=0, resolve=0):
    inp = Inputs(rt, N2)
    return SampleRef(rt, composer_for(oracle, rt, inp)).render(W2, H2, D2, spp=spp, base=base, total=total,
                                                               resolve=resolve, k=_k_by_index(N2))


def _scene1(rt):
    sc = Inputs(rt, N1).scene()
    sc.set_materials(_k_by_index(N1))
    return _many(sc)


def _scene2(rt):
    sc = Inputs(rt, N2).scene()
    sc.set_materials(_k_by_index(N2))
    return _many(sc)


# ----------------------------------------------------------------------------- 1. mirrors
def test_mirrors_against_the_reference(rt, oracle, gpu):
    ref = _ref1(rt, oracle)
    m = W1 * H1
    assert int(queued_disagree(ref["samples"], m).sum()) >= 32      # silhouettes of mirrors cross these pixels
    assert int(ends_differ(ref["samples"], m).sum()) >= 8
    assert ref["queue"][0] > 0 and ref["queue"][2] > 0
    assert (ref["rgba"][..., 3] == 4).all()
    sc = _scene1(rt)
    culled = _render(sc, W1, H1, reflect_depth=D1, spp=4)
    brute = _render(sc, W1, H1, reflect_depth=D1, spp=4, cull=False)
    _check(culled, ref, "culled")
    _check(brute, ref, "whole list")


# ----------------------------------------------------------------------------- 2. odd shape, group boundaries
@pytest.mark.parametrize("spp", [3, 5, 16])
def test_odd_shape_and_group_boundaries(rt, oracle, gpu, spp):
    """3: one group that is not full; 5: a group of four and a group of one; 16: four groups."""
    ref = _ref2(rt, oracle, spp)
    assert ref["queue"][0] > 0 and ref["queue"][1] > 0
    sc = _scene2(rt)
    _check(_render(sc, W2, H2, reflect_depth=D2, spp=spp), ref, spp)
    _check(_render(sc, W2, H2, reflect_depth=D2, spp=spp, cull=False), ref, (spp, "whole list"))


# ----------------------------------------------------------------------------- 3. sample ranges, progression
def test_a_sample_range(rt, oracle, gpu):
    """base 1, two samples of four: w = 2 and the packed word of the sum divided by four."""
    ref = _ref2(rt, oracle, 2, 1, 4)
    got = _render(_scene2(rt), W2, H2, reflect_depth=D2, spp=2, sample_base=1, sample_total=4)
    assert (got[1][..., 3] == 2).all()
    _check(got, ref)


def _buffers(w, h):
    import torch
    packed = torch.full((h, w), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rgba = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
    return packed, rgba


def _call(sc, w, h, packed, rgba, **kw):
    import torch
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), **kw)
    sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def test_progression_equals_the_single_call(rt, oracle, gpu):
    ref = _ref2(rt, oracle, 4)
    sc = _scene2(rt)
    single = _render(sc, W2, H2, reflect_depth=D2, spp=4)
    _check(single, ref, "single")
    packed, rgba = _buffers(W2, H2)
    queue = [0] * D2
    for k in range(4):
        _call(sc, W2, H2, packed, rgba, reflect_depth=D2, spp=1, sample_base=k, sample_total=4, accumulate=k > 0,
              resolve=0 if k == 3 else -1)
        queue = [a + b for a, b in zip(queue, sc.reflect_stats()["queue"])]
        if k < 3:
            assert bool((packed == 0x5a5a5a5a).all()), k          # resolve = -1 leaves the words alone
            assert bool((rgba[..., 3] == k + 1).all()), k
    prog = (packed.cpu().numpy().view(np.uint32), rgba.cpu().numpy(), queue)
    assert _same(prog, single)
    _check(prog, ref, "progressive")


def test_a_two_plus_two_split_is_old_plus_the_calls_sum(rt, oracle, gpu):
    first = _ref2(rt, oracle, 2, 0, 4, -1)
    inp = Inputs(rt, N2)
    second = SampleRef(rt, composer_for(oracle, rt, inp)).render(W2, H2, D2, spp=2, base=2, total=4, old=first["rgba"],
                                                                 k=_k_by_index(N2))
    assert first["packed"] is None and (second["rgba"][..., 3] == 4).all()
    sc = _scene2(rt)
    packed, rgba = _buffers(W2, H2)
    _call(sc, W2, H2, packed, rgba, reflect_depth=D2, spp=2, sample_base=0, sample_total=4, resolve=-1)
    assert bool((packed == 0x5a5a5a5a).all())
    assert np.array_equal(rgba.cpu().numpy().view(np.uint32), first["rgba"].view(np.uint32))
    assert sc.reflect_stats()["queue"] == first["queue"]
    _call(sc, W2, H2, packed, rgba, reflect_depth=D2, spp=2, sample_base=2, sample_total=4, accumulate=True)
    _check((packed.cpu().numpy().view(np.uint32), rgba.cpu().numpy(), sc.reflect_stats()["queue"]), second)


# ----------------------------------------------------------------------------- 4. the whole scene
def test_whole_scene_against_the_reference(rt, oracle, gpu):
    from test_reflect_scene_gpu import _scene, _stage
    W, H, depth = 64, 40, 3
    inp, mesh, mats = _stage(rt, oracle)
    ref = SampleRef(rt, SceneComposer(oracle, rt, inp, mesh)).render(W, H, depth, spp=4, **mats)
    assert int(kinds_differ(ref["samples"]).sum()) >= 8             # edges between kinds cross these pixels
    assert ref["queue"][0] > 0 and ref["queue"][2] > 0
    sc = _many(_scene(rt, inp, mesh, mats))
    _check(_render(sc, W, H, reflect_depth=depth, spp=4), ref, "culled")
    _check(_render(sc, W, H, reflect_depth=depth, spp=4, cull=False), ref, "whole list")


# ----------------------------------------------------------------------------- 5. glass, spheres only
def test_glass_against_the_reference(rt, oracle, gpu):
    W, H, n, depth = 64, 36, 128, 3
    inp = Inputs(rt, n)
    tau = np.array([0.9 if i % 3 == 0 else 0.0 for i in range(n)], dtype=np.float32)
    ior = np.where(tau > 0, 1.5, 0.0).astype(np.float32)
    k = np.where(tau > 0, 0.0, _k_by_index(n)).astype(np.float32)
    comp = glass_composer_for(oracle, rt, inp)
    ref = SampleRef(rt, comp).render(W, H, depth, spp=2, k=k, tau=tau, ior=ior)
    assert all(any((b["rule"] == 4).any() for b in s["trace"]) for s in ref["samples"])   # rays pass through spheres
    assert ref["queue"][2] > 0
    sc = inp.scene()
    sc.set_materials_ex(k, tau, ior)
    _many(sc)
    _check(_render(sc, W, H, reflect_depth=depth, spp=2), ref, "culled")
    _check(_render(sc, W, H, reflect_depth=depth, spp=2, cull=False), ref, "whole list")


# ----------------------------------------------------------------------------- 6. against the plain frame
def test_without_materials_it_is_the_plain_frame(rt, gpu):
    n = 1024
    sc = Inputs(rt, n).scene()
    plain = _render(sc, 1920, 1080, spp=4)
    sc.set_materials(np.zeros(n, dtype=np.float32))
    _many(sc)
    got = _render(sc, 1920, 1080, reflect_depth=3, spp=4)
    assert got[2] == [0, 0, 0]
    assert (got[1][..., 3] == 4).all()
    assert _same(got, plain)


def test_with_materials_culled_equals_the_whole_list(rt, gpu):
    n = 1024
    sc = Inputs(rt, n).scene()
    sc.set_materials([0.5 if i % 4 == 0 else 0.0 for i in range(n)])
    _many(sc)
    culled = _render(sc, 960, 540, reflect_depth=3, spp=4)
    brute = _render(sc, 960, 540, reflect_depth=3, spp=4, cull=False)
    assert culled[2][2] > 0 and culled[2] == brute[2]
    assert _same(culled, brute)
    assert not np.array_equal(culled[0], _render(sc, 960, 540, spp=4)[0])      # the mirrors show


# ----------------------------------------------------------------------------- 7. bands
def test_bands_equal_the_full_frame(rt, gpu):
    sc = _scene1(rt)
    full = _render(sc, W1, H1, reflect_depth=D1, spp=4)
    for y0, y1 in [(0, 17), (17, 41), (41, 54), (29, 30)]:
        band = _render(sc, W1, H1, reflect_depth=D1, spp=4, y0=y0, y1=y1)
        assert _same(band, (full[0][y0:y1], full[1][y0:y1])), (y0, y1)


# ----------------------------------------------------------------------------- 8. the switch and the refusals
def test_one_sample_under_many_is_the_frame_under_one(rt, gpu):
    sc = Inputs(rt, N1).scene()
    sc.set_materials(_k_by_index(N1))
    one = _render(sc, W1, H1, reflect_depth=D1)
    _many(sc)
    got = _render(sc, W1, H1, reflect_depth=D1)
    assert one[2][0] > 0 and got[2] == one[2]
    assert _same(got, one)
    assert _same(_render(sc, W1, H1, reflect_depth=D1, spp=1, sample_total=1), one)
    with pytest.raises(rt.RtError, match="status 1"):
        sc.set_reflect_samples(2)
    with pytest.raises(rt.RtError):
        sc.set_reflect_samples("several")
    assert (_render(sc, W1, H1, reflect_depth=D1, spp=4)[1][..., 3] == 4).all()   # still MANY after the errors


def _refused(sc, lib, w, h, **kw):
    import torch
    packed, rgba = _buffers(w, h)
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), **kw)
    rc = lib.rt_scene_render(sc.handle, C.byref(fd), None)
    torch.cuda.synchronize()
    return rc == 2 and bool((packed == 0x5a5a5a5a).all()) and bool((rgba == 3.0).all())


def test_back_to_one_refuses_samples_and_writes_nothing(rt, gpu):
    lib = rt.load_library()
    sc = _scene2(rt)
    assert not _refused(sc, lib, W2, H2, reflect_depth=D2, spp=4)             # under MANY the frame renders
    sc.set_reflect_samples("one")
    for kw in (dict(spp=4), dict(accumulate=True), dict(sample_base=1, sample_total=4), dict(sample_total=4)):
        assert _refused(sc, lib, W2, H2, reflect_depth=D2, **kw), kw


def test_refusals_under_many_write_nothing(rt, gpu):
    import torch
    lib = rt.load_library()
    w, h = 64, 64
    sc = Inputs(rt, 64).scene()
    sc.set_materials([0.5] * 64)
    _many(sc)
    for kw in (dict(interleave=(2, 0, 16)), dict(table_lds=True), dict(profile=True)):
        assert _refused(sc, lib, w, h, reflect_depth=2, spp=4, **kw), kw
    p24 = torch.full((h, w * 3 // 4), 5, dtype=torch.int32, device="cuda")
    assert _refused(sc, lib, w, h, reflect_depth=2, spp=4, packed24=p24.data_ptr())
    assert bool((p24 == 5).all())
    depth = torch.full((h, w), 9.0, dtype=torch.float32, device="cuda")
    assert _refused(sc, lib, w, h, reflect_depth=2, spp=4, aov_depth=depth.data_ptr())
    assert bool((depth == 9.0).all())
    # the sample range is checked as the plain frame checks it
    packed, rgba = _buffers(w, h)
    for kw in (dict(spp=17), dict(spp=2, sample_base=3, sample_total=4), dict(spp=1, sample_base=-1, sample_total=4)):
        fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=2, **kw)
        assert lib.rt_scene_render(sc.handle, C.byref(fd), None) == 1, kw
    torch.cuda.synchronize()
    assert bool((packed == 0x5a5a5a5a).all()) and bool((rgba == 3.0).all())
    # graphs and several devices (the multi-device path with one device and peer copies: no collective library)
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=2, spp=4)
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
    assert not _refused(sc, lib, w, h, reflect_depth=2, spp=4)               # and the plain request renders


# ----------------------------------------------------------------------------- 9. the scratch's life cycle
def test_scratch_life_cycle(rt, oracle, gpu):
    """A small frame of two groups, a larger one of one group (the scratch grows), the small one again: on one scene."""
    small, large = Inputs(rt, N2), Inputs(rt, N1)
    sc = _many(rt.Scene())
    sc.set_texture(small.tex)
    sc.set_sky(small.sky_box, small.sky)
    sc.set_lights(small.lights, small.n_lights)

    def frame(inp, n, w, h, depth, spp):
        sc.set_spheres(inp.spheres, n)
        sc.set_materials(_k_by_index(n))
        return _render(sc, w, h, reflect_depth=depth, spp=spp)

    a = frame(small, N2, W2, H2, D2, 5)
    b = frame(large, N1, W1, H1, D1, 4)
    c = frame(small, N2, W2, H2, D2, 5)
    _check(a, _ref2(rt, oracle, 5), "first")
    _check(b, _ref1(rt, oracle), "second")
    assert _same(c, a) and c[2] == a[2]


# ----------------------------------------------------------------------------- 10. timed frames
def test_timed_frames_are_the_untimed_ones(rt, gpu):
    """Timing on: pass_ms has depth + 2 finite entries >= 0 with a sum > 0, for a one-sample frame (one row of events, no
    resolve slot) and for 5 samples (two groups, 4 + 1: the second row and the resolve slot), and the queue and both
    outputs are those of the same frame with timing off, where pass_ms is None. Nothing about how long a pass takes."""
    w, h, n, depth = 32, 16, 8, 2                    # more than one bounce, a queue that is not empty
    sc = Inputs(rt, n).scene()
    sc.set_materials(_k_by_index(n))
    _many(sc)
    for spp in (1, 5):
        sc.set_reflect_timing(False)
        plain = _render(sc, w, h, reflect_depth=depth, spp=spp)
        assert sc.reflect_stats()["pass_ms"] is None, spp
        assert plain[2][0] > 0 and len(plain[2]) == depth, (spp, plain[2])
        sc.set_reflect_timing(True)
        timed = _render(sc, w, h, reflect_depth=depth, spp=spp)
        ms = sc.reflect_stats()["pass_ms"]
        assert ms is not None and len(ms) == depth + 2, (spp, ms)
        assert all(np.isfinite(t) and t >= 0 for t in ms), (spp, ms)
        assert sum(ms) > 0, (spp, ms)
        assert timed[2] == plain[2], (spp, timed[2], plain[2])
        assert _same(timed, plain), spp
    sc.set_reflect_timing(False)
    _render(sc, w, h, reflect_depth=depth, spp=5)
    assert sc.reflect_stats()["pass_ms"] is None      # off again after timed frames
