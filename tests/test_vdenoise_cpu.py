"""The variance-guided denoiser without a device (rt_scene_denoise_variance): the numpy restatement
(tests/vdenoise_ref.py) against rt_scene_denoise's (tests/denoise_ref.py) where the two must agree bit for bit, against
properties that follow from the definition, and on the synthetic frame that shows what the filter is for; the layout
of rt_vdenoise_desc, its defaults, and the refusals, which happen before the scene touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import vdenoise_ref as V
from postpass import bits as _bits
from scenes import Inputs, mixed_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_FIELDS = ("struct_size", "width", "height", "rgba_in", "depth", "normal", "albedo", "id", "rgba_out", "pixels",
           "moments", "variance_out", "iterations", "normal_shift", "sigma_depth", "sigma_colour", "sigma_floor",
           "min_history", "spatial_boost", "demodulate", "variant")


@pytest.fixture(scope="module")
def spheres(rt, oracle):
    return R.oracle_inputs(rt, oracle, Inputs(rt, 256), 160, 90)


@pytest.fixture(scope="module")
def mixed(rt, oracle):
    return R.oracle_inputs(rt, oracle, mixed_scene(rt), 160, 96)


def _converged(x, n=32):
    """A long history whose m2 == m1 m1: (rgba with w = n, moments)."""
    rgba = x[0].copy()
    rgba[..., 3] = n
    Y = R.luma(rgba)
    return rgba, np.stack([Y, (Y * Y).astype(f32)], axis=-1)


def _noisy_history(x, seed=5):
    """A history of mixed lengths with moments that have some variance: rows alternate in blocks of 8 between n = 2
    (spatial at min_history 4) and n = 9."""
    rng = np.random.default_rng(seed)
    rgba = x[0].copy()
    h, w = rgba.shape[:2]
    rgba[..., 3] = np.where((np.arange(h) // 8) % 2 == 0, 2, 9)[:, None]
    Y = R.luma(rgba)
    m2 = ((Y * Y).astype(f32) + rng.uniform(0, 0.02, (h, w)).astype(f32)).astype(f32)
    return rgba, np.stack([Y, m2], axis=-1)


# ----------------------------------------------------------------------------- the anchors
@pytest.mark.parametrize("scene", ["spheres", "mixed"])
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_zero_variance_is_the_plain_filter_at_sigma_floor(request, scene, demodulate, n):
    x = request.getfixturevalue(scene)
    rgba, mom = _converged(x)
    out, packed, v = V.denoise_variance(rgba, *x[1:], moments=mom, iterations=n, demodulate=demodulate)
    want, wpacked = R.denoise(rgba, *x[1:], iterations=n, sigma_colour=2.0 ** -6, demodulate=demodulate)
    assert np.array_equal(_bits(out), _bits(want))
    assert np.array_equal(packed, wpacked)
    assert (v == 0).all()


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
@pytest.mark.parametrize("demodulate", [False, True])
@pytest.mark.parametrize("n", [1, 3, 5])
def test_sigma_colour_zero_is_the_plain_filter_at_sigma_floor(request, scene, demodulate, n):
    x = request.getfixturevalue(scene)
    rgba, mom = _noisy_history(x)
    for moments, floor in ((mom, 2.0 ** -6), (None, 0.1)):
        out, packed, v = V.denoise_variance(rgba, *x[1:], moments=moments, iterations=n, sigma_colour=0.0,
                                            sigma_floor=floor, demodulate=demodulate)
        want, wpacked = R.denoise(rgba, *x[1:], iterations=n, sigma_colour=floor, demodulate=demodulate)
        assert np.array_equal(_bits(out), _bits(want))
        assert np.array_equal(packed, wpacked)
    assert (v[x[4][..., 0] >= 0] > 0).any()          # and there was a variance to ignore


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
def test_a_constant_variance_is_the_plain_filter_at_the_threshold_it_gives(request, scene):
    """moments = (0, 2^-4 - 2^-16), sigma_colour 1, sigma_floor 2^-8: S = 2^-4 exactly, at borders too (the 3 x 3
    weights are dyadic) -- one iteration is rt_scene_denoise's with sigma_colour = 0.25. Two are not: the variance the
    first leaves is no longer constant."""
    x = request.getfixturevalue(scene)
    rgba = x[0].copy()
    rgba[..., 3] = 4
    mom = np.zeros(rgba.shape[:2] + (2,), dtype=f32)
    mom[..., 1] = f32(2.0 ** -4 - 2.0 ** -16)
    kw = dict(moments=mom, sigma_colour=1.0, sigma_floor=2.0 ** -8, demodulate=False)
    out, packed, v = V.denoise_variance(rgba, *x[1:], iterations=1, **kw)
    want, wpacked = R.denoise(rgba, *x[1:], iterations=1, sigma_colour=0.25, demodulate=False)
    assert np.array_equal(_bits(out), _bits(want))
    assert np.array_equal(packed, wpacked)
    out2, _, _ = V.denoise_variance(rgba, *x[1:], iterations=2, **kw)
    want2, _ = R.denoise(rgba, *x[1:], iterations=2, sigma_colour=0.25, demodulate=False)
    assert not np.array_equal(_bits(out2), _bits(want2))


# ----------------------------------------------------------------------------- properties
@pytest.mark.parametrize("kw", [dict(iterations=1), dict(), dict(iterations=6), dict(demodulate=False),
                                dict(normal_shift=0, min_history=1)])
def test_sky_keeps_its_bits_and_the_variance_is_finite(spheres, kw):
    ids = spheres[4]
    sky = ids[..., 0] < 0
    rgba, mom = _noisy_history(spheres)
    for moments in (mom, None):
        out, packed, v = V.denoise_variance(rgba, *spheres[1:], moments=moments, **kw)
        assert np.array_equal(_bits(out)[sky], _bits(rgba)[sky])
        assert np.array_equal(packed[sky], R.pack(rgba)[sky])
        assert (out[~sky, 3] == 1).all()
        assert np.isfinite(v).all() and (v >= 0).all() and (v[sky] == 0).all()
        assert (v[~sky] > 0).any()


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
def test_the_variance_does_not_grow(request, scene):
    """With an all-temporal variance, v_{i+1}(p) = sum(w^2 v) / (sum w)^2 <= max v over the taps that counted (the
    weights are non-negative, so sum w^2 <= (sum w)^2), up to the rounding of 25 products and sums: 2^-19 relative."""
    x = request.getfixturevalue(scene)
    rgba, mom = _noisy_history(x)
    rgba[..., 3] = 16
    _, _, _, I0, _, v0, temporal = V.denoise_variance(rgba, *x[1:], moments=mom, want_irradiance=True)
    valid = x[4][..., 0] >= 0
    assert (temporal == valid).all()
    I, v = I0, v0
    for i in range(4):
        I, v2, vmax = V.iterate(I, v, x[1], x[2], x[4], 1 << i, 5, 0.05, 4.0, 2.0 ** -6, want_taps=True)
        assert (v2[valid] <= vmax[valid] * f32(1 + 2.0 ** -19)).all(), i
        assert (v2[valid] < vmax[valid]).any()              # a mean of several taps has less than the largest of them
        v = v2


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
def test_iterations_compose(request, scene):
    """iterations = k equals k single iterations chained, variance included."""
    x = request.getfixturevalue(scene)
    rgba, mom = _noisy_history(x)
    valid = x[4][..., 0] >= 0
    _, _, _, I0, _, v0, _ = V.denoise_variance(rgba, *x[1:], moments=mom, demodulate=False, want_irradiance=True)
    I, v = I0, v0
    for k in range(1, 5):
        I, v = V.iterate(I, v, x[1], x[2], x[4], 1 << (k - 1), 5, 0.05, 4.0, 2.0 ** -6)
        out, _, vk = V.denoise_variance(rgba, *x[1:], moments=mom, iterations=k, demodulate=False)
        assert np.array_equal(_bits(out[valid, :3]), _bits(I[valid])), k
        assert np.array_equal(_bits(vk), _bits(v)), k


def test_the_two_estimates_are_used_where_they_should(spheres):
    rgba, mom = _noisy_history(spheres)
    valid = spheres[4][..., 0] >= 0
    long_rows = ((np.arange(rgba.shape[0]) // 8) % 2 == 1)[:, None]
    for mh, want in ((4, valid & long_rows), (1, valid), (10, np.zeros_like(valid))):
        *_, v0, temporal = V.denoise_variance(rgba, *spheres[1:], moments=mom, min_history=mh, want_irradiance=True)
        assert np.array_equal(temporal, want), mh
    # without moments every pixel is spatial, and spatial_boost is a factor on it (powers of two: exact)
    *_, v1, temporal = V.denoise_variance(rgba, *spheres[1:], spatial_boost=1.0, want_irradiance=True)
    *_, v4, _ = V.denoise_variance(rgba, *spheres[1:], want_irradiance=True)
    assert not temporal.any()
    assert np.array_equal(_bits(v4), _bits((v1 * f32(4)).astype(f32))) and (v1[valid] > 0).any()
    # a NaN history length fails the test for "long": spatial
    r2 = rgba.copy()
    r2[..., 3] = np.nan
    *_, temporal = V.denoise_variance(r2, *spheres[1:], moments=mom, want_irradiance=True)
    assert not temporal.any()


def test_nonfinite_guides_and_moments_do_not_reach_other_pixels(spheres):
    """NaN / inf in depth, normal, moments and n of some pixels: the output is finite everywhere, and beyond the reach
    of those pixels (7 = 1 + 2 + 4 pixels after three iterations, plus 1 for the 3 x 3 mean of each) it is unchanged."""
    rgba, mom = _noisy_history(spheres)
    depth, normal, albedo, ids = spheres[1:]
    valid = ids[..., 0] >= 0
    ys, xs = np.nonzero(valid)
    pick = np.arange(0, len(ys), 211)
    d2, n2, m2, r2 = depth.copy(), normal.copy(), mom.copy(), rgba.copy()
    d2[ys[pick[0::6]], xs[pick[0::6]]] = np.nan
    d2[ys[pick[1::6]], xs[pick[1::6]]] = -np.inf
    n2[ys[pick[2::6]], xs[pick[2::6]], 1] = np.nan
    m2[ys[pick[3::6]], xs[pick[3::6]], 1] = np.inf
    m2[ys[pick[4::6]], xs[pick[4::6]], 0] = np.nan
    r2[ys[pick[5::6]], xs[pick[5::6]], 3] = np.nan
    base, _, vb = V.denoise_variance(rgba, depth, normal, albedo, ids, mom, iterations=3)
    out, _, v = V.denoise_variance(r2, d2, n2, albedo, ids, m2, iterations=3)
    assert np.isfinite(out[..., :3]).all() and np.isfinite(v).all() and (v >= 0).all()
    near = np.zeros_like(valid)
    for y, x in zip(ys[pick], xs[pick]):
        near[max(0, y - 24):y + 25, max(0, x - 24):x + 25] = True
    assert (~near & valid).sum() > 100
    assert np.array_equal(_bits(out[~near, :3]), _bits(base[~near, :3]))
    assert np.array_equal(_bits(v[~near]), _bits(vb[~near]))


# ----------------------------------------------------------------------------- what it is for
def _plane_frame(seed=7):
    """96 x 64, one plane: luminance 0.25 left of column 48, 0.75 from it on. Rows 0 ... 31 converged (n = 32, m2 = m1
    m1), rows 32 ... 63 the mean of 8 samples with Gaussian noise of standard deviation 0.25 (n = 8, their moments)."""
    h, w = 64, 96
    rng = np.random.default_rng(seed)
    clean = np.where(np.arange(w) < 48, 0.25, 0.75).astype(f32)[None, :].repeat(h, 0)
    samples = (clean[None] + rng.normal(0, 0.25, (8, h, w)).astype(f32)).astype(f32)
    lum = clean.copy()
    lum[32:] = samples.mean(0).astype(f32)[32:]
    rgba = np.zeros((h, w, 4), f32)
    rgba[..., :3] = lum[..., None]
    rgba[:32, :, 3], rgba[32:, :, 3] = 32, 8
    Y = R.luma(rgba)
    mom = np.stack([Y, (Y * Y).astype(f32)], axis=-1)
    mom[32:, :, 0] = samples.mean(0).astype(f32)[32:]
    mom[32:, :, 1] = (samples * samples).mean(0).astype(f32)[32:]
    depth = np.full((h, w), 5.0, f32)
    normal = np.zeros((h, w, 4), f32)
    normal[..., 1] = 1
    ids = np.zeros((h, w, 2), np.int32)
    ids[..., 0] = 3
    return rgba, depth, normal, np.ones((h, w, 4), f32), ids, mom, clean


def test_it_keeps_what_the_history_resolved_and_filters_what_it_has_not():
    """Figures of this seed (max |out - in| over rows 0 ... 29; RMS error over rows 36 ... 63, >= 31 columns from the
    edge; the input's RMS error there 0.0906): the new filter 0.0031 / 0.0038 at sigma_colour 1 and 0.0031 / 0.0020
    at 4; rt_scene_denoise 0.240 / 0.0020 at sigma_colour 0, 0.0028 / 0.0729 at 2^-6, 0.0214 / 0.0045 at 0.1,
    0.234 / 0.0020 at 1."""
    rgba, depth, normal, albedo, ids, mom, clean = _plane_frame()
    cols = np.r_[0:48 - 31 + 1, 48 + 31:96]

    def figures(out):
        moved = float(np.abs(out[:30, :, :3] - rgba[:30, :, :3]).max())
        e = out[36:, cols, 0].astype(np.float64) - clean[36:, cols]
        return moved, float(np.sqrt((e ** 2).mean()))
    _, rms_in = figures(rgba)
    for sc in (1.0, 4.0):
        out, _, _ = V.denoise_variance(rgba, depth, normal, albedo, ids, mom, iterations=4, sigma_colour=sc,
                                       demodulate=False)
        moved, rms = figures(out)
        print("variance-guided", sc, moved, rms, rms_in)
        assert moved <= 0.01 and rms <= rms_in / 8, (sc, moved, rms, rms_in)
    for sc in (0.0, 2.0 ** -6, 0.1, 1.0):
        out, _ = R.denoise(rgba, depth, normal, albedo, ids, iterations=4, sigma_colour=sc, demodulate=False)
        moved, rms = figures(out)
        print("plain", sc, moved, rms)
        assert moved > 0.01 or rms > rms_in / 8, (sc, moved, rms)


# ----------------------------------------------------------------------------- the C ABI
def test_desc_layout_and_defaults(rt, tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof(rt_vdenoise_desc, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof(rt_vdenoise_desc));\n{body}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(rt.VDenoiseDesc) == want[0]
    assert [getattr(rt.VDenoiseDesc, f).offset for f in _FIELDS] == want[1:]
    assert [f for f, _ in rt.VDenoiseDesc._fields_] == list(_FIELDS)
    lib = rt.load_library()
    d = rt.VDenoiseDesc()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    lib.rt_vdenoise_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.VDenoiseDesc)
    assert (d.iterations, d.normal_shift, d.demodulate, d.variant, d.min_history) == (4, 5, 1, 0, 4)
    assert f32(d.sigma_depth) == f32(0.05) and d.sigma_colour == 4.0 and d.sigma_floor == 2.0 ** -6 and d.spatial_boost == 4.0
    assert (d.width, d.height) == (0, 0)
    assert not any((d.rgba_in, d.depth, d.normal, d.albedo, d.id, d.rgba_out, d.pixels, d.moments, d.variance_out))
    assert lib.rt_abi_version() == 1
    assert V.DEFAULTS == dict(iterations=4, normal_shift=5, sigma_depth=0.05, sigma_colour=4.0, sigma_floor=2.0 ** -6,
                              min_history=4, spatial_boost=4.0, demodulate=True)


def test_refusals_without_a_device(rt):
    """Every refusal returns RT_ERR_INVALID before the scene is used: a host-only scene, host buffers standing in for
    the device's keep their sentinel."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(1 << 16, 0x5a5a5a5a, dtype=np.uint32)
        p = (sentinel.ctypes.data + 255) & ~255
        ptrs = dict(rgba_in=p, depth=p + 4096, normal=p + 8192, albedo=p + 12288, id=p + 16384, rgba_out=p + 20480,
                    pixels=p + 24576, moments=p + 28672, variance_out=p + 32768)

        def desc(**kw):
            d = rt.VDenoiseDesc()
            lib.rt_vdenoise_desc_init(C.byref(d))
            d.width, d.height = 16, 8
            for k, v in {**ptrs, **kw}.items():
                setattr(d, k, v)
            return d
        assert lib.rt_scene_denoise_variance(None, C.byref(desc()), None) == 1
        assert lib.rt_scene_denoise_variance(s, None, None) == 1
        nan, inf = float("nan"), float("inf")
        bad = [dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20),
               dict(rgba_in=0), dict(depth=0), dict(normal=0), dict(id=0), dict(rgba_out=0), dict(albedo=0),
               dict(rgba_in=p + 4), dict(rgba_in=p + 8), dict(normal=p + 8192 + 8), dict(albedo=p + 12288 + 4),
               dict(rgba_out=p + 20480 + 12), dict(id=p + 16384 + 4), dict(depth=p + 4096 + 2), dict(pixels=p + 24576 + 1),
               dict(moments=p + 28672 + 4), dict(variance_out=p + 32768 + 2),
               dict(iterations=0), dict(iterations=7), dict(iterations=-1), dict(normal_shift=-1), dict(normal_shift=9),
               dict(sigma_depth=0.0), dict(sigma_depth=-0.05), dict(sigma_depth=nan), dict(sigma_depth=inf),
               dict(sigma_colour=nan), dict(sigma_colour=inf), dict(sigma_colour=-1.0), dict(sigma_colour=2.0 ** 21),
               dict(sigma_floor=0.0), dict(sigma_floor=-1.0), dict(sigma_floor=nan), dict(sigma_floor=inf),
               dict(min_history=0), dict(min_history=257), dict(min_history=-4),
               dict(spatial_boost=-1.0), dict(spatial_boost=nan), dict(spatial_boost=inf),
               dict(variant=-1), dict(variant=3),
               # overlaps: an output on an input, an output on an output, rgba_out inside rgba_in but not equal to it
               dict(pixels=p), dict(variance_out=p + 4096), dict(rgba_out=p + 8192), dict(rgba_out=p + 28672),
               dict(variance_out=p + 24576), dict(pixels=p + 20480), dict(rgba_out=p + 16), dict(variance_out=p + 28672 + 64)]
        for kw in bad:
            assert lib.rt_scene_denoise_variance(s, C.byref(desc(**kw)), None) == 1, kw
            assert b"rt_scene_denoise_variance" in lib.rt_last_error()
        # these pass the checks, which this scene without a device cannot go beyond (a HIP or no-device error)
        import torch
        if not torch.cuda.is_available():
            for kw in (dict(albedo=0, demodulate=0), dict(rgba_out=p), dict(moments=0, variance_out=0, pixels=0),
                       dict(sigma_colour=0.0, spatial_boost=0.0, min_history=256), dict(variant=2)):
                assert lib.rt_scene_denoise_variance(s, C.byref(desc(**kw)), None) in (3, 4), kw
        n = C.c_int(7)
        ms = (C.c_float * 9)()
        assert lib.rt_scene_set_vdenoise_timing(None, 1) == 1
        assert lib.rt_scene_vdenoise_times(s, ms, 9, C.byref(n)) == 0 and n.value == 0
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_python_denoise_variance_checks_its_frame(rt):
    sc = rt.Scene()
    try:
        with pytest.raises(rt.RtError):
            sc.denoise_variance({"rgba": None, "aov": {}})
    finally:
        sc.close()
