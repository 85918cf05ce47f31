"""The denoiser without a device (rt_scene_denoise): the numpy restatement (tests/denoise_ref.py) checked
on its own against properties that follow from the definition, on inputs formed on the CPU (the oracle's colour,
CastRef.nearest's guides); the layout of rt_denoise_desc, its defaults, and the refusals, which happen before the
scene touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
from postpass import bits as _bits
from scenes import Inputs, mixed_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_FIELDS = ("struct_size", "width", "height", "rgba_in", "depth", "normal", "albedo", "id", "rgba_out", "pixels",
           "iterations", "normal_shift", "sigma_depth", "sigma_colour", "demodulate", "variant")


@pytest.fixture(scope="module")
def spheres(rt, oracle):
    """160 x 90 / 256 spheres: 65 % valid pixels, sky above."""
    return R.oracle_inputs(rt, oracle, Inputs(rt, 256), 160, 90)


@pytest.fixture(scope="module")
def mixed(rt, oracle):
    """scenes.mixed_scene at 160 x 96: spheres, cubes and planes; the planes fill the frame (no sky)."""
    return R.oracle_inputs(rt, oracle, mixed_scene(rt), 160, 96)


def _roughness(I, ids):
    """Sum over horizontally and vertically adjacent valid same-id pixel pairs of |Y(I)(a) - Y(I)(b)|."""
    Y = R.luma(I).astype(np.float64)
    k, ix = ids[..., 0], ids[..., 1]
    s = 0.0
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        m = (k[a] >= 0) & (k[a] == k[b]) & (ix[a] == ix[b])
        s += float(np.abs(Y[a] - Y[b])[m].sum())
    return s


def _largest_object(ids):
    key = ids[..., 0].astype(np.int64) * (1 << 32) + ids[..., 1]
    vals, cnt = np.unique(key[ids[..., 0] >= 0], return_counts=True)
    return key == vals[cnt.argmax()]


def test_inputs_are_what_the_tests_assume(spheres, mixed):
    ids = spheres[4]
    share = (ids[..., 0] >= 0).mean()
    assert 0.5 < share < 0.8                                  # sky and spheres
    assert (mixed[4][..., 0] >= 0).all()                      # no sky
    assert {1, 2, 3} <= set(np.unique(mixed[4][..., 0]).tolist())
    for x in (spheres, mixed):
        rgba, depth, normal, albedo, ids = x
        assert rgba.dtype == depth.dtype == normal.dtype == albedo.dtype == np.float32 and ids.dtype == np.int32
        hit = ids[..., 0] >= 0
        assert np.isposinf(depth[~hit]).all() and np.isfinite(depth[hit]).all()


@pytest.mark.parametrize("kw", [dict(iterations=1), dict(), dict(iterations=6), dict(sigma_colour=0.1),
                                dict(demodulate=False), dict(normal_shift=0)])
def test_sky_keeps_its_bits(spheres, kw):
    rgba, depth, normal, albedo, ids = spheres
    out, packed = R.denoise(*spheres, **kw)
    sky = ids[..., 0] < 0
    assert sky.any()
    assert np.array_equal(_bits(out)[sky], _bits(rgba)[sky])
    assert np.array_equal(packed[sky], R.pack(rgba)[sky])
    assert (out[~sky, 3] == 1).all()
    assert not np.array_equal(_bits(out)[~sky], _bits(rgba)[~sky])      # and the rest was filtered


def test_an_all_sky_frame_is_returned_unchanged(spheres):
    rgba, depth, normal, albedo, ids = spheres
    none = np.full_like(ids, -1)
    out, packed = R.denoise(rgba, np.full_like(depth, np.inf), np.zeros_like(normal), albedo, none)
    assert np.array_equal(_bits(out), _bits(rgba))
    assert np.array_equal(packed, R.pack(rgba))


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
@pytest.mark.parametrize("n", [1, 2, 4, 6])
def test_convexity(request, scene, n):
    """Every channel of I_n(p) lies within [min, max] of I_0 over the valid pixels, widened by a relative 2^-19 per
    iteration: an iteration is a weighted mean with non-negative weights, and 25 rounded products, 24 additions of
    non-negative terms and one division stay below 32 eps, eps = 2^-24."""
    x = request.getfixturevalue(scene)
    ids = x[4]
    valid = ids[..., 0] >= 0
    for kw in (dict(), dict(sigma_colour=0.1), dict(demodulate=False)):
        _, _, I0, In = R.denoise(*x, iterations=n, want_irradiance=True, **kw)
        for ch in range(3):
            lo, hi = float(I0[valid, ch].min()), float(I0[valid, ch].max())
            assert lo >= 0
            slack = n * 2.0 ** -19
            assert float(In[valid, ch].min()) >= lo * (1 - slack), (kw, ch)
            assert float(In[valid, ch].max()) <= hi * (1 + slack), (kw, ch)


@pytest.mark.parametrize("n", [1, 4, 6])
def test_a_constant_irradiance_stays_constant(spheres, n):
    rgba, depth, normal, albedo, ids = spheres
    valid = ids[..., 0] >= 0
    const = np.array([0.3, 0.55, 0.7], dtype=f32)
    flat = rgba.copy()
    flat[valid, :3] = const
    out, _, I0, In = R.denoise(flat, depth, normal, albedo, ids, iterations=n, demodulate=False, want_irradiance=True)
    assert (I0[valid] == const).all()
    rel = np.abs(In[valid].astype(np.float64) / const.astype(np.float64) - 1)
    assert rel.max() <= n * 2.0 ** -19
    # with demodulation: I_0 = const where the colour is const x albedo (up to the division's rounding)
    lit = flat.copy()
    lit[valid, :3] = (const * albedo[valid, :3]).astype(f32)
    _, _, I0, In = R.denoise(lit, depth, normal, albedo, ids, iterations=n, want_irradiance=True)
    for ch in range(3):
        lo, hi = float(I0[valid, ch].min()), float(I0[valid, ch].max())
        assert abs(lo / float(const[ch]) - 1) < 2.0 ** -22 and abs(hi / float(const[ch]) - 1) < 2.0 ** -22
        assert float(In[valid, ch].min()) >= lo * (1 - n * 2.0 ** -19)
        assert float(In[valid, ch].max()) <= hi * (1 + n * 2.0 ** -19)


def _centre_only(I, n):
    """n iterations in which only the centre tap contributes: I <- (w I) / w with w = h[0] h[0] = 9 / 64, both
    operations rounded. That is not the identity: 9 I needs up to four more bits than I has, and for about a third
    of all mantissas the rounded product divided by 9 rounds to a neighbour of I (one ulp)."""
    w = f32(0.140625)
    for _ in range(n):
        I = ((w * I).astype(f32) / w).astype(f32)
    return I


@pytest.mark.parametrize("kw", [dict(), dict(iterations=6, sigma_colour=0.1), dict(iterations=1, normal_shift=0)])
def test_a_pixel_without_agreeing_taps_is_the_demodulation_round_trip(spheres, kw):
    """Ids made unique: every tap of every step fails e_id and only the centre tap remains. The result is
    (C / max(A, 2^-10)) A bit for bit, with the centre tap's own rounding (w I) / w per iteration in between (see
    _centre_only: the definition's sums do not return I exactly, so the closed expression carries them; where they
    are exact -- which the test also counts -- it is the plain round trip)."""
    rgba, depth, normal, albedo, ids = spheres
    n = kw.get("iterations", 4)
    valid = ids[..., 0] >= 0
    uniq = ids.copy()
    uniq[..., 1] = np.arange(ids.shape[0] * ids.shape[1]).reshape(ids.shape[:2])
    out, packed = R.denoise(rgba, depth, normal, albedo, uniq, **kw)
    a = albedo[..., :3]
    I0 = (rgba[..., :3] / np.where(a > R.TINY, a, R.TINY).astype(f32)).astype(f32)
    want = (_centre_only(I0, n) * a).astype(f32)
    assert np.array_equal(_bits(out[valid, :3]), _bits(want[valid]))
    assert np.array_equal(_bits(out[~valid]), _bits(rgba[~valid]))
    assert np.array_equal(packed, R.pack(np.where(valid[..., None], want, rgba[..., :3])))
    # where the centre tap's rounding is exact the result is the plain round trip; elsewhere within an ulp per iteration
    plain_trip = (I0 * a).astype(f32)
    exact = (_bits(out[valid, :3]) == _bits(plain_trip[valid])).mean()
    assert exact > 0.3
    assert np.abs(out[valid, :3].astype(np.float64) - plain_trip[valid]).max() <= (n + 1) * 2.0 ** -23 * float(plain_trip[valid].max())
    plain, _ = R.denoise(rgba, depth, normal, albedo, uniq, demodulate=False, **kw)
    assert np.array_equal(_bits(plain[valid, :3]), _bits(_centre_only(rgba[..., :3], n)[valid]))
    # ... and a single valid pixel in a sky frame likewise
    one = np.full_like(ids, -1)
    y, x = np.argwhere(valid)[len(np.argwhere(valid)) // 2]
    one[y, x] = ids[y, x]
    out, _ = R.denoise(rgba, depth, normal, albedo, one, **kw)
    assert np.array_equal(_bits(out[y, x, :3]), _bits(want[y, x]))
    keep = np.ones(valid.shape, dtype=bool)
    keep[y, x] = False
    assert np.array_equal(_bits(out[keep]), _bits(rgba[keep]))


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
def test_iterations_compose(request, scene):
    """iterations = k equals k single iterations fed with their own output when demodulate = 0 and sigma_colour = 0:
    the ping-pong is not observable. (A single call's iteration i has step 2^i: the chain is built from `iterate`.)"""
    rgba, depth, normal, albedo, ids = request.getfixturevalue(scene)
    I = rgba[..., :3].copy()
    for k in range(1, 5):
        I = R.iterate(I, depth, normal, ids, 1 << (k - 1), 5, 0.05, 0.0)
        out, packed = R.denoise(rgba, depth, normal, albedo, ids, iterations=k, demodulate=False)
        valid = ids[..., 0] >= 0
        assert np.array_equal(_bits(out[valid, :3]), _bits(I[valid])), k
    # one iteration of a call is `iterate` at step 1 on the call's own input
    once, _ = R.denoise(rgba, depth, normal, albedo, ids, iterations=1, demodulate=False)
    again, _ = R.denoise(once, depth, normal, albedo, ids, iterations=1, demodulate=False)
    I2 = R.iterate(R.iterate(rgba[..., :3].copy(), depth, normal, ids, 1, 5, 0.05, 0.0), depth, normal, ids, 1, 5, 0.05, 0.0)
    assert np.array_equal(_bits(again[..., :3]), _bits(np.where((ids[..., 0] >= 0)[..., None], I2, rgba[..., :3])))


def test_it_smooths_the_penumbra_staircase(spheres, mixed):
    """A soft shadow is ten sample rays worth 0.1 of the light each: a staircase. After filtering the frame is
    smoother between neighbours of one object, and the object that covers the most pixels of the sphere scene shows
    more distinct brightness levels (a ramp). Both hold with room on these scenes (233.6 -> 199.0 after one iteration,
    176.1 at the defaults, 191.2 with sigma_colour 0.1; 597 -> 974 levels; the mixed scene 266.2 -> 225.6 -> 197.6)."""
    for x in (spheres, mixed):
        ids = x[4]
        _, _, I0, I1 = R.denoise(*x, iterations=1, want_irradiance=True)
        _, _, _, I4 = R.denoise(*x, want_irradiance=True)
        _, _, _, I4c = R.denoise(*x, sigma_colour=0.1, want_irradiance=True)
        r0, r1, r4, r4c = (_roughness(I, ids) for I in (I0, I1, I4, I4c))
        assert r4 < r1 < r0
        assert r4 < r4c < r0                     # the colour weight keeps some of the edges
    ids = spheres[4]
    big = _largest_object(ids)
    assert big.sum() > 200
    _, _, I0, I4 = R.denoise(*spheres, want_irradiance=True)
    assert len(np.unique(R.luma(I4)[big])) > len(np.unique(R.luma(I0)[big]))


def test_nonfinite_guides_do_not_poison(spheres):
    """A NaN or inf in a guide of some pixels: those taps are skipped by their neighbours, and the pixel itself keeps
    a finite value (its centre tap does not evaluate the factors)."""
    rgba, depth, normal, albedo, ids = spheres
    valid = ids[..., 0] >= 0
    ys, xs = np.nonzero(valid)
    pick = np.arange(0, len(ys), 37)
    d2, n2 = depth.copy(), normal.copy()
    d2[ys[pick[0::3]], xs[pick[0::3]]] = np.nan
    d2[ys[pick[1::3]], xs[pick[1::3]]] = -np.inf
    n2[ys[pick[2::3]], xs[pick[2::3]], 1] = np.nan
    out, _ = R.denoise(rgba, d2, n2, albedo, ids)
    assert np.isfinite(out).all()


def test_pack_is_the_oracles(oracle):
    lib = oracle.load()
    rng = np.random.default_rng(3)
    c = rng.uniform(-0.2, 1.4, (500, 3)).astype(f32)
    c[:4] = [[np.nan, 0.5, 2.0], [np.inf, -np.inf, 1.0], [1.0, 255 / 254, 256 / 254], [3e9, -3e9, 0.0]]
    want = np.array([lib.oracle_pack_color(float(r), float(g), float(b)) for r, g, b in c], dtype=np.uint32)
    assert np.array_equal(R.pack(c), want)


# ----------------------------------------------------------------------------- the C ABI
def test_desc_layout_and_defaults(rt, tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof(rt_denoise_desc, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof(rt_denoise_desc));\n{body}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(rt.DenoiseDesc) == want[0]
    assert [getattr(rt.DenoiseDesc, f).offset for f in _FIELDS] == want[1:]
    assert [f for f, _ in rt.DenoiseDesc._fields_] == list(_FIELDS)
    lib = rt.load_library()
    d = rt.DenoiseDesc()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    lib.rt_denoise_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.DenoiseDesc)
    assert (d.iterations, d.normal_shift, d.demodulate, d.variant) == (4, 5, 1, 0)
    assert f32(d.sigma_depth) == f32(0.05) and d.sigma_colour == 0.0
    assert (d.width, d.height) == (0, 0)
    assert not any((d.rgba_in, d.depth, d.normal, d.albedo, d.id, d.rgba_out, d.pixels))
    assert lib.rt_abi_version() == 1
    assert R.DEFAULTS == dict(iterations=4, normal_shift=5, sigma_depth=0.05, sigma_colour=0.0, demodulate=True)


def test_refusals_without_a_device(rt):
    """Every refusal returns RT_ERR_INVALID before the scene is used: a host-only scene, host buffers standing in for
    the device's keep their sentinel."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(1 << 16, 0x5a5a5a5a, dtype=np.uint32)
        p = (sentinel.ctypes.data + 255) & ~255
        ptrs = dict(rgba_in=p, depth=p + 4096, normal=p + 8192, albedo=p + 12288, id=p + 16384, rgba_out=p + 20480,
                    pixels=p + 24576)

        def desc(**kw):
            d = rt.DenoiseDesc()
            lib.rt_denoise_desc_init(C.byref(d))
            d.width, d.height = 16, 8
            for k, v in {**ptrs, **kw}.items():
                setattr(d, k, v)
            return d
        assert lib.rt_scene_denoise(None, C.byref(desc()), None) == 1
        assert lib.rt_scene_denoise(s, None, None) == 1
        bad = [dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20),
               dict(rgba_in=0), dict(depth=0), dict(normal=0), dict(id=0), dict(rgba_out=0), dict(albedo=0),
               dict(rgba_in=p + 4), dict(rgba_in=p + 8), dict(normal=p + 8192 + 8), dict(albedo=p + 12288 + 4),
               dict(rgba_out=p + 20480 + 12), dict(id=p + 16384 + 4), dict(depth=p + 4096 + 2), dict(pixels=p + 24576 + 1),
               dict(iterations=0), dict(iterations=7), dict(iterations=-1), dict(normal_shift=-1), dict(normal_shift=9),
               dict(sigma_depth=0.0), dict(sigma_depth=-0.05), dict(sigma_depth=float("nan")),
               dict(sigma_depth=float("inf")), dict(sigma_colour=float("nan")), dict(sigma_colour=float("inf")),
               dict(variant=-1), dict(variant=3)]
        for kw in bad:
            assert lib.rt_scene_denoise(s, C.byref(desc(**kw)), None) == 1, kw
            assert b"rt_scene_denoise" in lib.rt_last_error()
        # albedo may be NULL only with demodulate = 0: that description passes the checks, which this scene without a
        # device cannot go beyond (a HIP or no-device error, not INVALID)
        import torch
        if not torch.cuda.is_available():
            assert lib.rt_scene_denoise(s, C.byref(desc(albedo=0, demodulate=0)), None) in (3, 4)
        n = C.c_int(7)
        ms = (C.c_float * 8)()
        assert lib.rt_scene_set_denoise_timing(None, 1) == 1
        assert lib.rt_scene_denoise_times(s, ms, 8, C.byref(n)) == 0 and n.value == 0
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_python_denoise_checks_its_frame(rt):
    """A frame without rgba or guides is refused by the wrapper (and without a GPU every call is: no CPU fallback)."""
    sc = rt.Scene()
    try:
        with pytest.raises(rt.RtError):
            sc.denoise({"rgba": None, "aov": {}})
    finally:
        sc.close()
