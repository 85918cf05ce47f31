"""The display transform without a device (rt_scene_display): the layout of rt_display_desc and its
defaults, every refusal (which happens before the scene touches a device) and the field it names, the wrapper's own
errors and where its methods sit, the table of sRGB thresholds, and the numpy restatement (tests/display_ref.py) on its
own: the bin edges, the hand value, the codes at every threshold, and the histogram resolve against a second
restatement that ranks the luminances."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import display_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_FIELDS = ("struct_size", "width", "height", "rgba_in", "id", "rgba_out", "pixels", "state", "histogram_out", "meter",
           "exposure", "key", "min_exposure", "max_exposure", "meter_low", "meter_high", "adapt", "meter_sky", "curve",
           "white", "transfer", "variant")


# ----------------------------------------------------------------------------- the C ABI
def test_desc_layout_and_defaults(rt, tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof(rt_display_desc, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof(rt_display_desc));\n{body}'
                   '    printf("%d\\n", RT_DISPLAY_BINS);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(rt.DisplayDesc) == want[0] == 120
    assert [getattr(rt.DisplayDesc, f).offset for f in _FIELDS] == want[1:-1]
    assert [f for f, _ in rt.DisplayDesc._fields_] == list(_FIELDS)
    assert want[-1] == rt.RT_DISPLAY_BINS == D.BINS == 512
    lib = rt.load_library()
    d = rt.DisplayDesc()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    lib.rt_display_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.DisplayDesc)
    assert (d.meter, d.curve, d.transfer, d.variant, d.meter_sky) == (1, 2, 1, 0, 0)
    assert (d.meter_low, d.meter_high) == (512, 973)
    assert (d.exposure, d.min_exposure, d.max_exposure, d.adapt, d.white) == (1.0, 2.0 ** -6, 2.0 ** 6, 1.0, 4.0)
    assert f32(d.key) == f32(0.18)
    assert (d.width, d.height) == (0, 0)
    assert not any((d.rgba_in, d.id, d.rgba_out, d.pixels, d.state, d.histogram_out))
    assert (rt.RT_DISPLAY_METER_MANUAL, rt.RT_DISPLAY_METER_AUTO, rt.RT_DISPLAY_METER_LAGGED) == (0, 1, 2)
    assert (rt.RT_DISPLAY_CLIP, rt.RT_DISPLAY_REINHARD, rt.RT_DISPLAY_ACES) == (0, 1, 2)
    assert (rt.RT_DISPLAY_LINEAR, rt.RT_DISPLAY_SRGB) == (0, 1)
    assert D.DEFAULTS == dict(meter="auto", exposure=1.0, key=0.18, min_exposure=2.0 ** -6, max_exposure=2.0 ** 6,
                              meter_low=512, meter_high=973, adapt=1.0, meter_sky=False, curve="aces", white=4.0,
                              transfer="srgb")
    assert lib.rt_abi_version() == 1


def test_refusals_without_a_device(rt):
    """Every refusal returns RT_ERR_INVALID before the scene is used and names its field: a host-only scene, host
    buffers standing in for the device's keep their sentinel."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(1 << 14, 0x5a5a5a5a, dtype=np.uint32)
        p = (sentinel.ctypes.data + 255) & ~255
        names = ("rgba_in", "id", "rgba_out", "pixels", "state", "histogram_out")
        q = {k: p + 4096 * i for i, k in enumerate(names)}          # 16 x 8 pixels: at most 2 KiB each

        def desc(size=None, **kw):
            d = rt.DisplayDesc()
            lib.rt_display_desc_init(C.byref(d))
            d.width, d.height = 16, 8
            for k, v in {**q, **kw}.items():
                setattr(d, k, v)
            if size is not None:
                d.struct_size = size
            return d
        assert lib.rt_scene_display(None, C.byref(desc()), None) == 1
        assert lib.rt_scene_display(s, None, None) == 1
        nan, inf = float("nan"), float("inf")
        bad = [(dict(width=0), "width"), (dict(height=0), "height"), (dict(width=-3), "width"), (dict(height=-1), "height"),
               (dict(width=1 << 20), "width"), (dict(height=32769), "height"),
               (dict(meter=-1), "meter"), (dict(meter=3), "meter"), (dict(curve=-1), "curve"), (dict(curve=3), "curve"),
               (dict(transfer=-1), "transfer"), (dict(transfer=2), "transfer"), (dict(variant=-1), "variant"),
               (dict(variant=2), "variant"),
               (dict(rgba_in=0), "rgba_in"), (dict(state=0), "state"), (dict(state=0, meter=2), "state"),
               (dict(meter=0, rgba_out=0, pixels=0), "rgba_out"),
               (dict(rgba_in=q["rgba_in"] + 4), "rgba_in"), (dict(rgba_in=q["rgba_in"] + 8), "rgba_in"),
               (dict(rgba_out=q["rgba_out"] + 8), "rgba_out"), (dict(state=q["state"] + 4), "state"),
               (dict(state=q["state"] + 8), "state"), (dict(id=q["id"] + 4), "id"), (dict(pixels=q["pixels"] + 2), "pixels"),
               (dict(histogram_out=q["histogram_out"] + 1), "histogram_out"),
               (dict(exposure=0.0), "exposure"), (dict(exposure=-1.0), "exposure"), (dict(exposure=nan), "exposure"),
               (dict(exposure=inf), "exposure"),
               (dict(key=0.0), "key"), (dict(key=-0.18), "key"), (dict(key=nan), "key"), (dict(key=inf), "key"),
               (dict(min_exposure=0.0), "min_exposure"), (dict(min_exposure=nan), "min_exposure"),
               (dict(min_exposure=inf), "min_exposure"), (dict(min_exposure=-1.0), "min_exposure"),
               (dict(max_exposure=0.0), "max_exposure"), (dict(max_exposure=nan), "max_exposure"),
               (dict(max_exposure=inf), "max_exposure"), (dict(min_exposure=2.0, max_exposure=1.0), "min_exposure"),
               (dict(meter_low=-1), "meter_low"), (dict(meter_low=973), "meter_low"), (dict(meter_low=1000), "meter_low"),
               (dict(meter_high=1025), "meter_high"), (dict(meter_low=1024, meter_high=1024), "meter_high"),
               (dict(adapt=0.0), "adapt"), (dict(adapt=-0.5), "adapt"), (dict(adapt=1.5), "adapt"), (dict(adapt=nan), "adapt"),
               (dict(white=0.0), "white"), (dict(white=-4.0), "white"), (dict(white=nan), "white"), (dict(white=inf), "white"),
               # an output that overlaps an input or another output
               (dict(rgba_out=q["rgba_in"] + 16), "rgba_in"), (dict(rgba_out=q["rgba_in"] - 16), "rgba_in"),
               (dict(rgba_out=q["id"]), "id"), (dict(pixels=q["rgba_in"]), "rgba_in"), (dict(pixels=q["id"] + 1020), "id"),
               (dict(state=q["rgba_in"] + 2032), "rgba_in"), (dict(state=q["id"]), "id"),
               (dict(histogram_out=q["rgba_in"] + 2044), "rgba_in"), (dict(histogram_out=q["id"] - 2044), "id"),
               (dict(pixels=q["rgba_out"] + 2044), "pixels"), (dict(state=q["rgba_out"]), "state"),
               (dict(state=q["pixels"] + 496), "state"), (dict(histogram_out=q["pixels"] - 2044), "histogram_out"),
               (dict(histogram_out=q["state"] - 2032), "histogram_out"), (dict(state=q["histogram_out"] + 2032), "state"),
               (dict(meter=0, pixels=q["rgba_out"]), "pixels"), (dict(meter=0, pixels=q["rgba_in"] + 2044), "rgba_in"),
               # a shorter struct_size: what lies past it reads as 0
               (dict(size=rt.DisplayDesc.exposure.offset), "exposure"), (dict(size=rt.DisplayDesc.white.offset), "white"),
               (dict(size=rt.DisplayDesc.adapt.offset), "adapt"), (dict(size=rt.DisplayDesc.meter_high.offset), "meter_high"),
               # ... the metering mode too: MANUAL without a manual exposure
               (dict(size=rt.DisplayDesc.state.offset), "exposure")]
        for kw, field in bad:
            assert lib.rt_scene_display(s, C.byref(desc(**kw)), None) == 1, kw
            message = lib.rt_last_error().decode()
            assert message.startswith("rt_scene_display: ") and field in message, (kw, message)
        import torch
        if not torch.cuda.is_available():
            # these pass the checks, which a scene without a device cannot go beyond (a HIP or no-device error)
            ok = [dict(), dict(rgba_out=q["rgba_in"]), dict(id=0, histogram_out=0), dict(rgba_out=0), dict(pixels=0),
                  dict(rgba_out=0, pixels=0), dict(meter=2, rgba_out=0, pixels=0),
                  # MANUAL reads neither id, state nor histogram_out: wherever they point
                  dict(meter=0, state=0, id=q["rgba_out"] + 4, histogram_out=q["pixels"] + 1),
                  dict(meter=0, state=q["rgba_out"] + 4), dict(size=rt.DisplayDesc.variant.offset),
                  dict(size=0), dict(min_exposure=3.0, max_exposure=3.0), dict(meter_low=0, meter_high=1024),
                  dict(meter_low=1023, meter_high=1024), dict(adapt=2.0 ** -20)]
            for kw in ok:
                assert lib.rt_scene_display(s, C.byref(desc(**kw)), None) in (3, 4), kw
        n = C.c_int(7)
        ms = (C.c_float * 3)()
        assert lib.rt_scene_set_display_timing(None, 1) == 1
        assert lib.rt_scene_set_display_timing(s, 1) == 0
        assert lib.rt_scene_display_times(s, ms, 3, C.byref(n)) == 0 and n.value == 0
        assert lib.rt_scene_display_times(s, None, 3, C.byref(n)) == 1
        assert lib.rt_display_transfer_table(None) == 1
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_python_display_checks_its_arguments(rt):
    """The wrapper refuses unknown names and malformed knobs itself, and without a GPU every call (no CPU fallback);
    the builder passes the defaults through; the new methods sit behind indirect_paths_times, at the end of the class."""
    import torch
    sc = rt.Scene()
    try:
        frame = {"rgba": None, "aov": {}}
        for kw in (dict(meter="spot"), dict(curve="filmic"), dict(transfer="gamma"), dict(window=(1, 2, 3)),
                   dict(limits=(1.0,))):
            with pytest.raises(rt.RtError, match="display: " + next(iter(kw))):
                sc.display(frame, **kw)
        with pytest.raises(rt.RtError):
            sc.display(frame)
        if torch.cuda.is_available():
            with pytest.raises(rt.RtError, match="colour"):
                sc.display(torch.zeros(4, 4, 3))
        d = sc.display_desc(640, 360)
        assert (d.width, d.height, d.meter, d.curve, d.transfer, d.variant) == (640, 360, 1, 2, 1, 0)
        d = sc.display_desc(8, 4, rgba_in=4096, id=8192, rgba_out=12288, pixels=16384, state=20480, histogram_out=24576,
                            meter=2, exposure=2.0, key=0.25, min_exposure=0.5, max_exposure=8.0, meter_low=100,
                            meter_high=900, adapt=0.25, meter_sky=True, curve=1, white=2.0, transfer=0, variant=1)
        assert [getattr(d, f) for f in _FIELDS] == [C.sizeof(rt.DisplayDesc), 8, 4, 4096, 8192, 12288, 16384, 20480, 24576,
                                                    2, 2.0, 0.25, 0.5, 8.0, 100, 900, 0.25, 1, 1, 2.0, 0, 1]
        assert sc.display_raw(sc.display_desc(0, 4)) == 1
        assert sc.display_times() == []
    finally:
        sc.close()
    names = [n for n in vars(rt.Scene) if not n.startswith("__")]
    assert names[names.index("indirect_paths_times") + 1:] == ["display_desc", "display_raw", "display",
                                                               "set_display_timing", "display_times"]


# ----------------------------------------------------------------------------- the table of thresholds
def test_the_transfer_table(rt):
    T = D.table(rt)
    assert T.dtype == f32 and T.shape == (256,) and T[0] == 0
    assert (np.diff(T) > 0).all()
    exact = D.table_formula()
    assert (np.abs(T.astype(np.float64) - exact)[1:] <= np.spacing(T[1:]).astype(np.float64)).all()
    assert abs(float(T[1]) - 0.00015176) < 1e-8 and abs(float(T[255]) - 0.99554527) < 1e-7
    # the linear segment ends below code 11 (0.04045 * 255 = 10.3): both branches of the EOTF are in the table
    assert exact[10] == ((10 - 0.5) / 255.0) / 12.92 and exact[11] == (((11 - 0.5) / 255.0 + 0.055) / 1.055) ** 2.4


def test_codes_at_every_threshold(rt):
    T = D.table(rt)
    v = np.arange(256)
    assert np.array_equal(D.codes(T, T), v)
    below = np.nextafter(T[1:], f32(0))
    assert np.array_equal(D.codes(below, T), v[1:] - 1)
    odd = np.array([np.nan, -np.nan, -0.0, -1.0, -np.inf, np.inf, 1.0, 2.0 ** -149], dtype=f32)
    assert list(D.codes(odd, T)) == [0, 0, 0, 0, 0, 255, 255, 0]
    o = np.array([[0.5, 0.0, 1.0, 9.0]], dtype=f32)
    c = D.codes(o[0, :3], T)
    assert int(D.pack_srgb(o, T)[0]) == (int(c[0]) << 16) + (int(c[1]) << 8) + int(c[2]) and (c[1], c[2]) == (0, 255)
    assert c[0] == 188                                          # the sRGB code of 0.5


# ----------------------------------------------------------------------------- metering
def test_bin_edges():
    l = np.array([2.0 ** -17, 2.0 ** -16, 1, 1.5, 65535, 65536, 1e30], dtype=f32)
    assert list(D.bins(l)) == [0, 0, 256, 264, 511, 511, 511]
    odd = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 2.0 ** -149, 2.0 ** -126], dtype=f32)
    assert list(D.bins(odd)) == [-1, -1, -1, -1, -1, -1, 0, 0]
    # sixteen bins per octave, each an equal step of the mantissa
    assert list(D.bins(np.array([1 + i / 16 for i in range(16)], dtype=f32))) == list(range(256, 272))
    assert D.bins(np.nextafter(f32(2), f32(0)))[()] == 271 and D.bins(f32(2))[()] == 272


def test_hand_value_all_ones():
    rgba = np.ones((3, 5, 4), dtype=f32)
    assert (D.luma(rgba) == 1).all()             # 0.2126 + 0.7152 + 0.0722 in binary32
    h = D.histogram(rgba)
    assert h[256] == 15 and h.sum() == 15
    assert D.metered_luminance(h) == f32(1.03125)
    st = D.resolve(h, np.zeros(4, dtype=f32), 15)
    assert st[0] == f32(0.18) / f32(1.03125) and st[1] == f32(1.03125) and st[2] == 1 and st[3] == 1
    # half the way from a valid state's exposure
    st2 = D.resolve(h, np.array([1, 0, 0, 1], dtype=f32), 15, adapt=0.5)
    assert st2[0] == f32(1) + (st[0] - f32(1)) * f32(0.5)
    # a state that is not valid is not adapted from
    assert D.resolve(h, np.array([1, 0, 0, 0.5], dtype=f32), 15, adapt=0.5)[0] == st[0]
    # the limits
    assert D.resolve(h, np.zeros(4, dtype=f32), 15, min_exposure=0.5, max_exposure=2.0)[0] == f32(0.5)
    assert D.resolve(h, np.zeros(4, dtype=f32), 15, key=18.0, max_exposure=2.0)[0] == f32(2)
    # nothing metered: the valid state's exposure, else the fallback
    none = np.zeros(D.BINS, dtype=np.int64)
    assert list(D.resolve(none, np.array([3, 9, 9, 1], dtype=f32), 15, exposure=7.0)) == [3, 0, 0, 1]
    assert list(D.resolve(none, np.zeros(4, dtype=f32), 15, exposure=7.0)) == [7, 0, 0, 1]


@pytest.mark.parametrize("n", [1, 2, 3, 1023, 1024, 1025, 5000])
@pytest.mark.parametrize("low,high", [(512, 973), (0, 1024), (0, 1), (1023, 1024), (100, 101)])
def test_the_resolve_equals_the_ranked_restatement(n, low, high):
    rng = np.random.default_rng(1000 * n + low + high)
    for spread in (0.01, 2.0, 12.0):
        l = np.exp2(rng.normal(0, spread, n)).astype(f32)
        l[rng.random(n) < 0.05] = 0                           # not metered
        if not (l > 0).any():
            l[0] = 1
        N = int((l > 0).sum())
        lo, hi = D.window(N, low, high)
        assert 0 <= lo < hi <= N
        rgba = np.stack([l, l, l, np.ones_like(l)], axis=-1)[None]
        lum = D.luma(rgba)[0]
        h = D.histogram(rgba)
        assert h.sum() == int(((lum > 0) & np.isfinite(lum)).sum())
        assert D.metered_luminance(h, low, high) == D.resolve_sorted(lum, low, high)


def test_the_window_is_a_robust_log_average():
    """10^5 log-normal luminances: Lm lies within an eighth of an octave of the geometric mean over the same ranks."""
    rng = np.random.default_rng(5)
    l = np.exp2(rng.normal(0, 2, 100000)).astype(f32)
    rgba = np.stack([l, l, l, l], axis=-1)[None]
    lum = np.sort(D.luma(rgba)[0])
    Lm = float(D.metered_luminance(D.histogram(rgba)))
    lo, hi = D.window(len(lum), 512, 973)
    geo = float(np.exp2(np.log2(lum[lo:hi].astype(np.float64)).mean()))
    print("Lm", Lm, "geometric mean of the window", geo)
    assert abs(np.log2(Lm / geo)) < 0.125


# ----------------------------------------------------------------------------- curves and the pack
def test_curves_on_known_values(rt):
    T = D.table(rt)
    x = np.array([[0.0, 0.18, 1.0], [4.0, 1e30, -1.0], [np.nan, np.inf, -np.inf]], dtype=f32)
    clip = D.tone(x, 1.0, "clip")
    assert np.array_equal(clip.view(np.uint32), x.view(np.uint32))
    assert np.array_equal(D.tone(x, 2.0, "clip")[:2], (x[:2] * f32(2)).astype(f32))
    aces = D.tone(x, 1.0, "aces")
    assert aces[0, 0] == 0 and abs(float(aces[0, 1]) - 0.267) < 0.001 and abs(float(aces[0, 2]) - 0.8038) < 0.001
    assert 0.97 < aces[1, 0] < 0.98 and list(aces[1, 1:]) == [1, 0] and list(aces[2]) == [0, 1, 0]
    grey = np.array([[4.0, 4.0, 4.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]], dtype=f32)
    r = D.tone(grey, 1.0, "reinhard", white=4.0)
    assert np.allclose(r[0], 1, atol=1e-6) and np.allclose(r[1], (1 + 1 / 16) / 2, atol=1e-6) and (r[2] == 0).all()
    assert ((r >= 0) & (r <= 1)).all() and ((aces[:2] >= 0) & (aces[:2] <= 1)).all()
    # MANUAL, exposure 1, CLIP, LINEAR: the input's bits and today's pack
    rgba = np.random.default_rng(2).uniform(-0.5, 3, (6, 7, 4)).astype(f32)
    out = D.display(rgba, table=T, meter="manual", curve="clip", transfer="linear")
    assert np.array_equal(out["rgba"].view(np.uint32), rgba.view(np.uint32))
    assert np.array_equal(out["pixels"], D.pack(rgba)) and out["state"] is None and out["histogram"] is None
    # lagged shows with the state's exposure and resolves the frame's own
    st = np.array([0.5, 0, 0, 1], dtype=f32)
    lag = D.display(rgba, st, table=T, meter="lagged")
    man = D.display(rgba, table=T, meter="manual", exposure=0.5)
    auto = D.display(rgba, st, table=T, meter="auto")
    assert np.array_equal(lag["rgba"].view(np.uint32), man["rgba"].view(np.uint32)) and np.array_equal(lag["pixels"], man["pixels"])
    assert np.array_equal(lag["state"], auto["state"]) and auto["E"] == auto["state"][0] and lag["E"] == f32(0.5)
