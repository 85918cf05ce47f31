"""The bloom pass without a device (rt_scene_bloom): the layout of rt_bloom_desc and its defaults, every
refusal (which happens before the scene touches a device) and the field it names, the wrapper's own errors and where its
methods sit, and the numpy restatement (tests/bloom_ref.py) on its own: against a second restatement written as loops
over pixels, on hand values, on both identities, on special values and on the state."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bloom_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_FIELDS = ("struct_size", "width", "height", "rgba_in", "state", "rgba_out", "pixels", "glow_out", "levels", "threshold",
           "limit", "spread", "strength", "variant")


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


frame = B.hand_frame


def geometric(spread, levels):
    return sum(spread ** k for k in range(levels))


# ----------------------------------------------------------------------------- the C ABI
def test_desc_layout_and_defaults(rt, tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof(rt_bloom_desc, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof(rt_bloom_desc));\n{body}'
                   '    printf("%d\\n%d\\n", RT_BLOOM_MAX_LEVELS, RT_BLOOM_MAX_EVENTS);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(rt.BloomDesc) == want[0] == 80
    assert [getattr(rt.BloomDesc, f).offset for f in _FIELDS] == want[1:-2]
    assert [f for f, _ in rt.BloomDesc._fields_] == list(_FIELDS)
    assert want[-2] == rt.RT_BLOOM_MAX_LEVELS == B.MAX_LEVELS == 8
    assert want[-1] == rt.RT_BLOOM_MAX_EVENTS == 2 * rt.RT_BLOOM_MAX_LEVELS == 16
    lib = rt.load_library()
    d = rt.BloomDesc()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    lib.rt_bloom_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.BloomDesc)
    assert (d.levels, d.threshold, d.limit, d.spread, d.strength, d.variant) == (5, 1.0, 64.0, 0.75, 0.125, 0)
    assert (d.width, d.height) == (0, 0)
    assert not any((d.rgba_in, d.state, d.rgba_out, d.pixels, d.glow_out))
    assert B.DEFAULTS == dict(levels=5, threshold=1.0, limit=64.0, spread=0.75, strength=0.125)
    lib.rt_bloom_desc_init(None)
    assert lib.rt_abi_version() == 1


def test_refusals_without_a_device(rt):
    """Every refusal returns RT_ERR_INVALID before the scene is used and names its field: a host-only scene, host
    buffers standing in for the device's keep their sentinel."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(1 << 14, 0x5a5a5a5a, dtype=np.uint32)
        p = (sentinel.ctypes.data + 255) & ~255
        names = ("rgba_in", "state", "rgba_out", "pixels", "glow_out")
        q = {k: p + 4096 * i for i, k in enumerate(names)}          # 16 x 8 pixels: at most 2 KiB each

        def desc(size=None, **kw):
            d = rt.BloomDesc()
            lib.rt_bloom_desc_init(C.byref(d))
            d.width, d.height = 16, 8
            for k, v in {**q, **kw}.items():
                setattr(d, k, v)
            if size is not None:
                d.struct_size = size
            return d
        assert lib.rt_scene_bloom(None, C.byref(desc()), None) == 1
        assert lib.rt_last_error().decode().startswith("rt_scene_bloom: ")
        assert lib.rt_scene_bloom(s, None, None) == 1
        nan, inf = float("nan"), float("inf")
        bad = [(dict(width=0), "width"), (dict(height=0), "height"), (dict(width=-3), "width"), (dict(height=-1), "height"),
               (dict(width=1 << 20), "width"), (dict(height=32769), "height"),
               (dict(levels=0), "levels"), (dict(levels=-1), "levels"), (dict(levels=9), "levels"),
               (dict(variant=-1), "variant"), (dict(variant=2), "variant"),
               (dict(rgba_in=0), "rgba_in"), (dict(rgba_out=0, pixels=0, glow_out=0), "rgba_out"),
               (dict(rgba_in=q["rgba_in"] + 4), "rgba_in"), (dict(rgba_in=q["rgba_in"] + 8), "rgba_in"),
               (dict(state=q["state"] + 4), "state"), (dict(state=q["state"] + 8), "state"),
               (dict(rgba_out=q["rgba_out"] + 8), "rgba_out"), (dict(pixels=q["pixels"] + 2), "pixels"),
               (dict(glow_out=q["glow_out"] + 4), "glow_out"), (dict(glow_out=q["glow_out"] + 8), "glow_out"),
               (dict(threshold=-1.0), "threshold"), (dict(threshold=nan), "threshold"), (dict(threshold=inf), "threshold"),
               (dict(limit=0.0), "limit"), (dict(limit=-1.0), "limit"), (dict(limit=nan), "limit"), (dict(limit=inf), "limit"),
               (dict(spread=-0.25), "spread"), (dict(spread=4.5), "spread"), (dict(spread=nan), "spread"),
               (dict(spread=inf), "spread"),
               (dict(strength=-0.125), "strength"), (dict(strength=nan), "strength"), (dict(strength=inf), "strength"),
               # an output that overlaps an input or another output
               (dict(rgba_out=q["rgba_in"] + 16), "rgba_in"), (dict(rgba_out=q["rgba_in"] - 16), "rgba_in"),
               (dict(rgba_out=q["state"]), "state"), (dict(rgba_out=q["state"] - 2032), "state"),
               (dict(pixels=q["rgba_in"]), "rgba_in"), (dict(pixels=q["rgba_in"] + 2044), "rgba_in"),
               (dict(pixels=q["state"] + 12), "state"), (dict(glow_out=q["rgba_in"]), "rgba_in"),
               (dict(glow_out=q["rgba_in"] - 2032), "rgba_in"), (dict(glow_out=q["state"]), "state"),
               (dict(pixels=q["rgba_out"] + 2044), "pixels"), (dict(glow_out=q["rgba_out"]), "glow_out"),
               (dict(glow_out=q["rgba_out"] + 2032), "glow_out"), (dict(glow_out=q["pixels"] - 2032), "glow_out"),
               (dict(rgba_out=0, glow_out=q["pixels"]), "glow_out"),
               # a shorter struct_size: what lies past it reads as 0
               (dict(size=rt.BloomDesc.levels.offset), "levels"), (dict(size=rt.BloomDesc.threshold.offset), "limit"),
               (dict(size=rt.BloomDesc.limit.offset), "limit"), (dict(size=rt.BloomDesc.rgba_out.offset), "levels"),
               (dict(size=rt.BloomDesc.rgba_out.offset, levels=5), "levels"), (dict(size=rt.BloomDesc.rgba_in.offset), "levels"),
               (dict(size=4), "width")]
        for kw, field in bad:
            assert lib.rt_scene_bloom(s, C.byref(desc(**kw)), None) == 1, kw
            message = lib.rt_last_error().decode()
            assert message.startswith("rt_scene_bloom: ") and field in message, (kw, message)
        import torch
        if not torch.cuda.is_available():
            # these pass the checks, which a scene without a device cannot go beyond (a HIP or no-device error)
            ok = [dict(), dict(rgba_out=q["rgba_in"]), dict(state=0), dict(rgba_out=0), dict(pixels=0), dict(glow_out=0),
                  dict(rgba_out=0, pixels=0), dict(pixels=0, glow_out=0), dict(rgba_out=0, glow_out=0),
                  dict(levels=1), dict(levels=8), dict(variant=1), dict(threshold=0.0), dict(spread=0.0), dict(spread=4.0),
                  dict(strength=0.0), dict(limit=2.0 ** -20), dict(size=0), dict(size=rt.BloomDesc.variant.offset),
                  # spread, strength and variant read as 0, which each may be
                  dict(size=rt.BloomDesc.spread.offset)]
            for kw in ok:
                assert lib.rt_scene_bloom(s, C.byref(desc(**kw)), None) in (3, 4), kw
        n = C.c_int(7)
        ms = (C.c_float * 16)()
        assert lib.rt_scene_set_bloom_timing(None, 1) == 1
        assert lib.rt_scene_set_bloom_timing(s, 1) == 0
        assert lib.rt_scene_bloom_times(s, ms, 16, C.byref(n)) == 0 and n.value == 0
        assert lib.rt_scene_bloom_times(s, None, 16, C.byref(n)) == 1
        assert lib.rt_scene_bloom_times(None, ms, 16, C.byref(n)) == 1
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_python_bloom_checks_its_arguments(rt):
    """The wrapper refuses malformed arguments itself, and without a GPU every call (no CPU fallback); the builder
    passes the defaults through; the new methods sit directly behind denoise_times."""
    import torch
    sc = rt.Scene()
    try:
        frame_ = {"rgba": None, "aov": {}}
        for kw in (dict(levels="five"), dict(levels=2.5), dict(levels=True), dict(variant="plain"), dict(threshold="high"),
                   dict(limit=[64]), dict(spread=(1, 2)), dict(strength="some"), dict(strength=None, spread=b"1")):
            name = [k for k, v in kw.items() if v is not None][0]
            with pytest.raises(rt.RtError, match="bloom: " + name):
                sc.bloom(frame_, **kw)
        with pytest.raises(rt.RtError, match="bloom: want_rgba"):
            sc.bloom(frame_, want_rgba=False, want_packed=False)
        with pytest.raises(rt.RtError):
            sc.bloom(frame_)
        with pytest.raises(TypeError):
            sc.bloom(frame_, radius=3)
        if torch.cuda.is_available():
            with pytest.raises(rt.RtError, match="bloom: the colour"):
                sc.bloom(torch.zeros(4, 4, 3))
            with pytest.raises(rt.RtError, match="bloom: state"):
                sc.bloom(torch.zeros(4, 4, 4, device="cuda"), torch.zeros(4))
        d = sc.bloom_desc(640, 360)
        assert (d.width, d.height, d.levels, d.threshold, d.limit, d.spread, d.strength, d.variant) == \
               (640, 360, 5, 1.0, 64.0, 0.75, 0.125, 0)
        d = sc.bloom_desc(8, 4, rgba_in=4096, state=8192, rgba_out=12288, pixels=16384, glow_out=20480, levels=3,
                          threshold=2.0, limit=8.0, spread=0.5, strength=0.25, variant=1)
        assert [getattr(d, f) for f in _FIELDS] == [C.sizeof(rt.BloomDesc), 8, 4, 4096, 8192, 12288, 16384, 20480, 3, 2.0, 8.0,
                                                    0.5, 0.25, 1]
        assert sc.bloom_raw(sc.bloom_desc(0, 4)) == 1
        assert sc.bloom_times() == []
        sc.set_bloom_timing(True)
        assert sc.bloom_times() == []
    finally:
        sc.close()
    names = [n for n in vars(rt.Scene) if not n.startswith("__")]
    new = ["bloom_desc", "bloom_raw", "bloom", "set_bloom_timing", "bloom_times"]
    at = names.index("denoise_times")
    assert names[at + 1:at + 7] == new + ["indirect_desc"]
    # what the existing suites hold about the order still holds
    assert names[names.index("indirect_paths_times") + 1:] == ["display_desc", "display_raw", "display", "set_display_timing",
                                                               "display_times"]
    assert not set(new) & set(names[names.index("denoise_desc"):at + 1])


# ----------------------------------------------------------------------------- the restatement against loops
@pytest.mark.parametrize("levels", [1, 2, 3, 8])
@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (3, 1), (1, 3), (5, 3), (13, 7)])
def test_the_restatement_equals_the_loops(w, h, levels):
    rgba = frame(w, h, seed=10 * w + h)
    for kw in (dict(), dict(state=[0.5, 0, 0, 1]), dict(threshold=0.25, limit=3.0, spread=1.5, strength=2.0)):
        a = B.bloom(rgba, levels=levels, **kw)
        b = B.bloom_loops(rgba, levels=levels, **kw)
        assert np.array_equal(bits(a["rgba"]), bits(b["rgba"])), kw
        assert np.array_equal(bits(a["glow"]), bits(b["glow"])), kw
        assert np.array_equal(bits(a["rgba"][..., 3]), bits(rgba[..., 3]))
        assert not a["glow"][..., 3].any()


# ----------------------------------------------------------------------------- hand values
def test_level_sizes():
    assert B.level_sizes(13, 7, 8) == [(13, 7), (7, 4), (4, 2), (2, 1), (1, 1), (1, 1), (1, 1), (1, 1), (1, 1)]
    assert B.level_sizes(3840, 2160, 5) == [(3840, 2160), (1920, 1080), (960, 540), (480, 270), (240, 135), (120, 68)]
    assert [b.shape for b in B.bloom(np.ones((7, 13, 4), dtype=f32), levels=4)["B"]] == [(4, 7, 3), (2, 4, 3), (1, 2, 3), (1, 1, 3)]


@pytest.mark.parametrize("levels", [1, 3, 8])
def test_one_pixel(levels):
    """1 x 1: every tap is the pixel, every level equals Br and T = Br sum spread^k. Threshold 0: s = 1, Br = c."""
    rgba = np.array([[[2.0, 1.0, 0.5, -7.0]]], dtype=f32)
    out = B.bloom(rgba, levels=levels, threshold=0.0, spread=0.5, strength=0.25)
    for b in out["B"]:
        assert b.shape == (1, 1, 3) and list(b[0, 0]) == [2.0, 1.0, 0.5]
    g = geometric(0.5, levels)
    assert list(out["glow"][0, 0]) == [2.0 * g, 1.0 * g, 0.5 * g, 0.0]
    assert list(out["rgba"][0, 0]) == [2.0 + 0.5 * g, 1.0 + 0.25 * g, 0.5 + 0.125 * g, -7.0]


def test_a_constant_field_blooms_to_a_constant():
    """4 everywhere: l = 4, s = 3 / 4, Br = 3; the filter's weights sum to one in powers of two, so every level is 3."""
    rgba = np.full((7, 13, 4), 4.0, dtype=f32)
    assert (B.luma(rgba) == 4).all()
    out = B.bloom(rgba, levels=3, spread=0.5)
    assert (B.bright(rgba, f32(1), f32(64)) == 3).all()
    assert all((b == 3).all() for b in out["B"])
    assert (out["glow"][..., :3] == 3 * 1.75).all() and (out["rgba"][..., :3] == 4 + 0.125 * 5.25).all()
    # the limit: on the screen's scale
    assert (B.bright(rgba, f32(1), f32(2)) == 2).all()
    assert (B.bloom(rgba, [4, 0, 0, 1], levels=1, limit=8.0)["glow"][..., :3] == 2).all()      # t = 1 / 4: Br = 3.75, lim = 2


def test_the_clamp_table():
    assert B.down_taps(5).T.tolist() == [[0, 0, 1, 2], [1, 2, 3, 4], [3, 4, 4, 4]]               # odd ws
    assert B.down_taps(4).T.tolist() == [[0, 0, 1, 2], [1, 2, 3, 3]]                             # even ws
    assert B.down_taps(1).T.tolist() == [[0, 0, 0, 0]]
    assert B.down_taps(2).T.tolist() == [[0, 0, 1, 1]]
    assert [list(map(int, v)) for v in zip(*B.up_taps(5, 3))] == [[0, 0], [0, 1], [1, 0], [1, 2], [2, 1]]
    assert [list(map(int, v)) for v in zip(*B.up_taps(4, 2))] == [[0, 0], [0, 1], [1, 0], [1, 1]]
    assert [list(map(int, v)) for v in zip(*B.up_taps(1, 1))] == [[0, 0]]
    # one row 0 0 0 0 8: the last column's taps are 3 4 4 4 -> (0 + 8 + 3 (8 + 8)) / 8 = 7; the middle's 1 2 3 4 -> 1
    row = np.zeros((1, 5, 3), dtype=f32)
    row[0, 4] = 8
    assert B.down(row)[0, :, 0].tolist() == [0, 1, 7]
    # and up from 1 7 to three pixels: 1, 0.75 + 1.75, 5.25 + 0.25
    assert B.up(np.array([[[1.0], [7.0]]], dtype=f32), 3, 1)[0, :, 0].tolist() == [1, 2.5, 5.5]


# ----------------------------------------------------------------------------- the identities
def test_nothing_above_the_threshold():
    rgba = frame(13, 7, seed=3)
    rgba[..., :3] = np.where(np.isfinite(rgba[..., :3]), np.minimum(rgba[..., :3], f32(0.9)), rgba[..., :3])
    rgba[B.luma(rgba) == np.inf] = 0
    out = B.bloom(rgba)
    assert np.isnan(rgba).any() and (rgba == 0).any()
    assert np.array_equal(bits(out["rgba"]), bits(rgba)) and not out["glow"].any()
    assert np.array_equal(out["pixels"], B.pack(rgba))


def test_a_bright_corner_leaves_the_far_corner_alone():
    rgba = frame(40, 24, seed=4, salt=False) * f32(2.0 ** -12)
    rgba[0, 0, :3] = (50, 40, 30)
    rgba[-1, -1, :3] = (-0.0, np.nan, 0.25)
    rgba[-2, -1, :3] = (np.inf, 1.0, 1.0)                    # not finite: does not bloom
    out = B.bloom(rgba, levels=2)
    assert np.array_equal(bits(out["rgba"][8:]), bits(rgba[8:])) and not out["glow"][8:].any()
    assert (out["glow"][:4, :4, :3] > 0).all() and (out["rgba"][:4, :4, :3] > rgba[:4, :4, :3]).all()
    assert bits(out["rgba"][-1, -1]).tolist() == bits(rgba[-1, -1]).tolist()


# ----------------------------------------------------------------------------- special values, the state
@pytest.mark.parametrize("levels,spread", [(1, 0.75), (5, 0.75), (8, 2.0)])
def test_special_values_give_a_finite_bounded_glow(levels, spread):
    rgba = frame(13, 7, seed=5)
    assert np.isnan(rgba).any() and np.isinf(rgba).any() and (rgba < 0).any() and (rgba == f32(1e30)).any()
    out = B.bloom(rgba, levels=levels, spread=spread)
    glow = out["glow"]
    assert np.isfinite(glow).all() and (glow >= 0).all()
    assert glow.max() <= 64 * geometric(spread, levels) * (1 + 2.0 ** -20) and glow.max() > 0
    assert np.array_equal(bits(out["rgba"][..., 3]), bits(rgba[..., 3]))


def test_the_state():
    rgba = frame(13, 7, seed=6)
    plain = B.bloom(rgba)
    for state in (None, [0, 0, 0, 0], [4, 1, 1, 0], [4, 1, 1, 0.5], [4, 1, 1, np.nan]):
        out = B.bloom(rgba, state)
        assert np.array_equal(bits(out["rgba"]), bits(plain["rgba"])) and out["t"] == 1 and out["lim"] == 64
    out = B.bloom(rgba, [4, 9, 9, 1])
    same = B.bloom(rgba, threshold=0.25, limit=16.0)
    assert out["t"] == 0.25 and out["lim"] == 16
    assert np.array_equal(bits(out["rgba"]), bits(same["rgba"])) and np.array_equal(bits(out["glow"]), bits(same["glow"]))
    assert not np.array_equal(bits(out["glow"]), bits(plain["glow"]))
    # a state of no use (zero, negative or NaN exposure marked valid) is defined too: nothing blooms, or to the bit
    for e in (0.0, np.nan):
        out = B.bloom(rgba, [e, 0, 0, 1])
        assert not out["glow"].any() and np.array_equal(bits(out["rgba"]), bits(rgba))
