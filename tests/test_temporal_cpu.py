"""Temporal accumulation without a device (rt_scene_temporal): the numpy restatement
(tests/temporal_ref.py) checked on its own against properties that follow from the definition, on inputs formed on
the CPU (the oracle's colour, CastRef.nearest's guides, the oracle's primary rays); rt_view_terms against the oracle's
primary-ray construction; the layout of rt_temporal_desc, its defaults, and the refusals, which happen before the
scene touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as T
# WIDE_HIT_FLOOR and WIDE_SEGMENT: for the suites that take the wide path's constants from this module
from postpass import (TEMPORAL_FIELDS, WIDE_BLOCK, WIDE_CAMS, WIDE_FIRST, WIDE_HIT_FLOOR, WIDE_HISTORY_FLOOR,  # noqa: F401
                      WIDE_SEGMENT, View, bits as _bits, block_shares, cam as _cam)
from scenes import Inputs, mixed_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_FIELDS = TEMPORAL_FIELDS


def _pair(rt, oracle, inp, w, h):
    """The default camera, then the same camera half a unit to the side."""
    return View(rt, oracle, inp, _cam(rt, 4, 3, 10, 180, -20), w, h), View(rt, oracle, inp, _cam(rt, 4.5, 3, 10, 180, -20), w, h)


@pytest.fixture(scope="module")
def spheres(rt, oracle):
    return _pair(rt, oracle, Inputs(rt, 256), 160, 90)


@pytest.fixture(scope="module")
def mixed(rt, oracle):
    return _pair(rt, oracle, mixed_scene(rt), 160, 96)


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
@pytest.mark.parametrize("max_history", [2, 32])
def test_a_standing_camera_gives_the_running_mean(request, scene, max_history):
    """Identical views: k calls give n = min(k, max_history) on hits and 1 on sky, and (while n = k) a colour within
    4 k ulp of the largest component of the binary64 mean of the k inputs: each step H + (c - H) / n has three
    roundings of values no larger than that component."""
    v, _ = request.getfixturevalue(scene)
    hit = v.cur["id"][..., 0] >= 0
    rng = np.random.default_rng(5)
    hist, frames = None, []
    for k in range(1, 5):
        cur = dict(v.cur)
        cur["rgba"] = v.cur["rgba"].copy()
        cur["rgba"][..., :3] = (v.cur["rgba"][..., :3] * rng.uniform(0.5, 1.0, (v.h, v.w, 3)).astype(f32)).astype(f32)
        frames.append(cur["rgba"][..., :3].astype(np.float64))
        hist = T.temporal(cur, hist, v.O, v.D, v.terms, v.terms, v.aspect, True, max_history=max_history, details=True)
        n = hist["rgba"][..., 3]
        assert (n[hit] == min(k, max_history)).all() and (n[~hit] == 1).all()
        assert np.array_equal(hist["has_history"], hit if k > 1 else np.zeros_like(hit))
        assert np.array_equal(_bits(hist["rgba"][~hit, :3]), _bits(cur["rgba"][~hit, :3]))
        assert np.array_equal(hist["packed"], R.pack(hist["rgba"]))
        if k <= max_history:
            mean = np.mean(frames, axis=0)
            ulp = np.spacing(mean.max(axis=-1).astype(f32)).astype(np.float64)
            err = np.abs(hist["rgba"][..., :3].astype(np.float64) - mean).max(axis=-1)
            assert (err[hit] <= 4 * k * ulp[hit]).all()
            Ym = np.mean([R.luma(f.astype(f32)).astype(np.float64) for f in frames], axis=0)
            assert np.abs(hist["moments"][..., 0] - Ym)[hit].max() <= 4 * k * 2.0 ** -23 * max(1.0, Ym.max())


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
def test_a_sideways_step(request, scene):
    """After a sideways camera step every pixel with history has 1 < n <= 2 and a colour between the min and max of c
    and its counted taps; and the pair of cameras gives both classes of hit pixels a share of at least 5 %."""
    a, b = request.getfixturevalue(scene)
    h0 = a.onto(None, a)
    assert (h0["rgba"][..., 3] == 1).all() and not h0["has_history"].any()
    r = b.onto(h0, a)
    hit = b.cur["id"][..., 0] >= 0
    has = r["has_history"]
    assert not (has & ~hit).any()
    with_share, without_share = (has & hit).sum() / hit.sum(), (~has & hit).sum() / hit.sum()
    assert with_share >= 0.05 and without_share >= 0.05, (with_share, without_share)
    n = r["rgba"][..., 3]
    assert (n[has] > 1).all() and (n[has] <= 2).all() and (n[~has] == 1).all()
    c = b.cur["rgba"][..., :3]
    lo, hi = c.copy(), c.copy()
    for counted, pc in r["taps"]:
        lo = np.where(counted[..., None], np.minimum(lo, pc[..., :3]), lo)
        hi = np.where(counted[..., None], np.maximum(hi, pc[..., :3]), hi)
    out = r["rgba"][..., :3]
    slack = 8 * 2.0 ** -24                       # four products, three sums, a division, the blend: relative roundings
    assert (out[has] >= lo[has] * (1 - slack) - 1e-30).all() and (out[has] <= hi[has] * (1 + slack) + 1e-30).all()
    assert np.array_equal(_bits(out[~has]), _bits(c[~has]))
    Y = R.luma(c)
    assert np.array_equal(_bits(r["moments"][~has]), _bits(np.stack([Y, (Y * Y).astype(f32)], axis=-1)[~has]))


def test_the_wide_inputs_show_spheres_beyond_the_first_group_of_eight(rt, oracle):
    """Conditions on the inputs of the wide GPU tests (test_temporal_gpu, test_tmotion_gpu, test_vdenoise_gpu), from
    the restatement alone, so that those tests cannot pass on sky: 256 spheres, the first two cameras of WIDE_CAMS.
    The restatement's values -- 576 x 36: 9 tile columns, hit share 0.70, has_history share 0.57, 0.84 in column 8;
    1088 x 36: 17 tile columns, hit share 0.70, has_history share 0.46, the smallest of columns 8 .. 16 is column 12
    with 0.17; 2100 x 36: 9 row segments of 256, hit share 0.68 and 0.59 in columns >= 2048. The floors (0.1 of a
    column's pixels with history, 0.3 of the pixels hit) lie below the smallest of these by a factor of 1.7 at least."""
    inp = Inputs(rt, 256)
    for w, tiles in ((576, 9), (1088, 17)):
        assert -(-w // WIDE_BLOCK) == tiles and ((tiles + 7) >> 3) << 3 > 8            # nsegp = 16, 24
        a, b = (View(rt, oracle, inp, _cam(rt, *c), w, 36) for c in WIDE_CAMS[:2])
        r = b.onto(a.onto(None, a), a)
        shares = block_shares(r["has_history"])
        print(w, "hit share", (b.cur["id"][..., 0] >= 0).mean(), "has_history share", r["has_history"].mean(), "columns 8 ..:", shares)
        assert len(shares) == tiles - WIDE_FIRST and min(shares) >= WIDE_HISTORY_FLOOR, (w, shares)
    w = 2100
    assert (-(-w // 256) + 7) >> 3 == 2                                                # nseg8
    b = View(rt, oracle, inp, _cam(rt, *WIDE_CAMS[1]), w, 36)
    hit = b.cur["id"][..., 0] >= 0
    print(w, "hit share", hit.mean(), "in columns >= 2048:", hit[:, WIDE_SEGMENT:].mean())
    assert hit[:, WIDE_SEGMENT:].mean() >= WIDE_HIT_FLOOR


def test_a_camera_turned_round_has_no_history(rt, oracle, spheres):
    a, _ = spheres
    h0 = a.onto(None, a)
    back = rt.view_terms(a.w, a.h, a.aspect, _cam(rt, 4, 3, 10, 0, 20))
    r = T.temporal(a.cur, h0, a.O, a.D, a.terms, back, a.aspect, False, details=True)
    assert not r["has_history"].any() and (r["rgba"][..., 3] == 1).all()
    assert np.array_equal(_bits(r["rgba"][..., :3]), _bits(a.cur["rgba"][..., :3]))


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
def test_the_tolerances_decide_which_taps_count(request, scene):
    a, b = request.getfixturevalue(scene)
    h0 = a.onto(None, a)
    base = b.onto(h0, a)

    def counted(r):
        return np.stack([t[0] for t in r["taps"]])
    for kw in (dict(depth_tolerance=0.002), dict(depth_tolerance=0.5), dict(normal_cos_min=0.999), dict(normal_cos_min=0.0)):
        other = counted(b.onto(h0, a, **kw))
        assert (other != counted(base)).any(), kw
        tighter = kw.get("depth_tolerance", 0.02) < 0.02 or kw.get("normal_cos_min", 0.9) > 0.9
        assert not ((other & ~counted(base)) if tighter else (counted(base) & ~other)).any(), kw
    if scene == "mixed":
        # a cube's faces share an id, and the reference's cube normal turns across each face: the normal test alone
        # separates a cube's pixels from their neighbours of the same cube
        cube = b.cur["id"][..., 0] == 3                   # RT_HIT_CUBE
        assert (counted(base) & ~counted(b.onto(h0, a, normal_cos_min=0.999)))[:, cube].any()


def test_view_terms_are_the_oracles_view(rt, oracle):
    """The origin is the oracle's, bit for bit; and with the rotation terms a point on any of the oracle's primary rays
    lands, through the definition's own reprojection, on the ray's pixel."""
    inp = Inputs(rt, 8)
    from test_reflect_cpu import Composer
    w, h = 48, 27
    for cam in (_cam(rt, 4, 3, 10, 180, -20), _cam(rt, -2, 1.5, 3, 37, 11), _cam(rt, 0, 0, 0, 0, 0), _cam(rt, 1, 2, 3, -95, 60)):
        comp = Composer(oracle, None, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, cam, inp.aspect)
        O, D = comp.primary(w, h, 0, h)
        terms = rt.view_terms(w, h, inp.aspect, cam)
        assert terms.dtype == np.float32 and terms.shape == (7,)
        assert np.array_equal(_bits(O), _bits(np.broadcast_to(terms[:3], O.shape)))
        assert abs(float(terms[3]) ** 2 + float(terms[4]) ** 2 - 1) < 1e-6 and abs(float(terms[5]) ** 2 + float(terms[6]) ** 2 - 1) < 1e-6
        for t in (0.5, 7.0, 300.0):
            fx, fy, qq, ok = T.reproject(np.full((h, w), t, dtype=f32), O, D, terms, inp.aspect, w, h)
            yy, xx = np.mgrid[0:h, 0:w]
            assert ok.all()
            assert np.abs(fx - xx).max() < 1e-3 and np.abs(fy - yy).max() < 1e-3
            assert np.abs(qq / (t * t) - 1).max() < 1e-5
    lib = rt.load_library()
    out = (C.c_float * 7)()
    cam = rt.default_camera()
    assert lib.rt_view_terms(0, 4, 1.0, C.byref(cam), out) == 1
    assert lib.rt_view_terms(4, 4, 1.0, None, out) == 1
    assert lib.rt_view_terms(4, 4, 1.0, C.byref(cam), None) == 1


# ----------------------------------------------------------------------------- the C ABI
def test_desc_layout_and_defaults(rt, tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof(rt_temporal_desc, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof(rt_temporal_desc));\n{body}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(rt.TemporalDesc) == want[0]
    assert [getattr(rt.TemporalDesc, f).offset for f in _FIELDS] == want[1:]
    assert [f for f, _ in rt.TemporalDesc._fields_] == list(_FIELDS)
    lib = rt.load_library()
    d = rt.TemporalDesc()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    lib.rt_temporal_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.TemporalDesc)
    assert (d.max_history, d.reset, d.variant) == (32, 0, 0)
    assert f32(d.depth_tolerance) == f32(0.02) and f32(d.normal_cos_min) == f32(0.9)
    assert (d.width, d.height, d.aspect, d.prev_aspect) == (0, 0, 0.0, 0.0)
    assert bytes(d.cam) == bytes(36) and bytes(d.prev_cam) == bytes(36)
    assert not any((d.rgba_in, d.depth, d.normal, d.id, d.prev_rgba, d.prev_depth, d.prev_normal, d.prev_id,
                    d.prev_moments, d.rgba_out, d.moments_out, d.pixels))
    assert rt.RT_TEMPORAL_MAX_HISTORY == 256
    assert T.DEFAULTS == dict(max_history=32, depth_tolerance=0.02, normal_cos_min=0.9)
    assert lib.rt_abi_version() == 1


def test_refusals_without_a_device(rt):
    """Every refusal returns RT_ERR_INVALID before the scene is used: a host-only scene, host buffers standing in for
    the device's keep their sentinel."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(1 << 16, 0x5a5a5a5a, dtype=np.uint32)
        p = (sentinel.ctypes.data + 255) & ~255
        names = ("rgba_in", "depth", "normal", "id", "prev_rgba", "prev_depth", "prev_normal", "prev_id", "prev_moments",
                 "rgba_out", "moments_out", "pixels")
        ptrs = {k: p + 4096 * i for i, k in enumerate(names)}       # 16 x 8 pixels: at most 2 KiB each

        def desc(**kw):
            d = rt.TemporalDesc()
            lib.rt_temporal_desc_init(C.byref(d))
            d.width, d.height = 16, 8
            d.aspect = d.prev_aspect = 1.5
            d.cam = d.prev_cam = rt.default_camera()
            for k, v in {**ptrs, **kw}.items():
                setattr(d, k, v)
            return d
        assert lib.rt_scene_temporal(None, C.byref(desc()), None) == 1
        assert lib.rt_scene_temporal(s, None, None) == 1
        q = ptrs
        bad = [dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20), dict(height=32769),
               dict(rgba_in=0), dict(depth=0), dict(normal=0), dict(id=0), dict(rgba_out=0),
               dict(prev_rgba=0), dict(prev_depth=0), dict(prev_normal=0), dict(prev_id=0), dict(prev_moments=0),
               dict(rgba_in=q["rgba_in"] + 4), dict(rgba_in=q["rgba_in"] + 8), dict(normal=q["normal"] + 8),
               dict(rgba_out=q["rgba_out"] + 12), dict(prev_rgba=q["prev_rgba"] + 4), dict(prev_normal=q["prev_normal"] + 8),
               dict(id=q["id"] + 4), dict(prev_id=q["prev_id"] + 4), dict(prev_moments=q["prev_moments"] + 4),
               dict(moments_out=q["moments_out"] + 4), dict(depth=q["depth"] + 2), dict(prev_depth=q["prev_depth"] + 1),
               dict(pixels=q["pixels"] + 1),
               dict(max_history=0), dict(max_history=257), dict(max_history=-1), dict(variant=-1), dict(variant=2),
               dict(depth_tolerance=0.0), dict(depth_tolerance=-0.02), dict(depth_tolerance=float("nan")),
               dict(depth_tolerance=float("inf")), dict(normal_cos_min=-0.1), dict(normal_cos_min=1.5),
               dict(normal_cos_min=float("nan")), dict(normal_cos_min=float("inf")),
               # an output that overlaps an input: the same buffer, its tail, its head; every output against some input
               dict(rgba_out=q["rgba_in"]), dict(rgba_out=q["prev_rgba"] + 2032), dict(rgba_out=q["prev_rgba"] - 2032),
               dict(rgba_out=q["normal"]), dict(rgba_out=q["depth"]), dict(moments_out=q["prev_moments"]),
               dict(moments_out=q["id"] + 8), dict(pixels=q["depth"]), dict(pixels=q["prev_id"] + 1020),
               dict(pixels=q["rgba_out"] + 16), dict(moments_out=q["rgba_out"])]
        for kw in bad:
            assert lib.rt_scene_temporal(s, C.byref(desc(**kw)), None) == 1, kw
            assert b"rt_scene_temporal" in lib.rt_last_error()
        # reset lifts the need for prev_*, but not for the current buffers
        assert lib.rt_scene_temporal(s, C.byref(desc(reset=1, depth=0)), None) == 1
        assert lib.rt_scene_temporal(s, C.byref(desc(reset=1, rgba_out=q["rgba_in"])), None) == 1
        import torch
        if not torch.cuda.is_available():
            # these pass the checks, which a scene without a device cannot go beyond (a HIP or no-device error)
            none = {k: 0 for k in names if k.startswith("prev_")}
            assert lib.rt_scene_temporal(s, C.byref(desc(reset=1, **none)), None) in (3, 4)
            assert lib.rt_scene_temporal(s, C.byref(desc(prev_moments=0, moments_out=0)), None) in (3, 4)
            assert lib.rt_scene_temporal(s, C.byref(desc(rgba_out=q["prev_rgba"] + 2048)), None) in (3, 4)   # adjacent
        n = C.c_int(7)
        ms = (C.c_float * 2)()
        assert lib.rt_scene_set_temporal_timing(None, 1) == 1
        assert lib.rt_scene_set_temporal_timing(s, 1) == 0
        assert lib.rt_scene_temporal_times(s, ms, 2, C.byref(n)) == 0 and n.value == 0
        assert lib.rt_scene_temporal_times(s, None, 2, C.byref(n)) == 1
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_python_temporal_checks_its_frame(rt):
    """A frame without colour or guides is refused by the wrapper (and without a GPU every call is: no CPU fallback)."""
    sc = rt.Scene()
    try:
        with pytest.raises(rt.RtError):
            sc.temporal({"rgba": None, "aov": {}})
    finally:
        sc.close()
