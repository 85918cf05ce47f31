"""Guided upsampling without a device (rt_scene_upsample): the numpy restatement (tests/upsample_ref.py)
checked on its own against properties that follow from the definition, on inputs formed on the CPU (the oracle's
colour and CastRef.nearest's guides at both sizes, the composed reflective frame); the error relations DESIGN.md 6l
reports; the layout of rt_upsample_desc, its defaults, and the refusals, which happen before the scene touches a
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import upsample_ref as U
from postpass import bits as _bits, mae, mirror_k
from scenes import Inputs, mixed_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_FIELDS = ("struct_size", "width", "height", "lo_width", "lo_height", "rgba_lo", "depth_lo", "normal_lo", "albedo_lo",
           "id_lo", "depth", "normal", "albedo", "id", "base", "rgba_out", "pixels", "source", "sphere_select",
           "n_sphere_select", "plane_select", "n_plane_select", "cube_select", "n_cube_select", "use_tables",
           "normal_shift", "sigma_depth", "demodulate", "variant")


def frame(rt, oracle, inp, w, h):
    rgba, depth, normal, albedo, ids = R.oracle_inputs(rt, oracle, inp, w, h)
    return dict(rgba=rgba, depth=depth, normal=normal, albedo=albedo, id=ids)


@pytest.fixture(scope="module")
def plain(rt, oracle):
    inp = Inputs(rt, 256)
    return frame(rt, oracle, inp, 160, 90), frame(rt, oracle, inp, 80, 45)


@pytest.fixture(scope="module")
def mixed(rt, oracle):
    inp = mixed_scene(rt)
    return frame(rt, oracle, inp, 160, 96), frame(rt, oracle, inp, 80, 48)


@pytest.fixture(scope="module")
def reflective(rt, oracle, plain):
    """(hi, lo, full): the plain pair with lo's colour replaced by the composed reflective frame (k = 0.5 on every
    fourth sphere, depth 2) at 80 x 45, and the composed frame at 160 x 90."""
    from test_reflect_cpu import composer_for
    hi, lo = plain
    comp = composer_for(oracle, rt, Inputs(rt, 256))
    k = mirror_k(256)
    full, _ = comp.render(160, 90, k, 2)
    low, _ = comp.render(80, 45, k, 2)
    lo = dict(lo, rgba=low)
    return hi, lo, full, {"sphere": (k > 0).astype(np.uint8)}


# ----------------------------------------------------------------------------- properties of the definition
@pytest.mark.parametrize("scene", ["plain", "mixed"])
def test_sky_and_unselected_pixels_carry_the_base(request, scene):
    hi, lo = request.getfixturevalue(scene)
    H, W = hi["depth"].shape
    rng = np.random.default_rng(3)
    base = rng.uniform(-2, 2, (H, W, 4)).astype(f32)
    base[0, 0] = (np.nan, np.inf, -np.inf, -0.0)
    select = {"sphere": [1, 0] * 64, "cube": [0, 1]}        # shorter than the scene, and no plane table
    r = U.upsample(hi, lo, base=base, select=select, details=True)
    sel = r["selected"]
    kind, index = hi["id"][..., 0], hi["id"][..., 1]
    want = ((kind == 1) & (index < 128) & (index % 2 == 0)) | ((kind == 3) & (index == 1))
    assert ((kind == 1) & (index >= 128)).any()
    assert np.array_equal(sel, want)
    keep = r["source"] != 1
    assert (~sel).any() and sel.any() and ((kind < 0).any() or scene == "mixed")   # the mixed scene's planes leave no sky
    assert np.array_equal(_bits(r["rgba"][keep]), _bits(base[keep]))
    assert (r["source"][~sel] == 0).all() and (r["source"][kind < 0] == 0).all()
    assert np.array_equal(r["packed"], R.pack(r["rgba"]))
    # no tables: every hit pixel is selected
    r = U.upsample(hi, lo, base=base, details=True)
    assert np.array_equal(r["selected"], kind >= 0)
    assert np.array_equal(_bits(r["rgba"][kind < 0]), _bits(base[kind < 0]))


@pytest.mark.parametrize("scene", ["plain", "mixed"])
@pytest.mark.parametrize("demodulate", [True, False])
def test_equal_sizes_return_the_pixels_own_value(request, scene, demodulate):
    """W = w with identical guides: the only tap with a factor > 0 is the pixel itself, b = 1, e_n = m^(2^shift) of
    N.N, e_z = D / (D + 0) = 1: the result is ((wq I) / wq) A."""
    hi, _ = request.getfixturevalue(scene)
    r = U.upsample(hi, hi, demodulate=demodulate, details=True)
    hit = hi["id"][..., 0] >= 0
    N = hi["normal"][..., :3]
    with np.errstate(all="ignore"):
        m = U._max(((N[..., 0] * N[..., 0] + N[..., 1] * N[..., 1]).astype(f32) + N[..., 2] * N[..., 2]).astype(f32), f32(0))
        for _ in range(5):
            m = (m * m).astype(f32)
        wq = ((f32(1) * m).astype(f32) * f32(1)).astype(f32)
        I = R.demodulated(hi["rgba"], hi["albedo"]) if demodulate else hi["rgba"][..., :3]
        C = ((wq[..., None] * I).astype(f32) / wq[..., None]).astype(f32)
        if demodulate:
            C = (C * hi["albedo"][..., :3]).astype(f32)
    ok = hit & (wq > 0)
    assert ok.sum() >= 0.95 * hit.sum()
    assert (r["source"][ok] == 1).all() and (r["source"][hit & ~ok] == 2).all() and (r["source"][~hit] == 0).all()
    assert np.array_equal(_bits(r["rgba"][ok, :3]), _bits(C[ok]))
    assert (r["rgba"][ok, 3] == 1).all()
    # not upsampled, no base: the bilinear mean of one tap with b = 1, (1 c) / 1
    assert np.array_equal(_bits(r["rgba"][~ok, :3]), _bits(hi["rgba"][~ok, :3]))


@pytest.mark.parametrize("scene", ["plain", "mixed"])
def test_a_constant_colour_stays_constant(request, scene):
    """Within the rounding of one weighted mean: four products and three sums of values of one sign, a division: the
    result is within 8 ulp of the constant."""
    hi, lo = request.getfixturevalue(scene)
    const = np.array([0.3, 0.55, 0.8, 1.0], dtype=f32)
    lo = dict(lo, rgba=np.broadcast_to(const, lo["rgba"].shape).copy())
    r = U.upsample(hi, lo, demodulate=False)
    err = np.abs(r["rgba"][..., :3].astype(np.float64) - const[:3].astype(np.float64))
    assert (err <= 8 * np.spacing(const[:3]).astype(np.float64)).all()
    assert (r["rgba"][..., 3] == 1).all()


@pytest.mark.parametrize("scene", ["plain", "mixed"])
@pytest.mark.parametrize("demodulate", [True, False])
def test_an_upsampled_pixel_lies_within_its_counting_taps(request, scene, demodulate):
    hi, lo = request.getfixturevalue(scene)
    r = U.upsample(hi, lo, demodulate=demodulate, details=True)
    up = r["source"] == 1
    lo_v = np.full(up.shape + (3,), np.inf, dtype=f32)
    hi_v = np.full(up.shape + (3,), -np.inf, dtype=f32)
    counted = np.zeros(up.shape, dtype=int)
    for ok, I, wq, b, fok in r["taps"]:
        lo_v = np.where(ok[..., None], np.minimum(lo_v, I), lo_v)
        hi_v = np.where(ok[..., None], np.maximum(hi_v, I), hi_v)
        counted += ok
        assert not (ok & ~r["selected"]).any()
    assert np.array_equal(up, counted > 0)
    assert np.array_equal(r["source"] == 2, r["selected"] & (counted == 0))
    assert np.array_equal(r["source"] == 0, ~r["selected"])
    A = hi["albedo"][..., :3] if demodulate else f32(1)
    slack = 8 * 2.0 ** -24                      # the weighted mean's roundings and the product with the albedo
    out = r["rgba"][..., :3]
    with np.errstate(all="ignore"):
        lo_c, hi_c = (lo_v * A).astype(f32), (hi_v * A).astype(f32)
    assert (out[up] >= lo_c[up] * (1 - slack) - 1e-30).all() and (out[up] <= hi_c[up] * (1 + slack) + 1e-30).all()
    assert 0.5 < up.sum() / r["selected"].sum() <= 1


def test_the_bilinear_fallback_follows_the_closed_form(plain):
    """W = 2 w: the factors are 9/16, 3/16, 3/16, 1/16 in an order that depends on the pixel's parity; at the border
    the taps outside drop out of both sums."""
    hi, lo = plain
    c = lo["rgba"][..., :3]
    h, w = c.shape[:2]
    got = U.bilinear(lo["rgba"], 2 * w, 2 * h)
    for (x, y) in ((0, 0), (1, 0), (5, 7), (6, 8), (2 * w - 1, 2 * h - 1), (2 * w - 1, 3), (4, 2 * h - 1), (77, 30)):
        x0, y0 = (x + 1) // 2 - 1, (y + 1) // 2 - 1
        ax, ay = (f32(0.75), f32(0.25))[x & 1], (f32(0.75), f32(0.25))[y & 1]
        s, sw = np.zeros(3, dtype=f32), f32(0)
        for k in range(4):
            tx, ty = x0 + (k & 1), y0 + (k >> 1)
            b = f32((ax if k & 1 else f32(1) - ax) * (ay if k & 2 else f32(1) - ay))
            if 0 <= tx < w and 0 <= ty < h and b > 0:
                s = (s + (b * c[ty, tx]).astype(f32)).astype(f32)
                sw = f32(sw + b)
        assert np.array_equal(_bits((s / sw).astype(f32)), _bits(got[y, x])), (x, y)
    x0, ax = U.positions(2 * w, w)
    assert np.array_equal(x0, (np.arange(2 * w) + 1) // 2 - 1) and set(ax.tolist()) == {0.25, 0.75}
    for W, ww in ((96, 32), (96, 64), (161, 81), (256, 64), (7, 7), (3840, 1920)):
        x0, ax = U.positions(W, ww)
        assert x0.min() >= -1 and x0.max() <= ww - 1 and (ax >= 0).all() and (ax < 1).all()
        # at least one tap of every pixel is inside with a factor > 0
        assert (((x0 >= 0) & (ax < 1)) | ((x0 + 1 < ww) & (ax > 0))).all()


def test_nan_and_inf_guides_poison_only_their_own_pixels(plain):
    hi, lo = plain
    base = hi["rgba"]
    ref = U.upsample(hi, lo, base=base)
    H, W = hi["depth"].shape
    for bad in (np.nan, np.inf, -np.inf):
        # on the hi side: that pixel alone changes, to base with source 2
        for key in ("depth", "normal"):
            h2 = dict(hi, **{key: hi[key].copy()})
            ys, xs = np.nonzero(ref["source"] == 1)
            y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
            h2[key][y, x] = bad
            r = U.upsample(h2, lo, base=base)
            diff = (_bits(r["rgba"]) != _bits(ref["rgba"])).any(axis=-1) | (r["source"] != ref["source"])
            diff[y, x] = False
            assert not diff.any(), (key, bad)
            assert r["source"][y, x] == 2 and np.array_equal(_bits(r["rgba"][y, x]), _bits(base[y, x])), (key, bad)
        # on the lo side: only the hi pixels that have the lo pixel among their four taps can change
        for key in ("depth", "normal", "rgba"):
            l2 = dict(lo, **{key: lo[key].copy()})
            qy, qx = 30, 40
            l2[key][qy, qx] = bad
            r = U.upsample(hi, l2, base=base)
            diff = (_bits(r["rgba"]) != _bits(ref["rgba"])).any(axis=-1) | (r["source"] != ref["source"])
            near = np.zeros((H, W), dtype=bool)
            near[2 * qy - 1:2 * qy + 3, 2 * qx - 1:2 * qx + 3] = True
            assert not (diff & ~near).any(), (key, bad)
            if key != "rgba":
                assert np.isfinite(r["rgba"]).all(), (key, bad)


# ----------------------------------------------------------------------------- the reflective frame and the figures
def test_unselected_pixels_equal_the_full_resolution_reflective_frame(reflective):
    hi, lo, full, select = reflective
    r = U.upsample(hi, lo, base=hi["rgba"], select=select, demodulate=False, details=True)
    sel = r["selected"]
    assert 500 < sel.sum() < 0.25 * sel.size
    assert np.array_equal(_bits(r["rgba"][~sel]), _bits(full[~sel]))
    assert np.array_equal(r["packed"][~sel], R.pack(full)[~sel])
    assert (mirror_k(256)[hi["id"][sel][:, 1]] > 0).all()


def test_the_error_relations(plain, mixed, reflective):
    """Mean absolute error per channel against the full-resolution frame (DESIGN.md 6l gives the figures)."""
    hi, lo = plain
    W, H = 160, 90
    bil = np.concatenate([U.bilinear(lo["rgba"], W, H), np.ones((H, W, 1), dtype=f32)], axis=-1)
    e_bil = mae(bil, hi["rgba"])
    e_nobase = mae(U.upsample(hi, lo)["rgba"], hi["rgba"])
    r = U.upsample(hi, lo, base=hi["rgba"])
    e_base = mae(r["rgba"], hi["rgba"])
    hit = hi["id"][..., 0] >= 0
    print("plain 160x90 <- 80x45 demodulated: no base", e_nobase, "with base", e_base, "bilinear", e_bil,
          "hit pixels with a counting tap", float((r["source"][hit] == 1).mean()))
    assert e_base < 0.25 * e_bil
    assert (r["source"][hit] == 2).mean() <= 0.01 and not (r["source"][~hit] != 0).any()

    mh, ml = mixed
    e_mix = mae(U.upsample(mh, ml)["rgba"], mh["rgba"])
    e_mix_bil = mae(U.bilinear(ml["rgba"], 160, 96), mh["rgba"])
    print("mixed 160x96 <- 80x48 demodulated:", e_mix, "bilinear", e_mix_bil)
    assert e_mix < 0.5 * e_mix_bil

    hi, lo, full, select = reflective
    r = U.upsample(hi, lo, base=hi["rgba"], select=select, demodulate=False, details=True)
    sel = r["selected"]
    bil = U.bilinear(lo["rgba"], W, H)
    e_up, e_plain, e_bil = mae(r["rgba"], full), mae(hi["rgba"], full), mae(bil, full)
    m_up, m_plain, m_bil = mae(r["rgba"], full, sel), mae(hi["rgba"], full, sel), mae(bil, full, sel)
    print("reflective 160x90 <- 80x45: this pass", e_up, "bilinear", e_bil, "the plain frame", e_plain,
          "; on the", int(sel.sum()), "mirror pixels:", m_up, m_bil, m_plain,
          "; selected without a tap", int((r["source"] == 2).sum()))
    assert e_up < 0.75 * e_plain and e_up < 0.3 * e_bil
    assert m_up < m_bil
    assert (r["source"][sel] == 2).mean() <= 0.01


def test_the_mirror_pixels_at_320x180(rt, oracle, plain):
    """The reflective case one size up, 320 x 180 <- 160 x 90 (the lo guides are the plain fixture's hi guides): on
    the mirror pixels the pass is strictly below bilinear."""
    from test_reflect_cpu import composer_for
    inp = Inputs(rt, 256)
    hi = frame(rt, oracle, inp, 320, 180)
    comp = composer_for(oracle, rt, inp)
    k = mirror_k(256)
    full, _ = comp.render(320, 180, k, 2)
    low, _ = comp.render(160, 90, k, 2)
    lo = dict(plain[0], rgba=low)
    r = U.upsample(hi, lo, base=hi["rgba"], select={"sphere": (k > 0).astype(np.uint8)}, demodulate=False, details=True)
    sel = r["selected"]
    bil = U.bilinear(low, 320, 180)
    m_up, m_bil, m_plain = mae(r["rgba"], full, sel), mae(bil, full, sel), mae(hi["rgba"], full, sel)
    print("reflective 320x180 <- 160x90 on the", int(sel.sum()), "mirror pixels:", m_up, m_bil, m_plain,
          "; whole frame", mae(r["rgba"], full), mae(bil, full), mae(hi["rgba"], full))
    assert m_up < m_bil
    assert np.array_equal(_bits(r["rgba"][~sel]), _bits(full[~sel]))
    assert (r["source"][sel] == 2).mean() <= 0.01


# ----------------------------------------------------------------------------- the C ABI
def test_desc_layout_and_defaults(rt, tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof(rt_upsample_desc, {f}));\n' for f in _FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof(rt_upsample_desc));\n{body}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert C.sizeof(rt.UpsampleDesc) == want[0]
    assert [getattr(rt.UpsampleDesc, f).offset for f in _FIELDS] == want[1:]
    assert [f for f, _ in rt.UpsampleDesc._fields_] == list(_FIELDS)
    lib = rt.load_library()
    d = rt.UpsampleDesc()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    lib.rt_upsample_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.UpsampleDesc)
    assert (d.use_tables, d.normal_shift, d.demodulate, d.variant) == (0, 5, 1, 0)
    assert f32(d.sigma_depth) == f32(0.05)
    assert (d.width, d.height, d.lo_width, d.lo_height) == (0, 0, 0, 0)
    assert (d.n_sphere_select, d.n_plane_select, d.n_cube_select) == (0, 0, 0)
    assert not any((d.rgba_lo, d.depth_lo, d.normal_lo, d.albedo_lo, d.id_lo, d.depth, d.normal, d.albedo, d.id, d.base,
                    d.rgba_out, d.pixels, d.source, d.sphere_select, d.plane_select, d.cube_select))
    assert U.DEFAULTS == dict(normal_shift=5, sigma_depth=0.05, demodulate=True)
    assert lib.rt_abi_version() == 1


def test_refusals_without_a_device(rt):
    """Every refusal returns RT_ERR_INVALID before the scene is used: a host-only scene, host buffers standing in for
    the device's keep their sentinel."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(1 << 16, 0x5a5a5a5a, dtype=np.uint32)
        p = (sentinel.ctypes.data + 255) & ~255
        names = ("rgba_lo", "depth_lo", "normal_lo", "albedo_lo", "id_lo", "depth", "normal", "albedo", "id", "base",
                 "rgba_out", "pixels", "source", "sphere_select", "plane_select", "cube_select")
        ptrs = {k: p + 4096 * i for i, k in enumerate(names)}       # 16 x 8 hi pixels: at most 2 KiB each

        def desc(**kw):
            d = rt.UpsampleDesc()
            lib.rt_upsample_desc_init(C.byref(d))
            d.width, d.height, d.lo_width, d.lo_height = 16, 8, 8, 4
            d.n_sphere_select, d.n_plane_select, d.n_cube_select, d.use_tables = 16, 4, 4, 1
            for k, v in {**ptrs, **kw}.items():
                setattr(d, k, v)
            return d
        assert lib.rt_scene_upsample(None, C.byref(desc()), None) == 1
        assert lib.rt_scene_upsample(s, None, None) == 1
        q = ptrs
        bad = [dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20), dict(height=32769),
               dict(lo_width=0), dict(lo_height=0), dict(lo_width=-2), dict(lo_height=-8),
               dict(lo_width=17), dict(lo_height=9), dict(width=32769, lo_width=32769),
               dict(rgba_lo=0), dict(depth_lo=0), dict(normal_lo=0), dict(id_lo=0), dict(depth=0), dict(normal=0),
               dict(id=0), dict(rgba_out=0), dict(albedo=0), dict(albedo_lo=0),
               dict(rgba_lo=q["rgba_lo"] + 4), dict(normal_lo=q["normal_lo"] + 8), dict(albedo_lo=q["albedo_lo"] + 8),
               dict(normal=q["normal"] + 4), dict(albedo=q["albedo"] + 12), dict(base=q["base"] + 8),
               dict(rgba_out=q["rgba_out"] + 8), dict(id=q["id"] + 4), dict(id_lo=q["id_lo"] + 4),
               dict(depth=q["depth"] + 2), dict(depth_lo=q["depth_lo"] + 1), dict(pixels=q["pixels"] + 2),
               dict(normal_shift=-1), dict(normal_shift=9), dict(variant=-1), dict(variant=2),
               dict(sigma_depth=0.0), dict(sigma_depth=-0.05), dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf")),
               dict(n_sphere_select=-1), dict(n_plane_select=-1), dict(n_cube_select=-5),
               dict(sphere_select=0), dict(plane_select=0), dict(cube_select=0),
               # an output that overlaps an input or another output
               dict(rgba_out=q["rgba_lo"]), dict(rgba_out=q["normal"]), dict(rgba_out=q["depth"]),
               dict(rgba_out=q["base"] + 16), dict(rgba_out=q["base"] - 16), dict(rgba_out=q["id"] + 1008),
               dict(pixels=q["depth"]), dict(pixels=q["id_lo"] + 252), dict(pixels=q["rgba_out"] + 16),
               dict(source=q["rgba_out"] + 2047), dict(source=q["pixels"]), dict(source=q["sphere_select"] + 15),
               dict(source=q["depth_lo"] + 127), dict(pixels=q["cube_select"])]
        for kw in bad:
            assert lib.rt_scene_upsample(s, C.byref(desc(**kw)), None) == 1, kw
            assert b"rt_scene_upsample" in lib.rt_last_error()
        import torch
        if not torch.cuda.is_available():
            # these pass the checks, which a scene without a device cannot go beyond (a HIP or no-device error)
            ok = [dict(), dict(rgba_out=q["base"]), dict(base=0, pixels=0, source=0),
                  dict(demodulate=0, albedo=0, albedo_lo=0), dict(sphere_select=0, n_sphere_select=0),
                  dict(lo_width=16, lo_height=8), dict(source=q["depth_lo"] + 128)]
            for kw in ok:
                assert lib.rt_scene_upsample(s, C.byref(desc(**kw)), None) in (3, 4), kw
        n = C.c_int(7)
        ms = (C.c_float * 2)()
        assert lib.rt_scene_set_upsample_timing(None, 1) == 1
        assert lib.rt_scene_set_upsample_timing(s, 1) == 0
        assert lib.rt_scene_upsample_times(s, ms, 2, C.byref(n)) == 0 and n.value == 0
        assert lib.rt_scene_upsample_times(s, None, 2, C.byref(n)) == 1
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_python_upsample_checks_its_frames(rt):
    """Frames without colour or guides are refused by the wrapper (and without a GPU every call is: no CPU
    fallback); the material tables name mirrors and glass."""
    sc = rt.Scene()
    try:
        with pytest.raises(rt.RtError):
            sc.upsample({"rgba": None, "aov": {}}, {"rgba": None, "aov": {}})
        assert sc.upsample_select() == {"sphere": [], "plane": [], "cube": []}
    finally:
        sc.close()
