"""Temporal accumulation over moving objects without a device (rt_scene_temporal_motion): the numpy
restatement (tests/tmotion_ref.py) against temporal_ref.py where the two must agree, and against the properties that
follow from the definition, on frames formed on the CPU as test_temporal_cpu.View forms them; the layout of
rt_tmotion_desc, its defaults, and the refusals, which happen before the scene touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tmotion_ref as M
from postpass import TEMPORAL_FIELDS, View, bits as _bits, cam as _cam, move_cube, move_spheres
from scenes import Inputs, mixed_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_FIELDS = TEMPORAL_FIELDS + ("sphere_motion", "n_sphere_motion", "cube_motion", "n_cube_motion", "clamp", "clamp_slack",
                              "clamp_history")
CAM0, CAM1 = (4, 3, 10, 180, -20), (4.5, 3.1, 10.2, 180, -20)
SPHERE_MOVES = {21: (0, 0.2, 0), 207: (-0.15, 0.1, 0.2), 100: (0.1, 0, -0.1), 150: (0, -0.1, 0.1)}
# A box in mid-frame and a move that changes the depth of each of its faces, chosen with the restatement alone: it
# keeps 0.968 of the box's pixels with the displacement and none without.
CUBE, CUBE_MOVE = 1, (-0.1, 0.1, 0.15)


def run(v, hist, prev, same, **kw):
    """View v's frame blended into `hist`, which was accumulated in the view `prev`."""
    return M.temporal_motion(v.cur, hist, v.O, v.D, v.terms, prev.terms, prev.aspect, same, details=True, **kw)


@pytest.fixture(scope="module")
def spheres(rt, oracle):
    """The 256-sphere scene: the standing and the moved camera; four spheres moved under the standing camera; sphere
    252 moved under the moved camera."""
    a = View(rt, oracle, Inputs(rt, 256), _cam(rt, *CAM0), 160, 90)
    b = View(rt, oracle, Inputs(rt, 256), _cam(rt, *CAM1), 160, 90)
    inp = Inputs(rt, 256)
    tab = move_spheres(inp, SPHERE_MOVES)
    c = View(rt, oracle, inp, _cam(rt, *CAM0), 160, 90)
    inp = Inputs(rt, 256)
    tab252 = move_spheres(inp, {252: (0.3, 0, 0)})
    d = View(rt, oracle, inp, _cam(rt, *CAM1), 160, 90)
    return dict(a=a, b=b, c=c, d=d, tab=tab, tab252=tab252, h0=a.onto(None, a))


@pytest.fixture(scope="module")
def mixed(rt, oracle):
    a = View(rt, oracle, mixed_scene(rt), _cam(rt, *CAM0), 160, 96)
    b = View(rt, oracle, mixed_scene(rt), _cam(rt, *CAM1), 160, 96)
    inp = mixed_scene(rt)
    tab = move_cube(rt, inp, CUBE, CUBE_MOVE)
    c = View(rt, oracle, inp, _cam(rt, *CAM0), 160, 96)
    return dict(a=a, b=b, c=c, tab=tab, h0=a.onto(None, a))


def _same_bits(r, want, where=None):
    for k in ("rgba", "moments", "packed"):
        x, y = r[k], want[k]
        if k != "packed":
            x, y = _bits(x), _bits(y)
        if where is not None:
            x, y = x[where], y[where]
        assert np.array_equal(x, y), k


@pytest.mark.parametrize("scene", ["spheres", "mixed"])
def test_zero_displacements_and_no_clamp_are_rt_scene_temporal(request, scene):
    s = request.getfixturevalue(scene)
    a, b, h0 = s["a"], s["b"], s["h0"]
    zeros = np.zeros((300, 4), dtype=f32)
    for v, same in ((a, True), (b, False)):
        want = v.onto(h0, a, same=same)
        assert want["has_history"].any()
        for kw in (dict(), dict(sphere_motion=zeros, cube_motion=zeros), dict(sphere_motion=-zeros)):
            r = run(v, h0, a, same, clamp=False, **kw)
            _same_bits(r, want)
            assert np.array_equal(r["has_history"], want["has_history"]) and not r["clamped"].any()
    first = run(a, None, a, False)                                    # no history
    _same_bits(first, a.onto(None, a))


def _shares(v, hist, prev, same, kind, index, tab_kw):
    sel = (v.cur["id"][..., 0] == kind) & (v.cur["id"][..., 1] == index)
    assert sel.sum() >= 20, int(sel.sum())
    with_m = run(v, hist, prev, same, clamp=False, **tab_kw)
    without = run(v, hist, prev, same, clamp=False)
    return with_m["has_history"][sel].mean(), without["has_history"][sel].mean(), with_m


def test_moved_spheres_under_a_standing_camera(spheres):
    """The restatement's values: 0.913 / 0.036 for sphere 21, 0.918 / 0 for sphere 207."""
    s = spheres
    for i in (21, 207):
        w_, wo, r = _shares(s["c"], s["h0"], s["a"], True, M.RT_HIT_SPHERE, i, dict(sphere_motion=s["tab"]))
        print("sphere", i, "share with / without displacements:", w_, wo)
        assert w_ >= 0.85 and wo <= 0.10, (i, w_, wo)
    # every static pixel has rt_scene_temporal's bits
    want = s["c"].onto(s["h0"], s["a"], same=True)
    static = r["static"]
    ids = s["c"].cur["id"]
    moved = (ids[..., 0] == M.RT_HIT_SPHERE) & np.isin(ids[..., 1], list(SPHERE_MOVES))
    assert np.array_equal(static, ~moved) and 0.5 < static.mean() < 1
    _same_bits(r, want, static)


def test_a_moved_sphere_under_a_moved_camera(spheres):
    """The restatement's values: 0.989 / 0."""
    s = spheres
    w_, wo, r = _shares(s["d"], s["h0"], s["a"], False, M.RT_HIT_SPHERE, 252, dict(sphere_motion=s["tab252"]))
    print("sphere 252 share with / without displacements:", w_, wo)
    assert w_ >= 0.85 and wo <= 0.10, (w_, wo)
    want = s["d"].onto(s["h0"], s["a"], same=False)
    _same_bits(r, want, r["static"])


def test_a_moved_cube(mixed):
    """The restatement's values: 0.968 / 0."""
    s = mixed
    w_, wo, r = _shares(s["c"], s["h0"], s["a"], True, M.RT_HIT_CUBE, CUBE, dict(cube_motion=s["tab"]))
    print("cube share with / without displacements:", w_, wo)
    assert w_ >= 0.85 and wo <= 0.10, (w_, wo)
    _same_bits(r, s["c"].onto(s["h0"], s["a"], same=True), r["static"])
    # a sphere table does not move cubes
    other = run(s["c"], s["h0"], s["a"], True, clamp=False, sphere_motion=s["tab"])
    sel = (s["c"].cur["id"][..., 0] == M.RT_HIT_CUBE) & (s["c"].cur["id"][..., 1] == CUBE)
    assert other["has_history"][sel].mean() <= 0.10


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_displacement_that_is_not_finite_leaves_no_history(spheres, bad, axis):
    s = spheres
    tab = s["tab"].copy()
    tab[21, axis] = bad
    for v, same, clamp in ((s["c"], True, False), (s["c"], True, True), (s["d"], False, True)):
        r = run(v, s["h0"], s["a"], same, sphere_motion=tab, clamp=clamp)
        sel = (v.cur["id"][..., 0] == M.RT_HIT_SPHERE) & (v.cur["id"][..., 1] == 21)
        assert sel.any() and not r["has_history"][sel].any()
        assert (r["rgba"][sel, 3] == 1).all()
        assert np.array_equal(_bits(r["rgba"][sel, :3]), _bits(v.cur["rgba"][sel, :3]))
        # and every other pixel is what it is with the finite table
        ok = run(v, s["h0"], s["a"], same, sphere_motion=s["tab"], clamp=clamp)
        _same_bits(r, ok, ~sel)


def test_an_index_at_or_above_the_count_is_static(spheres):
    s = spheres
    r = run(s["c"], s["h0"], s["a"], True, sphere_motion=s["tab"][:207], clamp=False)
    full = run(s["c"], s["h0"], s["a"], True, sphere_motion=s["tab"], clamp=False)
    ids = s["c"].cur["id"]
    s207 = (ids[..., 0] == M.RT_HIT_SPHERE) & (ids[..., 1] == 207)
    assert r["static"][s207].all() and not full["static"][s207].any()
    _same_bits(r, s["c"].onto(s["h0"], s["a"], same=True), s207)
    _same_bits(r, full, ~s207)
    # the table of one kind is not the other's
    assert run(s["c"], s["h0"], s["a"], True, cube_motion=s["tab"], clamp=False)["static"].all()


# ----------------------------------------------------------------------------- the clamp
def test_an_unchanged_frame_is_clamped_nowhere(spheres, mixed):
    for s in (spheres, mixed):
        a = s["a"]
        hist = s["h0"]
        for _ in range(3):
            on = run(a, hist, a, True, clamp=True)
            off = run(a, hist, a, True, clamp=False)
            assert not on["clamped"].any()
            _same_bits(on, off)
            hist = on
        assert (hist["rgba"][..., 3].max() == 4)


@pytest.fixture(scope="module")
def light(rt, oracle, spheres):
    """Eight frames of the standing camera, then light 0 moved by +2 in x."""
    a = spheres["a"]
    hist = None
    for _ in range(8):
        hist = run(a, hist, a, True)
    inp = Inputs(rt, 256)
    inp.lights[0].pos.x += 2
    return a, hist, View(rt, oracle, inp, _cam(rt, *CAM0), 160, 90)


def test_the_clamp_follows_a_moved_light(light):
    """The restatement's values: mean error 0.0375 without the clamp, 0.0280 with it; mean n 9 against 7.2."""
    a, hist, moved = light
    assert (hist["rgba"][a.cur["id"][..., 0] >= 0, 3] == 8).all()
    new = moved.cur["rgba"][..., :3]
    changed = np.abs(new - a.cur["rgba"][..., :3]).max(axis=-1) > 0.05
    assert changed.sum() > 100
    on = run(moved, hist, a, True, clamp=True, clamp_slack=0.25, clamp_history=4)
    off = run(moved, hist, a, True, clamp=False)
    err = [float(np.abs(r["rgba"][..., :3] - new)[changed].mean()) for r in (on, off)]
    n = [float(r["rgba"][changed, 3].mean()) for r in (on, off)]
    print("mean error on changed pixels with / without the clamp:", err, "mean n:", n)
    assert err[0] < err[1]
    assert on["clamped"].any() and not off["clamped"].any()
    assert (on["rgba"][on["clamped"], 3] <= 4 + 1).all()
    assert (on["rgba"][~on["clamped"] & on["has_history"], 3] == 9).all()
    for ch in (1, 2, 256):
        r = run(moved, hist, a, True, clamp=True, clamp_history=ch)
        assert (r["rgba"][r["clamped"], 3] <= ch + 1).all()
        assert np.array_equal(r["clamped"], on["clamped"])


def test_without_slack_a_clamped_pixel_lies_in_the_box(light):
    a, hist, moved = light
    r = run(moved, hist, a, True, clamp=True, clamp_slack=0.0)
    lo, hi = M.box(moved.cur["rgba"])
    cl = r["clamped"]
    assert cl.sum() > 100
    out = r["rgba"][..., :3]
    # Hc and c lie in [lo, hi]; Hc + (c - Hc) / n leaves it by at most one rounding of a value no larger than hi
    ulp = np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(f32))
    assert (out[cl] >= (lo - ulp)[cl]).all() and (out[cl] <= (hi + ulp)[cl]).all()
    # slack widens the box: fewer pixels are clamped
    assert run(moved, hist, a, True, clamp=True, clamp_slack=0.5)["clamped"].sum() < cl.sum()


def test_the_box_does_not_depend_on_the_order(light):
    """Windows that mix +0 and -0 (equal as floats, different bits), denormals, infinities and NaNs of both signs."""
    rng = np.random.default_rng(11)
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 0.25, -0.25, np.inf, -np.inf, np.nan, -np.nan, 1.0], dtype=f32)
    img = np.zeros((9, 11, 4), dtype=f32)
    img[..., :3] = pool[rng.integers(0, len(pool), (9, 11, 3))]
    img[:4, :, :3] = pool[rng.integers(0, 2, (4, 11, 3))]              # only zeros of both signs
    lo, hi = M.box(img)
    assert (np.signbit(lo[:3]) != np.signbit(hi[:3])).any()            # -0 below +0
    for _ in range(6):
        order = rng.permutation(9)
        lo2, hi2 = M.box(img, order=order)
        assert np.array_equal(_bits(lo), _bits(lo2)) and np.array_equal(_bits(hi), _bits(hi2)), order
    # against the definition, pixel by pixel: the extreme keys of the window's pixels inside the buffer
    k = M.key(img[..., :3]).astype(np.int64)
    for y, x in ((0, 0), (0, 5), (8, 10), (4, 4), (8, 0)):
        win = k[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].reshape(-1, 3)
        assert np.array_equal(M.key(lo[y, x]), win.min(axis=0)) and np.array_equal(M.key(hi[y, x]), win.max(axis=0))
    assert np.array_equal(_bits(M.unkey(M.key(pool))), _bits(pool))
    # on a real frame: the same under a reversed order
    _, _, moved = light
    a1, a2 = M.box(moved.cur["rgba"]), M.box(moved.cur["rgba"], order=range(8, -1, -1))
    assert np.array_equal(_bits(a1[0]), _bits(a2[0])) and np.array_equal(_bits(a1[1]), _bits(a2[1]))


# ----------------------------------------------------------------------------- the C ABI
def test_desc_layout_and_defaults(rt, tmp_path):
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof(rt_tmotion_desc, {f}));\n' for f in _FIELDS)
    body += "".join(f'    printf("%zu\\n", offsetof(rt_temporal_desc, {f}));\n' for f in TEMPORAL_FIELDS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {\n'
                   f'    printf("%zu\\n", sizeof(rt_tmotion_desc));\n{body}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    want = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    n = len(_FIELDS)
    assert C.sizeof(rt.TMotionDesc) == want[0]
    assert [getattr(rt.TMotionDesc, f).offset for f in _FIELDS] == want[1:1 + n]
    assert [f for f, _ in rt.TMotionDesc._fields_] == list(_FIELDS)
    assert want[1:1 + len(TEMPORAL_FIELDS)] == want[1 + n:]              # rt_temporal_desc's fields, in place
    lib = rt.load_library()
    d = rt.TMotionDesc()
    C.memset(C.byref(d), 0xff, C.sizeof(d))
    lib.rt_tmotion_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.TMotionDesc)
    assert (d.max_history, d.reset, d.variant) == (32, 0, 0)
    assert f32(d.depth_tolerance) == f32(0.02) and f32(d.normal_cos_min) == f32(0.9)
    assert (d.clamp, d.clamp_history) == (1, 4) and f32(d.clamp_slack) == f32(0.25)
    assert (d.n_sphere_motion, d.n_cube_motion) == (0, 0) and not d.sphere_motion and not d.cube_motion
    assert (d.width, d.height, d.aspect, d.prev_aspect) == (0, 0, 0.0, 0.0)
    assert bytes(d.cam) == bytes(36) and bytes(d.prev_cam) == bytes(36)
    assert not any((d.rgba_in, d.depth, d.normal, d.id, d.prev_rgba, d.prev_depth, d.prev_normal, d.prev_id,
                    d.prev_moments, d.rgba_out, d.moments_out, d.pixels))
    assert {k: M.DEFAULTS[k] for k in ("clamp", "clamp_slack", "clamp_history")} == dict(clamp=1, clamp_slack=0.25, clamp_history=4)
    lib.rt_tmotion_desc_init(None)
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
                 "rgba_out", "moments_out", "pixels", "sphere_motion", "cube_motion")
        ptrs = {k: p + 4096 * i for i, k in enumerate(names)}       # 16 x 8 pixels: at most 2 KiB each

        def desc(**kw):
            d = rt.TMotionDesc()
            lib.rt_tmotion_desc_init(C.byref(d))
            d.width, d.height = 16, 8
            d.aspect = d.prev_aspect = 1.5
            d.cam = d.prev_cam = rt.default_camera()
            d.n_sphere_motion, d.n_cube_motion = 64, 8
            for k, v in {**ptrs, **kw}.items():
                setattr(d, k, v)
            return d
        assert lib.rt_scene_temporal_motion(None, C.byref(desc()), None) == 1
        assert lib.rt_scene_temporal_motion(s, None, None) == 1
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
               dict(rgba_out=q["rgba_in"]), dict(rgba_out=q["prev_rgba"] + 2032), dict(rgba_out=q["prev_rgba"] - 2032),
               dict(rgba_out=q["normal"]), dict(rgba_out=q["depth"]), dict(moments_out=q["prev_moments"]),
               dict(moments_out=q["id"] + 8), dict(pixels=q["depth"]), dict(pixels=q["prev_id"] + 1020),
               dict(pixels=q["rgba_out"] + 16), dict(moments_out=q["rgba_out"]),
               # what the new fields add
               dict(n_sphere_motion=-1), dict(n_cube_motion=-1), dict(n_sphere_motion=-(1 << 31)),
               dict(sphere_motion=0), dict(cube_motion=0), dict(sphere_motion=0, n_sphere_motion=1),
               dict(sphere_motion=q["sphere_motion"] + 4), dict(sphere_motion=q["sphere_motion"] + 8),
               dict(cube_motion=q["cube_motion"] + 12), dict(cube_motion=q["cube_motion"] + 1),
               dict(clamp_slack=-0.01), dict(clamp_slack=16.5), dict(clamp_slack=float("nan")),
               dict(clamp_slack=float("inf")), dict(clamp_slack=float("-inf")),
               dict(clamp_history=0), dict(clamp_history=257), dict(clamp_history=-4),
               dict(rgba_out=q["sphere_motion"]), dict(rgba_out=q["sphere_motion"] + 1008),
               dict(rgba_out=q["sphere_motion"] - 2032), dict(moments_out=q["cube_motion"]),
               dict(moments_out=q["cube_motion"] + 120), dict(pixels=q["cube_motion"] + 64),
               dict(pixels=q["sphere_motion"] + 1020)]
        for kw in bad:
            assert lib.rt_scene_temporal_motion(s, C.byref(desc(**kw)), None) == 1, kw
            assert b"rt_scene_temporal_motion" in lib.rt_last_error()
        # the checks hold with the clamp off and with reset too
        assert lib.rt_scene_temporal_motion(s, C.byref(desc(clamp=0, clamp_slack=-1.0)), None) == 1
        assert lib.rt_scene_temporal_motion(s, C.byref(desc(reset=1, depth=0)), None) == 1
        assert lib.rt_scene_temporal_motion(s, C.byref(desc(reset=1, rgba_out=q["sphere_motion"])), None) == 1
        import torch
        if not torch.cuda.is_available():
            # these pass the checks, which a scene without a device cannot go beyond (a HIP or no-device error)
            ok = [dict(), dict(sphere_motion=0, n_sphere_motion=0, cube_motion=0, n_cube_motion=0),
                  dict(n_sphere_motion=0), dict(clamp_slack=0.0), dict(clamp_slack=16.0), dict(clamp_history=1),
                  dict(clamp_history=256), dict(clamp=0), dict(rgba_out=q["sphere_motion"] + 1024),    # adjacent
                  dict(reset=1, **{k: 0 for k in names if k.startswith("prev_")})]
            for kw in ok:
                assert lib.rt_scene_temporal_motion(s, C.byref(desc(**kw)), None) in (3, 4), kw
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_python_temporal_motion_checks_its_frame(rt):
    sc = rt.Scene()
    try:
        with pytest.raises(rt.RtError):
            sc.temporal_motion({"rgba": None, "aov": {}})
    finally:
        sc.close()
