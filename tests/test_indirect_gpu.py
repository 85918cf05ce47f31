"""The indirect pass on the device (rt_scene_indirect), bit for bit: both variants, with the BVH and with the
whole lists, against the numpy restatement (tests/indirect_ref.py) fed by the composed castRay / rayTrace reference
(query_ref.CastRef) and by the device's own SHADE; exact furnace values; ray ranges and groups; the whole queue; every
output element; empty and full views; a long-lived scene against fresh ones; the refusals; the pipeline."""
import ctypes as C

import numpy as np
import pytest

import indirect_ref as I
import meshes
import postpass as P
import query_ref as Q
from scenes import Inputs, Scn, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
POISON = P.SENTINEL


# ----------------------------------------------------------------------------- helpers
def _frame(sc, inp, w, h, **kw):
    return sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=P.ALL, **kw)


def _np(frame):
    out = {k: v.cpu().numpy() for k, v in frame["aov"].items()}
    out["rgba"] = frame["rgba"].cpu().numpy()
    return out


def _primary(sc, inp, w, h):
    r = sc.primary_rays(w, h, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6).cpu().numpy()
    return np.ascontiguousarray(r[:, :3]), np.ascontiguousarray(r[:, 3:])


def _device_shade(sc, cull=True):
    def shade(O, D):
        import torch
        rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([O, D], axis=1), dtype=np.float32)).cuda()
        return sc.trace_rays(rays, "shade", cull=cull)["rgba"].cpu().numpy()
    return shade


def _recording(ref):
    """CastRef.shade as indirect_ref's callable, keeping the kind every gather ray hit."""
    kinds = []

    def shade(O, D):
        rgba, _, rec = ref.shade(O, D)
        kinds.append(rec["kind"].copy())
        return rgba
    return shade, kinds


def _reference(sc, inp, frame, w, h, shade, colour=True, modulate=True, **kw):
    g = _np(frame)
    O, D = _primary(sc, inp, w, h)
    return I.indirect(w, g["depth"], g["normal"], g["id"], O, D, shade, albedo=g["albedo"] if modulate else None,
                      rgba_in=g["rgba"] if colour else None, details=True, **kw)


def _call(sc, inp, frame, **kw):
    return sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, want_packed=True, **kw)


def _same(out, rgba, packed, what):
    got = P.tensor_bits(out["rgba"]).reshape(-1, 4)
    bad = (got != P.bits(rgba)).any(axis=1)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8])
    assert np.array_equal(P.tensor_bits(out["packed"]).reshape(-1), packed), what


def _same_outputs(a, b, what):
    assert np.array_equal(P.tensor_bits(a["rgba"]), P.tensor_bits(b["rgba"])), what
    assert np.array_equal(P.tensor_bits(a["packed"]), P.tensor_bits(b["packed"])), what


def _term(sc, inp, frame, **kw):
    """The irradiance term alone [m, 3]: no colour, no albedo."""
    return sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, colour=None, modulate=False, **kw)["rgba"].cpu().numpy().reshape(-1, 4)[:, :3]


def _box(rt, closed, **kw):
    """A camera inside a room of inward-facing planes (the top left out unless `closed`) with one sphere."""
    pl = [(100, 0, 0, -1, 0, 0), (-100, 0, 0, 1, 0, 0), (0, -100, 0, 0, 1, 0), (0, 0, 100, 0, 0, -1), (0, 0, -100, 0, 0, 1)]
    if closed:
        pl.append((0, 100, 0, 0, -1, 0))
    return Scn(rt, [(2, 1, 6, 1.0)], planes=pl, cam=P.cam(rt, 0, 0, 0, 0, 0), **kw)


# ----------------------------------------------------------------------------- against the independent reference
@pytest.mark.parametrize("case", ["view", "inside"])
def test_both_variants_equal_the_composed_reference(rt, oracle, gpu, case):
    """50 x 30 = 1 500 pixels (no multiple of 64 or 256, rows straddle waves) of 64 spheres; and, for negative depths, a
    camera inside a large sphere at 24 x 16."""
    import torch
    if case == "view":
        inp, w, h = Inputs(rt, 64), 50, 30
        kw = dict(rays=3, ray_base=5, seed=9, strength=0.75)
    else:
        inp, w, h = Scn(rt, [(0, 0, 0, 30.0), (2, 1, 6, 1.0), (-3, 0, 5, 1.5)], cam=P.cam(rt, 0, 0, 0, 180, 0)), 24, 16
        kw = dict(rays=2, ray_base=1, seed=3, strength=1.5)
    sc = inp.scene()
    frame = _frame(sc, inp, w, h)
    shade, kinds = _recording(Q.CastRef(oracle, inp))
    rgba, packed, det = _reference(sc, inp, frame, w, h, shade, **kw)
    kinds = np.concatenate(kinds)
    live = det["live"]
    assert (kinds >= 0).any() and (kinds < 0).any()                    # gather hits and gather misses
    g = _np(frame)
    if case == "view":
        assert live.any() and (~live).any()                             # surface and sky pixels
    else:
        assert (g["depth"].reshape(-1)[live] < 0).any() or det["flip"][live].any()
    for variant in (0, 1):
        for cull in (True, False):
            out = _call(sc, inp, frame, cull=cull, variant=variant, **kw)
            torch.cuda.synchronize()
            _same(out, rgba, packed, (case, variant, cull))
            # dead pixels keep their input bits
            assert np.array_equal(P.tensor_bits(out["rgba"]).reshape(-1, 4)[~live], P.bits(g["rgba"]).reshape(-1, 4)[~live])


def test_every_kind_of_primitive(rt, oracle, gpu):
    import torch
    inp, mesh, w, h = mixed_scene(rt), meshes.uv_sphere_obj(), 40, 24
    sc = P.scene(rt, inp, mesh)
    frame = _frame(sc, inp, w, h)
    shade, kinds = _recording(Q.CastRef(oracle, inp, mesh_text=mesh))
    rgba, packed, det = _reference(sc, inp, frame, w, h, shade, rays=2)
    pixel_kinds = set(_np(frame)["id"].reshape(-1, 2)[det["live"], 0].tolist())
    assert {0, 1, 2, 3} <= pixel_kinds and {0, 1, 2, 3} <= set(np.concatenate(kinds).tolist())
    assert det["flip"][det["live"]].any()                               # a normal that faces away from its primary ray
    for variant in (0, 1):
        out = _call(sc, inp, frame, rays=2, variant=variant)
        torch.cuda.synchronize()
        _same(out, rgba, packed, variant)


def test_both_variants_equal_the_restatement_over_the_device_shade(rt, gpu):
    import torch
    inp, w, h = Inputs(rt, 256), 160, 90
    sc = inp.scene()
    frame = _frame(sc, inp, w, h)
    rgba, packed, det = _reference(sc, inp, frame, w, h, _device_shade(sc), rays=4, seed=2)
    assert det["live"].sum() > 1000 and (~det["live"]).sum() > 1000
    for variant in (0, 1):
        out = _call(sc, inp, frame, rays=4, seed=2, variant=variant)
        torch.cuda.synchronize()
        _same(out, rgba, packed, variant)


# ----------------------------------------------------------------------------- exact values
def test_furnace(rt, gpu):
    """One sphere under a sky of constant 0.5: a sphere is convex, so every gather ray from it meets the sky, and every
    sphere pixel is exactly 0.5 -- or 0.5 x albedo."""
    import torch
    sky = [np.full((8, 16), 0.5, dtype=np.float32)] * 3
    inp = Scn(rt, [(0, 0, 6, 1.5)], sky=sky, cam=P.cam(rt, 0, 0, 0, 0, 0))
    sc = inp.scene()
    w, h = 64, 40
    frame = _frame(sc, inp, w, h)
    g = _np(frame)
    live = g["id"].reshape(-1, 2)[:, 0] >= 0
    assert live.sum() > 100 and (~live).sum() > 100
    for variant in (0, 1):
        out = sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, colour=None, modulate=False, rays=4, variant=variant)
        mod = sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, colour=None, modulate=True, rays=4, variant=variant)
        same = sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, strength=0.0, rays=4, variant=variant)
        torch.cuda.synchronize()
        o = out["rgba"].cpu().numpy().reshape(-1, 4)
        assert np.array_equal(P.bits(o[live]), P.bits(np.tile(np.array([0.5, 0.5, 0.5, 1], dtype=f32), (live.sum(), 1))))
        assert np.array_equal(P.bits(o[~live]), P.bits(np.tile(np.array([0, 0, 0, 1], dtype=f32), ((~live).sum(), 1))))
        m = mod["rgba"].cpu().numpy().reshape(-1, 4)
        want = (f32(0.5) * g["albedo"].reshape(-1, 4)[live, :3]).astype(f32)
        assert np.array_equal(P.bits(m[live, :3]), P.bits(want))
        assert np.array_equal(P.tensor_bits(same["rgba"]), P.tensor_bits(frame["rgba"]))


def test_ray_ranges_and_groups(rt, gpu):
    """A call's rays are rays ray_base .. ray_base + rays - 1: its mean is the binary32 composition of the one-ray calls,
    also across the scratch's groups of four; and the seed reaches every live pixel."""
    import torch
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    frame = _frame(sc, inp, w, h)
    g = _np(frame)
    live = g["id"].reshape(-1, 2)[:, 0] >= 0
    for base, rays in ((8, 4), (0, 16)):
        S = np.zeros((w * h, 3), dtype=f32)
        for j in range(rays):
            S = (S + _term(sc, inp, frame, rays=1, ray_base=base + j, seed=4)).astype(f32)
        want = (S / f32(rays)).astype(f32)
        for variant in (0, 1):
            got = _term(sc, inp, frame, rays=rays, ray_base=base, seed=4, variant=variant)
            assert np.array_equal(P.bits(got), P.bits(want)), (base, rays, variant)
        assert (want[live] != 0).any()
    # another seed: every live pixel's first direction, no dead pixel
    O, D = _primary(sc, inp, w, h)
    lv, n, start, _ = I.pixels(g["depth"], g["normal"], g["id"], O, D)
    assert np.array_equal(lv, live)
    _, G1 = I.gather_rays(w, lv, n, start, 1, 0, 1)
    _, G2 = I.gather_rays(w, lv, n, start, 1, 0, 2)
    assert (P.bits(G1[0]) != P.bits(G2[0])).any(axis=1).all()
    a, b = _call(sc, inp, frame, seed=1), _call(sc, inp, frame, seed=2)
    torch.cuda.synchronize()
    ab, bb = P.tensor_bits(a["rgba"]).reshape(-1, 4), P.tensor_bits(b["rgba"]).reshape(-1, 4)
    assert np.array_equal(ab[~live], bb[~live]) and (ab[live] != bb[live]).any()


def test_rays_are_distinct_samples(rt, gpu):
    """The 16 rays of a call are 16 samples, not one: against the mean of 64 the error of 16 is below half that of 1
    (expected sqrt((1/16 - 1/64) / (1 - 1/64)) = 0.22)."""
    inp, w, h = Inputs(rt, 256), 160, 90
    sc = inp.scene()
    frame = _frame(sc, inp, w, h)
    live = _np(frame)["id"].reshape(-1, 2)[:, 0] >= 0
    calls = [_term(sc, inp, frame, rays=16, ray_base=b, seed=6).astype(np.float64) for b in (0, 16, 32, 48)]
    mean = sum(calls) / 4
    one = _term(sc, inp, frame, rays=1, ray_base=0, seed=6).astype(np.float64)
    e16 = np.abs(calls[0] - mean)[live].mean()
    e1 = np.abs(one - mean)[live].mean()
    print("mean absolute error: 16 rays", e16, "1 ray", e1, "ratio", e16 / e1)
    assert e1 > 0 and e16 < 0.5 * e1


# ----------------------------------------------------------------------------- the queue, the outputs
def test_whole_queue(rt, gpu):
    """More slots than one pass of the shade launch's 2 048 x 256 grid stride: 16 spheres at 1 024 x 520; and a room whose
    four rays per pixel mostly hit, so that the queue itself is longer than one pass."""
    import torch
    w, h = 1024, 520
    inp = Inputs(rt, 16)
    sc = inp.scene()
    frame = _frame(sc, inp, w, h)
    a, b = _call(sc, inp, frame, variant=0), _call(sc, inp, frame, variant=1)
    torch.cuda.synchronize()
    _same_outputs(a, b, "16 spheres")
    room = _box(rt, closed=False)
    sc = room.scene()
    frame = _frame(sc, room, w, h)
    a = _call(sc, room, frame, rays=4, variant=0)
    counts = sc.indirect_counts()
    b = _call(sc, room, frame, rays=4, variant=1)
    torch.cuda.synchronize()
    _same_outputs(a, b, "room")
    assert len(counts) == 1 and 2048 * 256 < counts[0] < 4 * w * h
    assert (a["rgba"][..., :3] != frame["rgba"][..., :3]).any()


def _raw(sc, inp, frame, out, packed, rgba_in=True, **kw):
    a = frame["aov"]
    h, w = a["depth"].shape
    return sc.indirect_desc(w, h, cam=inp.cam, aspect=kw.pop("aspect", inp.aspect), depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(),
                            id=a["id"].data_ptr(), albedo=a["albedo"].data_ptr(),
                            rgba_in=frame["rgba"].data_ptr() if rgba_in else 0, rgba_out=out.data_ptr(),
                            pixels=packed.data_ptr(), **kw)


def _poisoned(w, h):
    import torch
    return (torch.full((h, w, 4), POISON, dtype=torch.int32, device="cuda"),
            torch.full((h, w), POISON, dtype=torch.int32, device="cuda"))


def test_every_output_element_is_written(rt, gpu):
    import torch
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    frame = _frame(sc, inp, w, h)
    want = _call(sc, inp, frame, rays=5, seed=3, variant=1)
    for variant in (0, 1):
        for rgba_in in (True, False):
            out, packed = _poisoned(w, h)
            assert sc.indirect_raw(_raw(sc, inp, frame, out, packed, rgba_in=rgba_in, rays=5, seed=3, variant=variant)) == 0
            torch.cuda.synchronize()
            assert not (out == POISON).any() and not (packed == POISON).any(), (variant, rgba_in)
            if rgba_in:
                assert np.array_equal(P.tensor_bits(out), P.tensor_bits(want["rgba"]))
                assert np.array_equal(P.tensor_bits(packed), P.tensor_bits(want["packed"]))
        # in place: rgba_out is rgba_in itself
        buf = frame["rgba"].clone()
        _, packed = _poisoned(w, h)
        d = _raw(sc, inp, frame, buf, packed, rays=5, seed=3, variant=variant)
        d.rgba_in = buf.data_ptr()
        assert sc.indirect_raw(d) == 0
        torch.cuda.synchronize()
        assert np.array_equal(P.tensor_bits(buf), P.tensor_bits(want["rgba"]))


def test_empty_and_full_views(rt, gpu):
    import torch
    # sky only: nothing is cast, the output is the input, and the timing entry still answers
    inp, w, h = Inputs(rt, 8), 50, 30
    sc = inp.scene()
    sc.set_spheres(inp.spheres, 0)
    sc.set_indirect_timing(True)
    frame = _frame(sc, inp, w, h)
    assert (frame["aov"]["id"][..., 0] < 0).all()
    for variant, passes in ((0, 3), (1, 1)):
        out = _call(sc, inp, frame, variant=variant)
        assert len(sc.indirect_times()) == passes
        assert np.array_equal(P.tensor_bits(out["rgba"]), P.tensor_bits(frame["rgba"]))
        assert np.array_equal(P.tensor_bits(out["packed"]), P.tensor_bits(frame["packed"]))
        if variant == 0:
            assert sc.indirect_counts() == [0]
    # a closed room: no dead pixel, no miss -- every slot of both groups is queued
    room = _box(rt, closed=True)
    sc = room.scene()
    sc.set_indirect_timing(True)
    w, h = 64, 40
    frame = _frame(sc, room, w, h)
    assert (frame["aov"]["id"][..., 0] >= 0).all()
    a = _call(sc, room, frame, rays=6, variant=0)
    assert sc.indirect_counts() == [4 * w * h, 2 * w * h]
    assert len(sc.indirect_times()) == 6
    b = _call(sc, room, frame, rays=6, variant=1)
    torch.cuda.synchronize()
    _same_outputs(a, b, "closed room")


# ----------------------------------------------------------------------------- state
def test_a_long_lived_scene_equals_fresh_scenes(rt, gpu):
    import torch
    inp = Inputs(rt, 64)
    sc = inp.scene()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    step = [0]

    def check(what, w=50, h=30, **kw):
        st = streams[step[0] % 2]
        step[0] += 1
        frame = _frame(sc, inp, w, h, stream=st)
        got = sc.indirect(frame, cam=inp.cam, aspect=inp.aspect, want_packed=True, stream=st, **kw)
        fresh = inp.scene()
        f2 = _frame(fresh, inp, w, h)
        want = _call(fresh, inp, f2, **kw)
        torch.cuda.synchronize()
        _same_outputs(got, want, what)
        assert (got["rgba"][..., :3] != frame["rgba"][..., :3]).any(), what
        fresh.close()

    check("first", rays=2)
    P.move_spheres(inp, {3: (0.5, 0.2, -0.3), 10: (-0.4, 0.1, 0.2)})
    sc.set_spheres(inp.spheres, inp.n)                                  # the BVH goes stale
    check("set_spheres", rays=2)
    inp.lights[0].pos.x += 3.0
    sc.set_lights(inp.lights, inp.n_lights)
    check("set_lights", rays=2)
    inp.tex = [np.ascontiguousarray(p[::-1] * f32(0.5)) for p in inp.tex]
    sc.set_texture(inp.tex)
    check("set_texture", rays=2)
    inp.sky = [np.ascontiguousarray(p[:, ::-1]) for p in inp.sky]
    sc.set_sky(inp.sky_box, inp.sky)
    check("set_sky", rays=2)
    sc.set_materials(P.mirror_k(inp.n))                                 # a reflective frame shares the BVH
    sc.render(50, 30, cam=inp.cam, aspect=inp.aspect, reflect_depth=2, stream=streams[0])
    check("after a reflective frame", rays=2)
    sc.denoise(_frame(sc, inp, 50, 30, stream=streams[1]), stream=streams[1])
    check("after a denoise", rays=2)
    check("a larger size", w=120, h=70, rays=2)                         # the scratch grows
    check("a smaller size", rays=2)
    check("more rays than a group", rays=9)                             # the running sum is allocated
    check("whole lists, the yardstick", rays=2, cull=False, variant=1)
    inp.n = 32
    sc.set_spheres(inp.spheres, inp.n)                                  # another count
    check("fewer spheres", rays=2)


# ----------------------------------------------------------------------------- refusals
def test_refusals_on_the_device_write_nothing(rt, gpu):
    import torch
    lib = rt.load_library()
    inp, w, h = Inputs(rt, 64), 50, 30
    sc = inp.scene()
    frame = _frame(sc, inp, w, h)
    out, packed = _poisoned(w, h)
    ok = dict(rays=2)
    bad = [dict(rays=0), dict(rays=17), dict(ray_base=-1), dict(ray_base=1 << 24), dict(cull=2), dict(variant=2),
           dict(strength=-1.0), dict(strength=float("nan")), dict(aspect=0.0)]
    for kw in bad:
        assert sc.indirect_raw(_raw(sc, inp, frame, out, packed, **{**ok, **kw})) == 1, kw
    for field, off in (("rgba_out", 8), ("pixels", 2), ("depth", 2), ("normal", 8), ("id", 4), ("albedo", 8), ("rgba_in", 8)):
        d = _raw(sc, inp, frame, out, packed, **ok)
        setattr(d, field, getattr(d, field) + off)
        assert sc.indirect_raw(d) == 1 and "aligned" in lib.rt_last_error().decode(), field
    for field in ("depth", "normal", "id", "rgba_out"):
        d = _raw(sc, inp, frame, out, packed, **ok)
        setattr(d, field, 0)
        assert sc.indirect_raw(d) == 1, field
    d = _raw(sc, inp, frame, out, packed, **ok)
    d.rgba_out = frame["aov"]["normal"].data_ptr()                      # an output over an input
    assert sc.indirect_raw(d) == 1 and "overlaps" in lib.rt_last_error().decode()
    d = _raw(sc, inp, frame, out, packed, **ok)
    d.width = 32769
    assert sc.indirect_raw(d) == 1
    # SHADE's own conditions: a scene without sky, a scene with primitives and no texture
    bare = rt.Scene()
    assert bare.indirect_raw(_raw(bare, inp, frame, out, packed, **ok)) == 1 and "sky" in lib.rt_last_error().decode()
    bare.set_sky(inp.sky_box, inp.sky)
    bare.set_spheres(inp.spheres, inp.n)
    assert bare.indirect_raw(_raw(bare, inp, frame, out, packed, **ok)) == 1 and "texture" in lib.rt_last_error().decode()
    bare.close()
    # a capturing stream
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = sc.indirect_raw(_raw(sc, inp, frame, out, packed, **ok), s.cuda_stream)
    assert rc == 2
    torch.cuda.synchronize()
    assert (out == POISON).all() and (packed == POISON).all()
    assert sc.indirect_raw(_raw(sc, inp, frame, out, packed, **ok)) == 0    # and the scene still works
    torch.cuda.synchronize()
    assert not (out == POISON).any()


# ----------------------------------------------------------------------------- the pipeline
def test_pipeline_half_resolution_upsample_temporal_denoise(rt, gpu):
    import torch
    inp = Inputs(rt, 256)
    sc = inp.scene()
    W, H = 160, 90
    hi = _frame(sc, inp, W, H)
    lo = _frame(sc, inp, W // 2, H // 2)
    sky = (hi["aov"]["id"][..., 0] < 0).cpu().numpy()
    assert sky.any() and (~sky).any()
    history = None
    for k in range(4):
        ind = sc.indirect(lo, cam=inp.cam, aspect=inp.aspect, rays=1, ray_base=k)
        assert tuple(ind["rgba"].shape) == (H // 2, W // 2, 4)
        up = sc.upsample(hi, lo, colour=ind["rgba"], base=True, demodulate=True)
        assert tuple(up["rgba"].shape) == (H, W, 4)
        history = sc.temporal(hi, history, cam=inp.cam, aspect=inp.aspect, colour=up["rgba"])
        torch.cuda.synchronize()
        for t in (ind["rgba"], up["rgba"], history["rgba"]):
            assert not torch.isnan(t).any()
        assert np.array_equal(P.tensor_bits(up["rgba"])[sky], P.tensor_bits(hi["rgba"])[sky])
        assert np.array_equal(P.tensor_bits(history["rgba"])[sky][:, :3], P.tensor_bits(hi["rgba"])[sky][:, :3])
    assert float(history["rgba"][..., 3].max()) == 4.0
    out = sc.denoise({"rgba": history["rgba"], "aov": hi["aov"]})
    torch.cuda.synchronize()
    assert tuple(out["rgba"].shape) == (H, W, 4) and not torch.isnan(out["rgba"]).any()
    assert np.array_equal(P.tensor_bits(out["rgba"])[sky][:, :3], P.tensor_bits(hi["rgba"])[sky][:, :3])
    # the indirect light is there: the result is brighter than the frame on the surfaces
    assert float(out["rgba"][..., :3].sum()) > float(hi["rgba"][..., :3].sum())
