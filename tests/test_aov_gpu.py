"""G-buffer outputs on the device (rt_frame_desc.aov_*): every guide bit for bit against NEAREST of the
frame's own primary rays and against the composed reference, the colour outputs unchanged, subsets, bands,
interleave, old struct sizes, `fast`, the drop-in boundary and the refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import meshes
from scenes import Inputs, mixed_scene
import query_ref as Q
from test_reflect_cpu import intersect, sphere_table
from test_reflect_gpu import _managed_sprite

pytestmark = pytest.mark.gpu

f32 = np.float32
ALL = ("depth", "normal", "id", "albedo")
SENTINEL = 0x5a5a5a5a


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


def _f2i(x):
    """(int)x as the frame kernel's f2i (v_cvt_i32_f32: truncation, saturation, NaN -> 0)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    x = np.where(np.isnan(x), 0.0, np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1))
    return np.trunc(x).astype(np.int64)


def _scene_of(rt, inp, mesh=None, spheres=True):
    sc = inp.scene()
    if not spheres:
        sc.set_spheres(inp.spheres, 0)
    if getattr(inp, "n_planes", 0):
        sc.set_planes(inp.planes, inp.n_planes)
    if getattr(inp, "n_cubes", 0):
        sc.set_cubes(inp.cubes, inp.n_cubes)
    if mesh is not None:
        sc.set_mesh(rt.mesh_from_obj_text(mesh))
    return sc


def _tie_scene(rt):
    """A triangle through a sphere's near point at t = 9 on the centre pixel's ray, which is exactly (0,0,0) + t (0,0,1)
    in a 161 x 161 frame with aspect 1, the camera at (0,0,1) (eyePos (0,0,-1)) and no yaw or pitch."""
    lib = rt.load_library()
    inp = Inputs(rt, 8)
    spheres = (rt.Sphere * 2)()
    lib.rt_sphere_init(C.byref(spheres[0]), 0.0, 0.0, 10.0, 1.0)
    lib.rt_sphere_init(C.byref(spheres[1]), 3.0, 0.0, 12.0, 1.0)
    inp.spheres, inp.n = spheres, 2
    inp.cam = rt.Camera(rt.Vec3(0, 0, 1), rt.Vec3(0, 0, 1), 0.0, 0.0, 0.0)
    inp.aspect = 1.0
    mesh = "v -1 -1 9\nv 1 -1 9\nv 0 1 9\nv 2 -1 11\nv 4 -1 11\nv 3 1 11\nf 1 2 3\nf 4 5 6\n"
    return inp, mesh


def _case(rt, name):
    """name -> (inputs, mesh text or None, 'spheres in the scene', width, height)"""
    if name == "c2_160x90_n256":
        return Inputs(rt, 256), None, True, 160, 90
    if name == "c3_960x540_n1024":
        return Inputs(rt, 1024), None, True, 960, 540
    if name == "c3_3840x2160":
        return Inputs(rt, 1024), None, True, 3840, 2160
    if name == "mixed_160x96":
        return mixed_scene(rt), None, True, 160, 96
    if name == "mesh_160x90":
        return Inputs(rt, 64), meshes.uv_sphere_obj(), True, 160, 90
    if name == "inside_sphere":
        inp = Inputs(rt, 256)
        lib = rt.load_library()
        sp = (rt.Sphere * 256)()
        C.memmove(sp, inp.spheres, C.sizeof(sp))
        lib.rt_sphere_init(C.byref(sp[5]), 4.0, 3.0, 9.5, 2.0)   # around the ray origin (4, 3, 10 - 1/aspect)
        inp.spheres = sp
        return inp, None, True, 160, 90
    if name == "duplicates":
        inp = Inputs(rt, 256)
        sp = (rt.Sphere * 256)()
        C.memmove(sp, inp.spheres, C.sizeof(sp))
        for i in range(64):   # list positions 192..255 repeat 0..63: the lower position wins every tie
            C.memmove(C.byref(sp[192 + i]), C.byref(sp[i]), C.sizeof(rt.Sphere))
        inp.spheres = sp
        return inp, None, True, 160, 90
    if name == "tie":
        inp, mesh = _tie_scene(rt)
        return inp, mesh, True, 161, 161
    raise KeyError(name)


def _texel(inp, txy):
    """The texel the frame fetches for (tx, ty): f2i(ty * h) * w + f2i(tx * w), clamped to the texture."""
    r, g, b = inp.tex
    th, tw = r.shape
    tx, ty = txy[:, 0].astype(np.float32), txy[:, 1].astype(np.float32)
    ci = _f2i(ty * f32(th)) * tw + _f2i(tx * f32(tw))
    ci = np.clip(ci, 0, tw * th - 1)
    return np.stack([r.reshape(-1)[ci], g.reshape(-1)[ci], b.reshape(-1)[ci]], axis=1).astype(np.float32)


def _check_frame(rt, sc, inp, w, h, cull, y0=0, y1=0):
    """The four guides of one frame against NEAREST of its own primary rays; returns (aov, NEAREST) as numpy."""
    import torch
    out = sc.render(w, h, y0=y0, y1=y1, cam=inp.cam, aspect=inp.aspect, cull=bool(cull), aov=ALL)
    rays = sc.primary_rays(w, h, y0=y0, y1=y1, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6)
    near = sc.trace_rays(rays, "nearest", cull=bool(cull))
    torch.cuda.synchronize()
    a = {k: v.cpu().numpy() for k, v in out["aov"].items()}
    nr = {k: v.cpu().numpy() for k, v in near.items()}
    rows = (y1 if y1 else h) - y0
    assert a["depth"].shape == (rows, w) and a["normal"].shape == (rows, w, 4)
    assert a["id"].shape == (rows, w, 2) and a["albedo"].shape == (rows, w, 4)
    depth, normal = a["depth"].reshape(-1), a["normal"].reshape(-1, 4)
    ids, albedo = a["id"].reshape(-1, 2), a["albedo"].reshape(-1, 4)
    assert np.array_equal(depth.view(np.uint32), nr["t"].view(np.uint32))
    assert np.array_equal(ids[:, 0], nr["kind"]) and np.array_equal(ids[:, 1], nr["index"])
    assert np.array_equal(normal[:, :3].view(np.uint32), np.ascontiguousarray(nr["normal"]).view(np.uint32))
    assert (normal[:, 3].view(np.uint32) == 0).all()
    hit = nr["kind"] >= 0
    assert (albedo[:, 3] == f32(1)).all()
    want = _texel(inp, nr["txy"][hit])
    assert np.array_equal(albedo[hit, :3].view(np.uint32), want.view(np.uint32))
    rgba = out["rgba"].cpu().numpy().reshape(-1, 4)
    assert np.array_equal(albedo[~hit, :3].view(np.uint32), rgba[~hit, :3].view(np.uint32))   # sky: the frame's colour
    assert np.isposinf(depth[~hit]).all() and (ids[~hit] == -1).all()
    return a, nr


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["c2_160x90_n256", "c3_960x540_n1024", "c3_3840x2160", "mixed_160x96", "mesh_160x90",
                                  "inside_sphere", "duplicates", "tie"])
def test_aov_equal_nearest_of_the_primary_rays(rt, gpu, name, cull):
    inp, mesh, spheres, w, h = _case(rt, name)
    sc = _scene_of(rt, inp, mesh, spheres)
    y0, y1 = (1056, 1120) if (name == "c3_3840x2160" and not cull) else (0, 0)   # the whole lists at 4K: a band
    a, nr = _check_frame(rt, sc, inp, w, h, cull, y0, y1)
    kinds = set(nr["kind"].tolist())
    if name in ("c2_160x90_n256", "c3_960x540_n1024", "c3_3840x2160"):
        assert ({1} if y1 else {-1, 1}) <= kinds   # (the band through the sphere field has no sky)
    if name == "mixed_160x96":
        assert {1, 2, 3} <= kinds
    if name == "mesh_160x90":
        assert {0, 1} <= kinds
    if name == "inside_sphere":
        assert (a["depth"] < 0).any() and (a["id"][..., 1][a["depth"] < 0] == 5).any()
    if name == "duplicates":
        idx = a["id"][..., 1][a["id"][..., 0] == 1]
        assert (idx < 64).any() and not (idx >= 192).any()
    if name == "tie":
        sh, st = intersect(np.zeros((1, 3), f32), np.array([[0, 0, 1]], f32), sphere_table(inp.spheres, 1))
        assert sh[0, 0] and st[0, 0] == f32(9)                        # the sphere reports t = 9 on that ray too
        assert tuple(a["id"][80, 80]) == (0, 0) and a["depth"][80, 80] == f32(9)   # the mesh is tested first: it wins


@pytest.mark.parametrize("case", ["mixed", "mesh_spheres"])
def test_aov_equal_the_composed_reference(rt, oracle, gpu, case):
    """A second check, against query_ref's castRay (checked against oracle_render in test_query_cpu.py)."""
    import torch
    if case == "mixed":
        inp, mesh, w, h = mixed_scene(rt), None, 80, 48
    else:
        inp, mesh, w, h = Inputs(rt, 64), meshes.uv_sphere_obj(), 64, 36
    sc = _scene_of(rt, inp, mesh)
    ref = Q.CastRef(oracle, inp, mesh)
    P = sc.primary_rays(w, h, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6).cpu().numpy()
    rec = ref.nearest(np.ascontiguousarray(P[:, :3]), np.ascontiguousarray(P[:, 3:]))
    for cull in (True, False):
        out = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, cull=cull, aov=ALL)
        torch.cuda.synchronize()
        a = {k: v.cpu().numpy() for k, v in out["aov"].items()}
        assert np.array_equal(a["depth"].reshape(-1).view(np.uint32), rec["t"].view(np.uint32))
        assert np.array_equal(a["id"].reshape(-1, 2)[:, 0], rec["kind"])
        assert np.array_equal(a["id"].reshape(-1, 2)[:, 1], rec["index"])
        assert np.array_equal(a["normal"].reshape(-1, 4)[:, :3].view(np.uint32),
                              np.ascontiguousarray(rec["normal"]).view(np.uint32))
    kinds = set(rec["kind"].tolist())
    assert ({1, 2, 3} if case == "mixed" else {0, 1}) <= kinds   # (the mixed scene's planes cover the sky)


# ----------------------------------------------------------------------------- the colour does not change
def _colour(out):
    return {k: _bits(out[k]) for k in ("packed", "rgba", "packed24") if out.get(k) is not None}


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["c2_160x90_n256", "mixed_160x96", "mesh_160x90", "c3_3840x2160"])
def test_colour_outputs_unchanged(rt, gpu, name, cull):
    import torch
    inp, mesh, spheres, w, h = _case(rt, name)
    sc = _scene_of(rt, inp, mesh, spheres)
    y0, y1 = (1056, 1120) if (name == "c3_3840x2160" and not cull) else (0, 0)
    kw = dict(y0=y0, y1=y1, cam=inp.cam, aspect=inp.aspect, cull=bool(cull), want_packed24=True)
    plain = sc.render(w, h, **kw)
    with_aov = sc.render(w, h, aov=ALL, **kw)
    torch.cuda.synchronize()
    p, q = _colour(plain), _colour(with_aov)
    assert p.keys() == q.keys() == {"packed", "rgba", "packed24"}
    for k in p:
        assert np.array_equal(p[k], q[k]), k


@pytest.mark.parametrize("cull", [1, 0])
def test_reflective_frames_keep_their_colour_and_give_the_primary_guides(rt, gpu, cull):
    import torch
    n, w, h = 1024, 960, 540
    inp = Inputs(rt, n)
    sc = inp.scene()
    k = [0.6 if i % 4 == 1 else 0.0 for i in range(n)]
    tau = [0.7 if i % 4 == 2 else 0.0 for i in range(n)]
    sc.set_materials_ex(reflectivity=k, transparency=tau, ior=[1.5] * n)
    kw = dict(cam=inp.cam, aspect=inp.aspect, cull=bool(cull))
    refl = sc.render(w, h, reflect_depth=2, **kw)
    refl_aov = sc.render(w, h, reflect_depth=2, aov=ALL, **kw)
    flat_aov = sc.render(w, h, aov=ALL, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(refl["packed"]), _bits(refl_aov["packed"]))
    assert np.array_equal(_bits(refl["rgba"]), _bits(refl_aov["rgba"]))
    assert not np.array_equal(_bits(refl["packed"]), _bits(flat_aov["packed"]))   # the bounces did change the colour
    for key in ALL:
        assert np.array_equal(_bits(refl_aov["aov"][key]), _bits(flat_aov["aov"][key])), key


# ----------------------------------------------------------------------------- subsets and layout
def _buffers(w, rows):
    import torch
    return {"depth": torch.full((rows, w), SENTINEL, dtype=torch.int32, device="cuda"),
            "normal": torch.full((rows, w, 4), SENTINEL, dtype=torch.int32, device="cuda"),
            "id": torch.full((rows, w, 2), SENTINEL, dtype=torch.int32, device="cuda"),
            "albedo": torch.full((rows, w, 4), SENTINEL, dtype=torch.int32, device="cuda")}


def test_every_subset_and_untouched_buffers(rt, gpu):
    import torch
    inp, mesh, spheres, w, h = _case(rt, "mixed_160x96")
    sc = _scene_of(rt, inp, mesh, spheres)
    full = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=ALL)
    torch.cuda.synchronize()
    want = {k: _bits(v) for k, v in full["aov"].items()}
    for r in range(1, 5):
        for subset in itertools.combinations(ALL, r):
            bufs = _buffers(w, h)
            packed = torch.empty((h, w), dtype=torch.int32, device="cuda")
            fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), cam=inp.cam, aspect=inp.aspect,
                               **{f"aov_{k}": bufs[k].data_ptr() for k in subset})
            sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(packed), _bits(full["packed"]))
            for k in ALL:
                if k in subset:
                    assert np.array_equal(_bits(bufs[k]), want[k]), (subset, k)
                else:
                    assert (_bits(bufs[k]) == SENTINEL).all(), (subset, k)
    # the guides alone (no pixels, rgba or packed24): a frame of its own
    bufs = _buffers(w, h)
    fd = sc.frame_desc(w, h, cam=inp.cam, aspect=inp.aspect, **{f"aov_{k}": bufs[k].data_ptr() for k in ALL})
    sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(_bits(bufs[k]), want[k]), k


@pytest.mark.parametrize("cull", [1, 0])
def test_bands_interleave_and_accumulate_are_rows_of_the_frame(rt, gpu, cull):
    import torch
    inp = Inputs(rt, 256)
    sc = inp.scene()
    w, h = 160, 96
    kw = dict(cam=inp.cam, aspect=inp.aspect, cull=bool(cull))
    full = sc.render(w, h, aov=ALL, **kw)
    torch.cuda.synchronize()
    want = {k: v.cpu().numpy() for k, v in full["aov"].items()}
    cases = [((16, 48), None, list(range(16, 48))), ((31, 47), None, list(range(31, 47))),
             ((0, 0), (3, 1, 16), rt.interleaved_rows(h, 1, 3, 16)),
             ((16, 96), (2, 1, 16), [16 + r for r in rt.interleaved_rows(80, 1, 2, 16)])]
    for (y0, y1), il, rows in cases:
        out = sc.render(w, h, y0=y0, y1=y1, interleave=il, want_packed24=True, aov=ALL, **kw)
        torch.cuda.synchronize()
        for k in ALL:
            got = out["aov"][k].cpu().numpy()
            assert got.shape[0] == len(rows)
            assert np.array_equal(got.view(np.uint32), want[k][rows].view(np.uint32)), ((y0, y1), il, k)
    # accumulate: the colour adds into rgba, the guides are overwritten
    rgba = torch.ones((h, w, 4), dtype=torch.float32, device="cuda")
    bufs = _buffers(w, h)
    fd = sc.frame_desc(w, h, rgba=rgba.data_ptr(), accumulate=True, cam=inp.cam, aspect=inp.aspect, cull=bool(cull),
                       **{f"aov_{k}": bufs[k].data_ptr() for k in ALL})
    sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k in ALL:
        assert np.array_equal(_bits(bufs[k]), want[k].view(np.uint32)), k
    assert (rgba[..., 3] == 3.0).all()


def test_old_struct_size_and_fast(rt, gpu):
    import torch
    inp = Inputs(rt, 1024)
    sc = inp.scene()
    w, h = 960, 540
    plain = sc.render(w, h, cam=inp.cam, aspect=inp.aspect)
    torch.cuda.synchronize()
    # a caller built before the fields: they read as NULL (the sentinel stays), the frame is today's
    bufs = _buffers(w, h)
    packed = torch.empty((h, w), dtype=torch.int32, device="cuda")
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), cam=inp.cam, aspect=inp.aspect,
                       **{f"aov_{k}": bufs[k].data_ptr() for k in ALL})
    fd.struct_size = rt.FrameDesc.aov_depth.offset
    sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(packed), _bits(plain["packed"]))
    for k in ALL:
        assert (_bits(bufs[k]) == SENTINEL).all(), k
    # `fast` is ignored with the guides: the exact kernel runs (the approximate one differs at C3 in a few pixels)
    exact = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=ALL)
    fast = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=ALL, fast=True)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fast["packed"]), _bits(plain["packed"]))
    for key in ("packed", "rgba"):
        assert np.array_equal(_bits(exact[key]), _bits(fast[key])), key
    for k in ALL:
        assert np.array_equal(_bits(exact["aov"][k]), _bits(fast["aov"][k])), k


def test_drop_in_boundary_has_no_guides(rt, gpu):
    """The guides live in rt_frame_desc; rt_launch_raytrace_ex takes rt_launch_opts, whose layout is unchanged, so the
    drop-in boundary renders today's frame: the same colour as rt_scene_render's frame with and without guides."""
    import torch
    lib = rt.load_library()
    w, h, n = 160, 90, 256
    inp = Inputs(rt, n)
    obj = rt.Object()
    obj.sphere_count = n
    obj.d_spheres = C.cast(inp.spheres, C.POINTER(rt.Sphere))
    obj.texture = _managed_sprite(rt, inp.tex)
    sky = rt.Skybox()
    box = inp.sky_box
    sky.box = C.pointer(box)
    sky.skyboxTex = _managed_sprite(rt, inp.sky)
    pixels = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    assert not any(f[0].startswith("aov_") for f in rt.LaunchOpts._fields_) and C.sizeof(rt.LaunchOpts) == 112
    o = rt.LaunchOpts()
    o.struct_size = C.sizeof(rt.LaunchOpts)
    o.cull = -1
    assert lib.rt_launch_raytrace_ex(pixels.data_ptr(), w, h, inp.aspect, C.byref(obj), inp.lights, 3, inp.cam,
                                     C.byref(sky), None, C.byref(o)) == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    sc = inp.scene()
    plain, guided = sc.render(w, h), sc.render(w, h, aov=ALL)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pixels), _bits(plain["packed"]))
    assert np.array_equal(_bits(pixels), _bits(guided["packed"]))


def test_refusals_write_nothing(rt, gpu):
    import torch
    lib = rt.load_library()
    inp = Inputs(rt, 64)
    sc = inp.scene()
    w, h = 64, 32
    bufs = _buffers(w, h)
    packed = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    rgba = torch.full((h, w, 4), SENTINEL, dtype=torch.int32, device="cuda")
    stats = torch.zeros(rt.RT_STATS_COUNT, dtype=torch.int64, device="cuda")
    ptrs = {f"aov_{k}": bufs[k].data_ptr() for k in ALL}
    refused = [(dict(spp=2), 2), (dict(spp=2, sample_total=2), 2), (dict(sample_total=2), 2), (dict(tile=16), 2),
               (dict(tile=32), 2), (dict(tile=64), 2), (dict(stats=stats.data_ptr()), 2),
               (dict(stats=stats.data_ptr(), profile=True), 2), (dict(force_slow=True), 2)]
    for field in ALL:
        for extra, status in refused:
            fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(),
                               **{f"aov_{field}": bufs[field].data_ptr()}, **extra)
            assert lib.rt_scene_render(sc.handle, C.byref(fd), None) == status, (field, extra)
    for field, off in (("depth", 2), ("normal", 8), ("id", 4), ("albedo", 4)):
        fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), **{**ptrs, f"aov_{field}": bufs[field].data_ptr() + off})
        assert lib.rt_scene_render(sc.handle, C.byref(fd), None) == 1, field
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), **ptrs)
    assert not lib.rt_graph_capture(sc.handle, C.byref(fd), 1, None, None)
    assert b"aov_depth" in lib.rt_last_error()
    dev = (C.c_int * 1)(0)
    m = C.c_void_p()
    assert lib.rt_multi_create_ex(dev, 1, 2, C.byref(m)) == 0, lib.rt_last_error()
    try:
        assert lib.rt_multi_render(m, C.byref(fd), packed.data_ptr()) == 2
        assert b"aov_depth" in lib.rt_last_error()
        assert lib.rt_multi_sync(m) == 0
    finally:
        lib.rt_multi_destroy(m)
    torch.cuda.synchronize()
    for t in (packed, rgba, *bufs.values()):
        assert (_bits(t) == SENTINEL).all()
    assert (stats == 0).all()
