"""Mirror reflections on the device (rt_launch_opts.reflect_depth): no-op cases, the composed CPU reference,
BVH against brute force, adversarial scenes, bands, the drop-in boundary and the rejections."""
import ctypes as C

import numpy as np
import pytest

from scenes import Inputs
from test_reflect_cpu import Composer, composer_for

pytestmark = pytest.mark.gpu


def _bits(a):
    return a.cpu().numpy().view(np.uint32)


def _render(scene, w, h, **kw):
    import torch
    out = scene.render(w, h, **kw)
    torch.cuda.synchronize()
    return out["packed"].cpu().numpy().view(np.uint32), out["rgba"].cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _k_by_index(n, table=(0.0, 0.25, 0.5, 1.0)):
    return np.array([table[i % 4] for i in range(n)], dtype=np.float32)


@pytest.mark.parametrize("w,h,n", [(960, 540, 1024), (3840, 2160, 1024)])
def test_depth_zero_is_todays_frame(rt, gpu, w, h, n):
    scene = Inputs(rt, n).scene()
    plain = _render(scene, w, h)
    scene.set_materials(_k_by_index(n))
    assert _same(_render(scene, w, h, reflect_depth=0), plain)
    # a caller built against the older, shorter structs (struct_size without reflect_depth) gets the same frame
    import torch
    packed = torch.empty((h, w), dtype=torch.int32, device="cuda")
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=3)
    fd.opts.struct_size = rt.LaunchOpts.reflect_depth.offset
    scene.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(packed.cpu().numpy().view(np.uint32), plain[0])
    assert np.array_equal(rgba.cpu().numpy().view(np.uint32), plain[1].view(np.uint32))


def test_zero_materials_are_todays_frame(rt, gpu):
    scene = Inputs(rt, 1024).scene()
    plain = _render(scene, 960, 540)
    scene.set_materials(np.zeros(1024, dtype=np.float32))
    assert _same(_render(scene, 960, 540, reflect_depth=3), plain)
    assert _same(_render(scene, 960, 540, reflect_depth=3, cull=False), plain)


@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_against_composed_reference(rt, oracle, gpu, depth):
    inp = Inputs(rt, 256)
    k = _k_by_index(256)
    scene = inp.scene()
    scene.set_materials(k)
    got = _render(scene, 160, 90, reflect_depth=depth)
    ref_rgba, ref_packed = composer_for(oracle, rt, inp).render(160, 90, k, depth)
    assert np.array_equal(got[0], ref_packed)
    assert np.array_equal(got[1].view(np.uint32), ref_rgba.view(np.uint32))
    assert _same(_render(scene, 160, 90, reflect_depth=depth, cull=False), got)
    if depth == 1:   # reflections change the frame: some pixel differs from the plain one
        assert not np.array_equal(got[0], _render(scene, 160, 90)[0])


def test_c3_materials_bvh_equals_brute_and_reference(rt, oracle, gpu):
    n = 1024
    inp = Inputs(rt, n)
    k = np.array([0.5 if i % 4 == 0 else 0.0 for i in range(n)], dtype=np.float32)
    scene = inp.scene()
    scene.set_materials(k)
    culled = _render(scene, 3840, 2160, reflect_depth=3)
    brute = _render(scene, 3840, 2160, reflect_depth=3, cull=False)
    assert _same(culled, brute)
    y0, y1 = 1064, 1096
    ref_rgba, ref_packed = composer_for(oracle, rt, inp).render(3840, 2160, k, 3, y0=y0, y1=y1)
    assert np.array_equal(culled[0][y0:y1], ref_packed)
    assert np.array_equal(culled[1][y0:y1].view(np.uint32), ref_rgba.view(np.uint32))
    band = _render(scene, 3840, 2160, reflect_depth=3, y0=y0, y1=y1)
    assert _same(band, (culled[0][y0:y1], culled[1][y0:y1]))


def _normalise3(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _custom(rt, oracle, build, W, H):
    """A scene of the default's textures, lights and camera whose spheres `build(O, D, D0, right)` places relative to the
    camera's own primary rays (O: origin, D: [H*W, 3] directions, D0: the centre pixel's). It returns (centre, R, k)
    triples with R the EFFECTIVE radius: rt_sphere_init stores r*r and intersect() squares that again, so R = r^2."""
    inp = Inputs(rt, 1)
    O, D = Composer.primary(composer_for(oracle, rt, inp), W, H, 0, H)
    D0 = D[(H // 2) * W + W // 2].astype(np.float64)
    right = _normalise3(np.cross(D0, [0.0, 1.0, 0.0]))
    items = build(O[0].astype(np.float64), D, D0, right)
    n = len(items)
    arr = (rt.Sphere * n)()
    lib = rt.load_library()
    k = np.zeros(n, dtype=np.float32)
    for j, (c, R, kk) in enumerate(items):
        lib.rt_sphere_init(C.byref(arr[j]), float(c[0]), float(c[1]), float(c[2]), float(np.sqrt(R)))
        k[j] = kk
    inp.spheres, inp.n = arr, n
    return inp, k


def _facing_mirrors(O, D, D0, right):
    # two large mirrors (k = 1) side by side with a narrow gap, seen from outside: rays that enter the gap bounce from
    # one to the other until the depth runs out; a plain sphere behind the gap
    P = O + D0 * 14.0
    return [(P + right * 5.3, 5.0, 1.0), (P - right * 5.3, 5.0, 1.0), (P + D0 * 8.0, 1.0, 0.0)]


def _start_inside_overlap(O, D, D0, right):
    # the camera inside a mirror (k = 1) on purpose: every primary hit is the negative root on the mirror's far side
    # behind the camera, and where a second sphere overlaps that side the reflected ray STARTS INSIDE it, so bounce 1's
    # nearest hit there is that sphere's negative root
    return [(O + D0 * 1.0, 3.0, 1.0), (O - D0 * 3.0, 1.5, 0.5), (O - D0 * 3.0 + right * 1.2, 0.6, 1.0)]


def _duplicates(O, D, D0, right):
    P = O + D0 * 8.0
    return [(P, 1.5, 0.75), (P, 1.5, 0.25), (P + right * 3.2, 1.0, 1.0), (P + right * 3.2, 1.0, 0.5),
            (P - right * 3.0, 1.2, 0.0)]


def _grazing_and_sky(O, D, D0, right):
    # a mirror in the middle of the view: its silhouette pixels hit it nearly tangentially and reflect past it, most
    # reflected rays leave for the sky; two small spheres just outside the silhouette catch some grazing reflections
    P = O + D0 * 10.0
    return [(P, 2.0, 1.0), (P + right * 2.35, 0.2, 0.5), (P - right * 2.2 + D0 * 0.5, 0.15, 1.0)]


def _far_camera_tiny(O, D, D0, right):
    # 300 spheres of radius 0.01 .. 0.03, 40 .. 300 units away, each centred on some pixel's primary ray
    rng = np.random.default_rng(7)
    pix = rng.choice(D.shape[0], 300, replace=False)
    dist = rng.uniform(40.0, 300.0, 300)
    R = rng.uniform(0.01, 0.03, 300)
    return [(O + D[p].astype(np.float64) * d, r, (0.0, 0.5, 1.0)[i % 3]) for i, (p, d, r) in enumerate(zip(pix, dist, R))]


def _check_trace(name, tr, depth):
    """The case each scene is named for happens in the reference's own evaluation."""
    hits = [(b["index"] >= 0) for b in tr]
    if name == "facing_mirrors":
        assert len(tr) == depth + 1 and tr[depth]["index"].size > 0 and (tr[depth]["index"] <= 1).any() and \
            (tr[depth]["index"] >= 0).any(), "no ray is still between the mirrors when the depth runs out"
        assert (tr[0]["t"][hits[0]] > 0).all(), "the camera is outside every sphere"
    elif name == "start_inside_overlap":
        b1 = tr[1]
        assert ((b1["index"] >= 1) & (b1["t"] < 0)).any(), "no reflected ray starts inside the overlapping sphere"
    elif name == "duplicates":
        seen = set(tr[0]["index"].tolist()) | set(tr[1]["index"].tolist() if len(tr) > 1 else [])
        assert 0 in seen and 2 in seen and 1 not in seen and 3 not in seen, seen
    elif name == "grazing_and_sky":
        assert (tr[0]["cos"][tr[0]["index"] == 0] < 0.1).any(), "no grazing hit at the mirror's silhouette"
        assert (tr[1]["index"] < 0).any() and (tr[1]["index"] >= 0).any(), "reflected rays must reach both the sky and spheres"
    elif name == "far_camera_tiny":
        assert hits[0].sum() > 0 and len(tr) > 1 and tr[1]["index"].size > 0, "no tiny sphere is hit"


ADVERSARIAL = {"facing_mirrors": _facing_mirrors, "start_inside_overlap": _start_inside_overlap,
               "duplicates": _duplicates, "grazing_and_sky": _grazing_and_sky, "far_camera_tiny": _far_camera_tiny}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_scenes(rt, oracle, gpu, name):
    W, H, D = 160, 90, 4
    inp, k = _custom(rt, oracle, ADVERSARIAL[name], W, H)
    comp = composer_for(oracle, rt, inp)
    ref_rgba, ref_packed = comp.render(W, H, k, D)
    _check_trace(name, comp.trace, D)
    scene = inp.scene()
    scene.set_materials(k)
    culled = _render(scene, W, H, reflect_depth=D)
    queue = scene.reflect_stats()["queue"]
    assert queue == [b["index"].size for b in comp.trace[1:]] + [0] * (D + 1 - len(comp.trace))
    brute = _render(scene, W, H, reflect_depth=D, cull=False)
    assert _same(culled, brute)
    assert np.array_equal(culled[0], ref_packed)
    assert np.array_equal(culled[1].view(np.uint32), ref_rgba.view(np.uint32))


def test_bands_equal_the_full_frame(rt, gpu):
    n = 1024
    scene = Inputs(rt, n).scene()
    scene.set_materials(_k_by_index(n))
    full = _render(scene, 960, 540, reflect_depth=3)
    for y0, y1 in [(0, 17), (17, 300), (300, 540), (123, 124)]:
        band = _render(scene, 960, 540, reflect_depth=3, y0=y0, y1=y1)
        assert _same(band, (full[0][y0:y1], full[1][y0:y1])), (y0, y1)


def _managed_sprite(rt, planes):
    lib = rt.load_library()
    h, w = planes[0].shape
    bufs = []
    for p in planes:
        b = C.cast(lib.rt_managed_alloc(C.sizeof(rt.Buffer)), C.POINTER(rt.Buffer))
        d = lib.rt_managed_alloc(4 * w * h)
        C.memmove(d, np.ascontiguousarray(p, dtype=np.float32).ctypes.data, 4 * w * h)
        b.contents.data = C.cast(d, C.POINTER(C.c_float))
        b.contents.size = 4 * w * h
        bufs.append(b)
    sp = C.cast(lib.rt_managed_alloc(C.sizeof(rt.Sprite)), C.POINTER(rt.Sprite))
    sp.contents.rBuff, sp.contents.gBuff, sp.contents.bBuff = bufs
    sp.contents.width, sp.contents.height = w, h
    return sp


def test_drop_in_boundary(rt, gpu):
    import torch
    lib = rt.load_library()
    w, h, n = 160, 90, 256
    inp = Inputs(rt, n)
    obj = rt.Object()
    obj.sphere_count = n
    obj.d_spheres = C.cast(inp.spheres, C.POINTER(rt.Sphere))
    obj.texture = _managed_sprite(rt, inp.tex)
    mat = rt.Material(0.5, 0.0, 0.0)
    obj.mat = C.cast(C.pointer(mat), C.c_void_p)
    sky = rt.Skybox()
    box = inp.sky_box
    sky.box = C.pointer(box)
    sky.skyboxTex = _managed_sprite(rt, inp.sky)
    pixels = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    o = rt.LaunchOpts()
    o.struct_size = C.sizeof(rt.LaunchOpts)
    o.rgba = rgba.data_ptr()
    o.cull = -1
    o.reflect_depth = 2
    assert lib.rt_launch_raytrace_ex(pixels.data_ptr(), w, h, inp.aspect, C.byref(obj), inp.lights, 3, inp.cam,
                                     C.byref(sky), None, C.byref(o)) == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    scene = inp.scene()
    scene.set_materials([0.5] * n)
    want = _render(scene, w, h, reflect_depth=2)
    assert np.array_equal(_bits(pixels), want[0])
    assert np.array_equal(_bits(rgba), want[1].view(np.uint32))
    # without opts the object's material is ignored: today's frame
    assert lib.rt_launch_raytrace(pixels.data_ptr(), w, h, inp.aspect, C.byref(obj), inp.lights, 3, inp.cam,
                                  C.byref(sky), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pixels), _render(inp.scene(), w, h)[0])


def test_material_validation(rt, gpu):
    scene = Inputs(rt, 8).scene()
    for bad in (float("nan"), -0.25, 1.5):
        with pytest.raises(rt.RtError, match="status 1"):
            scene.set_materials([0.0] * 7 + [bad])
    with pytest.raises(rt.RtError, match="status 1"):
        scene.set_materials([0.5] * 7)
    with pytest.raises(rt.RtError, match="status 2"):
        scene.set_materials([rt.Material(0.5, 0.1, 0.0)] * 8)
    with pytest.raises(rt.RtError, match="status 2"):
        scene.set_materials([rt.Material(0.5, 0.0, 0.3)] * 8)
    scene.set_materials([0.5] * 8)
    # a list of the same count keeps the materials, another count clears them
    scene.set_spheres(rt.generate_spheres(8, 2), 8)
    a = _render(scene, 64, 64, reflect_depth=2)
    scene.set_spheres(rt.generate_spheres(9, 2), 9)
    scene.set_spheres(rt.generate_spheres(8, 2), 8)
    b = _render(scene, 64, 64, reflect_depth=2)
    assert _same(b, _render(scene, 64, 64))
    scene.set_materials([0.5] * 8)
    assert _same(_render(scene, 64, 64, reflect_depth=2), a)


def test_rejections_write_nothing(rt, gpu):
    import torch
    lib = rt.load_library()
    n = 64
    scene = Inputs(rt, n).scene()
    scene.set_materials([0.5] * n)
    w, h = 64, 64
    cases = [dict(spp=4), dict(accumulate=True), dict(interleave=(2, 0, 16)), dict(table_lds=True), dict(profile=True)]
    for kw in cases:
        packed = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
        rgba = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
        fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=2, **kw)
        rc = lib.rt_scene_render(scene.handle, C.byref(fd), None)
        torch.cuda.synchronize()
        assert rc == 2, kw
        assert bool((packed == 7).all()) and bool((rgba == 3.0).all()), kw
    p24 = torch.full((h, w * 3 // 4), 5, dtype=torch.int32, device="cuda")
    fd = scene.frame_desc(w, h, packed24=p24.data_ptr(), reflect_depth=1)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((p24 == 5).all())
    fd = scene.frame_desc(w, h, pixels=p24.data_ptr(), reflect_depth=9)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 1
    # planes in the scene
    planes = (rt.Plane * 1)()
    lib.rt_plane_init(C.byref(planes[0]), 0, -1, 0, 0, 1, 0)
    scene.set_planes(planes, 1)
    packed = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
    fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), reflect_depth=1)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((packed == 7).all())
    scene.set_planes(planes, 0)
    # cubes, then a mesh
    import meshes
    cubes = (rt.Cube * 1)()
    lib.rt_cube_init(C.byref(cubes[0]), 1, 0, 5, 2, 1, 6)
    scene.set_cubes(cubes, 1)
    fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), reflect_depth=1)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((packed == 7).all())
    scene.set_cubes(cubes, 0)
    mesh = rt.mesh_from_obj_text(meshes.uv_sphere_obj())
    scene.set_mesh(mesh)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((packed == 7).all())
    scene.set_mesh(None)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 0     # spheres only again: the frame renders
    torch.cuda.synchronize()
    assert not bool((packed == 7).all())
    # graphs and several devices (the multi-device path with one device and peer copies: no collective library)
    packed.fill_(7)
    assert not lib.rt_graph_capture(scene.handle, C.byref(fd), 1, None, None)
    assert b"reflect" in lib.rt_last_error()
    dev = (C.c_int * 1)(0)
    m = C.c_void_p()
    assert lib.rt_multi_create_ex(dev, 1, 2, C.byref(m)) == 0, lib.rt_last_error()
    try:
        assert lib.rt_multi_render(m, C.byref(fd), packed.data_ptr()) == 2
        assert lib.rt_multi_sync(m) == 0
        torch.cuda.synchronize()
        assert bool((packed == 7).all())
    finally:
        lib.rt_multi_destroy(m)


def test_fast_is_ignored_by_reflective_frames(rt, gpu):
    """opts.fast selects the approximate frame kernel; a reflective frame takes its L from the frame kernel, so it
    ignores `fast` and stays exact: the same bits with and without it at C3."""
    n = 1024
    scene = Inputs(rt, n).scene()
    scene.set_materials([0.5 if i % 4 == 0 else 0.0 for i in range(n)])
    exact = _render(scene, 3840, 2160, reflect_depth=3)
    assert _same(_render(scene, 3840, 2160, reflect_depth=3, fast=True), exact)
