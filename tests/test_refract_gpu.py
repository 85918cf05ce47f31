"""Refraction on the device (rt_scene_set_materials_ex): no-op cases, the glass composer of test_refract_cpu.py, BVH
against brute force, adversarial scenes, validation and the rejections."""
import ctypes as C

import numpy as np
import pytest

from scenes import Inputs
from test_reflect_cpu import Composer, composer_for, intersect, sphere_table
from test_refract_cpu import glass_composer_for

pytestmark = pytest.mark.gpu


def _render(scene, w, h, **kw):
    import torch
    out = scene.render(w, h, **kw)
    torch.cuda.synchronize()
    return out["packed"].cpu().numpy().view(np.uint32), out["rgba"].cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _k_by_index(n, table=(0.0, 0.25, 0.5, 1.0)):
    return np.array([table[i % 4] for i in range(n)], dtype=np.float32)


def _mixed(n, iors=(1.0, 1.33, 1.5, 2.4)):
    """Diffuse, mirror and glass spheres by index: per 8, diffuse, k 0.5, glass, k 1, diffuse, glass, k 0.25, glass;
    the glass spheres take tau 0.9, 0.5, 1 and the iors in turn."""
    k = np.zeros(n, dtype=np.float32)
    tau = np.zeros(n, dtype=np.float32)
    ior = np.zeros(n, dtype=np.float32)
    g = 0
    for i in range(n):
        j = i % 8
        if j in (1, 3, 6):
            k[i] = {1: 0.5, 3: 1.0, 6: 0.25}[j]
        elif j in (2, 5, 7):
            tau[i] = {2: 0.9, 5: 0.5, 7: 1.0}[j]
            ior[i] = iors[g % len(iors)]
            g += 1
    return k, tau, ior


def _queue_of(trace, depth):
    return [b["index"].size for b in trace[1:]] + [0] * (depth + 1 - len(trace))


@pytest.mark.parametrize("w,h", [(960, 540), (3840, 2160)])
def test_no_glass_is_the_mirror_frame(rt, gpu, w, h):
    n = 1024
    scene = Inputs(rt, n).scene()
    k = _k_by_index(n)
    scene.set_materials(k)
    want = [_render(scene, w, h, reflect_depth=3), _render(scene, w, h, reflect_depth=3, cull=False)]
    scene.set_materials_ex(reflectivity=k, transparency=np.zeros(n), ior=np.zeros(n))
    assert _same(_render(scene, w, h, reflect_depth=3), want[0])
    assert _same(_render(scene, w, h, reflect_depth=3, cull=False), want[1])
    # any material at reflect_depth 0 is the plain frame
    plain = _render(scene, w, h)
    kk, tau, ior = _mixed(n)
    scene.set_materials_ex(kk, tau, ior)
    assert _same(_render(scene, w, h, reflect_depth=0), plain)
    # and the old entry after glass sets every tau to 0 again
    scene.set_materials(k)
    assert _same(_render(scene, w, h, reflect_depth=3), want[0])


@pytest.mark.parametrize("depth,iors", [(d, (1.0, 1.33, 1.5, 2.4)) for d in (1, 2, 3, 8)] +
                         [(3, (x,)) for x in (1.0, 1.33, 1.5, 2.4)])
def test_against_glass_composer(rt, oracle, gpu, depth, iors):
    n = 256
    inp = Inputs(rt, n)
    k, tau, ior = _mixed(n, iors)
    scene = inp.scene()
    scene.set_materials_ex(k, tau, ior)
    comp = glass_composer_for(oracle, rt, inp)
    ref_rgba, ref_packed = comp.render(160, 90, k, depth, tau=tau, ior=ior)
    assert (np.concatenate([b["rule"] for b in comp.trace]) == 4).any()        # some rays pass through glass
    got = _render(scene, 160, 90, reflect_depth=depth)
    assert scene.reflect_stats()["queue"] == _queue_of(comp.trace, depth)
    assert np.array_equal(got[0], ref_packed)
    assert np.array_equal(got[1].view(np.uint32), ref_rgba.view(np.uint32))
    brute = _render(scene, 160, 90, reflect_depth=depth, cull=False)
    assert scene.reflect_stats()["queue"] == _queue_of(comp.trace, depth)
    assert _same(brute, got)


def test_c3_glass_bvh_equals_brute_and_composer(rt, oracle, gpu):
    n = 1024
    inp = Inputs(rt, n)
    k = np.array([0.5 if i % 4 == 2 else 0.0 for i in range(n)], dtype=np.float32)
    tau = np.array([0.9 if i % 4 == 0 else 0.0 for i in range(n)], dtype=np.float32)
    ior = np.full(n, 1.5, dtype=np.float32)
    scene = inp.scene()
    scene.set_materials_ex(k, tau, ior)
    culled = _render(scene, 3840, 2160, reflect_depth=3)
    brute = _render(scene, 3840, 2160, reflect_depth=3, cull=False)
    assert _same(culled, brute)
    y0, y1 = 1064, 1096
    comp = glass_composer_for(oracle, rt, inp)
    ref_rgba, ref_packed = comp.render(3840, 2160, k, 3, y0=y0, y1=y1, tau=tau, ior=ior)
    assert (comp.trace[0]["rule"] == 4).any()
    assert np.array_equal(culled[0][y0:y1], ref_packed)
    assert np.array_equal(culled[1][y0:y1].view(np.uint32), ref_rgba.view(np.uint32))


# ----------------------------------------------------------------------------- adversarial scenes
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _custom_glass(rt, oracle, build, W, H):
    """A scene of the default's textures, lights and camera whose spheres `build(O, D, D0, right, up)` places relative to
    the camera's own primary rays. It returns (centre, R, k, tau, ior) with R the EFFECTIVE radius (rt_sphere_init
    stores r*r and intersect() squares that again, so R = r^2)."""
    inp = Inputs(rt, 1)
    O, D = Composer.primary(composer_for(oracle, rt, inp), W, H, 0, H)
    D0 = D[(H // 2) * W + W // 2].astype(np.float64)
    right = _unit(np.cross(D0, [0.0, 1.0, 0.0]))
    up = _unit(np.cross(right, D0))
    items = build(O[0].astype(np.float64), D, D0, right, up)
    n = len(items)
    arr = (rt.Sphere * n)()
    lib = rt.load_library()
    k, tau, ior = (np.zeros(n, dtype=np.float32) for _ in range(3))
    for j, (c, R, kk, tt, ii) in enumerate(items):
        lib.rt_sphere_init(C.byref(arr[j]), float(c[0]), float(c[1]), float(c[2]), float(np.sqrt(R)))
        k[j], tau[j], ior[j] = kk, tt, ii
    inp.spheres, inp.n = arr, n
    return inp, k, tau, ior


def _camera_inside(O, D, D0, right, up):
    # the camera inside a glass sphere: every primary ray meets it at intersect()'s negative near root behind the
    # camera, where dot(D, N) < 0, so it enters there, crosses the whole sphere and leaves ahead; a diffuse sphere and
    # a mirror outside
    return [(O + D0 * 0.5, 3.0, 0.0, 0.8, 1.5), (O + D0 * 8.0, 1.5, 0.0, 0.0, 0.0),
            (O + D0 * 7.0 + right * 3.0, 1.0, 1.0, 0.0, 0.0)]


def _overlap_diffuse(O, D, D0, right, up):
    # a diffuse sphere inside a glass sphere's interior: the chord passes through it and does not see it
    P = O + D0 * 10.0
    return [(P, 2.5, 0.0, 0.9, 1.5), (P + right * 0.8 + D0 * 0.5, 1.0, 0.0, 0.0, 0.0),
            (P + D0 * 9.0, 3.0, 0.0, 0.0, 0.0)]


def _grazing(O, D, D0, right, up):
    # glass spheres each tangent to one pixel's primary ray (offset R (1 - delta) from it): entries at grazing
    # incidence, where the exit radicand cos^2(theta_i) rounds to <= 0 or dot(D, N) rounds to >= 0 (rule 1)
    rng = np.random.default_rng(3)
    pix = rng.choice(D.shape[0], 240, replace=False)
    out = []
    for i, p in enumerate(pix):
        d = _unit(D[p])
        side = _unit(np.cross(d, rng.standard_normal(3)))
        R = rng.uniform(0.05, 0.4)
        delta = (0.0, 1e-7, 1e-6, 1e-5, 3e-5, -1e-7)[i % 6]
        c = O + d * rng.uniform(4.0, 20.0) + side * (R * (1.0 - delta))
        out.append((c, R, 0.0, 0.9, (1.0, 1.33, 1.5, 2.4)[i % 4]))
    return out


def _tiny_degenerate(O, D, D0, right, up):
    # glass spheres of radius 1e-6 .. 4e-6 a millimetre from the camera on pixel rays: P = new_org - 1e-5 N lies beyond
    # them, so no positive far root (rule 3); a diffuse backdrop
    rng = np.random.default_rng(5)
    pix = rng.choice(D.shape[0], 200, replace=False)
    out = [(O + _unit(D[p]) * 1e-3, rng.uniform(1e-6, 4e-6), 0.0, 0.9, 1.5) for p in pix]
    out.append((O + D0 * 30.0, 12.0, 0.0, 0.0, 0.0))
    return out


def _chains(O, D, D0, right, up):
    # glass -> mirror -> glass: a glass sphere in front of a large mirror that sends the rays back through it; two
    # glass spheres in contact; a row of five glass spheres in which rays run out of depth
    P = O + D0 * 8.0
    items = [(P - right * 2.5, 1.2, 0.0, 0.9, 1.5), (P - right * 2.5 + D0 * 6.0, 3.0, 1.0, 0.0, 0.0)]
    items += [(P + right * 0.6, 1.0, 0.0, 0.8, 1.33), (P + right * 0.6 + D0 * 2.0, 1.0, 0.0, 0.7, 2.4)]
    for j in range(5):
        items.append((P + right * 3.2 + up * 0.5 + D0 * (1.2 * j), 0.6, 0.0, 1.0, 1.5))
    return items


def _far_tiny(O, D, D0, right, up):
    # 300 spheres of radius 0.01 .. 0.03, 40 .. 300 units away, each centred on some pixel's primary ray
    rng = np.random.default_rng(7)
    pix = rng.choice(D.shape[0], 300, replace=False)
    dist = rng.uniform(40.0, 300.0, 300)
    R = rng.uniform(0.01, 0.03, 300)
    mats = [(0.0, 0.9, 1.5), (0.5, 0.0, 0.0), (0.0, 1.0, 2.4), (0.0, 0.0, 0.0)]
    return [(O + D[p].astype(np.float64) * d, r, *mats[i % 4]) for i, (p, d, r) in enumerate(zip(pix, dist, R))]


def _pixel_paths(tr):
    """pixel -> the sphere index met at each bounce"""
    paths = {}
    for b in tr:
        for p, i in zip(b["pix"].tolist(), b["index"].tolist()):
            paths.setdefault(p, []).append(i)
    return paths


def _check_trace(name, comp, tau, depth):
    """The case each scene is named for happens in the composer's own evaluation."""
    tr = comp.trace
    if name == "camera_inside":
        on0 = tr[0]["index"] == 0
        assert on0.any() and (tr[0]["t"][on0] < 0).all(), "the camera is not inside the glass sphere"
        assert (tr[0]["rule"][on0] == 4).sum() > on0.sum() // 2, "rays from inside do not pass through"
    elif name == "overlap_diffuse":
        ok = False
        for b in tr:
            sel = b["rule"] == 4
            if not sel.any():
                continue
            hit, t = intersect(b["P"][sel], b["T"][sel], comp.tab[1:2])
            ok = ok or bool((hit[:, 0] & (t[:, 0] > 0) & (t[:, 0] < b["t1"][sel])).any())
        assert ok, "no chord passes through the diffuse sphere"
    elif name == "grazing":
        rules = np.concatenate([b["rule"] for b in tr])
        assert (rules == 1).any(), "no grazing hit takes rule 1"
        assert np.concatenate([b["clamp"] for b in tr]).any(), "no refract radicand clamps"
    elif name == "tiny_degenerate":
        assert (tr[0]["rule"] == 3).sum() > 10, "no degenerate tiny sphere takes rule 3"
    elif name == "chains":
        paths = _pixel_paths(tr)
        glass = set(np.nonzero(tau > 0)[0].tolist())
        gmg = any(any(a in glass and b == 1 and c in glass for a, b, c in zip(q, q[1:], q[2:])) for q in paths.values())
        assert gmg, "no glass -> mirror -> glass chain"
        assert any(any(a == 2 and b == 3 for a, b in zip(q, q[1:])) for q in paths.values()), "no pass from 2 into 3"
        assert len(tr) == depth + 1 and np.isin(tr[depth]["index"], list(glass)).any(), "no ray runs out of depth in glass"
    elif name == "far_tiny":
        assert (tr[0]["index"] >= 0).sum() > 0 and (tr[0]["rule"] == 4).any(), "no tiny glass sphere is passed"


ADVERSARIAL = {"camera_inside": _camera_inside, "overlap_diffuse": _overlap_diffuse, "grazing": _grazing,
               "tiny_degenerate": _tiny_degenerate, "chains": _chains, "far_tiny": _far_tiny}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_scenes(rt, oracle, gpu, name):
    W, H, D = 160, 90, 4
    inp, k, tau, ior = _custom_glass(rt, oracle, ADVERSARIAL[name], W, H)
    comp = glass_composer_for(oracle, rt, inp)
    ref_rgba, ref_packed = comp.render(W, H, k, D, tau=tau, ior=ior)
    _check_trace(name, comp, tau, D)
    scene = inp.scene()
    scene.set_materials_ex(k, tau, ior)
    culled = _render(scene, W, H, reflect_depth=D)
    assert scene.reflect_stats()["queue"] == _queue_of(comp.trace, D)
    brute = _render(scene, W, H, reflect_depth=D, cull=False)
    assert _same(culled, brute)
    assert np.array_equal(culled[0], ref_packed)
    assert np.array_equal(culled[1].view(np.uint32), ref_rgba.view(np.uint32))


# ----------------------------------------------------------------------------- validation and rejections
def test_material_ex_validation(rt, gpu):
    n = 8
    scene = Inputs(rt, n).scene()
    M = rt.MaterialEx
    good = [M(0.0, 0.9, 0.0, 1.5)] * n
    scene.set_materials_ex(good)
    a = _render(scene, 64, 64, reflect_depth=2)
    bad_invalid = [M(float("nan"), 0, 0, 0), M(-0.1, 0, 0, 0), M(1.5, 0, 0, 0), M(0, float("nan"), 0, 1.5),
                   M(0, -0.5, 0, 1.5), M(0, 1.5, 0, 1.5), M(0, 0.5, 0, float("nan")), M(0, 0.5, 0, 0.99),
                   M(0, 0.5, 0, 4.5), M(0, 0.5, 0, float("inf")), M(0, 0.5, 0, 0.0)]
    for bad in bad_invalid:
        with pytest.raises(rt.RtError, match="status 1"):
            scene.set_materials_ex([M(0, 0, 0, 0)] * 7 + [bad])
    with pytest.raises(rt.RtError, match="status 1"):
        scene.set_materials_ex(good[:7])
    for bad in (M(0.5, 0.5, 0, 1.5), M(0, 0.5, 0.3, 1.5), M(0.5, 0, 0.3, 0)):
        with pytest.raises(rt.RtError, match="status 2"):
            scene.set_materials_ex([M(0, 0, 0, 0)] * 7 + [bad])
    # nothing changed: the same frame as before the rejected calls; ior is ignored where tau == 0
    assert _same(_render(scene, 64, 64, reflect_depth=2), a)
    scene.set_materials_ex([M(0, 0, 0, float("nan"))] * n)
    assert _same(_render(scene, 64, 64, reflect_depth=2), _render(scene, 64, 64))
    # the old entry still refuses transperancy (it has no ior)
    with pytest.raises(rt.RtError, match="status 2"):
        scene.set_materials([rt.Material(0.0, 0.5, 0.0)] * n)
    # a list of the same count keeps the materials, another count clears them
    scene.set_materials_ex(good)
    scene.set_spheres(rt.generate_spheres(8, 2), 8)
    b = _render(scene, 64, 64, reflect_depth=2)
    assert not _same(b, _render(scene, 64, 64))
    scene.set_spheres(rt.generate_spheres(9, 2), 9)
    scene.set_spheres(rt.generate_spheres(8, 2), 8)
    assert _same(_render(scene, 64, 64, reflect_depth=2), _render(scene, 64, 64))
    scene.set_materials_ex(good)
    assert _same(_render(scene, 64, 64, reflect_depth=2), b)
    scene.set_materials_ex(None)
    assert _same(_render(scene, 64, 64, reflect_depth=2), _render(scene, 64, 64))


def test_rejections_with_glass_write_nothing(rt, gpu):
    import torch
    lib = rt.load_library()
    n = 64
    scene = Inputs(rt, n).scene()
    k, tau, ior = _mixed(n)
    scene.set_materials_ex(k, tau, ior)
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
    packed = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
    planes = (rt.Plane * 1)()
    lib.rt_plane_init(C.byref(planes[0]), 0, -1, 0, 0, 1, 0)
    scene.set_planes(planes, 1)
    fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), reflect_depth=1)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((packed == 7).all())
    scene.set_planes(planes, 0)
    import meshes
    cubes = (rt.Cube * 1)()
    lib.rt_cube_init(C.byref(cubes[0]), 1, 0, 5, 2, 1, 6)
    scene.set_cubes(cubes, 1)
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((packed == 7).all())
    scene.set_cubes(cubes, 0)
    scene.set_mesh(rt.mesh_from_obj_text(meshes.uv_sphere_obj()))
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((packed == 7).all())
    scene.set_mesh(None)
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
    assert lib.rt_scene_render(scene.handle, C.byref(fd), None) == 0     # spheres only again: the frame renders
    torch.cuda.synchronize()
    assert not bool((packed == 7).all())
