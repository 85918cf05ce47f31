"""Reflective frames over the whole scene on the device (rt_scene_set_reflect_scope(RT_REFLECT_SCENE)):
parity with the composed reference of tests/reflect_scene_ref.py, the cases the scene is staged for, a scene without
spheres, the scope switch, untouched pixels, bands, the life cycle of the plane / cube materials and the rejections.
Everything is bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import meshes
from reflect_scene_ref import CUBE, PLANE, SPHERE, TRIANGLE, SceneComposer, chain, met, runs
from scenes import Inputs, Scn
from test_reflect_cpu import composer_for

pytestmark = pytest.mark.gpu

W, H = 64, 48
DEPTHS = (1, 2, 3, 8)
SKY = -1
# list positions in the staged scene
MIRROR, GLASS, UNDER = 0, 1, 4           # spheres: the mirror on the floor, the glass one, the mirror under the floor
FLOOR, SLAB, POST = 0, 0, 1              # plane 0; cube 0 (k = 0.6, a flat slab), cube 1


def _render(scene, w, h, **kw):
    import torch
    out = scene.render(w, h, **kw)
    torch.cuda.synchronize()
    return out["packed"].cpu().numpy().view(np.uint32), out["rgba"].cpu().numpy()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _stage(rt, oracle):
    """About 48 spheres, a floor, two cubes and a 12-triangle box, placed along the camera's own primary rays: pixel
    (x, y)'s ray meets the floor y = 0 at F(x, y) (the rows below the horizon, 0 .. 19, row 0 nearest; x runs against
    the world's)."""
    O, D = composer_for(oracle, rt, Inputs(rt, 1)).primary(W, H, 0, H)
    O = O[0].astype(np.float64)

    def F(x, y):
        d = D[y * W + x].astype(np.float64)
        return O + d * (-O[1] / d[1])

    up = np.array([0.0, 1.0, 0.0])
    spheres = [None] * 5                 # (centre, effective radius)
    spheres[MIRROR] = (F(32, 8) + up * 1.4, 1.4)          # rests on the floor in the middle of the view
    spheres[GLASS] = (F(50, 5) + up * 0.3, 1.1)          # sunk into the floor: part of every chord ends below it
    spheres[2] = (F(12, 3) + up * 0.5, 0.5)
    spheres[3] = (F(58, 11) + up * 0.4, 0.4)
    g = spheres[GLASS][0]
    spheres[UNDER] = (g + np.array([0.0, -3.5, -1.2]), 3.0)  # wholly under the floor, behind and below the glass sphere
    rng = np.random.default_rng(11)
    while len(spheres) < 48:             # small ones at the back of the floor
        x, y = int(rng.integers(0, W)), int(rng.integers(10, 15))
        r = float(rng.uniform(0.3, 0.6))
        spheres.append((F(x, y) + up * r, r))
    m = spheres[MIRROR][0]
    # a flat slab beside the mirror (hit - centre is far from the faces' normals near its ends) and a post farther out
    slab = (m[0] + 1.6, 0.0, m[2] - 1.0, m[0] + 3.8, 0.7, m[2] + 3.0)
    post = (m[0] + 4.5, 0.0, m[2] - 1.0, m[0] + 5.5, 1.5, m[2])
    mesh = meshes.box_obj_no_normals(m[0] - 3.2, 0.0, m[2] + 0.4, 1.6)          # 12 triangles left of the mirror
    inp = Scn(rt, [(c[0], c[1], c[2], np.sqrt(r)) for c, r in spheres], planes=[(0, 0, 0, 0, 1, 0)], cubes=[slab, post])
    n = len(spheres)
    k = np.array([0.5 if i % 4 == 0 else 0.0 for i in range(n)], dtype=np.float32)
    tau = np.zeros(n, dtype=np.float32)
    ior = np.zeros(n, dtype=np.float32)
    tau[GLASS], ior[GLASS] = 0.9, 1.5
    mats = {"k_sphere": k, "tau": tau, "ior": ior, "k_plane": np.array([0.3], dtype=np.float32),
            "k_cube": np.array([0.6, 0.0], dtype=np.float32)}
    return inp, mesh, mats


@functools.lru_cache(maxsize=None)
def _reference(rt, oracle):
    """The staged scene's frames at every depth of DEPTHS, from one walk of the reference; (frames, trace)."""
    inp, mesh, mats = _stage(rt, oracle)
    comp = SceneComposer(oracle, rt, inp, mesh)
    frames = comp.render_depths(W, H, DEPTHS, **mats)
    return frames, comp.trace


def _scene(rt, inp, mesh=None, mats=None, scope="scene"):
    sc = inp.scene()
    if mesh is not None:
        sc.set_mesh(rt.mesh_from_obj_text(mesh))
    if mats is not None:
        sc.set_materials_ex(mats["k_sphere"], mats["tau"], mats["ior"])
        sc.set_plane_materials(mats["k_plane"])
        sc.set_cube_materials(mats["k_cube"])
    sc.set_reflect_scope(scope)
    return sc


@functools.lru_cache(maxsize=None)
def _staged_scene(rt, oracle):
    inp, mesh, mats = _stage(rt, oracle)
    return _scene(rt, inp, mesh, mats)


# ----------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("depth", DEPTHS)
def test_parity_with_the_composed_reference(rt, oracle, gpu, depth):
    frames, _ = _reference(rt, oracle)
    ref_rgba, ref_packed, ref_queue = frames[depth]
    sc = _staged_scene(rt, oracle)
    got = _render(sc, W, H, reflect_depth=depth)
    queue = sc.reflect_stats()["queue"]
    brute = _render(sc, W, H, reflect_depth=depth, cull=False)
    brute_queue = sc.reflect_stats()["queue"]
    assert ref_queue[0] > 0 and (depth < 3 or ref_queue[2] > 0)
    assert queue == ref_queue and brute_queue == ref_queue
    for name, frame in (("cull", got), ("brute", brute)):
        bad = int((frame[1].view(np.uint32) != ref_rgba.view(np.uint32)).any(axis=2).sum())
        assert bad == 0, (name, bad)
        assert np.array_equal(frame[0], ref_packed), name


# ----------------------------------------------------------------------------- 2. the cases happen
def _case_counts(tr):
    """Rays of each case the scene is staged for, in the reference's trace."""
    floor = (PLANE, FLOOR)
    count = {
        "floor -> sphere": runs(tr, [floor, SPHERE]),
        "sphere -> floor": runs(tr, [SPHERE, floor]),
        "sphere -> cube": runs(tr, [SPHERE, CUBE]),
        "sphere -> triangle": runs(tr, [SPHERE, TRIANGLE]),
        "floor -> sphere -> floor": runs(tr, [floor, SPHERE, floor]),
        "floor -> sky": runs(tr, [floor, SKY]),
        "glass -> floor": int((met(tr, 1, PLANE, FLOOR) & np.isin(tr[1]["pix"], tr[0]["pix"][tr[0]["rule"] == 4])).sum()),
        "cube -> the same cube": runs(tr, [(CUBE, SLAB), (CUBE, SLAB)]),
    }
    # a reflected ray that starts below the floor, heads up and ends above it (or in the sky): it passed the floor's back
    through = 0
    for b in tr[1:]:
        below = (b["O"][:, 1] < 0) & (b["D"][:, 1] > 0)
        through += int((below & ((b["kind"] == SKY) | (b["hp"][:, 1] > 0))).sum())
    count["from under the floor through its back side"] = through
    count["a bounce hit shadowed by a non-sphere only"] = sum(int(b["shadow_nonsphere"].sum()) for b in tr[1:])
    return count


def test_the_staged_cases_happen_in_the_reference(rt, oracle, gpu):
    """Each case the scene is staged for, counted in the reference's own trace of the depth-8 walk (at least 8 rays
    each), then the device's frame at that depth against the reference."""
    frames, tr = _reference(rt, oracle)
    count = _case_counts(tr)
    assert min(count.values()) >= 8, count
    ref_rgba, ref_packed, _ = frames[8]
    got = _render(_staged_scene(rt, oracle), W, H, reflect_depth=8)
    assert np.array_equal(got[0], ref_packed)
    assert np.array_equal(got[1].view(np.uint32), ref_rgba.view(np.uint32))


# ----------------------------------------------------------------------------- 3. no spheres
def test_a_scene_without_spheres(rt, oracle, gpu):
    inp = Scn(rt, [], planes=[(0, 0, 0, 0, 1, 0)], cubes=[(3.2, 0.0, -3.0, 5.0, 1.6, -1.4)])
    comp = SceneComposer(oracle, rt, inp)
    kp, kc = np.array([0.5], dtype=np.float32), np.array([0.4], dtype=np.float32)
    ref_rgba, ref_packed, ref_queue = comp.render(W, H, 3, k_plane=kp, k_cube=kc)
    assert chain(comp.trace, [(PLANE, 0), (CUBE, 0)]).size >= 8 and chain(comp.trace, [(CUBE, 0), (PLANE, 0)]).size >= 8
    sc = inp.scene()
    sc.set_reflect_scope("scene")
    sc.set_plane_materials(kp)
    sc.set_cube_materials(kc)
    for cull in (True, False):
        got = _render(sc, W, H, reflect_depth=3, cull=cull)
        assert sc.reflect_stats()["queue"] == ref_queue
        assert np.array_equal(got[0], ref_packed), cull
        assert np.array_equal(got[1].view(np.uint32), ref_rgba.view(np.uint32)), cull


# ----------------------------------------------------------------------------- 4. scope
def test_scope_on_spheres_only_and_back(rt, gpu):
    import torch
    lib = rt.load_library()
    n = 96
    sc = Inputs(rt, n).scene()
    sc.set_materials_ex([0.5 if i % 4 == 0 else 0.0 for i in range(n)], [0.8 if i % 4 == 1 else 0.0 for i in range(n)],
                        [1.5 if i % 4 == 1 else 0.0 for i in range(n)])
    a = _render(sc, W, H, reflect_depth=3)
    qa = sc.reflect_stats()["queue"]
    sc.set_reflect_scope("scene")
    b = _render(sc, W, H, reflect_depth=3)
    assert qa[0] > 0 and sc.reflect_stats()["queue"] == qa
    assert _same(a, b)
    # scene, then spheres: the refusal of planes is back and writes nothing
    planes = (rt.Plane * 1)()
    lib.rt_plane_init(C.byref(planes[0]), 0, -1, 0, 0, 1, 0)
    sc.set_planes(planes, 1)
    packed = torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    rgba = torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda")
    fd = sc.frame_desc(W, H, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=2)
    assert lib.rt_scene_render(sc.handle, C.byref(fd), None) == 0          # under "scene" the frame renders
    torch.cuda.synchronize()
    assert not bool((packed == 7).all())
    sc.set_reflect_scope("spheres")
    packed.fill_(7)
    rgba.fill_(3.0)
    assert lib.rt_scene_render(sc.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((packed == 7).all()) and bool((rgba == 3.0).all())
    with pytest.raises(rt.RtError, match="status 1"):
        sc.set_reflect_scope(2)
    with pytest.raises(rt.RtError):
        sc.set_reflect_scope("planes")


# ----------------------------------------------------------------------------- 5. untouched pixels
def test_untouched_pixels_are_the_plain_frame(rt, oracle, gpu):
    _, tr = _reference(rt, oracle)
    inp, mesh, mats = _stage(rt, oracle)
    sc = _staged_scene(rt, oracle)
    plain = _render(sc, W, H)
    refl = _render(sc, W, H, reflect_depth=3)
    kind, index = tr[0]["kind"], tr[0]["index"]
    k = np.zeros(W * H, dtype=np.float32)
    for code, tab in ((SPHERE, np.maximum(mats["k_sphere"], mats["tau"])), (PLANE, mats["k_plane"]), (CUBE, mats["k_cube"])):
        sel = kind == code
        k[sel] = tab[index[sel]]
    still = (k == 0).reshape(H, W)
    assert (kind == SKY).sum() >= 8 and (kind == TRIANGLE).sum() >= 8 and ((kind == CUBE) & (k == 0)).sum() >= 8 and \
        ((kind == SPHERE) & (k == 0)).sum() >= 8
    assert np.array_equal(refl[0][still], plain[0][still])
    assert np.array_equal(refl[1].view(np.uint32)[still], plain[1].view(np.uint32)[still])
    assert not np.array_equal(refl[0][~still], plain[0][~still])


# ----------------------------------------------------------------------------- 6. bands
def test_bands_equal_the_full_frame(rt, oracle, gpu):
    sc = _staged_scene(rt, oracle)
    full = _render(sc, W, H, reflect_depth=3)
    for y0, y1 in [(0, 17), (17, 40), (40, 48), (29, 30)]:
        band = _render(sc, W, H, reflect_depth=3, y0=y0, y1=y1)
        assert _same(band, (full[0][y0:y1], full[1][y0:y1])), (y0, y1)


# ----------------------------------------------------------------------------- 7. material life cycle, guides
def test_material_life_cycle_and_guides(rt, oracle, gpu):
    lib = rt.load_library()
    inp, mesh, mats = _stage(rt, oracle)
    sc = _scene(rt, inp, mesh, mats)
    want = _render(sc, W, H, reflect_depth=2)
    # lists of the same count keep the tables
    sc.set_planes(inp.planes, inp.n_planes)
    sc.set_cubes(inp.cubes, inp.n_cubes)
    assert _same(_render(sc, W, H, reflect_depth=2), want)
    # another count clears a table: the frame is the one with that table's k = 0
    zero_p = _scene(rt, inp, mesh, dict(mats, k_plane=np.zeros(1, dtype=np.float32)))
    no_plane_k = _render(zero_p, W, H, reflect_depth=2)
    assert not _same(no_plane_k, want)
    two = (rt.Plane * 2)()
    two[0] = inp.planes[0]
    lib.rt_plane_init(C.byref(two[1]), 0, -50, 0, 0, 1, 0)
    sc.set_planes(two, 2)
    sc.set_planes(inp.planes, 1)
    assert _same(_render(sc, W, H, reflect_depth=2), no_plane_k)
    sc.set_plane_materials(mats["k_plane"])
    assert _same(_render(sc, W, H, reflect_depth=2), want)
    zero_c = _scene(rt, inp, mesh, dict(mats, k_cube=np.zeros(2, dtype=np.float32)))
    no_cube_k = _render(zero_c, W, H, reflect_depth=2)
    assert not _same(no_cube_k, want)
    sc.set_cubes(inp.cubes, 1)
    sc.set_cubes(inp.cubes, 2)
    assert _same(_render(sc, W, H, reflect_depth=2), no_cube_k)
    sc.set_cube_materials(mats["k_cube"])
    assert _same(_render(sc, W, H, reflect_depth=2), want)
    # validation with real lists: nothing changes on an error
    for bad in ([0.3, 0.2], [float("nan")], [1.5]):
        with pytest.raises(rt.RtError, match="status 1"):
            sc.set_plane_materials(bad)
    with pytest.raises(rt.RtError, match="status 2"):
        sc.set_cube_materials([rt.Material(0.5, 0.1, 0.0), rt.Material(0.0, 0.0, 0.0)])
    with pytest.raises(rt.RtError, match="status 1"):
        sc.set_cube_materials([0.5])
    assert _same(_render(sc, W, H, reflect_depth=2), want)
    # the guides of a reflective frame are those of the primary hit: the plain frame's
    names = ("depth", "normal", "id", "albedo")
    refl = sc.render(W, H, reflect_depth=2, aov=names)
    flat = sc.render(W, H, aov=names)
    import torch
    torch.cuda.synchronize()
    assert np.array_equal(refl["packed"].cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(refl["rgba"].cpu().numpy().view(np.uint32), want[1].view(np.uint32))
    for key in names:
        assert np.array_equal(refl["aov"][key].cpu().numpy().view(np.uint32), flat["aov"][key].cpu().numpy().view(np.uint32)), key
    kinds = set(refl["aov"]["id"].cpu().numpy()[..., 0].reshape(-1).tolist())
    assert {TRIANGLE, SPHERE, PLANE, CUBE} <= kinds, kinds


# ----------------------------------------------------------------------------- 8. rejections
def test_rejections_under_the_scene_scope_write_nothing(rt, oracle, gpu):
    import torch
    lib = rt.load_library()
    sc = _staged_scene(rt, oracle)
    w, h = W, H
    cases = [dict(spp=4), dict(accumulate=True), dict(interleave=(2, 0, 16)), dict(table_lds=True), dict(profile=True)]
    for kw in cases:
        packed = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
        rgba = torch.full((h, w, 4), 3.0, dtype=torch.float32, device="cuda")
        fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=2, **kw)
        rc = lib.rt_scene_render(sc.handle, C.byref(fd), None)
        torch.cuda.synchronize()
        assert rc == 2, kw
        assert bool((packed == 7).all()) and bool((rgba == 3.0).all()), kw
    p24 = torch.full((h, w * 3 // 4), 5, dtype=torch.int32, device="cuda")
    fd = sc.frame_desc(w, h, packed24=p24.data_ptr(), reflect_depth=1)
    assert lib.rt_scene_render(sc.handle, C.byref(fd), None) == 2
    torch.cuda.synchronize()
    assert bool((p24 == 5).all())
    packed = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
    fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), reflect_depth=2)
    assert not lib.rt_graph_capture(sc.handle, C.byref(fd), 1, None, None)
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
    assert lib.rt_scene_render(sc.handle, C.byref(fd), None) == 0     # and the plain reflective frame still renders
    torch.cuda.synchronize()
    assert not bool((packed == 7).all())
