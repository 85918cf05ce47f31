"""Ray queries on the device (rt_scene_trace_rays, rt_scene_primary_rays): the primary rays against the
oracle, SHADE of the frame's own primary rays against the frame kernel, NEAREST / OCCLUDED against numpy restatements
of castRay and castLightRay's any-hit on adversarial rays, the BVH against the whole lists, the scene's update rules
and the rejections."""
import ctypes as C

import numpy as np
import pytest

import meshes
from scenes import Inputs, mixed_scene
import query_ref as Q
from test_reflect_cpu import Composer, _rays, adversarial_spheres, intersect, nearest, sphere_table

pytestmark = pytest.mark.gpu

f32 = np.float32


def _bits(t):
    return t.contiguous().cpu().numpy().view(np.uint32)


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


def _torch_rays(O, D):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([O, D], axis=1), dtype=np.float32)).cuda()


# ----------------------------------------------------------------------------- primary rays
@pytest.mark.parametrize("y0,y1", [(0, 0), (31, 47)])
def test_primary_rays_equal_the_oracle(rt, oracle, gpu, y0, y1):
    import torch
    inp = Inputs(rt, 256)
    sc = inp.scene()
    w, h = 160, 90
    rays = sc.primary_rays(w, h, y0=y0, y1=y1, cam=inp.cam, aspect=inp.aspect)
    torch.cuda.synchronize()
    comp = Composer(oracle, rt, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam,
                    inp.aspect)
    O, D = comp.primary(w, h, y0, y1 if y1 else h)
    got = rays.reshape(-1, 6).cpu().numpy()
    assert np.array_equal(got[:, :3].view(np.uint32), O.view(np.uint32))
    assert np.array_equal(got[:, 3:].view(np.uint32), D.view(np.uint32))


# ----------------------------------------------------------------------------- SHADE == the frame kernel
def _shade_case(rt, name):
    if name == "c2_160x90_n256":
        return Inputs(rt, 256), None, True, 160, 90, (0, 0)
    if name == "mixed_160x96":
        return mixed_scene(rt), None, True, 160, 96, (0, 0)
    if name == "mesh_alone":
        return Inputs(rt, 64), meshes.uv_sphere_obj(), False, 160, 90, (0, 0)
    if name == "mesh_spheres":
        return Inputs(rt, 64), meshes.uv_sphere_obj(), True, 160, 90, (0, 0)
    if name == "c3_3840x2160":
        return Inputs(rt, 1024), None, True, 3840, 2160, (0, 0)
    raise KeyError(name)


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["c2_160x90_n256", "mixed_160x96", "mesh_alone", "mesh_spheres", "c3_3840x2160"])
def test_shade_of_primary_rays_is_the_frame(rt, gpu, name, cull):
    import torch
    inp, mesh, spheres, w, h, (y0, y1) = _shade_case(rt, name)
    if name == "c3_3840x2160" and cull == 0:
        y0, y1 = 1056, 1120   # the whole lists at 4K: a band of 64 rows through the middle of the sphere field
    sc = _scene_of(rt, inp, mesh, spheres)
    frame = sc.render(w, h, y0=y0, y1=y1, cam=inp.cam, aspect=inp.aspect, cull=bool(cull))
    rays = sc.primary_rays(w, h, y0=y0, y1=y1, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6)
    got = sc.trace_rays(rays, "shade", cull=bool(cull))
    near = sc.trace_rays(rays, "nearest", cull=bool(cull))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got["rgba"]), _bits(frame["rgba"].reshape(-1, 4)))
    assert np.array_equal(_bits(got["packed"]), _bits(frame["packed"].reshape(-1)))
    kinds = set(near["kind"].cpu().numpy().tolist())
    if name in ("c2_160x90_n256", "mesh_spheres") or (name == "c3_3840x2160" and cull):
        assert -1 in kinds   # sky pixels (the mixed scene's planes cover the sky)
    if mesh is not None:
        assert 0 in kinds
    if spheres:
        assert 1 in kinds
    if name == "mixed_160x96":
        assert {2, 3} <= kinds


# ----------------------------------------------------------------------------- NEAREST / OCCLUDED vs numpy
def _odd_directions(rng, O, D):
    """Non-unit (the list walk), zero, NaN and infinite directions, mixed into a ray set."""
    m = len(D)
    D = D.copy()
    sel = rng.random(m) < 0.05
    D[sel] = D[sel] * rng.choice(np.array([0.5, 2.0, 1.5, 0.01], dtype=np.float32), (sel.sum(), 1))
    special = np.array([[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0], [0, -np.inf, 1], [0, 0, 1], [1, 0, 0], [0, 1, 0]],
                       dtype=np.float32)
    k = min(len(special) * 8, m)
    D[:k] = special[np.arange(k) % len(special)]
    return O, D


def test_nearest_and_occluded_spheres_equal_numpy(rt, gpu):
    import torch
    sph, n = adversarial_spheres(rt)
    inp = Inputs(rt, 8)
    sc = inp.scene()
    sc.set_spheres(sph, n)
    rng = np.random.default_rng(5)
    m = 60000
    O, D = _rays(rt, sph, n, m, 21)
    O, D = _odd_directions(rng, O, D)
    rays = _torch_rays(O, D)
    res = {c: sc.trace_rays(rays, "nearest", cull=c) for c in (True, False)}
    occ = {c: sc.trace_rays(rays, "occluded", cull=c)["occluded"] for c in (True, False)}
    torch.cuda.synchronize()
    for key in ("t", "kind", "index", "uv", "txy", "normal", "new_org"):
        assert np.array_equal(_bits(res[True][key]), _bits(res[False][key])), key
    assert np.array_equal(occ[True].cpu().numpy(), occ[False].cpu().numpy())
    tab = sphere_table(sph, n)
    k = 20000
    idx, tt = nearest(O[:k], D[:k], tab)
    got_i = res[True]["index"].cpu().numpy()[:k]
    got_t = res[True]["t"].cpu().numpy()[:k]
    assert np.array_equal(got_i, idx.astype(np.int32))
    assert np.array_equal(got_t.view(np.uint32), tt.view(np.uint32))
    hit, _ = intersect(O[:k], D[:k], tab)
    assert np.array_equal(occ[True].cpu().numpy()[:k], hit.any(axis=1).astype(np.int32))
    # the cases occur: origins inside (negative t), duplicates (extras 1 and 2 are the same sphere: first wins)
    assert (got_t[got_i >= 0] < 0).any()
    dup_a, dup_b = 512 + 1, 512 + 2
    assert (got_i == dup_a).any() and not (got_i == dup_b).any()
    # the hit record of a sphere hit (kernel.cu:1396-1405)
    sel = np.nonzero((got_i >= 0) & np.isfinite(got_t) & (np.arange(k) >= 64))[0][:2000]
    c = tab[got_i[sel], :3]
    hp = (O[sel] + D[sel] * got_t[sel, None]).astype(np.float32)
    nr = (hp - c).astype(np.float32)
    ln = np.sqrt(((nr[:, 0] * nr[:, 0] + nr[:, 1] * nr[:, 1]) + nr[:, 2] * nr[:, 2]).astype(np.float32))
    with np.errstate(all="ignore"):
        nr = np.where(ln[:, None] != 0, nr / ln[:, None], nr).astype(np.float32)
    assert np.array_equal(res[True]["new_org"].cpu().numpy()[sel].view(np.uint32), hp.view(np.uint32))
    assert np.array_equal(res[True]["normal"].cpu().numpy()[sel].view(np.uint32), nr.view(np.uint32))
    # a miss: t = inf, kind = index = -1, zeros elsewhere
    miss = np.nonzero(res[True]["kind"].cpu().numpy() == -1)[0]
    assert len(miss) > 0
    assert np.isinf(res[True]["t"].cpu().numpy()[miss]).all()
    for key in ("uv", "txy", "normal", "new_org"):
        assert not res[True][key].cpu().numpy()[miss].any()


def _mixed_rays(rng, m, lo=-20.0, hi=20.0):
    O = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    D = rng.standard_normal((m, 3)).astype(np.float32)
    D = (D / np.sqrt((D * D).sum(axis=1, keepdims=True))).astype(np.float32)
    return O, D


def test_ties_across_kinds_and_zero_components(rt, gpu):
    """A plane tangent to a sphere at the same t (first kind found wins: the sphere), cubes hit along axes (zero
    direction components: infinite and NaN slabs), a triangle outside its own leaf's box (hidden by the gate)."""
    import torch
    lib = rt.load_library()
    inp = Inputs(rt, 8)
    spheres = (rt.Sphere * 2)()
    lib.rt_sphere_init(C.byref(spheres[0]), 0.0, 2.0, 10.0, 1.0)    # top at y = 3
    lib.rt_sphere_init(C.byref(spheres[1]), 5.0, 0.0, 10.0, 1.0)
    planes = (rt.Plane * 1)()
    lib.rt_plane_init(C.byref(planes[0]), 0.0, 3.0, 0.0, 0.0, 1.0, 0.0)   # y = 3, facing +y: tangent to sphere 0's top
    cubes = (rt.Cube * 1)()
    lib.rt_cube_init(C.byref(cubes[0]), -6.0, -1.0, 8.0, -4.0, 1.0, 12.0)
    sc = inp.scene()
    sc.set_spheres(spheres, 2)
    sc.set_planes(planes, 1)
    sc.set_cubes(cubes, 1)
    O = np.array([[0, 10, 10], [-5, 0, 0], [-5, 0.5, 0], [-5, 1.0, 0], [-10, 0, 10], [-5, -1.0, 0]], dtype=np.float32)
    D = np.array([[0, -1, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
    res = {c: sc.trace_rays(_torch_rays(O, D), "nearest", cull=c) for c in (True, False)}
    torch.cuda.synchronize()
    for key in ("t", "kind", "index", "normal", "new_org", "txy"):
        assert np.array_equal(_bits(res[True][key]), _bits(res[False][key])), key
    kind = res[True]["kind"].cpu().numpy()
    t = res[True]["t"].cpu().numpy()
    # straight down onto the sphere's top: sphere and plane both at t = 7, the sphere is found first
    assert kind[0] == 1 and t[0] == np.float32(7.0)
    import query_ref as Q
    ph, pt = Q.plane_hit(Q._vec(planes[0].orgin), Q._vec(planes[0].normal), O[:1], D[:1])
    assert ph[0] and pt[0] == np.float32(7.0)   # the plane reports the same t: a tie the sphere wins
    # axis-aligned rays into the cube, including ones in its faces' planes (0 * inf = NaN slabs)
    assert (kind[1:4] == 3).all()
    occ = sc.trace_rays(_torch_rays(O, D), "occluded")["occluded"].cpu().numpy()
    assert (occ[:4] == 1).all()
    # the reference's min/max macros on the NaN slab of a ray in a face's plane, restated: x = -5 is inside [-6, -4],
    # y = -1 lies in the face plane y = -1 (t3 = 0 * inf = NaN), the macros keep what the comparisons select
    with np.errstate(all="ignore"):
        inv = (f32(1) / D[5]).astype(np.float32)
        a = np.array([-6, -1, 8], dtype=np.float32)
        b = np.array([-4, 1, 12], dtype=np.float32)
        t1, t2 = (a - O[5]) * inv, (b - O[5]) * inv
    mn = [x if x < y else y for x, y in zip(t1, t2)]
    mx = [x if x > y else y for x, y in zip(t1, t2)]
    tmin = (mn[0] if mn[0] > mn[1] else mn[1])
    tmin = tmin if tmin > mn[2] else mn[2]
    tmax = (mx[0] if mx[0] < mx[1] else mx[1])
    tmax = tmax if tmax < mx[2] else mx[2]
    want_hit = not (tmax < 0) and not (tmax < tmin)
    assert (kind[5] == 3) == want_hit
    if want_hit:
        assert np.float32(t[5]).view(np.uint32) == np.float32(tmin).view(np.uint32)


def test_cull_equals_whole_lists_c3(rt, gpu):
    import torch
    inp = Inputs(rt, 1024)
    sc = inp.scene()
    rng = np.random.default_rng(9)
    m = 1 << 20
    O, D = _mixed_rays(rng, m, -30, 30)
    rays = _torch_rays(O, D)
    for mode in ("nearest", "occluded"):
        a = sc.trace_rays(rays, mode, cull=True)
        b = sc.trace_rays(rays, mode, cull=False)
        torch.cuda.synchronize()
        for key in a:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), (mode, key)
    sub = rays[:65536]
    a = sc.trace_rays(sub, "shade", cull=True)
    b = sc.trace_rays(sub, "shade", cull=False)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a["rgba"]), _bits(b["rgba"])) and np.array_equal(_bits(a["packed"]), _bits(b["packed"]))


def test_queries_follow_set_spheres_and_keep_reflective_frames(rt, gpu):
    import torch
    inp = Inputs(rt, 1024)
    sc = inp.scene()
    k = np.array([(0.0, 0.25, 0.5, 1.0)[i % 4] for i in range(1024)], dtype=np.float32)
    sc.set_materials(k)
    w, h = 3840, 2160
    before = sc.render(w, h, cam=inp.cam, reflect_depth=3)
    torch.cuda.synchronize()
    bp, br = _bits(before["packed"]), _bits(before["rgba"])
    O = np.array([[0.0, 0.0, -50.0]], dtype=np.float32)
    D = np.array([[0.0, 0.0, 1.0]], dtype=np.float32)
    rays = _torch_rays(O, D)
    sc.trace_rays(rays, "nearest")
    # move sphere 7 onto the ray, in front of everything
    lib = rt.load_library()
    moved = (rt.Sphere * 1024)()
    C.memmove(moved, inp.spheres, C.sizeof(moved))
    lib.rt_sphere_init(C.byref(moved[7]), 0.0, 0.0, -40.0, 1.0)
    sc.set_spheres(moved, 1024)
    a = sc.trace_rays(rays, "nearest", cull=True)
    b = sc.trace_rays(rays, "nearest", cull=False)
    torch.cuda.synchronize()
    assert int(a["index"][0]) == 7 and int(a["kind"][0]) == 1 and float(a["t"][0]) == 9.0
    for key in a:
        assert np.array_equal(_bits(a[key]), _bits(b[key]))
    # back to the first list: the reflective frame rendered after the queries is the one before them
    sc.set_spheres(inp.spheres, 1024)
    sc.trace_rays(rays, "shade")
    after = sc.render(w, h, cam=inp.cam, reflect_depth=3)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(after["packed"]), bp) and np.array_equal(_bits(after["rgba"]), br)


def test_rejections_write_nothing(rt, gpu):
    import torch
    inp = Inputs(rt, 64)
    sc = inp.scene()
    n = 1000
    rays = _torch_rays(*_mixed_rays(np.random.default_rng(1), n))
    hits = torch.full((n, 16), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    occ = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    rgba = torch.full((n, 4), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    packed = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    R, H, O_, F, P = rays.data_ptr(), hits.data_ptr(), occ.data_ptr(), rgba.data_ptr(), packed.data_ptr()
    bad = [sc.query(3, n, rays=R, hits=H, occluded=O_, rgba=F, packed=P),
           sc.query(-1, n, rays=R, hits=H),
           sc.query(0, -1, rays=R, hits=H),
           sc.query(0, (1 << 26) + 1, rays=R, hits=H),
           sc.query(0, n, rays=0, hits=H),
           sc.query(0, n, rays=R, occluded=O_, rgba=F, packed=P),
           sc.query(1, n, rays=R, hits=H, rgba=F, packed=P),
           sc.query(2, n, rays=R, hits=H, occluded=O_),
           sc.query(0, n, rays=R, hits=H, cull=2)]
    for q in bad:
        assert sc.trace_rays_raw(q) == 1
    assert sc.lib.rt_scene_trace_rays(None, C.byref(bad[1]), None) == 1
    assert sc.lib.rt_scene_trace_rays(sc.handle, None, None) == 1
    # a capturing stream is refused
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = sc.trace_rays_raw(sc.query(0, n, rays=R, hits=H), s.cuda_stream)
    assert rc == 2
    torch.cuda.synchronize()
    for buf in (hits, occ, rgba, packed):
        assert (buf == 0x5a5a5a5a).all()
    # n = 0 is a no-op
    assert sc.trace_rays_raw(sc.query(0, 0, rays=0, hits=H)) == 0


def test_python_wrappers_and_picking(rt, oracle, gpu):
    import torch
    inp = Inputs(rt, 256)
    sc = inp.scene()
    w, h = 160, 90
    rays = sc.primary_rays(w, h, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6)
    n = rays.shape[0]
    raw = torch.empty((n, 16), dtype=torch.int32, device="cuda")
    assert sc.trace_rays_raw(sc.query("nearest", n, rays=rays.data_ptr(), hits=raw.data_ptr()),
                             torch.cuda.current_stream().cuda_stream) == 0
    near = sc.trace_rays(rays, "nearest")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(near["kind"]), _bits(raw[:, 1])) and np.array_equal(_bits(near["t"]), _bits(raw[:, 0]))
    assert np.array_equal(_bits(near["normal"]), _bits(raw[:, 7:10]))
    # picking: pixel -> primary ray -> NEAREST -> (kind, index), against castRay restated over the oracle's rays
    comp = Composer(oracle, rt, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam,
                    inp.aspect)
    O, D = comp.primary(w, h, 0, h)
    idx, _ = nearest(O, D, sphere_table(inp.spheres, inp.n))
    chosen = [int(i) for i in np.nonzero(idx >= 0)[0][::97]][:12] + [int(np.nonzero(idx < 0)[0][0])]
    for p in chosen:
        y, x = divmod(p, w)
        kind, index = sc.pick(w, h, x, y, cam=inp.cam, aspect=inp.aspect)
        assert index == int(idx[p]) and kind == (1 if idx[p] >= 0 else -1)


# ----------------------------------------------------------------------------- every field against the composed reference
def _same_record(got, rec, what):
    pairs = [("t", rec["t"]), ("kind", rec["kind"]), ("index", rec["index"]),
             ("uv", np.stack([rec["u"], rec["v"]], axis=1)), ("txy", np.stack([rec["tx"], rec["ty"]], axis=1)),
             ("normal", rec["normal"]), ("new_org", rec["new_org"])]
    for key, want in pairs:
        g = got[key].contiguous().cpu().numpy()
        assert np.array_equal(g.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (what, key)


def _check_against_reference(sc, ref, O, D, what):
    import torch
    rays = _torch_rays(O, D)
    rec = ref.nearest(O, D)
    want_occ = ref.occluded(O, D)
    for cull in (True, False):
        got = sc.trace_rays(rays, "nearest", cull=cull)
        occ = sc.trace_rays(rays, "occluded", cull=cull)["occluded"]
        torch.cuda.synchronize()
        _same_record(got, rec, (what, cull))
        assert np.array_equal(occ.cpu().numpy(), want_occ), (what, cull)
    return rec, want_occ


def _aimed(rng, targets, m, spread, lo=-15.0, hi=15.0):
    O = rng.uniform(lo, hi, (m, 3)).astype(np.float32)
    tgt = (targets[rng.integers(0, len(targets), m)] + rng.uniform(-spread, spread, (m, 3))).astype(np.float32)
    D = (tgt - O).astype(np.float32)
    return O, (D / np.sqrt((D * D).sum(axis=1, keepdims=True))).astype(np.float32)


@pytest.mark.parametrize("case", ["mixed", "mesh_spheres"])
def test_nearest_and_occluded_every_field_equal_the_composed_reference(rt, oracle, gpu, case):
    """castRay's whole hit record (t, kind, index, u, v, tx, ty, normal, new_org) and castLightRay's any-hit, bit for
    bit against query_ref (checked against oracle_render in test_query_cpu.py), on primary, random, aimed and
    axis-aligned rays, with the BVH and with the whole lists."""
    rng = np.random.default_rng(17)
    if case == "mixed":
        inp, mesh = mixed_scene(rt), None
        targets = np.array([[2, 1, 2], [6.75, 1.75, 2.75], [4.5, 5, 4.5], [8.75, -2, 8.75], [3, 2.5, 8.5]], dtype=np.float32)
        w, h = 80, 48
    else:
        inp, mesh = Inputs(rt, 64), meshes.uv_sphere_obj()
        targets = np.array([[4.0, 2.0, 5.0]], dtype=np.float32)
        w, h = 64, 36
    sc = _scene_of(rt, inp, mesh)
    ref = Q.CastRef(oracle, inp, mesh)
    P = sc.primary_rays(w, h, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6).cpu().numpy()
    O1, D1 = _aimed(rng, targets, 3000, 2.0)
    O2, D2 = _mixed_rays(rng, 2000)
    # axis-aligned rays through the targets (zero direction components: infinite and NaN slabs)
    axes = np.eye(3, dtype=np.float32)
    k = rng.integers(0, 3, 600)
    D3 = (axes[k] * rng.choice(np.array([-1, 1], dtype=np.float32), (600, 1))).astype(np.float32)
    O3 = (targets[rng.integers(0, len(targets), 600)] - D3 * f32(12) + np.where(axes[k] == 0,
          rng.uniform(-1.6, 1.6, (600, 3)), 0)).astype(np.float32)
    O3[:50] = np.round(O3[:50])   # some of them in the faces' planes
    O = np.concatenate([P[:, :3], O1, O2, O3]).astype(np.float32)
    D = np.concatenate([P[:, 3:], D1, D2, D3]).astype(np.float32)
    rec, occ = _check_against_reference(sc, ref, O, D, case)
    kinds = set(rec["kind"].tolist())
    assert 1 in kinds and -1 in kinds and occ.any() and not occ.all()
    if case == "mixed":
        assert {2, 3} <= kinds
    else:
        assert 0 in kinds and (rec["u"][rec["kind"] == 0] != rec["v"][rec["kind"] == 0]).any()


def test_triangle_tied_with_a_sphere(rt, oracle, gpu):
    """A triangle through a sphere's hit point at the same t: the mesh is tested first, so the triangle wins."""
    lib = rt.load_library()
    inp = Inputs(rt, 8)
    spheres = (rt.Sphere * 2)()
    lib.rt_sphere_init(C.byref(spheres[0]), 0.0, 0.0, 10.0, 1.0)    # the ray (0,0,0) + t (0,0,1) enters at t = 9
    lib.rt_sphere_init(C.byref(spheres[1]), 3.0, 0.0, 12.0, 1.0)
    inp.spheres, inp.n = spheres, 2
    mesh = "v -1 -1 9\nv 1 -1 9\nv 0 1 9\nv 2 -1 11\nv 4 -1 11\nv 3 1 11\nf 1 2 3\nf 4 5 6\n"
    sc = _scene_of(rt, inp, mesh)
    ref = Q.CastRef(oracle, inp, mesh)
    O = np.array([[0, 0, 0], [3, 0, 0], [0.25, 0.25, 0], [0, 0, 20]], dtype=np.float32)
    D = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    rec, _ = _check_against_reference(sc, ref, O, D, "tie")
    th, tt, _, _ = Q.tri_hit(*ref.tris[0]["p"], O[:1], D[:1])
    sh, st = intersect(O[:1], D[:1], ref.tab[:1])
    assert th[0] and sh[0, 0] and tt[0] == st[0, 0] == np.float32(9)   # the tie occurs
    assert rec["kind"][0] == 0 and rec["index"][0] == 0


def test_leaf_gate_hides_triangles(rt, oracle, gpu):
    """A leaf's triangles are tested only if the ray passes the leaf's own box (castRay, castLightRay). Rays aimed at
    the vertices that span the box: Moller-Trumbore accepts some that the box's slab test rounds out -- the gate
    must hide those, for NEAREST and OCCLUDED."""
    inp = Inputs(rt, 8)
    mesh = "v -1.3 -0.7 9.1\nv 1.7 -1.1 8.3\nv 0.2 1.9 9.7\nv 3.1 0.3 10.2\nv 4.6 -1.2 9.4\nv 3.9 2.1 11.3\nf 1 2 3\nf 4 5 6\n"
    sc = _scene_of(rt, inp, mesh, spheres=False)
    ref = Q.CastRef(oracle, inp, mesh, spheres=False)
    rng = np.random.default_rng(2)
    m = 200000
    verts = np.array([p for t in ref.tris for p in t["p"]], dtype=np.float32)
    O, D = _aimed(rng, verts, m, 2e-6, -4, 4)
    rec, occ = _check_against_reference(sc, ref, O, D, "gate")
    hidden = rec["gated"] & (rec["kind"] != 0)
    assert hidden.sum() > 0 and (occ[hidden] == 0).any()
    assert (rec["kind"] == 0).sum() > 1000
