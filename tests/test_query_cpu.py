"""Ray queries, host side: the ctypes mirrors of rt_hit / rt_ray_query against the header's layout, and the argument
validation, which needs no device (every rejection happens before the scene touches one)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_HIT = ("t", "kind", "index", "u", "v", "tx", "ty", "normal", "new_org", "pad_")
_QUERY = ("struct_size", "mode", "n", "cull", "rays", "hits", "occluded", "rgba", "packed")


def _c_layout(tmp_path, struct, fields):
    """sizeof and offsetof as a C compiler lays the header's struct out."""
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof({struct}, {f}));\n' for f in fields)
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {{\n'
                   f'    printf("%zu\\n", sizeof({struct}));\n{body}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


@pytest.mark.parametrize("struct,fields,pyname", [("rt_hit", _HIT, "Hit"), ("rt_ray_query", _QUERY, "RayQuery")])
def test_layouts_match_the_header(rt, tmp_path, struct, fields, pyname):
    want = _c_layout(tmp_path, struct, fields)
    cls = getattr(rt, pyname)
    assert C.sizeof(cls) == want[0]
    assert [getattr(cls, f).offset for f in fields] == want[1:]
    if struct == "rt_hit":
        assert want[0] == 64


def test_constants(rt):
    assert (rt.RT_HIT_NONE, rt.RT_HIT_TRIANGLE, rt.RT_HIT_SPHERE, rt.RT_HIT_PLANE, rt.RT_HIT_CUBE) == (-1, 0, 1, 2, 3)
    assert (rt.RT_QUERY_NEAREST, rt.RT_QUERY_OCCLUDED, rt.RT_QUERY_SHADE) == (0, 1, 2)
    assert rt.RT_MAX_QUERY_RAYS == 1 << 26


def _query(rt, mode, n, **kw):
    q = rt.RayQuery()
    q.struct_size = C.sizeof(rt.RayQuery)
    q.mode, q.n, q.cull = mode, n, kw.get("cull", -1)
    for f in ("rays", "hits", "occluded", "rgba", "packed"):
        setattr(q, f, kw.get(f, 0))
    return q


def test_validation_without_a_device(rt):
    lib = rt.load_library()
    s = lib.rt_scene_create()           # host only: nothing is uploaded, no sky, no texture
    try:
        sentinel = np.full(4096, 0x5a5a5a5a, dtype=np.uint32)
        p = sentinel.ctypes.data          # stands for device buffers: a rejection must not write through them
        n = 64
        bad = [_query(rt, 3, n, rays=p, hits=p, occluded=p, rgba=p, packed=p),    # bad mode
               _query(rt, -1, n, rays=p, hits=p),
               _query(rt, 0, -1, rays=p, hits=p),                                   # n out of range
               _query(rt, 0, (1 << 26) + 1, rays=p, hits=p),
               _query(rt, 0, n, hits=p),                                            # rays NULL with n > 0
               _query(rt, 0, n, rays=p, occluded=p, rgba=p, packed=p),              # NEAREST without hits
               _query(rt, 1, n, rays=p, hits=p, rgba=p, packed=p),                  # OCCLUDED without occluded
               _query(rt, 2, n, rays=p, hits=p, occluded=p),                        # SHADE without rgba / packed
               _query(rt, 2, n, rays=p, rgba=p),                                    # SHADE without the scene's sky
               _query(rt, 0, n, rays=p, hits=p, cull=2),                            # bad cull
               _query(rt, 2, n, rays=p, rgba=p + 8),                                # rgba not 16-byte aligned
               _query(rt, 0, n, rays=p + 2, hits=p)]                                # rays not 4-byte aligned
        for q in bad:
            assert lib.rt_scene_trace_rays(s, C.byref(q), None) == 1
        assert lib.rt_scene_trace_rays(None, C.byref(bad[1]), None) == 1
        assert lib.rt_scene_trace_rays(s, None, None) == 1
        assert "rt_scene_trace_rays" in lib.rt_last_error().decode()
        # n = 0 with everything required present is a no-op (no device needed)
        assert lib.rt_scene_trace_rays(s, C.byref(_query(rt, 0, 0, hits=p)), None) == 0
        # a caller's shorter struct: fields past struct_size read as 0 (here `hits`, so NEAREST is refused)
        q = _query(rt, 0, n, rays=p, hits=p)
        q.struct_size = rt.RayQuery.hits.offset
        assert lib.rt_scene_trace_rays(s, C.byref(q), None) == 1
        # primary rays: null arguments, and a scene without sky / texture is refused like a frame
        fd = rt.FrameDesc()
        fd.struct_size = C.sizeof(rt.FrameDesc)
        fd.width, fd.height, fd.aspect = 16, 8, rt.default_aspect()
        fd.cam = rt.default_camera()
        fd.opts.struct_size = C.sizeof(rt.LaunchOpts)
        assert lib.rt_scene_primary_rays(None, C.byref(fd), p, None) == 1
        assert lib.rt_scene_primary_rays(s, None, p, None) == 1
        assert lib.rt_scene_primary_rays(s, C.byref(fd), None, None) == 1
        assert lib.rt_scene_primary_rays(s, C.byref(fd), p, None) == 1
        fd.width = 0
        assert lib.rt_scene_primary_rays(s, C.byref(fd), p, None) == 1
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


# ----------------------------------------------------------------------------- the composed reference (query_ref.py)
def _primary(oracle, inp, w, h):
    from test_reflect_cpu import Composer
    comp = Composer(oracle, None, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights,
                    inp.cam, inp.aspect)
    return comp.primary(w, h, 0, h)


def test_primitive_restatements_equal_the_oracle(rt, oracle):
    """query_ref's numpy sphere, cube, plane and Moller-Trumbore tests against the oracle's own, ray by ray."""
    import meshes
    import query_ref as Q
    from scenes import mixed_scene
    lib = oracle.load()
    inp = mixed_scene(rt)
    ref = Q.CastRef(oracle, inp, meshes.uv_sphere_obj())
    rng = np.random.default_rng(4)
    m = 1500
    O = rng.uniform(-12, 12, (m, 3)).astype(np.float32)
    D = rng.standard_normal((m, 3)).astype(np.float32)
    D[: m // 3] = (np.array([4.0, 2.0, 5.0], dtype=np.float32) - O[: m // 3])      # at the mesh
    D[m // 3: m // 2] = (np.array([4.5, 5.0, 4.5], dtype=np.float32) - O[m // 3: m // 2])   # at a cube
    D[:8] = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [1, 1, 0], [0, -1, 0], [np.nan, 0, 1], [np.inf, 0, 1]])
    r = oracle.ORay()
    t = C.c_float()
    u, v = C.c_float(), C.c_float()
    with np.errstate(all="ignore"):
        inv = (np.float32(1) / D).astype(np.float32)
    seen = {"cube": 0, "plane": 0, "tri": 0}
    ocubes = C.cast(inp.cubes, C.POINTER(oracle.OCube))
    oplanes = C.cast(inp.planes, C.POINTER(oracle.OPlane))
    osph = C.cast(inp.spheres, C.POINTER(oracle.OSphere))
    tp = lib.oracle_mesh_triangles(ref.mesh.handle)
    cube_h = [Q.slab(lo, hi, O, inv) for lo, hi, _ in ref.cubes]
    plane_h = [Q.plane_hit(p, n, O, D) for p, n in ref.planes]
    tri_h = [Q.tri_hit(*ref.tris[j]["p"], O, D) for j in range(0, len(ref.tris), 7)]
    sph_h, sph_t = Q.intersect(O, D, ref.tab[:40])
    for i in range(m):
        r.Org.x, r.Org.y, r.Org.z = (float(x) for x in O[i])
        r.Dir.x, r.Dir.y, r.Dir.z = (float(x) for x in D[i])
        for c, (h, tt) in enumerate(cube_h):
            got = lib.oracle_cube_intersect(C.byref(ocubes[c]), C.byref(r), C.byref(t))
            assert bool(got) == bool(h[i])
            if got:
                seen["cube"] += 1
                assert np.float32(t.value).view(np.uint32) == tt[i].view(np.uint32)
        for p, (h, tt) in enumerate(plane_h):
            got = lib.oracle_plane_intersect(C.byref(oplanes[p]), C.byref(r), C.byref(t))
            assert bool(got) == bool(h[i])
            if got:
                seen["plane"] += 1
                assert np.float32(t.value).view(np.uint32) == tt[i].view(np.uint32)
        for k, (h, tt, uu, vv) in enumerate(tri_h):
            got = lib.oracle_triangle_intersect(C.byref(tp[7 * k]), C.byref(r), C.byref(t), C.byref(u), C.byref(v))
            assert bool(got) == bool(h[i])
            if got:
                seen["tri"] += 1
                assert (np.float32(t.value).view(np.uint32), np.float32(u.value).view(np.uint32),
                        np.float32(v.value).view(np.uint32)) == (tt[i].view(np.uint32), uu[i].view(np.uint32),
                                                                 vv[i].view(np.uint32))
        for s in range(0, 40, 3):
            got = lib.oracle_sphere_intersect(C.byref(osph[s]), C.byref(r), C.byref(t))
            assert bool(got) == bool(sph_h[i, s])
            if got:
                assert np.float32(t.value).view(np.uint32) == sph_t[i, s].view(np.uint32)
    assert min(seen.values()) > 20, seen


@pytest.mark.parametrize("case", ["spheres_80x45_n256", "mixed_80x48", "mesh_64x36_n64"])
def test_composed_reference_shades_primary_rays_as_the_oracle(rt, oracle, case):
    import meshes
    import query_ref as Q
    from scenes import Inputs, mixed_scene
    mesh = None
    if case == "spheres_80x45_n256":
        inp, w, h = Inputs(rt, 256), 80, 45
    elif case == "mixed_80x48":
        inp, w, h = mixed_scene(rt), 80, 48
    else:
        inp, w, h, mesh = Inputs(rt, 64), 64, 36, meshes.uv_sphere_obj()
    om = oracle.Mesh(mesh) if mesh is not None else None
    want_rgba, want_packed, _ = oracle.render(inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights,
                                              inp.n_lights, inp.cam, w, h, inp.aspect, nthreads=8,
                                              cubes=getattr(inp, "cubes", None), n_cubes=getattr(inp, "n_cubes", 0),
                                              planes=getattr(inp, "planes", None), n_planes=getattr(inp, "n_planes", 0),
                                              mesh=om.handle if om else None)
    ref = Q.CastRef(oracle, inp, mesh)
    O, D = _primary(oracle, inp, w, h)
    rgba, packed, rec = ref.shade(O, D)
    kinds = set(rec["kind"].tolist())
    assert 1 in kinds
    if case != "mixed_80x48":
        assert -1 in kinds   # sky (the mixed scene's planes cover it)
    if case == "mixed_80x48":
        assert {2, 3} <= kinds
    if mesh is not None:
        assert 0 in kinds
    assert np.array_equal(rgba.reshape(h, w, 4).view(np.uint32), want_rgba.view(np.uint32))
    assert np.array_equal(packed.reshape(h, w), want_packed)
