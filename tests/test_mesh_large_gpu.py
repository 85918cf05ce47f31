"""The frame kernel's mesh paths that only large meshes reach, bit for bit against the oracle on the device: leaves of
more than 63 triangles (the chunk loop of the primary walk and the position it reports for shading), leaf lists of 65
to 128 entries and lists that overflow RT_BOX_CAP for the primary and the shadow rays, more than 1024 leaves (the
builder's outer loop), and a dense mesh in reflective frames and occlusion queries. Every test first asserts, from a
reference or from the work counters of the stats build, that its scene does reach the path it is about. The scenes
are built, and their CPU-side conditions tested, in tests/test_mesh_large_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import query_ref as Q
from reflect_scene_ref import SPHERE, TRIANGLE, SceneComposer, runs
from scenes import Scn
from test_aov_gpu import _check_frame
from test_mesh import _render_both
from test_mesh_large_cpu import (BIG_SPHERE_CENTRE, BIG_SPHERE_RADIUS, FAN_H, FAN_W, ONE_TILE_DISTANCES, ONE_TILE_FRAMES,
                                 RT_BLOCK, RT_BOX_CAP, SHADOW_H, SHADOW_W, HandMesh, assert_fans_reach_every_chunk,
                                 beam_leaf_bounds, fan_reference, fan_scene, mean_direction, obj_text, one_tile_scene,
                                 oracle_frame, shadow_mesh_text, shadow_scene, split_scene, split_sphere)

pytestmark = pytest.mark.gpu

# stats build, MESH launch (tools/mesh_stats.py): slot -> what it counts, summed over the frame's tiles
WALKED, P_LISTED, S_LISTED = 17, 18, 21      # walked tile-lights; primary leaves listed; shadow leaves listed by those walks

# _render_both's launches (tests/test_mesh.py), for scenes it cannot build: a hand-made mesh, an aspect of the frame's own
LAUNCHES = (dict(cull=True), dict(cull=False), dict(cull=True, tile=16), dict(cull=True, tile=32), dict(cull=False, tile=64),
            dict(cull=True, force_slow=True), dict(cull=True, want_stats=True), dict(cull=True, table_lds=True))
BRUTE_STATS = dict(cull=False, want_stats=True)


def _scene(inp, mesh_ptr):
    sc = inp.scene()
    sc.set_mesh(mesh_ptr)
    return sc


def _slots(sc, inp, w, h, **kw):
    import torch
    out = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, cull=True, want_stats=True, **kw)
    torch.cuda.synchronize()
    return list(out["stats"].values()), out["stats"]


def _same_counters(stats, cnt, cull):
    """The oracle's hit pixels, and its unshadowed samples from the brute-force launch: the culled one leaves out the
    lights a surface faces away from (as tests/test_gpu_parity.py has it)."""
    assert stats["hit_pixels"] == cnt["hit_pixels"]
    if cull:
        assert stats["unshadowed"] <= cnt["unshadowed"]
    else:
        assert stats["unshadowed"] == cnt["unshadowed"]


def _render_all(sc, inp, w, h, want, more=()):
    """Every launch of LAUNCHES (and `more`) of scene `sc` against the oracle's (rgba, packed, counters)."""
    import torch
    rgba, packed, cnt = want
    for opts in LAUNCHES + tuple(more):
        out = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, **opts)
        torch.cuda.synchronize()
        got = out["rgba"].cpu().numpy()
        bad = int((got.view(np.uint32) != rgba.view(np.uint32)).any(axis=2).sum())
        assert bad == 0, (opts, bad)
        assert np.array_equal(out["packed"].cpu().numpy().view(np.uint32), packed), opts
        if "stats" in out:
            _same_counters(out["stats"], cnt, opts["cull"])


# ----------------------------------------------------------------------------- 1, 2: leaves of more than 63 triangles
@pytest.mark.parametrize("view,name", [("front", "fans"), ("grazing", "fans"), ("front", "fans_normals"), ("grazing", "fans_normals")])
def test_fans_whole_frame(rt, oracle, gpu, view, name):
    """Fans of 150, 63, 127, 64, 126, 70, 5 and 1 triangles, one leaf each, among spheres over a floor under three
    lights: every launch against the oracle."""
    _, D, rec = fan_reference(rt, oracle, view, "fans")
    seen = assert_fans_reach_every_chunk(oracle, rec, D, view)
    print(view, name, "(leaf length, pixels, at position >= 63, >= 126, least |cos|):", seen)
    cnt = _render_both(rt, fan_scene(rt, view), obj_text(name), FAN_W, FAN_H)
    assert cnt["hit_pixels"] == int((rec["kind"] >= 0).sum())      # the oracle's frame is the frame of that record


@pytest.mark.parametrize("view,name", [("front", "fans_normals"), ("grazing", "fans")])
def test_fans_guides(rt, oracle, gpu, view, name):
    """The guides name the triangle a pixel sees: equal to NEAREST of the frame's primary rays (rt_cast.h's loops, one
    triangle at a time) and to the composed reference's record, with and without the culls."""
    import torch
    O, D, rec = fan_reference(rt, oracle, view, name)
    assert_fans_reach_every_chunk(oracle, rec, D, view)
    inp = fan_scene(rt, view)
    sc = _scene(inp, rt.mesh_from_obj_text(obj_text(name)))
    P = sc.primary_rays(FAN_W, FAN_H, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6).cpu().numpy()
    assert np.array_equal(P[:, :3].view(np.uint32), O.view(np.uint32)) and np.array_equal(P[:, 3:].view(np.uint32), D.view(np.uint32))
    for cull in (1, 0):
        a, nr = _check_frame(rt, sc, inp, FAN_W, FAN_H, cull)
        torch.cuda.synchronize()
        assert np.array_equal(a["depth"].reshape(-1).view(np.uint32), rec["t"].view(np.uint32)), cull
        assert np.array_equal(a["id"].reshape(-1, 2)[:, 0], rec["kind"]), cull
        assert np.array_equal(a["id"].reshape(-1, 2)[:, 1], rec["index"]), cull
        assert np.array_equal(a["normal"].reshape(-1, 4)[:, :3].view(np.uint32),
                              np.ascontiguousarray(rec["normal"]).view(np.uint32)), cull
        assert np.array_equal(nr["uv"].view(np.uint32), np.stack([rec["u"], rec["v"]], axis=1).view(np.uint32)), cull


# ----------------------------------------------------------------------------- 3: the primary leaf list
@pytest.mark.parametrize("w,h,tile", ONE_TILE_FRAMES)
@pytest.mark.parametrize("where", sorted(ONE_TILE_DISTANCES))
def test_one_tile_lists_or_overflows(rt, oracle, gpu, w, h, tile, where):
    """A frame of exactly one tile on the 635-leaf sphere: a list of 65 .. 128 leaves (more than the four marked
    blocks of one step) and lists that overflow, when the tile walks the whole table after the builder has written
    up to the list's end. What the tile lists: the stats build's count for the 8 x 8 tile (there is no stats build of
    the other tile shapes for mesh scenes), which must lie between the bounds restated on the CPU; those bounds alone
    for the 64 x 1 tile."""
    om = oracle.Mesh(obj_text("uv_sphere_40x64"))
    inp = one_tile_scene(rt, oracle, w, h, BIG_SPHERE_CENTRE, ONE_TILE_DISTANCES[where])
    sc = _scene(inp, rt.mesh_from_obj_text(obj_text("uv_sphere_40x64")))
    lower, upper = beam_leaf_bounds(oracle, rt, om, inp, w, h)
    if where == "list":
        assert 65 <= lower <= upper <= RT_BOX_CAP
    else:
        assert lower > RT_BOX_CAP
    if tile == 8:
        slots, stats = _slots(sc, inp, w, h)
        print(where, (w, h), "primary leaves listed by the tile:", slots[P_LISTED], "of", om.bvhbox_count, "bounds", lower, upper)
        if where == "list":
            assert 65 <= lower <= slots[P_LISTED] <= upper <= RT_BOX_CAP
        else:
            assert slots[P_LISTED] == om.bvhbox_count      # the list was dropped: the walk takes every leaf
    want = oracle_frame(oracle, inp, w, h, mesh=om.handle)
    assert want[2]["hit_pixels"] >= w * h // 2
    # (of the other tile shapes a mesh scene has the plain culled and brute-force kernels, no force_slow or stats build)
    _render_all(sc, inp, w, h, want, more=(dict(cull=True, tile=tile), dict(cull=False, tile=tile), BRUTE_STATS))


# ----------------------------------------------------------------------------- 4: the shadow leaf list
@pytest.mark.parametrize("light", ["wide", "narrow"])
def test_shadow_lists_overflow_or_hold(rt, oracle, gpu, light):
    """The 635-leaf sphere between a floor and one light. Under the wide light the shadow beams of the tiles beneath
    hold more leaves than a list can (the second build_box_list call, whose result is then dropped); under the
    narrow light the lists hold. Either way some samples are shadowed by the mesh and some are not."""
    import torch
    txt = shadow_mesh_text()
    inp = shadow_scene(rt, light)
    sc = _scene(inp, rt.mesh_from_obj_text(txt))
    slots, stats = _slots(sc, inp, SHADOW_W, SHADOW_H)
    ratio = slots[S_LISTED] / max(slots[WALKED], 1)
    print(light, "walked tile-lights", slots[WALKED], "shadow leaves listed", slots[S_LISTED], "per walk %.1f" % ratio)
    assert slots[WALKED] > 0
    if light == "wide":
        # a list holds at most RT_BOX_CAP leaves: a mean above that needs walks that took the whole table
        # (observed: 34697 leaves over 74 walks, 469 per walk)
        assert slots[S_LISTED] > RT_BOX_CAP * slots[WALKED]
    else:
        assert 0 < slots[S_LISTED] <= RT_BOX_CAP * slots[WALKED]      # (observed: 6211 over 109 walks, 57 per walk)
    bare = oracle_frame(oracle, inp, SHADOW_W, SHADOW_H)
    cnt = _render_both(rt, inp, txt, SHADOW_W, SHADOW_H)
    assert cnt["hit_pixels"] == SHADOW_W * SHADOW_H                      # floor, spheres or mesh everywhere
    assert 1000 < bare[2]["unshadowed"] - cnt["unshadowed"] < cnt["unshadowed"]      # the mesh shadows some samples, not all
    _same_counters(stats, cnt, True)
    brute = sc.render(SHADOW_W, SHADOW_H, cam=inp.cam, aspect=inp.aspect, **BRUTE_STATS)
    torch.cuda.synchronize()
    _same_counters(brute["stats"], cnt, False)


# ----------------------------------------------------------------------------- 5: more than 1024 leaves
def _leaf_of_triangle(om):
    leaf = np.zeros(om.poly_count, dtype=int)
    for j, (_, _, idx) in enumerate(om.boxes()):
        leaf[idx] = j
    return leaf


def test_more_than_1024_leaves(rt, oracle, gpu):
    """1840 leaves of one triangle each, 115 blocks -- the leaf-list builder takes 64 blocks per pass -- handed over as
    a caller-built rt_mesh: a 96 x 64 frame whose tiles list leaves from both passes, one tile that lists only a few
    of them, one tile that overflows, then the same mesh through rt_launch_raytrace's objs->mesh1."""
    import torch
    from test_gpu_parity import _managed_sprite
    lib = rt.load_library()
    om = split_sphere(oracle, 1)
    assert om.bvhbox_count == 1840 and (om.bvhbox_count + RT_BLOCK - 1) // RT_BLOCK == 115 > 64
    hm = HandMesh(rt, om)
    leaf = _leaf_of_triangle(om)
    second_pass = 64 * RT_BLOCK      # leaves from here on are listed by the builder's second pass

    def leaves_seen(sc, inp, w, h):
        out = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, cull=False, aov=("id",))      # the brute-force walk's guide
        torch.cuda.synchronize()
        ids = out["aov"]["id"].cpu().numpy().reshape(-1, 2)
        return leaf[ids[ids[:, 0] == 0, 1]]

    # the whole frame
    w, h = 96, 64
    inp = split_scene(rt)
    sc = _scene(inp, hm.ptr)
    seen = leaves_seen(sc, inp, w, h)
    slots, _ = _slots(sc, inp, w, h)
    tiles = (w // 8) * (h // 8)
    print("96 x 64: pixels on leaves of the first / second pass", int((seen < second_pass).sum()), int((seen >= second_pass).sum()),
          "leaves listed per tile %.1f" % (slots[P_LISTED] / tiles))
    assert (seen < second_pass).sum() >= 8
    # a tile that overflows counts every leaf: at most this many did, and they hold 64 pixels each -- the rest of the
    # pixels on second-pass leaves belong to tiles that walked a list
    overflowed = slots[P_LISTED] // om.bvhbox_count
    assert (seen >= second_pass).sum() - 64 * overflowed >= 8 and overflowed < tiles
    want = oracle_frame(oracle, inp, w, h, mesh=om.handle)
    _render_all(sc, inp, w, h, want, more=(BRUTE_STATS,))

    # one tile: near a triangle of the second pass (a short list), and the whole sphere from afar (an overflow)
    c = mean_direction(oracle, 8, 8)
    centroids = om.triangles()[:, :9].reshape(-1, 3, 3).mean(axis=1).astype(np.float64)
    outward = (centroids - BIG_SPHERE_CENTRE) / BIG_SPHERE_RADIUS
    first_tri = np.array([idx[0] for _, _, idx in om.boxes()])
    towards_eye = outward[first_tri] @ c < -0.6                              # leaves that face the tile's eye
    near, far = centroids[first_tri[:second_pass][towards_eye[:second_pass]]], centroids[first_tri[second_pass:][towards_eye[second_pass:]]]
    assert len(near) and len(far)
    # the one of the second pass farthest from every leaf of the first: the tile sees second-pass leaves all round it
    target = far[np.argmax(np.linalg.norm(far[:, None, :] - near[None, :, :], axis=2).min(axis=1))]
    for where, focus, dist in (("list", target, 1.5), ("overflow", BIG_SPHERE_CENTRE, 30.0)):
        inp1 = one_tile_scene(rt, oracle, 8, 8, focus, dist)
        sc1 = _scene(inp1, hm.ptr)
        slots, _ = _slots(sc1, inp1, 8, 8)
        seen = leaves_seen(sc1, inp1, 8, 8)
        print("one tile,", where, ": leaves listed", slots[P_LISTED], "pixels on leaves of the second pass", int((seen >= second_pass).sum()))
        if where == "list":
            assert 1 <= slots[P_LISTED] <= RT_BOX_CAP and (seen >= second_pass).sum() >= 8
        else:
            assert slots[P_LISTED] == om.bvhbox_count
        _render_all(sc1, inp1, 8, 8, oracle_frame(oracle, inp1, 8, 8, mesh=om.handle))

    # the drop-in entry point with objs->mesh1 = the same hand-made mesh
    obj = rt.Object()
    obj.sphere_count = inp.n
    obj.d_spheres = C.cast(inp.spheres, C.POINTER(rt.Sphere))
    obj.texture = _managed_sprite(rt, inp.tex)
    obj.mesh1 = hm.ptr
    sky = rt.Skybox()
    box = inp.sky_box
    sky.box = C.pointer(box)
    sky.skyboxTex = _managed_sprite(rt, inp.sky)
    pixels = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    assert lib.rt_launch_raytrace(pixels.data_ptr(), w, h, inp.aspect, C.byref(obj), inp.lights, inp.n_lights, inp.cam,
                                  C.byref(sky), None) == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(pixels.cpu().numpy().view(np.uint32), want[1])
    obj.mesh1 = None                                   # and without it: the entry point forgets the hand-made mesh
    assert lib.rt_launch_raytrace(pixels.data_ptr(), w, h, inp.aspect, C.byref(obj), inp.lights, inp.n_lights, inp.cam,
                                  C.byref(sky), None) == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(pixels.cpu().numpy().view(np.uint32), oracle_frame(oracle, inp, w, h)[1])


# ----------------------------------------------------------------------------- 6: the other consumers of a mesh
def _dense_scene(rt, lights=None):
    """The 24 x 40 sphere (1840 triangles, 349 leaves) at (4, 2, 5) over a floor, with spheres beside and behind
    it, under the default camera (and lights)."""
    return Scn(rt, [(1.0, 1.2, 5.5, 1.0), (7.0, 2.0, 6.0, 0.9), (4.0, 5.0, 4.0, 0.7), (3.5, 0.8, 1.5, 0.6)],
               lights=lights, planes=[(0, -0.2, 0, 0, 1, 0)])


def test_dense_mesh_in_reflective_frames(rt, oracle, gpu):
    """Bounce rays walk the mesh too (scene scope, depth 2): against the composed reference."""
    import torch
    w, h = 64, 36
    txt = obj_text("uv_sphere_24x40")
    inp = _dense_scene(rt, lights=[((20, 20, 20), 20, 1, 0.9, 0.8)])      # one light: a third of the reference's shadow rays
    comp = SceneComposer(oracle, rt, inp, txt)
    k = np.full(inp.n, 0.6, dtype=np.float32)
    kp = np.array([0.5], dtype=np.float32)
    ref_rgba, ref_packed, ref_queue = comp.render(w, h, 2, k_sphere=k, k_plane=kp)
    assert ref_queue[0] > 0 and runs(comp.trace, [SPHERE, TRIANGLE]) >= 8      # bounce rays that end on the mesh
    sc = _scene(inp, rt.mesh_from_obj_text(txt))
    sc.set_materials_ex(k, np.zeros(inp.n, dtype=np.float32), np.zeros(inp.n, dtype=np.float32))
    sc.set_plane_materials(kp)
    sc.set_reflect_scope("scene")
    for cull in (True, False):
        out = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, reflect_depth=2, cull=cull)
        torch.cuda.synchronize()
        assert sc.reflect_stats()["queue"] == ref_queue, cull
        assert np.array_equal(out["packed"].cpu().numpy().view(np.uint32), ref_packed), cull
        assert np.array_equal(out["rgba"].cpu().numpy().view(np.uint32), ref_rgba.view(np.uint32)), cull


def test_dense_mesh_in_occlusion_queries(rt, oracle, gpu):
    """OCCLUDED over 349 leaves: the frame's primary rays and rays aimed at and past the mesh from all round."""
    import torch
    w, h = 64, 36
    txt = obj_text("uv_sphere_24x40")
    inp = _dense_scene(rt)
    ref = Q.CastRef(oracle, inp, txt)
    sc = _scene(inp, rt.mesh_from_obj_text(txt))
    P = sc.primary_rays(w, h, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6).cpu().numpy()
    rng = np.random.default_rng(23)
    O = rng.uniform(-6.0, 14.0, (1500, 3)).astype(np.float32)
    T = (np.float32(BIG_SPHERE_CENTRE) + rng.uniform(-2.4, 2.4, (1500, 3))).astype(np.float32)
    D = (T - O).astype(np.float32)
    D = (D / np.sqrt((D * D).sum(axis=1, keepdims=True))).astype(np.float32)
    O = np.concatenate([P[:, :3], O]).astype(np.float32)
    D = np.concatenate([P[:, 3:], D]).astype(np.float32)
    want = ref.occluded(O, D)
    bare = Q.CastRef(oracle, inp).occluded(O, D)
    assert 200 < int((want != bare).sum()) and not want.all()      # rays only the mesh stops, and rays nothing stops
    rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([O, D], axis=1))).cuda()
    for cull in (True, False):
        occ = sc.trace_rays(rays, "occluded", cull=cull)["occluded"]
        torch.cuda.synchronize()
        assert np.array_equal(occ.cpu().numpy(), want), cull
