"""Meshes large enough to reach the frame kernel's size-dependent paths -- leaf lists past RT_BOX_CAP, leaves past one
chunk of 63 triangles, more leaf blocks than one pass takes -- built and checked on the CPU: the loader against the
oracle's (tests/test_mesh.py takes the meshes as further cases), and the conditions without which the device tests of
tests/test_mesh_large_gpu.py would pass without testing anything. That module imports its scenes from here."""
import ctypes as C
import functools

import numpy as np

import meshes
import query_ref as Q
from scenes import Scn
from test_reflect_cpu import composer_for

RT_BOX_CAP = 128          # rt_device.h: leaf-list capacity of a tile
RT_BLOCK = 16             # leaves per block of the leaf table
CHUNK = 63                # triangles a tile takes from a leaf at a time
FAN_W, FAN_H = 96, 64
DENSE = {"uv_sphere_24x40": dict(n_lat=24, n_lon=40), "uv_sphere_40x64": dict(n_lat=40, n_lon=64)}


@functools.lru_cache(maxsize=None)
def obj_text(name):
    if name == "fans":
        return meshes.fans_obj()
    if name == "fans_normals":
        return meshes.fans_obj(normals=True)
    return meshes.uv_sphere_obj(**DENSE[name])


def leaf_lengths(om):
    return [len(idx) for _, _, idx in om.boxes()]


# ----------------------------------------------------------------------------- the fan scene
def _cam(rt, org, yaw, pitch):
    return rt.Camera(rt.Vec3(*org), rt.Vec3(0, 0, 1), 0.0, yaw, pitch)


# "front" sees every fan; "grazing" looks along the fans' planes (they face -z, the view is 70 degrees off that:
# some triangles of every long fan are edge-on to the tiles' beams, the case the per-triangle cull must not cull)
FAN_CAMERAS = {"front": ((1.6, 3.3, 3.3), 0.0, 0.0), "grazing": ((-1.5, 2.0, 4.5), 70.0, 0.0)}


def fan_scene(rt, view):
    """20 spheres behind, between and before the fans, a floor under them, three lights (one close: wide shadow
    beams), the camera of FAN_CAMERAS[view]."""
    rng = np.random.default_rng(7)
    spheres = []
    for i in range(20):
        z = rng.uniform(9.8, 12.0) if i < 12 else rng.uniform(6.3, 9.0) if i < 17 else rng.uniform(4.2, 5.2)
        r = rng.uniform(0.3, 0.6) if i < 12 else rng.uniform(0.12, 0.2)
        spheres.append((rng.uniform(-1.0, 4.2), rng.uniform(-0.6, 3.8), z, r))
    lights = [((10, 15, -15), 20, 1, 0.2, 0.1), ((-8, 12, -10), 10, 0.1, 0.2, 1), ((1, 6, -2), 20, 0.2, 1, 0.2)]
    org, yaw, pitch = FAN_CAMERAS[view]
    return Scn(rt, spheres, lights=lights, cam=_cam(rt, org, yaw, pitch), planes=[(0, -1.1, 0, 0, 1, 0)])


@functools.lru_cache(maxsize=None)
def fan_reference(rt, oracle, view, name):
    """(primary rays O, D; castRay's record of every pixel) of the fan scene's 96 x 64 frame, from query_ref's
    per-ray loops -- one triangle at a time, nothing in runs of 63 or 7."""
    inp = fan_scene(rt, view)
    O, D = composer_for(oracle, rt, inp).primary(FAN_W, FAN_H, 0, FAN_H)
    ref = Q.CastRef(oracle, inp, obj_text(name))
    return O, D, ref.nearest(O, D)


def fan_positions_seen(oracle, rec, D):
    """Per leaf of the fan mesh: (length, pixels whose nearest hit is one of its triangles, ... at position >= 63 in
    the leaf, ... at position >= 126, the least |cos| between such a pixel's ray and its triangle's plane)."""
    om = oracle.Mesh(obj_text("fans"))
    tris = om.triangles()
    boxes = om.boxes()
    leaf, pos = np.zeros(om.poly_count, dtype=int), np.zeros(om.poly_count, dtype=int)
    for j, (_, _, idx) in enumerate(boxes):
        leaf[idx], pos[idx] = j, np.arange(len(idx))
    hit = rec["kind"] == 0
    tri = rec["index"][hit]
    cosn = np.abs((tris[tri, 9:12].astype(np.float64) * D[hit]).sum(axis=1))
    out = []
    for j, (_, _, idx) in enumerate(boxes):
        m = leaf[tri] == j
        p = pos[tri][m]
        out.append((len(idx), int(m.sum()), int((p >= CHUNK).sum()), int((p >= 2 * CHUNK).sum()),
                    float(cosn[m].min()) if m.any() else 1.0))
    return out


def assert_fans_reach_every_chunk(oracle, rec, D, view):
    """The precondition of the fan frames: every leaf of more than 63 triangles shows at least 8 pixels whose nearest
    hit lies in its second chunk or later, every leaf of more than 126 at least 8 in its third."""
    seen = fan_positions_seen(oracle, rec, D)
    for length, pixels, second, third, _ in seen:
        if length > CHUNK:
            assert second >= 8, (view, seen)
        if length > 2 * CHUNK:
            assert third >= 8, (view, seen)
    if view == "front":
        assert all(s[1] >= 4 for s in seen), seen          # every fan is in the picture
    if view == "grazing":
        # ... and rays that run nearly inside a triangle's plane do hit long leaves
        assert min(s[4] for s in seen if s[0] > CHUNK) < 0.05, seen
    return seen


# ----------------------------------------------------------------------------- a mesh the loader cannot make
class HandMesh:
    """An rt_mesh laid out by hand from an oracle mesh's triangles and leaves (whatever they are: the leaves of
    oracle_mesh_split_leaves are more than the loader's ten passes can make). Both sides then gate every triangle by
    the same box. `ptr` is what rt_scene_set_mesh and objs->mesh1 take; this object owns the arrays it points into and
    must outlive every scene that was given `ptr`."""

    def __init__(self, rt, om):
        lib = rt.load_library()
        tris = np.ascontiguousarray(om.triangles(), dtype=np.float32)
        boxes = om.boxes()
        self.tris = (rt.Triangle * om.poly_count)()
        C.memmove(self.tris, tris.ctypes.data, tris.nbytes)
        self.cubes = (rt.Cube * len(boxes))()
        self.leaves = (rt.BvhBox * len(boxes))()
        self.index_arrays = []
        self.all_indexes = (C.c_int * om.poly_count)(*range(om.poly_count))
        for j, (b, org, idx) in enumerate(boxes):
            lib.rt_cube_init(C.byref(self.cubes[j]), *b)
            c = self.cubes[j]
            assert [c.bounds[0].x, c.bounds[0].y, c.bounds[0].z, c.bounds[1].x, c.bounds[1].y, c.bounds[1].z] == b
            arr = (C.c_int * len(idx))(*idx)
            self.index_arrays.append(arr)
            cube = C.pointer(self.cubes[j])
            ip = C.cast(arr, C.POINTER(C.c_int))
            self.leaves[j] = rt.BvhBox(cube, cube, ip, ip, len(idx))
        tp = C.cast(self.tris, C.POINTER(rt.Triangle))
        bp = C.cast(self.leaves, C.POINTER(rt.BvhBox))
        self.mesh = rt.Mesh(tp, tp, om.poly_count, len(boxes), 10, 1 if om.has_normals else 0, bp, bp,
                            C.cast(self.all_indexes, C.POINTER(C.c_int)))
        self.ptr = C.pointer(self.mesh)


def split_sphere(oracle, max_len=1):
    """The 24 x 40 sphere with every leaf cut into leaves of max_len triangles."""
    return oracle.Mesh(obj_text("uv_sphere_24x40")).split_leaves(max_len)


def split_scene(rt):
    """A few spheres around the 24 x 40 sphere (centre (4, 2, 5), radius 1.6) under the default camera and lights."""
    return Scn(rt, [(1.2, 1.0, 5.5, 0.8), (6.5, 3.0, 6.0, 0.7), (4.0, 4.6, 5.0, 0.5), (3.0, 1.0, 8.0, 0.6), (5.5, 0.5, 3.0, 0.4)])


# ----------------------------------------------------------------------------- frames of exactly one tile
ONE_TILE_ASPECT = 0.25      # rays within 4 degrees of the frame's mean direction: a beam the tile does cull with
BIG_SPHERE_CENTRE, BIG_SPHERE_RADIUS = (4.0, 2.0, 5.0), 1.6      # meshes.uv_sphere_obj's defaults


def mean_direction(oracle, w, h, aspect=ONE_TILE_ASPECT):
    """Unit mean of the primary directions of a w x h frame of a camera without yaw or pitch."""
    lib = oracle.load()
    zero, r = oracle.OCamera(), oracle.ORay()
    c = np.zeros(3)
    for y in range(h):
        for x in range(w):
            lib.oracle_primary_ray(x, y, w, h, aspect, C.byref(zero), 0.5, 0.5, C.byref(r))
            c += (r.Dir.x, r.Dir.y, r.Dir.z)
    return c / np.linalg.norm(c)


def one_tile_camera(rt, oracle, w, h, target, dist, aspect=ONE_TILE_ASPECT):
    """A camera without yaw or pitch whose w x h frame looks at `target` along its mean primary direction, the eye
    `dist` before it."""
    c = mean_direction(oracle, w, h, aspect)
    org = np.asarray(target, dtype=np.float64) - dist * c + (0.0, 0.0, 1.0 / aspect)      # the eye is Org - (0, 0, 1 / aspect)
    return _cam(rt, [float(np.float32(v)) for v in org], 0.0, 0.0)


def one_tile_scene(rt, oracle, w, h, target, dist):
    """Spheres beside and behind the default uv sphere's place, seen through one narrow tile."""
    inp = split_scene(rt)
    inp.aspect = ONE_TILE_ASPECT
    inp.cam = one_tile_camera(rt, oracle, w, h, target, dist)
    return inp


# eye this far from the 40 x 64 sphere's centre -> what the one tile must list: all 635 leaves from afar, a part that
# is still more than the list holds from nearer, and from 6 away about a hundred
ONE_TILE_DISTANCES = {"all": 30.0, "overflow": 12.0, "list": 6.0}
ONE_TILE_FRAMES = ((8, 8, 8), (64, 1, 64))      # width, height, tile


def beam_leaf_bounds(oracle, rt, om, inp, w, h):
    """(lower, upper) bounds of the leaves a tile that is the whole w x h frame lists for its primary rays, restated
    in binary64 from build_box_list's test (rt_cull.h): a leaf is kept when its bounding sphere comes within
    k reach + r of the cone's axis, the axis the normalised sum of the tile's directions, k the tangent of their
    largest deviation. The kernel pads the deviation (x 1.01 + 1e-5), the radius (r^2 x 1.001 + 1e-6 on the host, then
    + 4e-6 |v|^2 + 8e-5) and the comparison (x 1.0005): `lower` drops every pad and shrinks the reach by a thousandth
    instead, `upper` pads more than the kernel does. (The work counters say what a tile did list, but the stats build
    exists for 8 x 8 tiles only; tests/test_mesh_large_gpu.py checks these bounds against it there.)"""
    O, D = composer_for(oracle, rt, inp).primary(w, h, 0, h)
    O, D = O[0].astype(np.float64), D.astype(np.float64)
    u = D.sum(axis=0)
    u /= np.linalg.norm(u)
    s = np.sqrt((np.cross(D, u) ** 2).sum(axis=1).max())
    assert s * s < 0.2                                   # the tile does cull (the kernel gives up at sin^2 >= 0.25)
    b = np.array([bb for bb, _, _ in om.boxes()], dtype=np.float64)
    v = 0.5 * (b[:, :3] + b[:, 3:]) - O
    r2 = (0.25 * (b[:, 3:] - b[:, :3]) ** 2).sum(axis=1)
    vv, sa = (v * v).sum(axis=1), v @ u
    dist = np.sqrt(np.maximum(vv - sa * sa, 0))

    def kept(sn, rc, slack):
        k = sn / np.sqrt(1 - sn * sn)
        reach = sa + rc
        return int(((reach >= 0) & (dist <= (k * np.maximum(reach, 0) + rc) * slack)).sum())

    lower = kept(s, np.sqrt(r2), 0.999)
    upper = kept(s * 1.03 + 1e-4, np.sqrt(r2 * 1.01 + 1e-5 * vv + 1e-3) * 1.001 + 1e-3, 1.01)
    return lower, upper


# ----------------------------------------------------------------------------- the shadow scene
SHADOW_W, SHADOW_H = 96, 64
HOVER_CENTRE = (4.0, 4.5, 5.0)
# shadow rays leave along l.pos / |l.pos| and stray from it by up to asin(1 / |l.pos|) (kernel.cu:1442-1468):
# "wide" is a light five units from the origin, whose beams open by a third per unit length and hold much of the
# sphere that hovers above the floor; "narrow" one forty units away
SHADOW_LIGHTS = {"wide": ((0.8, 4.5, 0.4), 20, 1, 1, 1), "narrow": ((8, 40, 12), 5, 1, 1, 1)}


def shadow_mesh_text():
    return meshes.uv_sphere_obj(*HOVER_CENTRE, r=1.6, **DENSE["uv_sphere_40x64"])


def shadow_scene(rt, light):
    """The 40 x 64 sphere hovering over a floor with a few small spheres on it, one light, the camera looking down at
    the floor under the mesh from close by: an 8 x 8 tile of the 96 x 64 frame spans about one unit of floor, well
    under RT_R0_CAP = 4 and, under the narrow light, less than the sphere a list's worth of leaves covers."""
    spheres = [(1.0, 0.5, 4.0, 0.5), (7.0, 0.6, 6.5, 0.6), (4.5, 0.4, 8.5, 0.4), (2.5, 0.3, 7.5, 0.3)]
    return Scn(rt, spheres, lights=[SHADOW_LIGHTS[light]], cam=_cam(rt, (4, 5, 8), 180.0, 50.0), planes=[(0, 0, 0, 0, 1, 0)])


def oracle_frame(oracle, inp, w, h, mesh=None, nthreads=16):
    return oracle.render(inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam, w, h,
                         inp.aspect, nthreads=nthreads, mesh=mesh, cubes=inp.cubes, n_cubes=inp.n_cubes,
                         planes=inp.planes, n_planes=inp.n_planes)


# ----------------------------------------------------------------------------- tests
def test_fans_become_leaves_of_their_own_length(rt, oracle):
    for name in ("fans", "fans_normals"):
        om = oracle.Mesh(obj_text(name))
        assert leaf_lengths(om) == list(meshes.FAN_SIZES) == [150, 63, 127, 64, 126, 70, 5, 1]
        start = 0
        for _, _, idx in om.boxes():                       # in the order written: position in the leaf = place in the fan
            assert idx == list(range(start, start + len(idx)))
            start += len(idx)
        assert om.has_normals == (name == "fans_normals")
        pm = rt.mesh_from_obj_text(obj_text(name))
        assert [pm.contents.d_box[j].length for j in range(pm.contents.bvhbox_count)] == list(meshes.FAN_SIZES)
        rt.load_library().rt_mesh_free(pm)
        # the last leaf, whose staged load runs past the end of the vertex array, has length 1 = 1 mod 7
        assert leaf_lengths(om)[-1] % 7 == 1
        tris = om.triangles()
        n = tris[:, 9:12].astype(np.float64)
        assert (np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-5).all()                    # no degenerate triangle
        fan = np.repeat(np.arange(len(meshes.FAN_SIZES)), meshes.FAN_SIZES)
        # neighbours are not coplanar: their unit normals (binary32, so known to 1e-7) are 2e-4 rad apart or more
        sines = np.linalg.norm(np.cross(n[1:], n[:-1]), axis=1)[fan[1:] == fan[:-1]]
        assert sines.min() > 2e-4
    vn = oracle.Mesh(obj_text("fans_normals")).triangles()[:, 12:21].reshape(-1, 3, 3)
    assert (vn[:, 0] == np.float32([0, 0, -1])).all() and (vn[:, 1] != vn[:, 2]).any(axis=1).all()


def test_dense_spheres_exceed_the_leaf_list(oracle):
    small = oracle.Mesh(meshes.uv_sphere_obj())
    assert small.bvhbox_count < RT_BOX_CAP and max(leaf_lengths(small)) < CHUNK     # what the other mesh tests render
    for name in DENSE:
        om = oracle.Mesh(obj_text(name))
        assert om.bvhbox_count > RT_BOX_CAP, (name, om.bvhbox_count)
        assert (om.bvhbox_count + RT_BLOCK - 1) // RT_BLOCK > 64 // RT_BLOCK           # more marked blocks than one step takes
    om = oracle.Mesh(obj_text("uv_sphere_40x64"))
    assert (om.poly_count, om.bvhbox_count) == (4992, 635)
    assert sum(1 for n in leaf_lengths(om) if n > CHUNK) >= 1 and max(leaf_lengths(om)) == 126
    assert oracle.Mesh(obj_text("uv_sphere_24x40")).poly_count == 1840


def test_one_tile_frames_list_or_overflow(rt, oracle):
    om = oracle.Mesh(obj_text("uv_sphere_40x64"))
    for w, h, _ in ONE_TILE_FRAMES:
        for where, dist in ONE_TILE_DISTANCES.items():
            inp = one_tile_scene(rt, oracle, w, h, BIG_SPHERE_CENTRE, dist)
            lower, upper = beam_leaf_bounds(oracle, rt, om, inp, w, h)
            print((w, h), where, "leaves listed: between", lower, "and", upper)
            if where == "list":
                assert 65 <= lower <= upper <= RT_BOX_CAP
            else:
                assert RT_BOX_CAP < lower <= upper <= om.bvhbox_count
            if where == "all":
                assert lower == om.bvhbox_count


def test_fan_cameras_reach_every_chunk(rt, oracle):
    for view in FAN_CAMERAS:
        _, D, rec = fan_reference(rt, oracle, view, "fans")
        assert_fans_reach_every_chunk(oracle, rec, D, view)
        assert {-1, 0, 1, 2} <= set(rec["kind"].tolist())          # sky, triangles, spheres and the floor


def test_split_leaves_is_a_partition_with_the_loaders_bounds(oracle):
    whole = oracle.Mesh(obj_text("uv_sphere_24x40"))
    tris = whole.triangles()
    order = [i for _, _, idx in whole.boxes() for i in idx]
    for max_len in (1, 3, 1000):
        om = split_sphere(oracle, max_len)
        boxes = om.boxes()
        assert om.bvhbox_count == len(boxes) == sum((n + max_len - 1) // max_len for n in leaf_lengths(whole))
        assert [i for _, _, idx in boxes for i in idx] == order             # same order, every triangle exactly once
        assert sorted(order) == list(range(whole.poly_count))
        assert max(len(idx) for _, _, idx in boxes) <= max_len
        for b, org, idx in boxes:                                           # getMinMaxP over the leaf's vertices
            p = tris[idx, :9].reshape(-1, 3)
            assert b == p.min(axis=0).tolist() + p.max(axis=0).tolist()
            assert org == [np.float32((np.float32(b[k]) + np.float32(b[k + 3])) / 2) for k in range(3)]
        if max_len == 1000:
            assert [b[:2] for b in boxes] == [b[:2] for b in whole.boxes()]  # nothing to cut: the loader's own leaves
    om = split_sphere(oracle, 1)
    assert om.bvhbox_count == 1840 > 1024 and (om.bvhbox_count + RT_BLOCK - 1) // RT_BLOCK == 115 > 64
    assert np.array_equal(om.triangles().view(np.uint32), tris.view(np.uint32))
    try:
        om.split_leaves(0)
    except ValueError:
        pass
    else:
        raise AssertionError("max_len = 0 was accepted")


def test_split_mesh_renders_the_unsplit_frame_where_the_mesh_plays_no_part(rt, oracle):
    """A tighter box can only hide a triangle from a ray that would have met it (and then only by rounding), so
    wherever the unsplit mesh changes nothing -- sky and sphere pixels it neither covers nor shadows -- the split
    mesh changes nothing either; and the mesh does take part in a good share of the frame."""
    inp = split_scene(rt)
    w, h = 64, 40
    bare, bare_packed, _ = oracle_frame(oracle, inp, w, h)
    whole = oracle.Mesh(obj_text("uv_sphere_24x40"))
    full, full_packed, cnt = oracle_frame(oracle, inp, w, h, mesh=whole.handle)
    cut, cut_packed, cnt_cut = oracle_frame(oracle, inp, w, h, mesh=split_sphere(oracle, 1).handle)
    untouched = (full.view(np.uint32) == bare.view(np.uint32)).all(axis=2)
    assert 200 < int(untouched.sum()) < w * h - 400
    assert np.array_equal(cut.view(np.uint32)[untouched], bare.view(np.uint32)[untouched])
    assert np.array_equal(cut_packed[untouched], bare_packed[untouched])
    differ = int((cut.view(np.uint32) != full.view(np.uint32)).any(axis=2).sum())
    print("pixels where the split mesh's frame differs from the unsplit one's:", differ, "of", w * h)
    assert cnt_cut["hit_pixels"] <= cnt["hit_pixels"]


def test_hand_made_mesh_flattens_like_the_loaders(rt, oracle):
    """HandMesh of an unsplit oracle mesh is, field by field, what rt_mesh_from_obj_text makes of the same text."""
    txt = obj_text("fans_normals")
    hm = HandMesh(rt, oracle.Mesh(txt))
    pm = rt.mesh_from_obj_text(txt).contents
    mm = hm.mesh
    assert (mm.poly_count, mm.bvhbox_count, mm.has_normals) == (pm.poly_count, pm.bvhbox_count, pm.has_normals)
    assert C.string_at(mm.d_tri_arr, 108 * mm.poly_count) == C.string_at(pm.d_tri_arr, 108 * pm.poly_count)
    for j in range(mm.bvhbox_count):
        a, b = mm.d_box[j], pm.d_box[j]
        assert a.length == b.length and [a.d_indexes[i] for i in range(a.length)] == [b.d_indexes[i] for i in range(b.length)]
        assert C.string_at(C.addressof(a.d_bvhbox.contents) + 8, 72) == C.string_at(C.addressof(b.d_bvhbox.contents) + 8, 72)
