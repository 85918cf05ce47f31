"""Mirror reflections (rt_launch_opts.reflect_depth), host side: the composed CPU reference the GPU tests compare
with, the sphere BVH through its host debug entries, reflect() known answers, layouts and validation.

The composed reference follows the semantics of DESIGN.md "Reflections" bounce by bounce, from the oracle's unit
entry points (primary ray, castLightRay, atan2f / acosf, the pack) and numpy binary32 arrays for the intersections
(numpy has no FMA: every product and sum is rounded as the reference's expressions are)."""
import ctypes as C

import numpy as np
import pytest

f32 = np.float32
RT_T_MIN = 0.0001


# ----------------------------------------------------------------------------- numpy binary32 building blocks
def sphere_table(spheres, n):
    """{cx, cy, cz, radius*radius} per sphere: what sphere::intersect reads (the `radius` field is already r*r)."""
    tab = np.empty((n, 4), dtype=np.float32)
    for i in range(n):
        s = spheres[i]
        tab[i] = (s.orgin.x, s.orgin.y, s.orgin.z, f32(s.radius) * f32(s.radius))
    return tab


def intersect(O, D, tab):
    """sphere::intersect (kernel.cu:293-354) of rays O, D [m, 3] against spheres tab [n, 4] -> hit [m, n], t [m, n]."""
    with np.errstate(all="ignore"):
        ocx = O[:, 0:1] - tab[None, :, 0]
        ocy = O[:, 1:2] - tab[None, :, 1]
        ocz = O[:, 2:3] - tab[None, :, 2]
        dx, dy, dz = D[:, 0:1], D[:, 1:2], D[:, 2:3]
        A = (dx * dx + dy * dy) + dz * dz
        B = f32(2) * ((dx * ocx + dy * ocy) + dz * ocz)
        Cq = ((ocx * ocx + ocy * ocy) + ocz * ocz) - tab[None, :, 3]
        disc = B * B - (f32(4) * A) * Cq
        sq = np.sqrt(disc)
        a2 = f32(2) * A
        t = (-B + sq) / a2
        t2 = (-B - sq) / a2
        far = t.astype(np.float64) >= RT_T_MIN
        hit = (t == 0) | far
        t = np.where(far & (t > t2), t2, t)
    return hit, t.astype(np.float32)


def nearest(O, D, tab, chunk=4096):
    """castRay's sphere loop: strict t < nt, the first index wins ties. -> index (-1: none), t."""
    m = O.shape[0]
    idx = np.full(m, -1, dtype=np.int64)
    tt = np.full(m, np.inf, dtype=np.float32)
    for a in range(0, m, chunk):
        hit, t = intersect(O[a:a + chunk], D[a:a + chunk], tab)
        tv = np.where(hit, t, f32(np.inf))
        j = np.argmin(tv, axis=1)
        best = tv[np.arange(tv.shape[0]), j]
        ok = best < np.inf
        idx[a:a + chunk] = np.where(ok, j, -1)
        tt[a:a + chunk] = best
    return idx, tt


def normalise(v):
    with np.errstate(all="ignore"):
        l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        nz = l != 0
        out = np.where(nz[:, None], v / np.where(nz, l, f32(1))[:, None], f32(0)).astype(np.float32)
    return out


def reflect(I, N):
    """reflect(), kernel.cu:1282-1285: sub(I, multiply(multiply(N, dot(I, N)), 2)), dot left to right."""
    d = (I[:, 0] * N[:, 0] + I[:, 1] * N[:, 1]) + I[:, 2] * N[:, 2]
    return (I - (N * d[:, None]) * f32(2)).astype(np.float32)


def f2i(v):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        r = np.where(np.isnan(v), 0.0, np.clip(np.trunc(v.astype(np.float64)), -2147483648.0, 2147483647.0))
    return r.astype(np.int64)


# ----------------------------------------------------------------------------- the composed reference
class Composer:
    def __init__(self, oracle, rt, spheres, n, tex, sky, sky_box, lights, n_lights, cam, aspect):
        self.lib = oracle.load()
        self.oracle = oracle
        self.spheres, self.n = spheres, n
        self.tab = sphere_table(spheres, n)
        self.tex = [np.ascontiguousarray(p, dtype=np.float32) for p in tex]
        self.sky = [np.ascontiguousarray(p, dtype=np.float32) for p in sky]
        self.sky_box = sky_box
        self.sky_c = np.array([sky_box.orgin.x, sky_box.orgin.y, sky_box.orgin.z], dtype=np.float32)
        self.sky_w = f32(sky_box.radius) * f32(sky_box.radius)
        self.lights, self.n_lights = lights, n_lights
        self.cam, self.aspect = cam, aspect
        self.osph = C.cast(spheres, C.POINTER(oracle.OSphere))
        self.olights = C.cast(lights, C.POINTER(oracle.OLight))

    def primary(self, W, H, y0, y1):
        lib, oc = self.lib, self.oracle
        cam = C.cast(C.pointer(self.cam), C.POINTER(oc.OCamera))
        r = oc.ORay()
        rows = y1 - y0
        O = np.empty((rows * W, 3), dtype=np.float32)
        D = np.empty((rows * W, 3), dtype=np.float32)
        k = 0
        for y in range(y0, y1):
            for x in range(W):
                lib.oracle_primary_ray(x, y, W, H, self.aspect, cam, 0.5, 0.5, C.byref(r))
                O[k] = (r.Org.x, r.Org.y, r.Org.z)
                D[k] = (r.Dir.x, r.Dir.y, r.Dir.z)
                k += 1
        return O, D

    def sky_color(self, O, D):
        """skybox::getFColor, kernel.cu:1147-1166."""
        lib = self.lib
        tab = np.array([[*self.sky_c, self.sky_w]], dtype=np.float32)
        _, t = intersect(O, D, tab)
        t = t[:, 0]
        with np.errstate(all="ignore"):
            hp = O + D * t[:, None]
        nrm = normalise((hp - self.sky_c[None, :]).astype(np.float32))
        h, w = self.sky[0].shape
        out = np.empty((O.shape[0], 3), dtype=np.float32)
        for i in range(O.shape[0]):
            nx, ny, nz = (float(v) for v in nrm[i])
            a = f32(lib.oracle_atan2f(nz, nx))
            ix = f2i(f32(f32(f32(f32(1) + f32(a / f32(3.1415))) * f32(0.5)) * f32(w)))
            iy = f2i(f32(f32(f32(lib.oracle_acosf(ny)) / f32(3.1415)) * f32(h)))
            idx = int(min(max(int(iy) * w + int(ix), 0), w * h - 1))
            out[i] = (self.sky[0].flat[idx], self.sky[1].flat[idx], self.sky[2].flat[idx])
        return out

    def shade(self, O, D, idx, t):
        """Hit frame (kernel.cu:1398-1405, 1647) and the three-light sum L (kernel.cu:1643-1679) for hit rays."""
        lib, oc = self.lib, self.oracle
        with np.errstate(all="ignore"):
            new_org = (O + D * t[:, None]).astype(np.float32)
        N = normalise((new_org - self.tab[idx, :3]).astype(np.float32))
        start = (N * f32(0.00001) + new_org).astype(np.float32)
        th, tw = self.tex[0].shape
        L = np.zeros((O.shape[0], 3), dtype=np.float32)
        sv, nv = oc.OVec3(), oc.OVec3()
        for i in range(O.shape[0]):
            nx, ny, nz = (float(v) for v in N[i])
            tx = f32((1.0 + float(f32(lib.oracle_atan2f(nz, nx))) / 3.1415) * 0.5)
            ty = f32(float(f32(lib.oracle_acosf(ny))) / 3.1415)
            ci = int(f2i(f32(ty * f32(th)))) * tw + int(f2i(f32(tx * f32(tw))))
            ci = min(max(ci, 0), tw * th - 1)
            texel = (self.tex[0].flat[ci], self.tex[1].flat[ci], self.tex[2].flat[ci])
            sv.x, sv.y, sv.z = (float(v) for v in start[i])
            nv.x, nv.y, nv.z = nx, ny, nz
            acc = [f32(0), f32(0), f32(0)]
            for li in range(self.n_lights):
                b = f32(lib.oracle_cast_light_ray(self.osph, self.n, C.byref(sv), C.byref(self.olights[li]), C.byref(nv)))
                lc = (self.lights[li].r, self.lights[li].g, self.lights[li].b)
                for ch in range(3):
                    acc[ch] = f32(acc[ch] + f32(f32(b * f32(lc[ch])) * texel[ch]))
            L[i] = acc
        return N, start, L

    def render(self, W, H, k, depth, y0=0, y1=None):
        """rgba [rows, W, 4] float32 and packed [rows, W] uint32 of the reflective frame (DESIGN.md "Reflections").
        self.trace[b] records what bounce b's rays met: `index` (-1 = sky), `t` and, for hits, `cos` = |D.N|."""
        y1 = H if y1 is None else y1
        self.trace = []
        O, D = self.primary(W, H, y0, y1)
        m = O.shape[0]
        c = np.zeros((m, 3), dtype=np.float32)
        w = np.ones(m, dtype=np.float32)
        first = np.ones(m, dtype=bool)
        live = np.arange(m)
        k = np.asarray(k, dtype=np.float32)
        for b in range(depth + 1):
            if live.size == 0:
                break
            Ob, Db, wb = O[live], D[live], w[live]
            idx, t = nearest(Ob, Db, self.tab)
            term = np.zeros((live.size, 3), dtype=np.float32)
            hit = idx >= 0
            go = np.zeros(live.size, dtype=bool)
            cos = np.full(live.size, np.nan, dtype=np.float32)
            if (~hit).any():
                term[~hit] = wb[~hit, None] * self.sky_color(Ob[~hit], Db[~hit])
            if hit.any():
                hi = np.nonzero(hit)[0]
                N, start, L = self.shade(Ob[hi], Db[hi], idx[hi], t[hi])
                cos[hi] = np.abs((Db[hi] * N).sum(axis=1))
                kk = k[idx[hi]]
                stop = (kk == 0) | (b == depth)
                fac = np.where(stop, wb[hi], wb[hi] * (f32(1) - kk)).astype(np.float32)
                term[hi] = fac[:, None] * L
                cont = hi[~stop]
                go[cont] = True
                O[live[cont]] = start[~stop]
                D[live[cont]] = reflect(Db[cont], N[~stop])
                w[live[cont]] = wb[cont] * kk[~stop]
            self.trace.append({"index": idx, "t": t, "cos": cos})
            fl = first[live]
            c[live[fl]] = term[fl]
            c[live[~fl]] = c[live[~fl]] + term[~fl]
            first[live] = False
            live = live[go]
        rows = y1 - y0
        rgba = np.ones((m, 4), dtype=np.float32)
        rgba[:, :3] = c
        packed = np.empty(m, dtype=np.uint32)
        for i in range(m):
            packed[i] = self.lib.oracle_pack_color(float(c[i, 0]), float(c[i, 1]), float(c[i, 2]))
        return rgba.reshape(rows, W, 4), packed.reshape(rows, W)


def composer_for(oracle, rt, inp):
    return Composer(oracle, rt, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam,
                    inp.aspect)


# ----------------------------------------------------------------------------- tests
def test_composed_reference_equals_the_oracle_without_reflections(oracle, rt):
    """All k = 0: the composition is the reference's frame bit for bit (the c3_160x90_n1024 fixture's scene)."""
    from scenes import Inputs
    inp = Inputs(rt, 1024)
    W, H = 160, 90
    ref_rgba, ref_packed, _ = inp.oracle_render(oracle, W, H)
    comp = composer_for(oracle, rt, inp)
    rgba, packed = comp.render(W, H, np.zeros(inp.n, dtype=np.float32), 3)
    assert np.array_equal(rgba.view(np.uint32), ref_rgba.reshape(H, W, 4).view(np.uint32))
    assert np.array_equal(packed, ref_packed.reshape(H, W))
    gold = np.load(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "c3_160x90_n1024.npz"))
    key = [k for k in gold.files if "packed" in k]
    if key:
        assert np.array_equal(packed.reshape(-1), gold[key[0]].reshape(-1).view(np.uint32))


def test_reflect_known_answers(rt):
    lib = rt.load_library()
    V = rt.Vec3
    I = (V * 3)(V(0, 0, 1), V(1, -1, 0), V(0.6, -0.8, 0))
    N = (V * 3)(V(0, 0, -1), V(0, 1, 0), V(0, 1, 0))
    out = (V * 3)()
    assert lib.rt_debug_reflect(I, N, 3, out) == 0
    got = [(o.x, o.y, o.z) for o in out]
    assert got[0] == (0.0, 0.0, -1.0)            # head-on mirror: straight back along -I
    assert got[1] == (1.0, 1.0, 0.0)             # 45 degrees: the normal component flips
    assert got[2] == (float(f32(0.6)), float(f32(f32(-0.8) - f32(f32(f32(-0.8)) * f32(2)))), 0.0)
    # and the numpy restatement agrees bit for bit on random vectors
    rng = np.random.default_rng(5)
    a = rng.standard_normal((1000, 3)).astype(np.float32)
    nn = normalise(rng.standard_normal((1000, 3)).astype(np.float32))
    Ia = (V * 1000)(*[V(*map(float, r)) for r in a])
    Na = (V * 1000)(*[V(*map(float, r)) for r in nn])
    outa = (V * 1000)()
    assert lib.rt_debug_reflect(Ia, Na, 1000, outa) == 0
    got = np.array([(o.x, o.y, o.z) for o in outa], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), reflect(a, nn).view(np.uint32))


def test_layouts(rt):
    assert C.sizeof(rt.Material) == 12
    assert rt.Material.transperancy.offset == 4 and rt.Material.roughness.offset == 8
    assert rt.LaunchOpts.reflect_depth.offset == 104          # appended after `fast`: the older layout is 104 bytes
    assert C.sizeof(rt.LaunchOpts) == 112
    assert rt.FrameDesc.opts.offset + rt.LaunchOpts.reflect_depth.offset == 168
    assert rt.RT_MAX_REFLECT_DEPTH == 8


def test_materials_need_one_per_sphere(rt):
    lib = rt.load_library()
    s = lib.rt_scene_create()          # host only: no sphere list yet (count 0)
    try:
        m = (rt.Material * 2)()
        assert lib.rt_scene_set_materials(s, m, 2) == 1          # RT_ERR_INVALID: 2 materials for 0 spheres
        assert lib.rt_scene_set_materials(s, None, 0) == 0       # clearing is always fine
    finally:
        lib.rt_scene_destroy(s)


def _bvh(rt, sph, n):
    lib = rt.load_library()
    cap = 2 * n + 2
    lohi = np.zeros(cap * 6, dtype=np.float32)
    meta = np.zeros(cap * 2, dtype=np.int32)
    order = np.zeros(n, dtype=np.int32)
    nn, dep = C.c_int(), C.c_int()
    rc = lib.rt_debug_sphere_bvh(sph, n, lohi.ctypes.data_as(C.POINTER(C.c_float)), meta.ctypes.data_as(C.POINTER(C.c_int)),
                                 order.ctypes.data_as(C.POINTER(C.c_int)), cap, C.byref(nn), C.byref(dep))
    assert rc == 0, lib.rt_last_error()
    return lohi[:6 * nn.value].reshape(-1, 6), meta[:2 * nn.value].reshape(-1, 2), order, dep.value


def adversarial_spheres(rt):
    """The default scene's spheres plus overlapping, duplicate, nested and tiny far ones."""
    base = rt.generate_spheres(512, 3)
    extra = [(0, 2, 0, 1.5), (0.5, 2, 0, 1.5), (0.5, 2, 0, 1.5), (0, 2, 0, 0.5), (3, 3, 3, 1.0), (3, 3, 3, 1.0),
             (40, 5, 40, 0.03), (41, 5, 40, 0.02), (-120, 8, 200, 0.03), (2, 2, 2, 1.2)]
    n = 512 + len(extra)
    arr = (rt.Sphere * n)()
    for i in range(512):
        arr[i] = base[i]
    lib = rt.load_library()
    for j, (x, y, z, r) in enumerate(extra):
        lib.rt_sphere_init(C.byref(arr[512 + j]), x, y, z, r)
    return arr, n


def test_bvh_structure(rt):
    sph, n = adversarial_spheres(rt)
    boxes, meta, order, depth = _bvh(rt, sph, n)
    tab = sphere_table(sph, n)
    assert sorted(order.tolist()) == list(range(n))              # every sphere in exactly one leaf
    parent = {}
    for j, (first, cnt) in enumerate(meta):
        if cnt == 0:
            parent[first] = j
            parent[first + 1] = j
    seen = 0
    for j, (first, cnt) in enumerate(meta):
        if cnt == 0:
            continue
        assert 1 <= cnt <= 4
        for p in range(first, first + cnt):
            s = tab[order[p]]
            R = np.sqrt(np.float64(s[3]))
            node = j
            while True:                                          # inside its leaf's box and every ancestor's
                lo, hi = boxes[node, :3].astype(np.float64), boxes[node, 3:].astype(np.float64)
                assert np.all(lo <= s[:3].astype(np.float64) - R) and np.all(hi >= s[:3].astype(np.float64) + R)
                if node == 0:
                    break
                node = parent[node]
            seen += 1
    assert seen == n
    assert depth <= 2 + int(np.ceil(np.log2(n / 4)))


def _rays(rt, sph, n, m, seed):
    """Rays of every kind the passes send: from far and near, from inside one or several spheres, tangent to
    silhouettes, and from sphere surfaces along reflected directions."""
    rng = np.random.default_rng(seed)
    tab = sphere_table(sph, n)
    R = np.sqrt(tab[:, 3].astype(np.float64)).astype(np.float32)
    O = np.empty((m, 3), dtype=np.float32)
    D = np.empty((m, 3), dtype=np.float32)
    kind = rng.integers(0, 5, m)
    pick = rng.integers(0, n, m)
    c = tab[pick, :3]
    R = R[pick]
    u = normalise(rng.standard_normal((m, 3)).astype(np.float32))
    v = normalise(rng.standard_normal((m, 3)).astype(np.float32))
    # 0: anywhere in the scene box towards anywhere
    O0 = (rng.uniform(-30, 30, (m, 3))).astype(np.float32)
    # 1: inside a sphere (possibly several overlapping)
    O1 = (c + u * (R[:, None] * rng.uniform(0, 0.99, (m, 1)).astype(np.float32))).astype(np.float32)
    # 2: tangent to a silhouette: aimed at a point on the sphere's rim as seen from the origin
    dirc = normalise((c - O0).astype(np.float32))
    perp = normalise(np.cross(dirc, v).astype(np.float32))
    rim = (c + perp * (R[:, None] * rng.choice([0.9999, 1.0, 1.0001], (m, 1)).astype(np.float32))).astype(np.float32)
    D2 = normalise((rim - O0).astype(np.float32))
    # 3: the reference's start_O on a sphere surface, along a reflected direction
    surf = (c + u * R[:, None]).astype(np.float32)
    N3 = normalise((surf - c).astype(np.float32))
    start = (N3 * f32(0.00001) + surf).astype(np.float32)
    D3 = reflect(normalise((surf - O0).astype(np.float32)), N3)
    # 4: far camera (40..300 units) at the tiny spheres
    O4 = (rng.standard_normal((m, 3)) * 150).astype(np.float32)
    D4 = normalise((c - O4).astype(np.float32))
    for k, (Ok, Dk) in enumerate([(O0, u), (O1, v), (O0, D2), (start, D3), (O4, D4)]):
        sel = kind == k
        O[sel], D[sel] = Ok[sel], Dk[sel]
    return O, D


def test_bvh_cast_equals_brute_force(rt, oracle):
    lib = rt.load_library()
    sph, n = adversarial_spheres(rt)
    m = 120000
    O, D = _rays(rt, sph, n, m, 11)
    rays = (rt.Ray * m)()
    buf = np.frombuffer(rays, dtype=np.float32).reshape(m, 6)
    buf[:, :3], buf[:, 3:] = O, D
    out = {}
    for use in (1, 0):
        h = np.zeros(m, dtype=np.int32)
        t = np.zeros(m, dtype=np.float32)
        a = np.zeros(m, dtype=np.int32)
        assert lib.rt_debug_bvh_cast(sph, n, rays, m, use, h.ctypes.data_as(C.POINTER(C.c_int)),
                                     t.ctypes.data_as(C.POINTER(C.c_float)), a.ctypes.data_as(C.POINTER(C.c_int))) == 0
        out[use] = (h, t, a)
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1].view(np.uint32), out[0][1].view(np.uint32))
    assert np.array_equal(out[1][2], out[0][2])
    assert (out[0][0] >= 0).sum() > m // 4 and (out[0][1][out[0][0] >= 0] < 0).any()   # hits, some from inside
    # the brute-force walk is sphere::intersect with the reference's loop (numpy restatement, a subset)
    tab = sphere_table(sph, n)
    idx, tt = nearest(O[:20000], D[:20000], tab)
    assert np.array_equal(idx, out[0][0][:20000].astype(np.int64))
    assert np.array_equal(tt.view(np.uint32), out[0][1][:20000].view(np.uint32))
