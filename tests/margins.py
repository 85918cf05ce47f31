"""Scenes placed on the margins of the sphere path's culling bounds (the exactness ledger), each with a
WITNESS: the pixels and shadow samples that sit on the bound, and the quantity that puts them there.

Witnesses come from the reference's arithmetic only, never from the device: primary rays from oracle_primary_ray,
closest hits and hit records from query_ref.CastRef, starts `new_org + normal * 1e-5f` (kernel.cu:1647), sample
directions from oracle_light_dirs, sphere::intersect (kernel.cu:293-354) restated in numpy binary32 below with its
intermediates, the occluder lists from the host builder (rt_debug_occluder_lists). Host computation only: the CPU tests
check that every witness is non-empty and on its bound; the GPU tests render the same scenes culled, brute force and
through the oracle and require the same bits.

Builders take (rt, oracle, seed) and return a Margin. Frames stay at or below 64x48 so that the oracle stays fast.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np

f32 = np.float32
START_OFF = f32(0.00001)          # kernel.cu:1647
CAP = 128                         # RT_CAND_CAP


class Margin:
    """A free-form scene (spheres as (x, y, z, constructor radius), lights as (pos, size, r, g, b), the camera as
    (org, yaw, pitch), aspect, frame size) and its witness (a dict; `pixels` lists (x, y) of the pixels on the bound)."""

    def __init__(self, row, seed, spheres, lights, cam, aspect, w, h, witness):
        self.row, self.seed = row, seed
        self.spheres, self.lights, self.cam, self.aspect, self.w, self.h = spheres, lights, cam, aspect, w, h
        self.witness = witness

    def __repr__(self):
        return f"Margin({self.row}, seed={self.seed}, n={len(self.spheres)}, lights={len(self.lights)})"


# ---------------------------------------------------------------------------------------------- the reference's arithmetic
def quad(tab, O, D):
    """sphere::intersect (kernel.cu:293-354) of rays O, D [m, 3] against entries tab [n, 4] = {centre, radius^2}, binary32 in
    the reference's order of operations -> dict of [m, n] arrays: h = D.oc, A, B, C, disc, the far root t and hit."""
    with np.errstate(all="ignore"):
        ocx = (O[:, 0:1] - tab[None, :, 0]).astype(f32)
        ocy = (O[:, 1:2] - tab[None, :, 1]).astype(f32)
        ocz = (O[:, 2:3] - tab[None, :, 2]).astype(f32)
        dx, dy, dz = D[:, 0:1], D[:, 1:2], D[:, 2:3]
        A = ((dx * dx + dy * dy) + dz * dz).astype(f32)
        h = ((dx * ocx + dy * ocy) + dz * ocz).astype(f32)
        B = (f32(2) * h).astype(f32)
        Cq = (((ocx * ocx + ocy * ocy) + ocz * ocz) - tab[None, :, 3]).astype(f32)
        disc = (B * B - (f32(4) * A) * Cq).astype(f32)
        t = ((-B + np.sqrt(disc)) / (f32(2) * A)).astype(f32)
        hit = (t == 0) | (t.astype(np.float64) >= 0.0001)
    return {"h": h, "A": A, "B": B, "C": Cq, "disc": disc, "t": t, "hit": hit}


def line_dist(tab, O, D):
    """float64 distance of the lines O + s D from the centres, [m, n] (the exact geometry the float test rounds)."""
    O64, D64 = O.astype(np.float64), D.astype(np.float64)
    D64 = D64 / np.linalg.norm(D64, axis=1, keepdims=True)
    v = tab[None, :, :3].astype(np.float64) - O64[:, None, :]
    s = (v * D64[:, None, :]).sum(axis=2)
    return np.sqrt(np.maximum((v * v).sum(axis=2) - s * s, 0.0))


def table(spheres):
    """{centre, radius^2} as sphere::intersect reads it: the constructor stores r * r, the test squares that again."""
    tab = np.array([[x, y, z, 0.0] for x, y, z, _ in spheres], dtype=np.float32).reshape(-1, 4)
    for i, (_, _, _, r) in enumerate(spheres):
        rr = f32(f32(r) * f32(r))
        tab[i, 3] = f32(rr * rr)
    return tab


def inputs(rt, m):
    """The scene's inputs as the library and the oracle take them (the fields tests/scenes.py Inputs has)."""
    lib = rt.load_library()
    n = len(m.spheres)
    sph = (rt.Sphere * max(n, 1))()
    for i, (x, y, z, r) in enumerate(m.spheres):
        lib.rt_sphere_init(C.byref(sph[i]), float(x), float(y), float(z), float(r))
    lights = (rt.Light * max(len(m.lights), 1))()
    for i, (p, size, r, g, b) in enumerate(m.lights):
        lights[i] = rt.Light(rt.Vec3(*[float(v) for v in p]), size, r, g, b)
    cam = rt.Camera(rt.Vec3(*[float(v) for v in m.cam[0]]), rt.Vec3(0, 0, 1), 0.0, float(m.cam[1]), float(m.cam[2]))
    return SimpleNamespace(n=n, spheres=sph, lights=lights, n_lights=len(m.lights), cam=cam, aspect=m.aspect,
                           tex=rt.synth_texture(0), sky=rt.synth_texture(1), sky_box=rt.sky_sphere(10000.0))


def primary_rays(oracle, cam, aspect, w, h):
    lib = oracle.load()
    ocam = C.cast(C.pointer(cam), C.POINTER(oracle.OCamera))
    r = oracle.ORay()
    O = np.empty((w * h, 3), dtype=np.float32)
    D = np.empty((w * h, 3), dtype=np.float32)
    for y in range(h):
        for x in range(w):
            lib.oracle_primary_ray(x, y, w, h, aspect, ocam, 0.5, 0.5, C.byref(r))
            O[y * w + x] = (r.Org.x, r.Org.y, r.Org.z)
            D[y * w + x] = (r.Dir.x, r.Dir.y, r.Dir.z)
    return O, D


def aim(oracle, eye, target, aspect, w, h, rt=None):
    """(org, yaw, pitch) of a camera whose centre pixel looks from `eye` at `target`. The ray origin is
    cam.Org + (0, 0, -1/aspect) (kernel.cu:248-258, unrotated), the direction rotateDir(nd, yaw, pitch)."""
    if rt is None:
        import rt_amd
        rt = rt_amd.load()
    org = np.array(eye, dtype=np.float64) + np.array([0.0, 0.0, 1.0 / f32(aspect)])
    cam0 = rt.Camera(rt.Vec3(*[float(v) for v in org]), rt.Vec3(0, 0, 1), 0.0, 0.0, 0.0)
    r = oracle.ORay()
    oracle.load().oracle_primary_ray(w // 2, h // 2, w, h, aspect, C.cast(C.pointer(cam0), C.POINTER(oracle.OCamera)),
                                     0.5, 0.5, C.byref(r))
    a, b, c = r.Dir.x, r.Dir.y, r.Dir.z
    v = np.array(target, dtype=np.float64) - np.array(eye, dtype=np.float64)
    v /= np.linalg.norm(v)
    rho, phi = np.hypot(b, c), np.arctan2(c, b)
    p = np.arccos(np.clip(v[1] / rho, -1, 1)) - phi             # b cos p - c sin p = v_y
    zp = b * np.sin(p) + c * np.cos(p)
    yaw = np.arctan2(v[0], v[2]) - np.arctan2(a, zp)            # (x, z) = rotation of (a, z') by yaw
    return tuple(float(x) for x in org), float(yaw * 180 / 3.1415), float(p * 180 / 3.1415)


def trace(rt, oracle, m):
    """Primary rays, closest hits, starts and sample directions of every hit pixel for every light."""
    import query_ref
    inp = inputs(rt, m)
    O, D = primary_rays(oracle, inp.cam, m.aspect, m.w, m.h)
    ref = query_ref.CastRef(oracle, inp)
    rec = ref.nearest(O, D)
    hits = np.nonzero(rec["kind"] == 1)[0]
    starts = (rec["normal"][hits] * START_OFF + rec["new_org"][hits]).astype(np.float32)
    olib = oracle.load()
    olights = C.cast(inp.lights, C.POINTER(oracle.OLight))
    dirs = np.zeros((len(hits), len(m.lights), 10, 3), dtype=np.float32)
    buf = (C.c_float * 30)()
    sv = oracle.OVec3()
    for k in range(len(hits)):
        sv.x, sv.y, sv.z = (float(v) for v in starts[k])
        for li in range(len(m.lights)):
            olib.oracle_light_dirs(C.byref(sv), C.byref(olights[li]), buf)
            dirs[k, li] = np.frombuffer(buf, dtype=np.float32).reshape(10, 3)
    return SimpleNamespace(O=O, D=D, rec=rec, hits=hits, index=rec["index"][hits], starts=starts, dirs=dirs,
                           normal=rec["normal"][hits], tab=table(m.spheres), inp=inp)


def occluder_lists(rt, inp, li):
    """Host-built occluder lists of light li: counts [n], member sets."""
    lib = rt.load_library()
    n = inp.n
    counts, kcaps, members = (C.c_int * n)(), (C.c_float * n)(), (C.c_int * (n * CAP))()
    assert lib.rt_debug_occluder_lists(inp.spheres, n, C.byref(inp.lights[li]), counts, kcaps, members, CAP) == 0
    cnt = np.array(counts[:])
    mem = np.array(members[:]).reshape(n, CAP)
    return cnt, [set(int(v) for v in mem[i, :cnt[i]]) if cnt[i] >= 0 else None for i in range(n)]


def kbeam(rt, tab, si, lpos):
    """The slope every group on sphere si takes for this light (rt_sphere_beam_slope over the list's ball), <= 0: none."""
    R = np.sqrt(np.float64(tab[si, 3]))
    return rt.load_library().rt_debug_sphere_beam_slope((C.c_double * 3)(*[float(v) for v in lpos]),
                                                        (C.c_double * 3)(*[float(v) for v in tab[si, :3]]),
                                                        R * 1.001 + 1.0e-3)


def ball_excess(tr, si):
    """|start - c_S| - (R_S 1.001 + 1e-3) in float64 for every hit pixel (positive: outside the list's ball)."""
    c = tr.tab[si, :3].astype(np.float64)
    R = np.sqrt(np.float64(tr.tab[si, 3]))
    return np.linalg.norm(tr.starts.astype(np.float64) - c, axis=1) - (R * 1.001 + 1.0e-3)


def facing(tr, lpos):
    toL = lpos[None, :].astype(np.float64) - tr.starts.astype(np.float64)
    toL /= np.linalg.norm(toL, axis=1, keepdims=True)
    return (tr.normal.astype(np.float64) * toL).sum(axis=1)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def _pix(tr, m, k):
    p = int(tr.hits[k])
    return (p % m.w, p // m.w)


# ---------------------------------------------------------------------------------------------- row 1: the list's ball
def list_ball(rt, oracle, seed):
    """Ledger row "spheres not on a group's sphere's occluder list": a small sphere S seen from 40, 100 or 300 units, so
    that float hit points of grazing primary rays (the discriminant cancels) lie OUTSIDE the ball R 1.001 + 1e-3 the
    lists and kbeam are built for; an occluder T is put on a sample ray of such a start, where S's list does not have it.
    Odd seeds put the light close to S, where S has no kbeam (the kernel forms its own slope and checks it against kcap).
    Witness: pixels whose closest hit is S, whose start lies outside the ball, with a sample of a facing light that T
    hits, T not on S's list, and no listed sphere hitting that sample: the pixel's brightness from that light differs
    between "list trusted" and the reference."""
    rng = np.random.default_rng(100 + seed)
    d = (40.0, 100.0, 300.0)[seed % 3]
    R = 0.01 if d < 50 else float(rng.choice([0.02, 0.025, 0.03]))
    no_kbeam = seed % 2 == 1
    w, h = 64, 48
    lib = rt.load_library()
    for attempt in range(30):
        c = np.array([5.0, 5.0, 5.0]) + rng.uniform(-2, 2, 3)
        if no_kbeam:     # within r0 / 0.3 of the centre: rt_sphere_beam_slope has no bound there
            lp = c + _unit(rng) * (R * 1.001 + 1e-3) / 0.3 * rng.uniform(0.6, 0.9)
        else:
            lp = _unit(rng) * rng.uniform(20, 60)
            lp[1] = abs(lp[1]) + 10
        nl = int(rng.integers(1, 4))
        lights = [(tuple(lp), float(rng.uniform(5, 25)), 1.0, 0.8, 0.6)]
        for _ in range(nl - 1):
            q = _unit(rng) * rng.uniform(20, 60)
            lights.append((tuple(q), float(rng.uniform(5, 25)), *[float(v) for v in rng.uniform(0.2, 1.0, 3)]))
        # the camera across the light's direction, so that the silhouette has lit starts displaced sideways
        tl = (lp - c) / np.linalg.norm(lp - c)
        v = _unit(rng)
        v = v - v.dot(tl) * tl
        v = v / np.linalg.norm(v) + tl * rng.uniform(-0.1, 0.3)
        eye = c + v / np.linalg.norm(v) * d
        aspect = float(np.sqrt(2.2 * R / d / 1.4))
        S = (*c, np.sqrt(R))
        # the scene builds occluder lists from 64 spheres on: 62 more, far behind S from light 0, out of view
        uu = (lp - c) / np.linalg.norm(lp - c)
        clutter = [(*(c - uu * rng.uniform(40, 80) + _unit(rng) * 8.0), 0.1) for _ in range(62)]
        m = Margin("list_ball", seed, [S] + clutter, lights, aim(oracle, eye, c, aspect, w, h, rt), aspect, w, h, {})
        tr = trace(rt, oracle, m)
        if len(tr.hits) < 20:
            continue
        ex = np.where(tr.index == 0, ball_excess(tr, 0), -1.0)
        fa = facing(tr, lp)
        # lateral excess: how far the start lies outside the ball's cylinder along the light's axis
        u = lp / np.linalg.norm(lp)
        rel = tr.starts.astype(np.float64) - c
        lat = np.linalg.norm(rel - (rel @ u)[:, None] * u[None, :], axis=1)
        cand = np.nonzero((ex > 0) & (fa > 0.05))[0]
        for k in cand[np.argsort(-lat[cand])][:6]:
            st = tr.starts[k]
            for j in range(10):
                dj = tr.dirs[k, 0, j]
                if quad(tr.tab[:1], st[None, :], dj[None, :])["hit"][0, 0]:
                    continue
                for s_, rT in ((0.05, 0.055), (0.2, 0.1)):
                    tc = (st.astype(np.float64) + dj.astype(np.float64) * s_).astype(np.float32)
                    si = int(rng.random() < 0.5)
                    spheres = [S, (*[float(x) for x in tc], rT)]
                    if si:
                        spheres = spheres[::-1]
                    spheres += clutter
                    m2 = Margin("list_ball", seed, spheres, lights, m.cam, aspect, w, h, {})
                    inp = inputs(rt, m2)
                    cnt, mem = occluder_lists(rt, inp, 0)
                    if cnt[si] < 0 or (1 - si) in mem[si]:
                        continue
                    if (kbeam(rt, table(spheres), si, np.array(lp, dtype=np.float32)) > 0) == no_kbeam:
                        continue
                    m2.witness = list_ball_witness(rt, oracle, m2, si)
                    if m2.witness["pixels"]:
                        return m2
                    break
    raise AssertionError(f"list_ball: no scene on the bound for seed {seed}")


def list_ball_witness(rt, oracle, m, si):
    tr = trace(rt, oracle, m)
    lp = np.array(m.lights[0][0], dtype=np.float32)
    cnt, mem = occluder_lists(rt, tr.inp, 0)
    kb = kbeam(rt, tr.tab, si, lp)
    ex = ball_excess(tr, si)
    fa = facing(tr, lp)
    wit = {"pixels": [], "samples": [], "excess": [], "kbeam": kb, "count": int(cnt[si]), "sphere": si}
    if cnt[si] < 0:
        return wit
    listed = sorted(mem[si])
    others = [i for i in range(len(m.spheres)) if i not in mem[si]]
    for k in np.nonzero((tr.index == si) & (ex > 0) & (fa > 1e-3))[0]:
        q = quad(tr.tab, np.repeat(tr.starts[k:k + 1], 10, axis=0), tr.dirs[k, 0])
        for j in range(10):
            if q["hit"][j, others].any() and not q["hit"][j, listed].any():
                wit["pixels"].append(_pix(tr, m, k))
                wit["samples"].append(j)
                wit["excess"].append(float(ex[k]))
                break
    return wit


# ---------------------------------------------------------------------------------------------- row 2: primary padding
def primary_rounding(rt, oracle, seed):
    """Ledger row of the primary cull's padding (RT_PAD_REL |v|^2 + RT_PAD_ABS, rt_device.h): far, tiny and zero-radius
    spheres filling the frame, so that the float discriminant decides hits by its rounding alone. Witness, both sides:
    pixels whose closest hit is a sphere the float test reports hit although the float64 distance of the ray's line from
    the centre exceeds R ("over"), and rays whose line passes within R (or, for R = 0, within the rounding band) that the
    float test rejects ("under")."""
    rng = np.random.default_rng(200 + seed)
    d = (60.0, 150.0, 400.0)[seed % 3]
    Rs = [0.0, 1e-4, 1e-3][(seed // 3) % 3]
    w, h = 48, 36
    c = np.array([3.0, 4.0, -2.0]) + rng.uniform(-3, 3, 3)
    eye = c + _unit(rng) * d
    band = np.sqrt(Rs * Rs + 9.5e-7 * d * d)
    aspect = float(np.sqrt(2.0 * band / d / 1.4))
    # a handful of spheres around the aim point, spaced by a few bands
    spheres = [(*c, np.sqrt(Rs))]
    axis = (c - eye) / np.linalg.norm(c - eye)
    e1 = np.cross(axis, [0.0, 1.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(axis, e1)
    for _ in range(int(rng.integers(2, 6))):
        off = (e1 * rng.uniform(-1, 1) + e2 * rng.uniform(-1, 1)) * band * 0.8 + axis * rng.uniform(-2, 2)
        spheres.append((*(c + off), float(np.sqrt(rng.choice([0.0, Rs, 2 * Rs])))))
    lights = [(tuple(_unit(rng) * rng.uniform(20, 50)), float(rng.uniform(5, 25)), *[float(v) for v in rng.uniform(0.3, 1, 3)])
              for _ in range(int(rng.integers(1, 4)))]
    m = Margin("primary_rounding", seed, spheres, lights, aim(oracle, eye, c, aspect, w, h, rt), aspect, w, h, {})
    tr = trace(rt, oracle, m)
    tab = tr.tab
    R = np.sqrt(tab[:, 3].astype(np.float64))
    q = quad(tab, tr.O, tr.D)
    ld = line_dist(tab, tr.O, tr.D)
    over = np.nonzero([(tr.rec["kind"][p] == 1 and ld[p, tr.rec["index"][p]] > R[tr.rec["index"][p]]) for p in range(len(tr.O))])[0]
    dist = np.linalg.norm(tab[None, :, :3].astype(np.float64) - tr.O[:, None, :].astype(np.float64), axis=2)
    under_m = ~q["hit"] & (ld <= np.sqrt(R[None, :] ** 2 + 9.5e-7 * dist ** 2))
    under = np.nonzero(under_m.any(axis=1))[0]
    m.witness = {"pixels": [(int(p) % w, int(p) // w) for p in over],
                 "over": [float(ld[p, tr.rec["index"][p]] - R[tr.rec["index"][p]]) for p in over],
                 "under": [(int(p) % w, int(p) // w) for p in under]}
    return m


# ---------------------------------------------------------------------------------------------- rows 3-6: one patch of S
def _clutter(rng, c, u, k=62):
    """Scenes build occluder lists from 64 spheres on: k small spheres far behind c as seen from the light (direction u)."""
    return [(*(c - u * rng.uniform(40, 80) + _unit(rng) * 8.0), 0.1) for _ in range(k)]


def _patch(rt, oracle, rng, R, width, cos_l, w=48, h=36):
    """Sphere S (effective radius R) near the world origin, light 0 at an angle acos(cos_l) from the normal of a point p of
    S, and a camera 4 units out that sees a patch `width` across around p. -> (margin, trace, k0, j): the hit pixel
    nearest the frame's centre and the sample of light 0 whose direction is nearest the normal's side of the light."""
    c = rng.uniform(-0.5, 0.5, 3)
    nrm = _unit(rng)
    t1 = np.cross(nrm, _unit(rng)); t1 /= np.linalg.norm(t1)
    tl = nrm * cos_l + t1 * np.sqrt(1 - cos_l * cos_l)
    p = c + nrm * R
    lp = p + tl * rng.uniform(25, 40)
    lights = [(tuple(lp), float(rng.uniform(2, 10)), 1.0, 0.9, 0.7)]
    for _ in range(int(rng.integers(0, 3))):
        lights.append((tuple(_unit(rng) * rng.uniform(20, 50)), float(rng.uniform(5, 20)), *[float(v) for v in rng.uniform(0.2, 1, 3)]))
    view = nrm * 0.8 - t1 * 0.6                      # the camera on the other side of the normal from the light
    eye = p + view * 4.0
    aspect = float(np.sqrt(width / 4.0 / 2.0))
    u = lp / np.linalg.norm(lp)
    spheres = [(*c, np.sqrt(R))] + _clutter(rng, c, u)
    m = Margin("patch", 0, spheres, lights, aim(oracle, eye, p, aspect, w, h, rt), aspect, w, h, {})
    tr = trace(rt, oracle, m)
    on = np.nonzero(tr.index == 0)[0]
    assert len(on) > w * h // 2, len(on)
    px = tr.hits[on]
    k0 = on[np.argmin((px % w - w / 2) ** 2 + (px // w - h / 2) ** 2)]
    return m, tr, k0


def _samples(tr, rows, si, li=0):
    """quad() of the ten samples of light li from the starts of hit pixels `rows` against entry si -> dict of [k, 10]."""
    O = np.repeat(tr.starts[rows], 10, axis=0)
    D = tr.dirs[rows, li].reshape(-1, 3)
    q = quad(tr.tab[si:si + 1], O, D)
    out = {k: v[:, 0].reshape(len(rows), 10) for k, v in q.items()}
    out["ld"] = line_dist(tr.tab[si:si + 1], O, D)[:, 0].reshape(len(rows), 10)
    out["oc"] = np.linalg.norm(O.astype(np.float64) - tr.tab[si, :3].astype(np.float64), axis=1).reshape(len(rows), 10)
    return out


def _with(rt, oracle, m, row, seed, extra):
    m2 = Margin(row, seed, m.spheres[:1] + extra + m.spheres[1:], m.lights, m.cam, m.aspect, m.w, m.h, {})
    return m2, trace(rt, oracle, m2)


def _on_s(tr, si=0):
    return np.nonzero(tr.index == si)[0]


def _sweep(seed):
    """bound x (1 + delta): delta from {0, +-1e-7, +-1e-6, +-1e-5, +-1e-4}, by seed."""
    return (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4)[seed % 9]


def shadow_rounding(rt, oracle, seed):
    """Row 3, shadow-ray rounding hits: a zero-radius or tiny occluder T 10-40 units out on a sample ray of the patch's
    centre pixel, so that every sample of that index from the patch passes T inside the rounding band of the float test
    (9.5e-7 |oc|^2 on the squared distance). Witness, both sides: samples the float test calls hit although the float64
    line misses T by more than R_T ("over"), and samples whose line passes inside the band that it calls a miss
    ("under"); `listed`: T is on S's list (the list's padding must cover rounding hits)."""
    rng = np.random.default_rng(300 + seed)
    m, tr, k0 = _patch(rt, oracle, rng, float(rng.uniform(0.3, 1.0)), 2e-3, 0.7)
    j = int(rng.integers(0, 10))
    L = float(rng.choice([10.0, 20.0, 40.0]))
    RT = (0.0, 1e-4, 1e-3)[seed % 3] * (1 + _sweep(seed // 3))
    tc = tr.starts[k0].astype(np.float64) + tr.dirs[k0, 0, j].astype(np.float64) * L
    m, tr = _with(rt, oracle, m, "shadow_rounding", seed, [(*tc, float(np.sqrt(RT)))])
    on = _on_s(tr)
    q = _samples(tr, on, 1)
    band = np.sqrt(RT * RT + 9.5e-7 * q["oc"] ** 2)
    over = q["hit"] & (q["ld"] > RT)
    under = ~q["hit"] & (q["ld"] <= band)
    cnt, mem = occluder_lists(rt, tr.inp, 0)
    m.witness = {"pixels": [_pix(tr, m, on[k]) for k in np.nonzero(over.any(axis=1))[0]],
                 "over": int(over.sum()), "under": int(under.sum()), "listed": cnt[0] >= 0 and 1 in mem[0]}
    return m


def t_threshold(rt, oracle, seed):
    """Row 4, the t threshold ((double)t >= 0.0001, kernel.cu:342): even seeds put a tiny occluder T (R_T = 3e-5) next to
    the patch's centre start so that a sample ray's FAR root is 1e-4 x (1 + delta); odd seeds put the camera inside a
    sphere, 1e-4 x (1 + delta) below its surface, looking out, so that the primary rays' far roots straddle 1e-4 (a hit
    there is the negative near root, kernel.cu:1335). Witness, both sides: rays whose float far root lies within 1e-3
    relative of 1e-4, some at or above RT_T_MIN (hit) and some below (miss). (Closer than that no scene can be placed: a
    start's coordinates are quantised at 1e-10 and more, over ten ulp of 1e-4.)"""
    rng = np.random.default_rng(400 + seed)
    delta = _sweep(seed // 2)
    if seed % 2 == 0:
        m, tr, k0 = _patch(rt, oracle, rng, float(rng.uniform(0.2, 0.6)), 6e-5, 0.6)
        j = int(rng.integers(0, 10))
        RT = 3e-5
        tc = tr.starts[k0].astype(np.float64) + tr.dirs[k0, 0, j].astype(np.float64) * (1e-4 * (1 + delta) - RT)
        m, tr = _with(rt, oracle, m, "t_threshold", seed, [(*tc, float(np.sqrt(RT)))])
        on = _on_s(tr)
        q = _samples(tr, on, 1)
        t = q["t"]
        near = np.abs(t.astype(np.float64) / 1e-4 - 1) < 1e-3
        hit, miss = near & q["hit"], near & ~q["hit"]
        pix = [_pix(tr, m, on[k]) for k in np.nonzero((hit | miss).any(axis=1))[0]]
    else:
        w, h = 48, 36
        c = rng.uniform(-1, 1, 3)
        R = float(rng.uniform(0.5, 2.0))
        nrm = _unit(rng)
        eye = c + nrm * (R - 1e-4 * (1 - 4e-3) * (1 + delta))   # (the origin is quantised at ~1e-3 of 1e-4)
        aspect = float(np.sqrt(0.3 / 2.0))
        lights = [(tuple(_unit(rng) * 30), 10.0, 1.0, 1.0, 1.0)]
        m = Margin("t_threshold", seed, [(*c, np.sqrt(R)), (*(c + nrm * (R + 3)), 0.8)], lights,
                   aim(oracle, eye, c + nrm * (R + 5), aspect, w, h, rt), aspect, w, h, {})
        tr = trace(rt, oracle, m)
        q = quad(tr.tab[:1], tr.O, tr.D)
        t = q["t"][:, 0]
        near = np.abs(t.astype(np.float64) / 1e-4 - 1) < 1e-3
        hit, miss = near & q["hit"][:, 0], near & ~q["hit"][:, 0]
        pix = [(int(p) % w, int(p) // w) for p in np.nonzero(hit | miss)[0]]
    m.witness = {"pixels": pix, "hit": int(hit.sum()), "miss": int(miss.sum()), "primary": seed % 2 == 1}
    return m


def shortcut_sure(rt, oracle, seed):
    """Row 5a, the `sure` clause of the shadow test (h < -5e-5 * 4A, rt_shadow.h: shadow_test) and the pre-pass's
    hq + eta < -2.1e-4: a tiny occluder T whose centre projects 2e-4 x (1 + delta) (odd seeds: 2.1e-4) ahead of the patch's
    centre start on a sample ray, 1e-4 off it, radius 1.5e-4: the ray passes through T, the start stays outside. Witness,
    both sides: samples that pass T with h / A within 1e-5 of the threshold above it and below it."""
    rng = np.random.default_rng(500 + seed)
    m, tr, k0 = _patch(rt, oracle, rng, float(rng.uniform(0.2, 0.8)), 3e-4, 0.6)
    j = int(rng.integers(0, 10))
    thr = (2e-4, 2.1e-4)[seed % 2]
    d = tr.dirs[k0, 0, j].astype(np.float64)
    side = np.cross(d, _unit(rng)); side /= np.linalg.norm(side)
    tc = tr.starts[k0].astype(np.float64) + d * thr * (1 + _sweep(seed // 2)) + side * 1e-4
    m, tr = _with(rt, oracle, m, "shortcut_sure", seed, [(*tc, float(np.sqrt(1.5e-4)))])
    on = _on_s(tr)
    q = _samples(tr, on, 1)
    r = q["h"].astype(np.float64) / q["A"].astype(np.float64)
    ok = q["disc"] >= 0
    above = ok & (r > -thr) & (r < -thr + 1e-5)
    below = ok & (r <= -thr) & (r > -thr - 1e-5)
    m.witness = {"pixels": [_pix(tr, m, on[k]) for k in np.nonzero((above | below).any(axis=1))[0]],
                 "above": int(above.sum()), "below": int(below.sum()), "threshold": thr}
    return m


def shortcut_behind(rt, oracle, seed):
    """Row 5b, the `behind` clause (h > 0 and disc < RT_BEHIND_FACTOR B^2 = 0.99999 B^2, rt_cull.h: RT_BEHIND_FACTOR) and the
    pre-pass's C > 1.002e-5 hp^2: S's own test of its shadow rays. A start 1e-5 above S has C ~ 2e-5 R and h ~ R cos,
    so disc / B^2 = 1 - AC / h^2 = 1 - 2e-5 / (R cos^2): with R cos^2 ~ 2 the patch's samples sit on 0.99999. Witness,
    both sides: samples of light 0 against S with h > 0 and disc / B^2 within 1e-6 of 0.99999, above and below."""
    rng = np.random.default_rng(600 + seed)
    R = float(rng.uniform(2.6, 4.0))
    cos_l = float(np.sqrt(2.0 / R)) * (1 + _sweep(seed) * 10)
    m, tr, k0 = _patch(rt, oracle, rng, R, 0.2, min(cos_l, 0.999))
    m.row, m.seed = "shortcut_behind", seed
    on = _on_s(tr)
    q = _samples(tr, on, 0)
    with np.errstate(all="ignore"):
        r = q["disc"].astype(np.float64) / (q["B"].astype(np.float64) ** 2)
    pos = q["h"] > 0
    above = pos & (r >= 0.99999) & (r < 0.99999 + 1e-6)
    below = pos & (r < 0.99999) & (r > 0.99999 - 1e-6)
    pre = q["C"].astype(np.float64) / (q["h"].astype(np.float64) ** 2)
    m.witness = {"pixels": [_pix(tr, m, on[k]) for k in np.nonzero((above | below).any(axis=1))[0]],
                 "above": int(above.sum()), "below": int(below.sum()),
                 "pre_above": int((pos & (pre > 1.002e-5) & (pre < 1.002e-5 * 1.1)).sum()),
                 "pre_below": int((pos & (pre <= 1.002e-5) & (pre > 1.002e-5 * 0.9)).sum())}
    return m


def prepass_guard(rt, oracle, seed):
    """Row 6, the pre-pass's guard (RT_PRE_DELTA, eta = (delta + 2e-6) |oc|, margin 3e-6 |oc|^2, rt_shadow.h: presure_test): an occluder
    T (R_T 0.02-0.1) 0.5-2 units out whose surface a sample ray of the patch's centre start just grazes (distance of the
    line from the centre R_T x (1 + delta)). Witness: samples with |h^2 - C| below 3e-6 |oc|^2, some that the float test
    calls hit and some it calls a miss."""
    rng = np.random.default_rng(700 + seed)
    m, tr, k0 = _patch(rt, oracle, rng, float(rng.uniform(0.3, 1.0)), 2e-4, 0.6)
    j = int(rng.integers(0, 10))
    RT = float(rng.uniform(0.02, 0.1))
    L = float(rng.uniform(0.5, 2.0))
    d = tr.dirs[k0, 0, j].astype(np.float64)
    d /= np.linalg.norm(d)
    side = np.cross(d, _unit(rng)); side /= np.linalg.norm(side)
    tc = tr.starts[k0].astype(np.float64) + d * L + side * RT * (1 + _sweep(seed))
    m, tr = _with(rt, oracle, m, "prepass_guard", seed, [(*tc, float(np.sqrt(RT)))])
    on = _on_s(tr)
    q = _samples(tr, on, 1)
    g = np.abs(q["h"].astype(np.float64) ** 2 - q["C"].astype(np.float64)) < 3e-6 * q["oc"] ** 2
    hit, miss = g & q["hit"], g & ~q["hit"]
    m.witness = {"pixels": [_pix(tr, m, on[k]) for k in np.nonzero((hit | miss).any(axis=1))[0]],
                 "hit": int(hit.sum()), "miss": int(miss.sum())}
    return m


# ---------------------------------------------------------------------------------------------- row 6b: facing away
FACING = -1.0e-4          # the kernel's `a0 < -1.0e-4f` (rt_trace.inc: "facing away: takes no part")


def _amap(m, tr, a):
    """Per hit pixel values `a` as a frame [h, w]; NaN where the closest hit is not sphere 0."""
    out = np.full(m.w * m.h, np.nan)
    on = _on_s(tr)
    out[tr.hits[on]] = a[on]
    return out.reshape(m.h, m.w)


def facing_tiles(m, tr, a, lo=None, hi=None):
    """(tx, ty) of the 8 x 8 tiles that lie wholly inside the frame, whose 64 pixels all hit sphere 0 and whose 64 values
    of `a` (per hit pixel, as facing() returns them) all lie below `hi` / above `lo`."""
    amap = _amap(m, tr, a)
    out = []
    for ty in range(m.h // 8):
        for tx in range(m.w // 8):
            t = amap[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
            if np.isnan(t).any():
                continue
            if (hi is None or (t < hi).all()) and (lo is None or (t > lo).all()):
                out.append((tx, ty))
    return out


def facing_away(rt, oracle, seed):
    """Ledger row "a light for lanes facing away" (normal.toL < -1e-4 with finite factors: the lane takes no part in the
    light; a group all of whose lanes do leaves the light, which is the first of the three exits a light verdict records).
    Light 0 is placed so that the binary64 a = normal.toL of the patch's centre pixel, from the reference's start and
    normal, is -1e-4 x (1 + delta), and the patch is so narrow that a changes by a few 1e-6 per pixel: the bound crosses
    the frame. Nothing but S and the far clutter: S hides no shadow ray that leaves it this flat (|a| < sqrt(2e-5 / R)).
    Witness: hit pixels on S within 5e-6 of the bound on either side; 8 x 8 tiles of S-hits wholly 1e-5 below the bound
    (ten times the 1e-6 the kernel's approximate toL is good for) and tiles wholly 1e-5 above it; `open`: every pixel of
    S has a sample of light 0 that no sphere hits, so the light is not dark for any tile."""
    rng = np.random.default_rng(650 + seed)
    R = float(rng.uniform(0.4, 1.0))
    target = FACING * (1 + _sweep(seed // 2))
    w, h = 48, 36
    m, tr, k0 = _patch(rt, oracle, rng, R, 3.0e-6 * w * R, FACING, w, h)
    # light 0 again, from the reference's start and normal of the centre pixel: a(k0) = target
    n0 = tr.normal[k0].astype(np.float64)
    n0 /= np.linalg.norm(n0)
    lp0 = np.array(m.lights[0][0], dtype=np.float64) - tr.starts[k0].astype(np.float64)
    dist = float(np.linalg.norm(lp0))
    t0 = lp0 - lp0.dot(n0) * n0
    t0 /= np.linalg.norm(t0)
    lp = tr.starts[k0].astype(np.float64) + (n0 * target + t0 * np.sqrt(1 - target * target)) * dist
    size = (0.0, m.lights[0][1])[seed % 2]           # even seeds: a point light, ten identical samples
    lights = [(tuple(lp), size, *m.lights[0][2:])] + m.lights[1:]
    m = Margin("facing_away", seed, m.spheres, lights, m.cam, m.aspect, w, h, {})
    tr = trace(rt, oracle, m)
    a = facing(tr, np.array(lights[0][0], dtype=np.float32))
    on = _on_s(tr)
    below = on[(a[on] >= FACING - 5e-6) & (a[on] < FACING)]
    above = on[(a[on] >= FACING) & (a[on] <= FACING + 5e-6)]
    open_ = True
    for k in on:
        q = quad(tr.tab, np.repeat(tr.starts[k:k + 1], 10, axis=0), tr.dirs[k, 0])
        open_ = open_ and bool((~q["hit"].any(axis=1)).any())
    # the texel most pixels of the patch read (kernel.cu:1653: int(ty * height) * width + int(tx * width), clamped)
    from query_ref import f2i
    th, tw = tr.inp.tex[0].shape
    ci = [min(max(int(f2i(f32(tr.rec["ty"][p] * f32(th)))) * tw + int(f2i(f32(tr.rec["tx"][p] * f32(tw)))), 0), tw * th - 1)
          for p in tr.hits[on]]
    vals, counts = np.unique(ci, return_counts=True)
    texel = int(vals[np.argmax(counts)])
    amap = _amap(m, tr, a)
    with np.errstate(all="ignore"):
        per_pixel = float(np.hypot(np.nanmedian(np.abs(np.diff(amap, axis=1))), np.nanmedian(np.abs(np.diff(amap, axis=0)))))
    m.witness = {"pixels": [_pix(tr, m, k) for k in np.concatenate([below, above])],
                 "below": len(below), "above": len(above), "centre": float(a[k0]), "target": target, "per_pixel": per_pixel,
                 "away_tiles": facing_tiles(m, tr, a, hi=FACING - 1e-5), "lit_tiles": facing_tiles(m, tr, a, lo=FACING + 1e-5),
                 "open": open_, "texel": (texel // tw, texel % tw), "texel_pixels": int(counts.max())}
    return m


# ---------------------------------------------------------------------------------------------- row 7: full occluder
FULL_STEPS = 40


def full_occluder(rt, oracle, seed):
    """Ledger row "all ten samples of a light": one scene per base (seed // FULL_STEPS) in which a large occluder sits
    between S and the light; step seed % FULL_STEPS sets its radius, log-spaced within +-1e-2 relative around r_edge, the
    radius at which it just contains the centre pixel's shadow beam (its ten sample rays, float64). Up to four more spheres
    have their centres 1e-6 ... 1e-3 in front of or behind the plane through that start across the light's direction.
    Witness: the centre pixel's number of hit samples (10 above r_edge, 1-9 below it: asserted over a sweep) and the
    pixels where all ten / one to nine samples hit."""
    base, step = divmod(seed, FULL_STEPS)
    rng = np.random.default_rng(800 + base)
    w, h = 32, 24
    c = np.array([2.0, 1.0, 3.0]) + rng.uniform(-1, 1, 3)
    R = float(rng.uniform(0.5, 1.2))
    lp = c + np.array([rng.uniform(-3, 3), rng.uniform(15, 30), rng.uniform(-3, 3)])
    lights = [(tuple(lp), float(rng.uniform(2, 8)), 1.0, 1.0, 1.0)]
    if base % 2:
        lights.append((tuple(_unit(rng) * 40), 10.0, 0.5, 0.2, 0.9))
    eye = c + np.array([rng.uniform(-1, 1), 1.5, 1.0]) / np.sqrt(4.25) * rng.uniform(6, 12)
    aspect = float(np.sqrt(2.0 * 0.15 * R / np.linalg.norm(eye - c) / 1.4))
    cam = aim(oracle, eye, c + np.array([0, R * 0.9, 0]), aspect, w, h, rt)
    u = lp / np.linalg.norm(lp)
    clutter = _clutter(rng, c, u)
    m0 = Margin("full_occluder", seed, [(*c, np.sqrt(R))] + clutter, lights, cam, aspect, w, h, {})
    tr = trace(rt, oracle, m0)
    on = _on_s(tr)
    k0 = on[len(on) // 2]
    st, dj = tr.starts[k0].astype(np.float64), tr.dirs[k0, 0].astype(np.float64)
    ub = dj.mean(axis=0); ub /= np.linalg.norm(ub)
    oc = st + ub * 5.0
    s = ((oc[None, :] - st[None, :]) * dj).sum(axis=1) / (dj * dj).sum(axis=1)
    r_edge = float(np.max(np.linalg.norm(st[None, :] + dj * s[:, None] - oc[None, :], axis=1)))
    rr = float(r_edge * np.exp(np.linspace(np.log(1 - 1e-2), np.log(1 + 1e-2), FULL_STEPS))[step])
    extra = []
    for _ in range(int(rng.integers(0, 5))):
        off = float(rng.choice([1e-6, 1e-5, 1e-4, 1e-3])) * float(rng.choice([-1, 1]))
        pp = st + ub * off + np.cross(ub, _unit(rng)) * rng.uniform(0.5, 2)
        extra.append((*pp, float(np.sqrt(rng.uniform(0.05, 0.3)))))
    # (constructor radius: the effective radius is its square)
    m = Margin("full_occluder", seed, [(*c, np.sqrt(R)), (*oc, float(np.sqrt(rr)))] + extra + clutter, lights, cam, aspect,
               w, h, {})
    tr = trace(rt, oracle, m)
    full, part, centre = [], [], None
    for k in _on_s(tr):
        q = quad(tr.tab, np.repeat(tr.starts[k:k + 1], 10, axis=0), tr.dirs[k, 0])
        nh = int(q["hit"].any(axis=1).sum())
        if tr.hits[k] == tr.hits[k0] if k0 < len(tr.hits) else False:
            centre = nh
        (full if nh == 10 else part if nh > 0 else []).append(_pix(tr, m, k))
    eff = float(np.sqrt(np.float64(tr.tab[1, 3])))
    m.witness = {"pixels": full + part, "full": full, "partial": part, "centre_hits": centre, "rel": eff / r_edge - 1}
    return m


def full_occluder_inside(rt, oracle, seed):
    """The same ledger row away from its edge: the base scenes of full_occluder with the occluder's radius 3 and 4 times
    r_edge. The sweep above stays within 1e-2 of the edge, where the kernel's test of the whole group's beam against one
    sphere (conservative: the group's ball, the padded slope) never holds -- measured: not below 1.5 r_edge, in every tile
    only from about 3 r_edge on -- so that none of its scenes takes the exit that skips the light. These do. Witness: pixels
    of S whose ten samples of light 0 all hit the occluder, and the 8 x 8 tiles that consist of such pixels only."""
    base, big = seed % 2, (3.0, 4.0)[(seed // 2) % 2]
    m = full_occluder(rt, oracle, base * FULL_STEPS + FULL_STEPS - 1)
    x, y, z, r = m.spheres[1]
    spheres = list(m.spheres)
    spheres[1] = (x, y, z, float(np.sqrt(r * r * big)))
    m = Margin("full_occluder_inside", seed, spheres, m.lights, m.cam, m.aspect, m.w, m.h, {})
    tr = trace(rt, oracle, m)
    on = _on_s(tr)
    q = _samples(tr, on, 1)
    full = [_pix(tr, m, k) for k, row in zip(on, q["hit"]) if row.all()]
    fmap = np.zeros((m.h, m.w), dtype=bool)
    for x_, y_ in full:
        fmap[y_, x_] = True
    tiles = sum(bool(fmap[ty:ty + 8, tx:tx + 8].all()) for ty in range(0, m.h - 7, 8) for tx in range(0, m.w - 7, 8))
    m.witness = {"pixels": full, "full": len(full), "on_s": len(on), "full_tiles": tiles, "factor": big}
    return m


# ---------------------------------------------------------------------------------------------- row 8: front to back
def front_to_back(rt, oracle, seed):
    """Ledger row of the front-to-back walk of the primary list (allowance 1e-3 + 1.5e-3 (dist + R), rt_cull.h: build_list2) and of
    "first index wins" (kernel.cu:1335). Two DIFFERENT spheres whose near roots meet, seen through a frame zoomed onto
    where they meet: even seeds, two spheres whose surfaces cross (the camera aims at a point of the crossing circle);
    odd seeds, internally tangent at the point facing the camera. Their order in the list alternates every two seeds. Witness: pixels whose two nearest float near roots are equal or one ulp apart,
    with the two spheres' normals different there (so which one wins shows in the shading)."""
    rng = np.random.default_rng(900 + seed)
    w, h = 32, 24
    kind = seed % 2
    c = np.array([1.0, 2.0, 0.0]) + rng.uniform(-2, 2, 3)
    eye = c + _unit(rng) * 3.0     # (near roots carry rounding noise of ~1e-5 dist^2: close up it stays below an ulp)
    axis = (c - eye) / np.linalg.norm(c - eye)
    R = float(rng.uniform(0.3, 1.2))
    a = np.sqrt(R)
    if kind == 0:      # crossing: a second sphere whose surface passes through the point p seen at the frame's centre
        side = np.cross(axis, _unit(rng)); side /= np.linalg.norm(side)
        p = c - axis * R * 0.6 + side * R * 0.8
        p = c + (p - c) / np.linalg.norm(p - c) * R
        r2 = R * float(rng.uniform(0.4, 0.8))
        q_ = side * rng.uniform(0.2, 0.6) - axis * rng.uniform(0.2, 0.6); q_ /= np.linalg.norm(q_)
        c2 = p - q_ * r2
        second, target, width = (*c2, np.sqrt(r2)), p, 3e-5
    elif kind == 1:    # internally tangent at the point facing the camera
        r2 = R * float(rng.uniform(0.3, 0.9))
        second, target, width = (*(c - axis * (R - r2)), float(np.sqrt(r2))), c - axis * R, 2e-3
    spheres = [(*c, float(f32(a))), second]
    if (seed // 2) % 2:
        spheres = spheres[::-1]
    lights = [(tuple(_unit(rng) * rng.uniform(15, 40)), float(rng.uniform(5, 20)), *[float(v) for v in rng.uniform(0.3, 1, 3)])
              for _ in range(int(rng.integers(1, 4)))]
    dist = float(np.linalg.norm(target - eye))
    aspect = float(np.sqrt(width / dist / 2.0))
    m = Margin("front_to_back", seed, spheres, lights, aim(oracle, eye, target, aspect, w, h, rt), aspect, w, h, {})
    tr = trace(rt, oracle, m)
    q = quad(tr.tab, tr.O, tr.D)
    with np.errstate(all="ignore"):
        tn = ((-q["B"] - np.sqrt(q["disc"]).astype(f32)) / (f32(2) * q["A"])).astype(f32)
    both = q["hit"].all(axis=1) & (tn > 0).all(axis=1)
    gap = np.abs(tn[:, 0].view(np.int32).astype(np.int64) - tn[:, 1].view(np.int32).astype(np.int64))
    sel = np.nonzero(both & (gap <= 1))[0]
    with np.errstate(all="ignore"):
        hp = (tr.O[sel] + tr.D[sel] * tn[sel, :1]).astype(f32)
    n0 = hp - tr.tab[0, :3]
    n1 = hp - tr.tab[1, :3]
    differ = [bool(not np.array_equal(n0[i] / np.linalg.norm(n0[i]), n1[i] / np.linalg.norm(n1[i]))) for i in range(len(sel))]
    m.witness = {"pixels": [(int(p) % w, int(p) // w) for p in sel], "ulp_gaps": [int(gap[p]) for p in sel],
                 "normals_differ": int(sum(differ)), "kind": ("crossing", "tangent")[kind]}
    return m


# seeds of each builder the tests render; list_ball's odd seeds (no kbeam) find a scene on the bound only at some seeds
LIST_BALL_SEEDS = [0, 2, 4, 6, 8, 10, 11, 12, 14, 16, 18, 19, 20, 22]
BUILDERS = {
    "list_ball": (list_ball, LIST_BALL_SEEDS),
    "primary_rounding": (primary_rounding, list(range(18))),
    "shadow_rounding": (shadow_rounding, list(range(27))),
    "t_threshold": (t_threshold, list(range(18))),
    "shortcut_sure": (shortcut_sure, list(range(18))),
    "shortcut_behind": (shortcut_behind, list(range(9))),
    "prepass_guard": (prepass_guard, list(range(18))),
    "facing_away": (facing_away, list(range(18))),
    "full_occluder": (full_occluder, list(range(2 * FULL_STEPS))),
    "full_occluder_inside": (full_occluder_inside, list(range(4))),
    "front_to_back": (front_to_back, list(range(16))),
}
