"""Refraction (rt_scene_set_materials_ex, DESIGN.md "Refraction"), host side: the glass composer the GPU tests compare
with, refract() and the glass step through their host debug entries (bit for bit against a numpy binary32 restatement,
and against float64 physics), layouts and validation.

The glass composer extends the mirror composer of test_reflect_cpu.py: the same bounce loop, with one more kind of
continuation per hit -- through the sphere instead of off it."""
import ctypes as C

import numpy as np
import pytest

from test_reflect_cpu import Composer, composer_for, normalise, reflect, nearest, sphere_table

f32 = np.float32


# ----------------------------------------------------------------------------- numpy binary32 restatement of the rules
def dot_rows(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def refract(I, N, eta):
    """refract(I, n, eta): c = -dot(I, n), q = 1 - (eta*eta) * (1 - c*c), s = sqrt(max(q, 0)), I*eta + n*(eta*c - s).
    Also returns whether the radicand was clamped (q <= 0)."""
    eta = np.broadcast_to(np.asarray(eta, dtype=np.float32), (I.shape[0],))
    with np.errstate(all="ignore"):
        c = -dot_rows(I, N)
        q = f32(1) - (eta * eta) * (f32(1) - c * c)
        s = np.sqrt(np.where(q > 0, q, f32(0))).astype(np.float32)
        f = (eta * c - s).astype(np.float32)
        out = (I * eta[:, None] + N * f[:, None]).astype(np.float32)
    return out, ~(q > 0)


def far_root(P, T, tab):
    """(-B + sqrt(disc)) / a2 of sphere::intersect for rays (P, T) against one sphere row each of tab [m, 4]."""
    with np.errstate(all="ignore"):
        oc = (P - tab[:, :3]).astype(np.float32)
        B = f32(2) * dot_rows(T, oc)
        Cq = dot_rows(oc, oc) - tab[:, 3]
        A = dot_rows(T, T)
        disc = B * B - (f32(4) * A) * Cq
        a2 = f32(2) * dot_rows(T, T)
        return ((-B + np.sqrt(disc)) / a2).astype(np.float32)


def transmit(D, N, start, new_org, tab, ior):
    """The glass step for hits (rows): -> origin, direction, rule (1, 3 or 4), clamp (a refract radicand <= 0), and the
    chord's P, T, t1 (NaN where the ray did not enter)."""
    m = D.shape[0]
    ior = np.asarray(ior, dtype=np.float32)
    rule = np.where(dot_rows(D, N) >= 0, 1, 4)
    with np.errstate(all="ignore"):
        T, cl_in = refract(D, N, f32(1) / ior)
        P = (N * f32(-0.00001) + new_org).astype(np.float32)
        t1 = far_root(P, T, tab)
        rule = np.where((rule == 4) & ~(t1 > 0), 3, rule)
        Q = (P + T * t1[:, None]).astype(np.float32)
        M = normalise((Q - tab[:, :3]).astype(np.float32))
        U, cl_out = refract(T, -M, ior)
        Oout = (M * f32(0.00001) + Q).astype(np.float32)
    through = rule == 4
    ro = np.where(through[:, None], Oout, start).astype(np.float32)
    rd = np.where(through[:, None], U, D).astype(np.float32)
    nan = np.full((m, 3), np.nan, dtype=np.float32)
    return (ro, rd, rule, (cl_in | cl_out) & through, np.where(through[:, None], P, nan),
            np.where(through[:, None], T, nan), np.where(through, t1, np.nan).astype(np.float32))


# ----------------------------------------------------------------------------- the glass composer
class GlassComposer(Composer):
    def render(self, W, H, k, depth, y0=0, y1=None, tau=None, ior=None):
        """rgba [rows, W, 4] and packed [rows, W] of a frame with mirrors (k) and glass (tau, ior). self.trace[b] records
        bounce b: `pix` (band-local pixels), `index` (-1 = sky), `t`, `cos` = |D.N| for hits, and for glass hits that
        continue `rule` (1, 3, 4; 0 elsewhere), `clamp`, and the chord `P`, `T`, `t1` of the rays that entered."""
        y1 = H if y1 is None else y1
        self.trace = []
        O, D = self.primary(W, H, y0, y1)
        m = O.shape[0]
        c = np.zeros((m, 3), dtype=np.float32)
        w = np.ones(m, dtype=np.float32)
        first = np.ones(m, dtype=bool)
        live = np.arange(m)
        k = np.asarray(k, dtype=np.float32)
        tau = np.zeros(self.n, dtype=np.float32) if tau is None else np.asarray(tau, dtype=np.float32)
        ior = np.zeros(self.n, dtype=np.float32) if ior is None else np.asarray(ior, dtype=np.float32)
        for b in range(depth + 1):
            if live.size == 0:
                break
            Ob, Db, wb = O[live], D[live], w[live]
            idx, t = nearest(Ob, Db, self.tab)
            term = np.zeros((live.size, 3), dtype=np.float32)
            hit = idx >= 0
            go = np.zeros(live.size, dtype=bool)
            cos = np.full(live.size, np.nan, dtype=np.float32)
            rule = np.zeros(live.size, dtype=np.int64)
            clamp = np.zeros(live.size, dtype=bool)
            Pc = np.full((live.size, 3), np.nan, dtype=np.float32)
            Tc = np.full((live.size, 3), np.nan, dtype=np.float32)
            t1c = np.full(live.size, np.nan, dtype=np.float32)
            if (~hit).any():
                term[~hit] = wb[~hit, None] * self.sky_color(Ob[~hit], Db[~hit])
            if hit.any():
                hi = np.nonzero(hit)[0]
                N, start, L = self.shade(Ob[hi], Db[hi], idx[hi], t[hi])
                with np.errstate(all="ignore"):
                    new_org = (Ob[hi] + Db[hi] * t[hi][:, None]).astype(np.float32)
                cos[hi] = np.abs((Db[hi] * N).sum(axis=1))
                kk, tt = k[idx[hi]], tau[idx[hi]]
                stop = ((kk == 0) & (tt == 0)) | (b == depth)
                mm = np.where(tt > 0, tt, kk).astype(np.float32)
                fac = np.where(stop, wb[hi], wb[hi] * (f32(1) - mm)).astype(np.float32)
                term[hi] = fac[:, None] * L
                glass = ~stop & (tt > 0)
                mirror = ~stop & ~(tt > 0)
                if mirror.any():
                    sel = hi[mirror]
                    O[live[sel]] = start[mirror]
                    D[live[sel]] = reflect(Db[sel], N[mirror])
                if glass.any():
                    sel = hi[glass]
                    ro, rd, ru, cl, P, T, t1 = transmit(Db[sel], N[glass], start[glass], new_org[glass],
                                                        self.tab[idx[sel]], ior[idx[sel]])
                    O[live[sel]] = ro
                    D[live[sel]] = rd
                    rule[sel], clamp[sel], Pc[sel], Tc[sel], t1c[sel] = ru, cl, P, T, t1
                cont = hi[~stop]
                go[cont] = True
                w[live[cont]] = wb[cont] * mm[~stop]
            self.trace.append({"index": idx, "t": t, "cos": cos, "rule": rule, "clamp": clamp, "P": Pc, "T": Tc,
                               "t1": t1c, "pix": live.copy()})
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


def glass_composer_for(oracle, rt, inp):
    return GlassComposer(oracle, rt, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights,
                         inp.cam, inp.aspect)


# ----------------------------------------------------------------------------- helpers
def _vec3s(rt, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    arr = (rt.Vec3 * a.shape[0])()
    np.frombuffer(arr, dtype=np.float32).reshape(-1, 3)[:] = a
    return arr


def _dev_refract(rt, I, N, eta):
    lib = rt.load_library()
    m = I.shape[0]
    out = (rt.Vec3 * m)()
    eta = np.ascontiguousarray(np.broadcast_to(np.asarray(eta, dtype=np.float32), (m,)))
    assert lib.rt_debug_refract(_vec3s(rt, I), _vec3s(rt, N), eta.ctypes.data_as(C.POINTER(C.c_float)), m, out) == 0
    return np.frombuffer(out, dtype=np.float32).reshape(m, 3).copy()


def _one_sphere(rt, c, R):
    """An rt_sphere whose EFFECTIVE radius is R: intersect() squares the radius field (pack_list: w = field^2)."""
    s = rt.Sphere()
    s.orgin.x, s.orgin.y, s.orgin.z = (float(v) for v in c)
    s.radius = float(R)
    return s


def _dev_transmit(rt, sph, O, D, ior):
    lib = rt.load_library()
    m = O.shape[0]
    rays = (rt.Ray * m)()
    buf = np.frombuffer(rays, dtype=np.float32).reshape(m, 6)
    buf[:, :3], buf[:, 3:] = O, D
    out = (rt.Ray * m)()
    ent = np.zeros(m, dtype=np.int32)
    ior = np.ascontiguousarray(np.broadcast_to(np.asarray(ior, dtype=np.float32), (m,)))
    assert lib.rt_debug_transmit(C.byref(sph), ior.ctypes.data_as(C.POINTER(C.c_float)), rays, m, out,
                                 ent.ctypes.data_as(C.POINTER(C.c_int))) == 0
    ob = np.frombuffer(out, dtype=np.float32).reshape(m, 6).copy()
    return ob[:, :3], ob[:, 3:], ent


def _rand_unit(rng, m):
    v = rng.standard_normal((m, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ----------------------------------------------------------------------------- tests
def test_layouts_and_validation(rt):
    assert C.sizeof(rt.MaterialEx) == 16
    assert rt.MaterialEx.reflectivness.offset == 0 and rt.MaterialEx.transperancy.offset == 4
    assert rt.MaterialEx.roughness.offset == 8 and rt.MaterialEx.ior.offset == 12
    assert C.sizeof(rt.Material) == 12                        # the old material does not grow
    lib = rt.load_library()
    s = lib.rt_scene_create()                                  # host only: no sphere list yet (count 0)
    try:
        m = (rt.MaterialEx * 2)()
        assert lib.rt_scene_set_materials_ex(s, m, 2) == 1     # RT_ERR_INVALID: 2 materials for 0 spheres
        assert lib.rt_scene_set_materials_ex(s, None, 0) == 0  # clearing is always fine
        assert lib.rt_scene_set_materials_ex(s, m, 0) == 0
    finally:
        lib.rt_scene_destroy(s)


def _refract_cases(rng):
    """>= 100 000 (I, N, eta): random, grazing incidence (some exactly tangent), normal incidence, eta = 1, eta > 1
    past the critical angle (the radicand clamps), and the glass etas 1/ior and ior."""
    m = 30000
    N = normalise(_rand_unit(rng, m).astype(np.float32))
    I_rand = normalise(_rand_unit(rng, m).astype(np.float32))
    I_rand = np.where((dot_rows(I_rand, N) > 0)[:, None], -I_rand, I_rand).astype(np.float32)   # N faces against I
    # grazing: I nearly perpendicular to N
    perp = np.cross(N.astype(np.float64), _rand_unit(rng, m))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    tilt = rng.choice([0.0, 1e-7, 1e-5, 1e-3, 1e-2], m)
    I_graze = normalise((perp - N.astype(np.float64) * tilt[:, None]).astype(np.float32))
    I_norm = (-N).astype(np.float32)                                                 # normal incidence
    etas = rng.choice(np.array([1 / 1.33, 1 / 1.5, 1 / 2.4, 1.0, 1.33, 1.5, 2.4, 1 / 4.0, 4.0], dtype=np.float32), m)
    eta_u = rng.uniform(0.25, 4.0, m).astype(np.float32)
    I = np.concatenate([I_rand, I_graze, I_norm, I_rand]).astype(np.float32)
    NN = np.concatenate([N, N, N, N]).astype(np.float32)
    eta = np.concatenate([etas, etas, etas, eta_u]).astype(np.float32)
    return I, NN, eta


def test_refract_bit_for_bit(rt):
    rng = np.random.default_rng(21)
    I, N, eta = _refract_cases(rng)
    assert I.shape[0] >= 100000
    got = _dev_refract(rt, I, N, eta)
    want, clamped = refract(I, N, eta)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert clamped.sum() > 1000 and (~clamped).sum() > 50000                # both branches are exercised
    # known answers: normal incidence passes straight on, eta = 1 leaves any direction unchanged up to rounding
    V = np.array([[0.0, 0.0, 1.0]], dtype=np.float32)
    n = np.array([[0.0, 0.0, -1.0]], dtype=np.float32)
    assert np.array_equal(_dev_refract(rt, V, n, 1 / 1.5), V)
    sel = (eta == 1.0) & ~clamped
    assert np.abs(got[sel] - I[sel]).max() < 1e-3 and np.abs(got[sel] - I[sel])[dot_rows(I[sel], N[sel]) < -0.1].max() < 1e-6


def test_refract_physics(rt):
    """Snell's law, unit length, and the plane of I and N, in float64 from the binary32 results."""
    rng = np.random.default_rng(22)
    m = 50000
    N = normalise(_rand_unit(rng, m).astype(np.float32))
    I = normalise(_rand_unit(rng, m).astype(np.float32))
    I = np.where((dot_rows(I, N) > 0)[:, None], -I, I).astype(np.float32)
    eta = rng.choice(np.array([1 / 1.33, 1 / 1.5, 1 / 2.4, 1 / 4.0, 1.0, 1.33, 1.5, 2.4], dtype=np.float32), m)
    T = _dev_refract(rt, I, N, eta).astype(np.float64)
    I64, N64 = I.astype(np.float64), N.astype(np.float64)
    I64 /= np.linalg.norm(I64, axis=1, keepdims=True)
    N64 /= np.linalg.norm(N64, axis=1, keepdims=True)
    sin_i = np.linalg.norm(np.cross(I64, N64), axis=1)
    ok = eta.astype(np.float64) * sin_i < 0.999                              # no total internal reflection
    assert ok.sum() > 30000
    T, I64, N64, sin_i, e = T[ok], I64[ok], N64[ok], sin_i[ok], eta[ok].astype(np.float64)
    assert np.abs(np.linalg.norm(T, axis=1) - 1.0).max() < 1e-5
    sin_t = np.linalg.norm(np.cross(T, N64), axis=1) / np.linalg.norm(T, axis=1)
    assert np.abs(sin_t - e * sin_i).max() < 1e-5
    plane = np.cross(I64, N64)
    big = np.linalg.norm(plane, axis=1) > 1e-3
    plane = plane[big] / np.linalg.norm(plane[big], axis=1, keepdims=True)
    assert np.abs((T[big] * plane).sum(axis=1)).max() < 1e-5
    assert (np.einsum("ij,ij->i", T, -N64) > 0).all()                        # it goes on through the surface


def _transmit_rays(rng, c, R, m, sin_max=0.99, dmax=300.0):
    """Rays from up to dmax units away that hit the sphere (c, R) with sin(theta_i) < sin_max: -> O, D (binary32) and the
    aimed impact parameter b / R."""
    dist = rng.uniform(2.0 * R + 0.1, dmax, m)
    u = _rand_unit(rng, m)
    O = c[None, :] + u * dist[:, None]
    a = _rand_unit(rng, m)
    a -= u * (a * u).sum(axis=1, keepdims=True)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    bR = rng.uniform(0.0, sin_max, m)
    target = c[None, :] + a * (bR * R)[:, None]
    D = target - O
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    return O.astype(np.float32), normalise(D.astype(np.float32)), bR


def _f64_path(O, D, c, R, ior, X1):
    """The glass step in float64 from the binary32 hit point X1 (the same 1e-5 offsets the rules define):
    -> exit point Q, outgoing direction U, theta_i, theta_t."""
    n1 = X1 - c
    n1 /= np.linalg.norm(n1, axis=1, keepdims=True)
    Dd = D / np.linalg.norm(D, axis=1, keepdims=True)
    ci = -(Dd * n1).sum(axis=1)
    eta = 1.0 / ior
    T = Dd * eta + n1 * (eta * ci - np.sqrt(1 - eta * eta * (1 - ci * ci)))[:, None]
    P = X1 - n1 * 1e-5
    oc = P - c
    h = (T * oc).sum(axis=1)
    t1 = -h + np.sqrt(h * h - ((oc * oc).sum(axis=1) - R * R))
    Q = P + T * t1[:, None]
    M = (Q - c) / np.linalg.norm(Q - c, axis=1, keepdims=True)
    c2 = (T * M).sum(axis=1)
    U = T * ior + (-M) * (ior * c2 - np.sqrt(np.maximum(1 - ior * ior * (1 - c2 * c2), 0)))[:, None]
    th_i = np.arccos(np.clip(ci, -1, 1))
    th_t = np.arcsin(np.clip(eta * np.sin(th_i), -1, 1))
    return Q, U, th_i, th_t


@pytest.mark.parametrize("R", [1e-2, 0.1, 1.0, 10.0])
def test_transmit_against_float64(rt, R):
    """Rays from up to 300 units away, and at most 30 R: beyond that intersect()'s binary32 discriminant (B^2 - 4AC with
    |B^2| ~ 4 d^2) no longer places the hit point within 1e-4 R of the surface, which float64 physics would need."""
    rng = np.random.default_rng(int(R * 1000) + 3)
    c = rng.uniform(-1, 1, 3)
    sph = _one_sphere(rt, c, R)
    tab = sphere_table((sph,), 1)
    cf = tab[0, :3].astype(np.float64)
    Reff = float(np.sqrt(np.float64(tab[0, 3])))
    m = 4000
    O, D, bR = _transmit_rays(rng, cf, Reff, m, dmax=min(300.0, 30.0 * Reff))
    for ior in (1.0, 1.33, 1.5, 2.4):
        ro, rd, ent = _dev_transmit(rt, sph, O, D, ior)
        # the restatement of the rules, bit for bit (from intersect()'s hit)
        idx, t = nearest(O, D, tab)
        hit = idx >= 0
        assert hit.mean() > 0.99
        assert (ent[~hit] == -1).all()
        Oh, Dh, th = O[hit], D[hit], t[hit]
        new_org = (Oh + Dh * th[:, None]).astype(np.float32)
        N = normalise((new_org - tab[0, :3]).astype(np.float32))
        start = (N * f32(0.00001) + new_org).astype(np.float32)
        wo, wd, rule, _, _, _, _ = transmit(Dh, N, start, new_org, np.repeat(tab, hit.sum(), 0), ior)
        assert np.array_equal(ro[hit].view(np.uint32), wo.view(np.uint32))
        assert np.array_equal(rd[hit].view(np.uint32), wd.view(np.uint32))
        assert np.array_equal(ent[hit], (rule == 4).astype(np.int32))
        assert (rule == 4).all()                                  # sin(theta_i) < 0.99 and R >= 1e-2: every ray passes
        # float64 physics of the same step
        Q, U, th_i, th_t = _f64_path(Oh.astype(np.float64), Dh.astype(np.float64), cf, Reff, ior,
                                     new_org.astype(np.float64))
        got = rd[hit].astype(np.float64)
        assert np.abs(got - U).max() < 1e-4, (R, ior)
        # the exit point is on the sphere (the outgoing origin is 1e-5 outside it)
        dist = np.linalg.norm(ro[hit].astype(np.float64) - cf, axis=1) - Reff
        assert np.abs(dist - 1e-5).max() < 1e-5 + 2e-6 * Reff, (R, ior)
        # the deviation is 2 (theta_i - theta_t), up to what the 1e-5 offsets and the binary32 hit point's distance
        # from the surface (delta) move: a few (1e-5 + delta) / R
        D64 = Dh.astype(np.float64)
        dev = np.arctan2(np.linalg.norm(np.cross(got, D64), axis=1), (got * D64).sum(axis=1))
        delta = np.abs(np.linalg.norm(new_org.astype(np.float64) - cf, axis=1) - Reff)
        assert (np.abs(dev - 2 * (th_i - th_t)) < 1e-6 + 8 * (1e-5 + delta) / Reff).all(), (R, ior)
        if ior == 1.0:                                           # no refraction: the incoming direction
            assert np.abs(got - Dh).max() < 1e-5


def test_transmit_through_the_centre(rt):
    sph = _one_sphere(rt, (0.5, -1.0, 2.0), 1.0)
    c = np.array([0.5, -1.0, 2.0])
    rng = np.random.default_rng(4)
    u = _rand_unit(rng, 2000)
    O = (c + u * rng.uniform(3, 300, (2000, 1))).astype(np.float32)
    D = normalise((c - O).astype(np.float32))
    for ior in (1.33, 1.5, 2.4, 4.0):
        _, rd, ent = _dev_transmit(rt, sph, O, D, ior)
        assert (ent == 1).all()
        assert np.abs(rd - D).max() < 1e-4


def test_transmit_rules_1_and_3(rt):
    """A ray whose hit has dot(D, N) >= 0 (t == 0 on the far side) and a degenerate tiny sphere leave undeviated."""
    # rule 3: spheres of radius 1e-6 .. 4e-6 -- P = new_org - 1e-5 N lies beyond them, the far root is negative
    rng = np.random.default_rng(9)
    n3 = 0
    for R in (1e-6, 2e-6, 4e-6):
        sph = _one_sphere(rt, (0.0, 0.0, 0.0), R)
        tab = sphere_table((sph,), 1)
        D = normalise(np.c_[rng.uniform(-R, R, (4000, 2)), np.full(4000, 1e-4)].astype(np.float32))
        O = np.tile(np.array([0.0, 0.0, -1e-4], dtype=np.float32), (4000, 1))
        ro, rd, ent = _dev_transmit(rt, sph, O, D, 1.5)
        idx, t = nearest(O, D, tab)
        hit = idx >= 0
        new_org = (O[hit] + D[hit] * t[hit][:, None]).astype(np.float32)
        N = normalise((new_org - tab[0, :3]).astype(np.float32))
        start = (N * f32(0.00001) + new_org).astype(np.float32)
        _, _, rule, _, _, _, _ = transmit(D[hit], N, start, new_org, np.repeat(tab, hit.sum(), 0), 1.5)
        r3 = rule == 3
        n3 += r3.sum()
        assert (ent[hit][r3] == 0).all() and np.array_equal(rd[hit][r3], D[hit][r3])
        assert np.array_equal(ro[hit][r3], start[r3])
    assert n3 > 1000
    # rule 1: intersect()'s `t == 0` case returns the far root -- the origin on the far surface, looking out
    sph = _one_sphere(rt, (0.0, 0.0, 0.0), 1.0)
    O = np.array([[0, 0, 1]], dtype=np.float32)
    D = np.array([[0, 0, 1]], dtype=np.float32)
    ro, rd, ent = _dev_transmit(rt, sph, O, D, 1.5)
    assert ent[0] == 0 and np.array_equal(rd, D)
    assert np.array_equal(ro, np.array([[0, 0, f32(f32(1) * f32(0.00001) + f32(1))]], dtype=np.float32))


def test_glass_composer_without_glass_is_the_mirror_composer(oracle, rt):
    from scenes import Inputs
    inp = Inputs(rt, 256)
    k = np.array([(0.0, 0.25, 0.5, 1.0)[i % 4] for i in range(256)], dtype=np.float32)
    W, H = 160, 90
    a = composer_for(oracle, rt, inp).render(W, H, k, 3)
    b = glass_composer_for(oracle, rt, inp).render(W, H, k, 3, tau=np.zeros(256), ior=np.full(256, 1.5))
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1], b[1])
