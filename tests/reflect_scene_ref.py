"""The composed reference of reflective frames over the whole scene (rt_scene_set_reflect_scope(RT_REFLECT_SCENE),
DESIGN.md 6g).

The loop is Composer.render's (tests/test_reflect_cpu.py); per bounce, query_ref.CastRef.shade gives castRay's nearest
hit over every kind of primitive, its hit record and L (or the sky texel); continuations use reflect() for mirrors and
transmit() (tests/test_refract_cpu.py) at glass spheres. Beside the frame it keeps a trace per bounce -- kind, index and
t of what each ray met, the rays themselves -- and, per shaded hit, whether some shadow sample was blocked by a
non-sphere while no sphere blocked it."""
import numpy as np

import query_ref as Q
from test_reflect_cpu import composer_for, intersect, reflect
from test_refract_cpu import transmit

f32 = np.float32
TRIANGLE, SPHERE, PLANE, CUBE = 0, 1, 2, 3


class _Cast(Q.CastRef):
    """CastRef that also notes, per shaded hit, a shadow sample only a non-sphere blocks."""

    def occluded(self, O, D):
        occ = super().occluded(O, D)
        sph = np.zeros(O.shape[0], dtype=bool)
        for c0 in range(0, self.n, 256):
            sph |= intersect(O, D, self.tab[c0:c0 + 256])[0].any(axis=1)
        self.last_nonsphere = (occ != 0) & ~sph
        return occ


class SceneComposer:
    def __init__(self, oracle, rt, inp, mesh_text=None):
        self.cast = _Cast(oracle, inp, mesh_text)
        self.prim = composer_for(oracle, rt, inp)      # the primary rays and the pack
        self.lib = oracle.load()
        self.n = self.cast.n
        self.n_planes, self.n_cubes = len(self.cast.planes), len(self.cast.cubes)

    def _pack(self, c):
        return np.array([self.lib.oracle_pack_color(float(x[0]), float(x[1]), float(x[2])) for x in c], dtype=np.uint32)

    def render_depths(self, W, H, depths, k_sphere=None, k_plane=None, k_cube=None, tau=None, ior=None, y0=0, y1=None):
        """{depth: (rgba [rows, W, 4], packed [rows, W], queue)} for every depth asked for, from one walk to the
        largest: a frame of depth d is the walk's colour before bounce d plus w * L (or w * sky) for every ray still
        live there. queue[b] = rays entering bounce b + 1 (rt_reflect_stats.queue, d entries). self.trace[b] records
        bounce b of the walk: `pix`, `O`, `D`, `kind` (-1 sky, 0 triangle, 1 sphere, 2 plane, 3 cube), `index`, `t`,
        `hp` (the hit point), `shadow_nonsphere` (a shadow sample of the hit blocked by a non-sphere and by no sphere),
        `rule` (transmit's rule at glass hits that continue, else 0)."""
        y1 = H if y1 is None else y1
        zeros = lambda n: np.zeros(n, dtype=np.float32)
        ks = zeros(self.n) if k_sphere is None else np.asarray(k_sphere, dtype=np.float32)
        kp = zeros(self.n_planes) if k_plane is None else np.asarray(k_plane, dtype=np.float32)
        kc = zeros(self.n_cubes) if k_cube is None else np.asarray(k_cube, dtype=np.float32)
        tau = zeros(self.n) if tau is None else np.asarray(tau, dtype=np.float32)
        ior = zeros(self.n) if ior is None else np.asarray(ior, dtype=np.float32)
        assert ks.shape == (self.n,) and kp.shape == (self.n_planes,) and kc.shape == (self.n_cubes,)
        depths = sorted(set(depths))
        top = depths[-1]
        self.trace = []
        O, D = self.prim.primary(W, H, y0, y1)
        m = O.shape[0]
        c = np.zeros((m, 3), dtype=np.float32)
        w = np.ones(m, dtype=np.float32)
        first = np.ones(m, dtype=bool)
        live = np.arange(m)
        frames, sizes = {}, []
        for b in range(top + 1):
            if live.size == 0:
                break
            if b > 0:
                sizes.append(live.size)
            Ob, Db, wb = O[live].copy(), D[live].copy(), w[live]
            shaded, _, rec = self.cast.shade(Ob, Db)
            L = shaded[:, :3]
            kind, index, t = rec["kind"], rec["index"], rec["t"]
            hit = kind >= 0
            hi = np.nonzero(hit)[0]
            nons = np.zeros(live.size, dtype=bool)
            if hi.size:
                nons[hi] = self.cast.last_nonsphere.reshape(hi.size, -1).any(axis=1)
            fl = first[live]
            if b in depths:          # depth b: every live ray ends here with w * L (a hit) or w * sky (a miss)
                fc = c.copy()
                end = (wb[:, None] * L).astype(np.float32)
                fc[live[fl]] = end[fl]
                fc[live[~fl]] = fc[live[~fl]] + end[~fl]
                frames[b] = fc
            # the walk goes on as a deeper frame does
            term = np.zeros((live.size, 3), dtype=np.float32)
            term[~hit] = wb[~hit, None] * L[~hit]
            go = np.zeros(live.size, dtype=bool)
            rule = np.zeros(live.size, dtype=np.int64)
            if hi.size:
                N, new_org = rec["normal"][hi], rec["new_org"][hi]
                start = (N * f32(0.00001) + new_org).astype(np.float32)
                kk, tt, io = zeros(hi.size), zeros(hi.size), zeros(hi.size)
                for code, tab in ((SPHERE, ks), (PLANE, kp), (CUBE, kc)):
                    sel = kind[hi] == code
                    kk[sel] = tab[index[hi][sel]]
                sph = kind[hi] == SPHERE
                tt[sph], io[sph] = tau[index[hi][sph]], ior[index[hi][sph]]
                stop = (kk == 0) & (tt == 0)
                mm = np.where(tt > 0, tt, kk).astype(np.float32)
                fac = np.where(stop, wb[hi], wb[hi] * (f32(1) - mm)).astype(np.float32)
                term[hi] = fac[:, None] * L[hi]
                glass = ~stop & (tt > 0)
                mirror = ~stop & ~(tt > 0)
                if mirror.any():
                    sel = hi[mirror]
                    O[live[sel]] = start[mirror]
                    D[live[sel]] = reflect(Db[sel], N[mirror])
                if glass.any():
                    sel = hi[glass]
                    ro, rd, ru = transmit(Db[sel], N[glass], start[glass], new_org[glass],
                                          self.cast.tab[index[sel]], io[glass])[:3]
                    O[live[sel]], D[live[sel]], rule[sel] = ro, rd, ru
                cont = hi[~stop]
                go[cont] = True
                w[live[cont]] = wb[cont] * mm[~stop]
            with np.errstate(all="ignore"):
                hp = (Ob + Db * t[:, None]).astype(np.float32)
            self.trace.append({"pix": live.copy(), "O": Ob, "D": Db, "kind": kind.copy(), "index": index.copy(),
                               "t": t.copy(), "hp": hp, "shadow_nonsphere": nons, "rule": rule})
            c[live[fl]] = term[fl]
            c[live[~fl]] = c[live[~fl]] + term[~fl]
            first[live] = False
            live = live[go]
        rows = y1 - y0
        out = {}
        for d in depths:
            fc = frames.get(d, c)    # the walk ran dry before bounce d: the frame is what it had
            rgba = np.ones((m, 4), dtype=np.float32)
            rgba[:, :3] = fc
            queue = (sizes + [0] * d)[:d]
            out[d] = (rgba.reshape(rows, W, 4), self._pack(fc).reshape(rows, W), queue)
        return out

    def render(self, W, H, depth, **kw):
        """rgba, packed, queue of the frame with reflect_depth = depth."""
        return self.render_depths(W, H, (depth,), **kw)[depth]


def met(trace, b, kind, index=None):
    """Rays of bounce b that met `kind` (and `index`)."""
    if b >= len(trace):
        return np.zeros(0, dtype=bool)
    sel = trace[b]["kind"] == kind
    return sel if index is None else sel & (trace[b]["index"] == index)


def chain(trace, steps, start=0):
    """Pixels whose bounces start, start + 1, ... met steps[0], steps[1], ...; a step is a kind or (kind, index).
    -> the pixel array."""
    pix = None
    for j, st in enumerate(steps):
        kind, index = st if isinstance(st, tuple) else (st, None)
        sel = met(trace, start + j, kind, index)
        here = trace[start + j]["pix"][sel] if start + j < len(trace) else np.zeros(0, dtype=np.int64)
        pix = here if pix is None else np.intersect1d(pix, here)
    return pix


def runs(trace, steps):
    """How many rays met steps[0], then steps[1], ... on consecutive bounces, from any bounce on."""
    return sum(chain(trace, steps, start).size for start in range(len(trace)))
