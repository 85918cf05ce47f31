"""Glossy reflections (rt_scene_set_roughness): a numpy restatement of the draws and of rf_gloss, and the
composed reference of glossy frames.

Nothing here traces a ray of its own. A glossy frame is a frame of one of the composers the repository already trusts --
Composer (tests/test_reflect_cpu.py), GlassComposer (tests/test_refract_cpu.py), SceneComposer
(tests/reflect_scene_ref.py) -- in which the reflect(...) of a continuing mirror hit is replaced by the glossy
continuation. The composers call reflect(D[rows], N[rows]) from inside their bounce loop; for the length of a render the
subclasses below put `_GlossState.reflect` in its place, which computes reflect() itself and then reads from the calling
loop what reflect()'s arguments do not carry: the bounce b, the band-local pixels of the rows, the primitives they hit
and the band's first row. SampleRef (tests/reflect_samples_ref.py) wraps them for spp > 1 as it wraps the others;
GlossSampleRef hands the absolute sample index to the key.

Beside the frame every render leaves `gloss_trace`: per call of the replacement {"b", "pix", "rho", "what"} with what =
rf_gloss's result per row (0 nothing drawn; 1 perturbed; | 2 the halved fourth draw; | 4 R' rejected)."""
import sys

import numpy as np

import test_reflect_cpu as _mirror
from reflect_samples_ref import SampleRef
from reflect_scene_ref import CUBE, PLANE, SPHERE, SceneComposer
from test_refract_cpu import GlassComposer

f32 = np.float32
u32 = np.uint32
_reflect = _mirror.reflect       # the mirror direction itself (the name in the composers' modules is what gets replaced)
PERTURBED, HALVED, REJECTED = 1, 2, 4


# ----------------------------------------------------------------------------- the restatement
def mix(x):
    x = np.array(x, dtype=np.uint32, copy=True, ndmin=1)
    x ^= x >> u32(16)
    x *= u32(0x7feb352d)
    x ^= x >> u32(15)
    x *= u32(0x846ca68b)
    x ^= x >> u32(16)
    return x


def _u32(v, m=None):
    a = np.asarray(v).astype(np.int64) & 0xffffffff
    a = a.astype(np.uint32).reshape(-1)
    return a if m is None else np.broadcast_to(a, (m,)).copy()


def key(px, py, s, seed):
    px = _u32(px)
    m = px.shape[0]
    return mix(mix(mix(mix(_u32(seed, m)) ^ _u32(s, m)) ^ _u32(py, m)) ^ px)


def draw(k, b, t):
    """[m, 3] float32 in [-1, 1): draw t of hit b under the keys k."""
    k = _u32(k)
    b = _u32(b, k.shape[0])
    out = np.empty((k.shape[0], 3), dtype=np.float32)
    for a in range(3):
        c = (b * u32(4) + u32(t)) * u32(3) + u32(a + 1)
        h = mix(k + u32(0x9e3779b9) * c)
        out[:, a] = (h >> u32(8)).astype(np.float32) * f32(2.0 ** -23) - f32(1)
    return out


def ball(k, b):
    """u [m, 3] of rf_gloss and whether the halved fourth draw was taken."""
    k = _u32(k)
    u = np.zeros((k.shape[0], 3), dtype=np.float32)
    found = np.zeros(k.shape[0], dtype=bool)
    for t in range(4):
        d = draw(k, b, t)
        ok = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) <= f32(1)
        take = ok & ~found
        u[take] = d[take]
        found |= ok
    u[~found] = d[~found] * f32(0.5)
    return u, ~found


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def gloss(R, N, rho, k, b):
    """rf_gloss for rows: -> the continuation [m, 3] and `what` [m]."""
    R = np.asarray(R, dtype=np.float32)
    N = np.asarray(N, dtype=np.float32)
    rho = np.asarray(rho, dtype=np.float32).reshape(-1)
    u, halved = ball(k, b)
    with np.errstate(all="ignore"):
        G = (R + rho[:, None] * u).astype(np.float32)
        l = np.sqrt((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2])
        nz = l != 0
        Rp = np.where(nz[:, None], G / np.where(nz, l, f32(1))[:, None], G).astype(np.float32)
        ok = (_dot(Rp, N) * _dot(R, N)) > 0
    drawn = ~(rho == 0)
    out = np.where((drawn & ok)[:, None], Rp, R).astype(np.float32)
    what = np.where(drawn, PERTURBED | np.where(halved, HALVED, 0) | np.where(ok, 0, REJECTED), 0)
    return out, what.astype(np.int64)


# ----------------------------------------------------------------------------- the composed reference
class _GlossState:
    """What the replacement of reflect() needs beside its arguments: the tables, the seed and the sample index."""

    def set_gloss(self, sphere=None, plane=None, cube=None, seed=0):
        tab = lambda v: None if v is None else np.asarray(v, dtype=np.float32)
        self.gloss_rough = {SPHERE: tab(sphere), PLANE: tab(plane), CUBE: tab(cube)}
        self.gloss_seed = seed
        return self

    gloss_rough = {SPHERE: None, PLANE: None, CUBE: None}
    gloss_seed = 0
    gloss_s = 0                  # the absolute sample index (GlossSampleRef sets it per sample)
    gloss_rows = "sel"           # the caller's name for the rows it passes to reflect()

    def _rho(self, loc, rows):
        if "kind" in loc:        # SceneComposer: kind and index per live ray
            kind, index = loc["kind"][rows], loc["index"][rows]
        else:
            kind, index = np.full(rows.shape[0], SPHERE), loc["idx"][rows]
        rho = np.zeros(rows.shape[0], dtype=np.float32)
        for code, tab in self.gloss_rough.items():
            sel = kind == code
            if tab is not None and sel.any():
                rho[sel] = tab[index[sel]]
        return rho

    def reflect(self, I, N):
        R = _reflect(I, N)
        loc = sys._getframe(1).f_locals          # the composer's bounce loop
        rows = loc[self.gloss_rows]
        assert rows.shape[0] == R.shape[0]
        pix = loc["live"][rows]
        W, y0, b = loc["W"], loc["y0"], loc["b"]
        rho = self._rho(loc, rows)
        k = key(pix % W, y0 + pix // W, self.gloss_s, self.gloss_seed)
        out, what = gloss(R, N, rho, k, b)
        self.gloss_trace.append({"b": b, "pix": pix.copy(), "rho": rho, "what": what})
        return out

    def _with_gloss(self, fn, *a, **kw):
        g = fn.__globals__
        saved = g["reflect"]
        self.gloss_trace = []
        g["reflect"] = self.reflect
        try:
            return fn(self, *a, **kw)
        finally:
            g["reflect"] = saved


class GlossComposer(_GlossState, _mirror.Composer):
    gloss_rows = "cont"

    def render(self, *a, **kw):
        return self._with_gloss(_mirror.Composer.render, *a, **kw)


class GlossGlassComposer(_GlossState, GlassComposer):
    def render(self, *a, **kw):
        return self._with_gloss(GlassComposer.render, *a, **kw)


class GlossSceneComposer(_GlossState, SceneComposer):
    def render_depths(self, *a, **kw):
        return self._with_gloss(SceneComposer.render_depths, *a, **kw)


def gloss_composer_for(oracle, rt, inp, glass=False):
    cls = GlossGlassComposer if glass else GlossComposer
    return cls(oracle, rt, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam, inp.aspect)


class GlossSampleRef(SampleRef):
    """SampleRef over a gloss composer: sample k's frame is drawn under s = k; each sample keeps its gloss trace."""

    def render(self, W, H, depth, *, base=0, **kw):
        self._next = base
        return super().render(W, H, depth, base=base, **kw)

    def _one(self, *a, **kw):
        self.comp.gloss_s = self._next
        self._next += 1
        try:
            one = super()._one(*a, **kw)
        finally:
            self.comp.gloss_s = 0
        one["gloss"] = self.comp.gloss_trace
        return one


# ----------------------------------------------------------------------------- reading a gloss trace
def count(trace, bit=PERTURBED):
    return int(sum(((t["what"] & bit) != 0).sum() for t in trace))


def perturbed_pixels(trace, m):
    """[m] bool: the band-local pixels with at least one perturbed continuation."""
    out = np.zeros(m, dtype=bool)
    for t in trace:
        out[t["pix"][(t["what"] & PERTURBED) != 0]] = True
    return out
