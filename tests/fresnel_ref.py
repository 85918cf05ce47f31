"""Fresnel glass (rt_scene_set_glass_model(RT_GLASS_FRESNEL)): a numpy binary32 restatement of the
reflectance, the draw and the choice, and the composed reference of frames under that model.

Nothing here traces a ray of its own. A frame under the Fresnel model is a frame of GlossGlassComposer or
GlossSceneComposer (tests/gloss_ref.py) in which the transmit(...) of a continuing glass hit is replaced by the choice
between the mirror ray and the ray through the sphere -- the way _GlossState._with_gloss replaces reflect(...). The
replacement computes the plain glass step with the transmit() of tests/test_refract_cpu.py and reads from the calling
loop what the arguments do not carry: the bounce b, the band-local pixels of the rows and the spheres they hit.

Beside the frame every render leaves `fresnel_trace`: per call of the replacement {"b", "pix", "rho", "F", "u",
"choice", "what"} with choice per row = RULE1 (nothing drawn), REFLECTED, THROUGH (rule 4) or RULE3, and what =
rf_gloss's result for the ray that was taken. SceneComposer walks one bounce past the frame's depth: the readers below
take the depth and ignore what lies beyond it.

force = "reflect" | "transmit" takes that branch at every glass hit that draws (F and u are recorded all the same)."""
import sys

import numpy as np

import gloss_ref as G
import test_refract_cpu as _glass
from reflect_scene_ref import SceneComposer
from test_reflect_cpu import normalise, reflect as _reflect
from test_refract_cpu import GlassComposer, dot_rows

f32 = np.float32
u32 = np.uint32
_transmit = _glass.transmit      # the plain glass step (the name in the composers' modules is what gets replaced)
RULE1, REFLECTED, THROUGH, RULE3 = 1, 2, 3, 4
PLAIN, FRESNEL = "plain", "fresnel"


# ----------------------------------------------------------------------------- the restatement
def fresnel(c, ior):
    """F(c, ior) in binary32, step by step as the header states it."""
    c = np.asarray(c, dtype=np.float32).reshape(-1)
    ior = np.broadcast_to(np.asarray(ior, dtype=np.float32), c.shape)
    with np.errstate(all="ignore"):
        eta = f32(1) / ior
        q = f32(1) - (eta * eta) * (f32(1) - c * c)
        ct = np.sqrt(np.where(q > 0, q, f32(0))).astype(np.float32)
        rs = (c - ior * ct) / (c + ior * ct)
        rp = (ct - ior * c) / (ct + ior * c)
        return ((rs * rs + rp * rp) * f32(0.5)).astype(np.float32)


def draw(k, b):
    """u [m] float32 in [0, 1): the draw of hit b under the keys k."""
    k = G._u32(k)
    b = G._u32(b, k.shape[0])
    h = G.mix(G.mix(k ^ u32(0x46726573)) + u32(0x9e3779b9) * (b + u32(1)))
    return (h >> u32(8)).astype(np.float32) * f32(2.0 ** -24)


def glass_choice(D, N, start, new_org, tab, ior, rho, k, b, force=None):
    """A glass hit under the Fresnel model, for rows: -> (ro, rd, choice, F, u, what) and the plain step's 7-tuple."""
    m = D.shape[0]
    ior = np.broadcast_to(np.asarray(ior, dtype=np.float32), (m,))
    rho = np.broadcast_to(np.asarray(rho, dtype=np.float32), (m,))
    k = G._u32(k, m) if np.ndim(k) == 0 else G._u32(k)
    b = G._u32(b, m)
    plain = _transmit(D, N, start, new_org, tab, ior)
    ro, rd, rule = plain[0].copy(), plain[1].copy(), plain[2]
    P, T, t1 = plain[4], plain[5], plain[6]
    with np.errstate(all="ignore"):
        dn = dot_rows(D, N)
    drawn = ~(dn >= 0)                                     # not rule 1 (a NaN draws, as in rf_transmit)
    F = np.where(drawn, fresnel(-dn, ior), f32(0)).astype(np.float32)
    u = np.where(drawn, draw(k, b), f32(0)).astype(np.float32)
    if force is None:
        refl = drawn & (u < F)                             # a NaN F fails
    else:
        assert force in ("reflect", "transmit")
        refl = drawn & (force == "reflect")
    choice = np.where(rule == 1, RULE1, np.where(rule == 3, RULE3, THROUGH))
    choice[refl] = REFLECTED
    what = np.zeros(m, dtype=np.int64)
    if refl.any():                                         # step 4: what a mirror hit on that sphere would do
        R = _reflect(D[refl], N[refl])
        ro[refl] = start[refl]
        rd[refl], what[refl] = G.gloss(R, N[refl], rho[refl], k[refl], b[refl])
    thr = choice == THROUGH
    if thr.any():                                          # step 5: the exit direction against the exit normal M
        with np.errstate(all="ignore"):
            Q = (P[thr] + T[thr] * t1[thr][:, None]).astype(np.float32)
            M = normalise((Q - tab[thr, :3]).astype(np.float32))
        rd[thr], what[thr] = G.gloss(rd[thr], M, rho[thr], k[thr], b[thr])
    return (ro, rd, choice, F, u, what), plain


# ----------------------------------------------------------------------------- the composed reference
class _FresnelState:
    """What the replacement of transmit() needs beside _GlossState's: the model and the forced branch."""
    glass_model = FRESNEL
    fresnel_force = None

    def set_glass_model(self, model=FRESNEL, force=None):
        assert model in (PLAIN, FRESNEL)
        self.glass_model, self.fresnel_force = model, force
        return self

    def transmit(self, D, N, start, new_org, tab, ior):
        loc = sys._getframe(1).f_locals                    # the composer's bounce loop
        rows = loc["sel"]
        assert rows.shape[0] == D.shape[0]
        pix = loc["live"][rows]
        W, y0, b = loc["W"], loc["y0"], loc["b"]
        rho = self._rho(loc, rows)
        k = G.key(pix % W, y0 + pix // W, self.gloss_s, self.gloss_seed)
        (ro, rd, choice, F, u, what), plain = glass_choice(D, N, start, new_org, tab, ior, rho, k, b, self.fresnel_force)
        self.fresnel_trace.append({"b": b, "pix": pix.copy(), "rho": rho, "F": F, "u": u, "choice": choice, "what": what})
        refl = choice == REFLECTED
        nan3 = np.full((1, 3), np.nan, dtype=np.float32)
        rule = np.where(refl, 2, plain[2])                 # the composers' `rule`: 2 = reflected off the glass
        return (ro, rd, rule, plain[3] & ~refl, np.where(refl[:, None], nan3, plain[4]),
                np.where(refl[:, None], nan3, plain[5]), np.where(refl, np.nan, plain[6]).astype(np.float32))

    def _with_fresnel(self, g, call):
        self.fresnel_trace = []
        if self.glass_model == PLAIN:
            return call()
        saved = g["transmit"]
        g["transmit"] = self.transmit
        try:
            return call()
        finally:
            g["transmit"] = saved


class FresnelGlassComposer(_FresnelState, G.GlossGlassComposer):
    def render(self, *a, **kw):
        return self._with_fresnel(GlassComposer.render.__globals__, lambda: G.GlossGlassComposer.render(self, *a, **kw))


class FresnelSceneComposer(_FresnelState, G.GlossSceneComposer):
    def render_depths(self, *a, **kw):
        return self._with_fresnel(SceneComposer.render_depths.__globals__,
                                  lambda: G.GlossSceneComposer.render_depths(self, *a, **kw))


def fresnel_composer_for(oracle, rt, inp):
    return FresnelGlassComposer(oracle, rt, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights,
                                inp.cam, inp.aspect)


class FresnelSampleRef(G.GlossSampleRef):
    """GlossSampleRef over a Fresnel composer: each sample keeps its Fresnel trace as well."""

    def _one(self, *a, **kw):
        one = super()._one(*a, **kw)
        one["fresnel"] = self.comp.fresnel_trace
        return one


# ----------------------------------------------------------------------------- reading a Fresnel trace
def _rows(trace, depth):
    return [t for t in trace if depth is None or t["b"] < depth]


def count(trace, choice, b=None, depth=None):
    return int(sum((t["choice"] == choice).sum() for t in _rows(trace, depth) if b is None or t["b"] == b))


def count_perturbed(trace, choice, depth=None):
    """Rays of `choice` whose direction rf_gloss perturbed (drawn and not rejected)."""
    return int(sum(((t["choice"] == choice) & ((t["what"] & (G.PERTURBED | G.REJECTED)) == G.PERTURBED)).sum()
                   for t in _rows(trace, depth)))


def drawn_pixels(trace, m, depth=None):
    """[m] bool: the band-local pixels with at least one draw -- of u, or of rf_gloss for the ray taken."""
    out = np.zeros(m, dtype=bool)
    for t in _rows(trace, depth):
        out[t["pix"][(t["choice"] != RULE1) & (t["choice"] != RULE3) | (t["what"] != 0)]] = True
    return out


def reflected_pixels(trace, m, depth=None):
    out = np.zeros(m, dtype=bool)
    for t in _rows(trace, depth):
        out[t["pix"][t["choice"] == REFLECTED]] = True
    return out
