"""One case per instantiation of the reflective passes ("The matrix of instantiations"): for each of the
20 cells (GLASS, KINDS, SAMPLES, GLOSS, FRESNEL) of rt_reflect_primary a scene, the call that renders it, the composed
reference of that call and the cell the frame must dispatch to (rt_debug_reflect_dispatch).

Nothing here traces a ray or restates a rule: a cell's reference is the least derived composer that has the cell's
features -- Composer, GlassComposer, SceneComposer, their Gloss* and Fresnel* subclasses -- on its own for one sample and
under SampleRef / GlossSampleRef / FresnelSampleRef for many. Where an existing suite already holds a cell's case, its
cached reference is the one used.

Shapes: the spheres-only cells (KINDS = 0) are 48 spheres at 50 x 30 (1 500 pixels, a multiple of neither 64 nor 256),
depth 2; the scene cells the staged scene of tests/test_reflect_scene_gpu.py at its 64 x 48, depth 3, with the glass
sphere's tau set to 0 in the cells without glass. SAMPLES cells take 5 samples from sample 2 of 8: a group of four and a
group of one, and an absolute sample index that is not the index in the slab. GLOSS cells (FRESNEL ones included, so
that the glass is frosted) put RHO_TABLE on the spheres by index and, in the scene, roughness on the floor and the slab;
scene cells without GLOSS keep an all-zero plane table set. Every cell sets the seed SEED."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

import fresnel_ref as FR
import gloss_ref as G
from reflect_samples_ref import SampleRef, _live_pixels
from reflect_scene_ref import CUBE, PLANE, SPHERE, TRIANGLE, SceneComposer
from scenes import Inputs
from test_fresnel_cpu import K_TABLE, glass_mats
from test_reflect_cpu import composer_for
from test_refract_cpu import glass_composer_for

Cell = namedtuple("Cell", "glass kinds samples gloss fresnel")
# FRESNEL comes with GLASS and GLOSS only: 16 cells without it, 4 with it
CELLS = tuple(Cell(*(int(ch) for ch in f"{v:04b}"), 0) for v in range(16)) + \
    tuple(Cell(1, k, s, 1, 1) for k in (0, 1) for s in (0, 1))
SKY = -1
N_SPHERES = 48
RHO_TABLE = (0.0, 0.05, 0.3, 1.0)
SEED = 7
SPP, BASE, TOTAL = 5, 2, 8
GROUP = 4                                # RT_REFLECT_SAMPLE_GROUP
ROUGH_PLANE = (1.0,)                     # the camera looks along the floor: many R' dip below it and are rejected
ROUGH_CUBE = (0.3, 0.5)                  # the slab; the post has k = 0, its roughness is idle
DISPATCH_FIELDS = ("glass", "kinds", "samples", "gloss", "fresnel", "bvh", "groups")
NONE = dict(zip(DISPATCH_FIELDS, (-1,) * 6 + (0,)))


def name(cell):
    return "".join(str(v) for v in cell)


def bounce_kernel(cell):
    """The instantiation of rt_reflect_bounce<GLASS, KINDS, GLOSS, FRESNEL> a cell's frame runs."""
    return (cell.glass, cell.kinds, cell.gloss, cell.fresnel)


def shape(cell):
    """(W, H, depth)"""
    return (64, 48, 3) if cell.kinds else (50, 30, 2)


def rho_by_index(n):
    """RHO_TABLE by index so that every pair with K_TABLE occurs. The phase 2 makes sphere 0 (the staged scene's large
    mirror) and sphere 1 (its glass sphere) rough, and of the four phases it is the one under which the spheres-only
    cells perturb the most continuations after bounce 0 (13 to 17 of them; 4 to 7 under phase 1)."""
    return np.array([RHO_TABLE[(i // 4 + 2) % 4] for i in range(n)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _staged(rt, oracle):
    from test_reflect_scene_gpu import _stage
    return _stage(rt, oracle)


def inputs(rt, oracle, cell):
    """(inp, mesh text or None)"""
    if cell.kinds:
        inp, mesh, _ = _staged(rt, oracle)
        return inp, mesh
    return Inputs(rt, N_SPHERES), None


def materials(rt, oracle, cell):
    """The cell's material tables as the composers take them (the scene cells: SceneComposer's keywords)."""
    if cell.kinds:
        mats = dict(_staged(rt, oracle)[2])
        if not cell.glass:
            mats["tau"] = np.zeros_like(mats["tau"])
            mats["ior"] = np.zeros_like(mats["ior"])
        return mats
    if cell.glass:
        k, tau, ior = glass_mats(N_SPHERES)
        return {"k": k, "tau": tau, "ior": ior}
    return {"k": np.array([K_TABLE[i % 4] for i in range(N_SPHERES)], dtype=np.float32)}


def roughness(rt, oracle, cell):
    """{"sphere" / "plane" / "cube": table} of a GLOSS cell, else {}."""
    if not cell.gloss:
        return {}
    inp, _ = inputs(rt, oracle, cell)
    rough = {"sphere": rho_by_index(inp.n)}
    if cell.kinds:
        rough["plane"] = np.array(ROUGH_PLANE, dtype=np.float32)
        rough["cube"] = np.array(ROUGH_CUBE, dtype=np.float32)
    return rough


def call(cell):
    """The frame's keywords for Scene.frame_desc beside its buffers."""
    kw = {"reflect_depth": shape(cell)[2]}
    if cell.samples:
        kw.update(spp=SPP, sample_base=BASE, sample_total=TOTAL)
    return kw


def expected_dispatch(cell, cull=True):
    groups = (SPP + GROUP - 1) // GROUP if cell.samples else 1
    return dict(zip(DISPATCH_FIELDS, tuple(cell) + (1 if cull else 0, groups)))


# ----------------------------------------------------------------------------- the device side
def scene(rt, oracle, cell, *, gloss=None, fresnel=None):
    """A fresh scene set up for the cell. gloss / fresnel = False: the cell's neighbour without that feature (the same
    scene without its roughness tables / under the plain glass model)."""
    gloss = bool(cell.gloss) if gloss is None else gloss
    fresnel = bool(cell.fresnel) if fresnel is None else fresnel
    inp, mesh = inputs(rt, oracle, cell)
    mats = materials(rt, oracle, cell)
    sc = inp.scene()
    if cell.kinds:
        sc.set_mesh(rt.mesh_from_obj_text(mesh))
        sc.set_materials_ex(mats["k_sphere"], mats["tau"], mats["ior"])      # no tau > 0: no glass table
        sc.set_plane_materials(mats["k_plane"])
        sc.set_cube_materials(mats["k_cube"])
        sc.set_reflect_scope("scene")
    elif cell.glass:
        sc.set_materials_ex(mats["k"], mats["tau"], mats["ior"])
    else:
        sc.set_materials(mats["k"])
    if gloss:
        for kind, v in roughness(rt, oracle, cell).items():
            sc.set_roughness(kind, v)
    elif cell.kinds:
        sc.set_roughness("plane", np.zeros(inp.n_planes, dtype=np.float32))  # an all-zero table costs nothing
    sc.set_gloss_seed(SEED)
    sc.set_glass_model("fresnel" if fresnel else "plain")
    if cell.samples:
        sc.set_reflect_samples("many")
    return sc


def dispatch(rt, sc):
    """rt_debug_reflect_dispatch on the scene's handle -> {field: value} (NONE before any reflective frame)."""
    out = (C.c_int * len(DISPATCH_FIELDS))()
    rc = rt.load_library().rt_debug_reflect_dispatch(sc.handle, out, len(DISPATCH_FIELDS))
    assert rc == 0, rt.load_library().rt_last_error()
    return dict(zip(DISPATCH_FIELDS, (int(v) for v in out)))


# ----------------------------------------------------------------------------- the reference
def _composer(rt, oracle, cell):
    inp, mesh = inputs(rt, oracle, cell)
    if cell.kinds:
        cls = FR.FresnelSceneComposer if cell.fresnel else (G.GlossSceneComposer if cell.gloss else SceneComposer)
        comp = cls(oracle, rt, inp, mesh)
    elif cell.fresnel:
        comp = FR.fresnel_composer_for(oracle, rt, inp)
    elif cell.gloss:
        comp = G.gloss_composer_for(oracle, rt, inp, glass=bool(cell.glass))
    else:
        comp = glass_composer_for(oracle, rt, inp) if cell.glass else composer_for(oracle, rt, inp)
    if cell.gloss:
        comp.set_gloss(seed=SEED, **roughness(rt, oracle, cell))
    if cell.fresnel:
        comp.set_glass_model(FR.FRESNEL)
    return comp


def _one_sample(comp, cell, W, H, depth, mats):
    """A one-sample cell's frame in the shape SampleRef.render returns."""
    if cell.kinds:
        rgba, packed, queue = comp.render(W, H, depth, **mats)
        trace = comp.trace
        pix = [t["pix"] for t in trace]
        kind0 = trace[0]["kind"].copy()
    else:
        extra = {"tau": mats["tau"], "ior": mats["ior"]} if cell.glass else {}
        rgba, packed = comp.render(W, H, mats["k"], depth, **extra)
        trace = comp.trace
        cont = (mats["k"] > 0) | (mats.get("tau", mats["k"]) > 0)
        pix = [t["pix"] for t in trace] if "pix" in trace[0] else _live_pixels(trace, W * H, cont)
        queue = ([p.size for p in pix[1:]] + [0] * depth)[:depth]
        kind0 = None
    one = {"k": 0, "rgba": rgba, "queue": list(queue), "trace": trace, "pix": pix, "kind0": kind0,
           "gloss": getattr(comp, "gloss_trace", []), "fresnel": getattr(comp, "fresnel_trace", [])}
    return {"rgba": rgba, "packed": packed, "queue": list(queue), "samples": [one]}


def _existing(rt, oracle, cell):
    """The cell's reference where an existing suite already holds its case (the same inputs, shape and call)."""
    if cell == Cell(0, 0, 1, 0, 0):
        from test_reflect_samples_gpu import _ref2
        return _ref2(rt, oracle, SPP, BASE, TOTAL)
    if cell == Cell(1, 1, 0, 0, 0):
        from test_reflect_scene_gpu import _reference
        W, H, depth = shape(cell)
        frames, trace = _reference(rt, oracle)
        rgba, packed, queue = frames[depth]
        one = {"k": 0, "rgba": rgba, "queue": list(queue), "trace": trace, "pix": [t["pix"] for t in trace],
               "kind0": trace[0]["kind"].copy(), "gloss": [], "fresnel": []}
        return {"rgba": rgba, "packed": packed, "queue": list(queue), "samples": [one]}
    return None


@functools.lru_cache(maxsize=None)
def reference(rt, oracle, cell):
    """{"rgba" [H, W, 4], "packed" [H, W], "queue" (depth ints, summed over the samples), "samples"}: per sample
    {"k", "rgba", "queue", "trace" (the composer's walk), "pix" (live pixels per bounce), "kind0" (scene cells: the kind
    of the primary hit), "gloss", "fresnel" (the traces of gloss_ref / fresnel_ref; [] without the feature)}. Computed
    once per cell and shared: leave it unchanged."""
    ref = _existing(rt, oracle, cell)
    if ref is None:
        W, H, depth = shape(cell)
        comp = _composer(rt, oracle, cell)
        mats = materials(rt, oracle, cell)
        if cell.samples:
            wrap = FR.FresnelSampleRef if cell.fresnel else (G.GlossSampleRef if cell.gloss else SampleRef)
            ref = wrap(rt, comp).render(W, H, depth, spp=SPP, base=BASE, total=TOTAL, **mats)
        else:
            ref = _one_sample(comp, cell, W, H, depth, mats)
    else:          # (the other suite's object stays as it is)
        ref = dict(ref, samples=[{"gloss": [], "fresnel": [], **s} for s in ref["samples"]])
    return ref


# ----------------------------------------------------------------------------- reading the traces
def _kind_at(sample, b, pix):
    """The kind that the pixels `pix`, live at bounce b, met there (spheres-only cells: SPHERE or SKY)."""
    tr = sample["trace"][b]
    at = np.searchsorted(sample["pix"][b], pix)
    assert np.array_equal(sample["pix"][b][at], pix)
    return tr["kind"][at] if "kind" in tr else np.where(tr["index"][at] >= 0, SPHERE, SKY)


def conditions(cell, ref):
    """{condition: count} -- how often the code the cell adds does work, from the reference's traces alone. Only the
    bounces below the frame's depth count (SceneComposer walks one past it)."""
    W, H, depth = shape(cell)
    m = W * H
    samples = ref["samples"]
    out = {}
    if cell.gloss:
        rows = [(s, t) for s in samples for t in s["gloss"] if t["b"] < depth]
        hit = lambda t: (t["what"] & G.PERTURBED) != 0
        out["perturbed at bounce 0"] = sum(int(hit(t).sum()) for _, t in rows if t["b"] == 0)
        out["perturbed at a later bounce"] = sum(int(hit(t).sum()) for _, t in rows if t["b"] > 0)
        out["halved or rejected"] = sum(int(((t["what"] & (G.HALVED | G.REJECTED)) != 0).sum()) for _, t in rows)
        if cell.kinds:
            for label, code in (("sphere", SPHERE), ("plane", PLANE), ("cube", CUBE)):
                out[f"perturbed on a {label}"] = sum(int((_kind_at(s, t["b"], t["pix"][hit(t)]) == code).sum())
                                                     for s, t in rows)
    if cell.glass:
        out["rule-4 passes"] = min(sum(int((tr["rule"] == 4).sum()) for tr in s["trace"][:depth]) for s in samples)
    if cell.fresnel:
        out["reflect choices in the poorest sample"] = min(FR.count(s["fresnel"], FR.REFLECTED, depth=depth) for s in samples)
        out["transmit choices in the poorest sample"] = min(FR.count(s["fresnel"], FR.THROUGH, depth=depth) for s in samples)
        out["perturbed exits"] = sum(FR.count_perturbed(s["fresnel"], FR.THROUGH, depth=depth) for s in samples)
    if cell.samples:
        queued = np.zeros((len(samples), m), dtype=bool)
        for j, s in enumerate(samples):
            if len(s["pix"]) > 1:
                queued[j, s["pix"][1]] = True
        out["queued in one sample and not in another"] = int((queued.any(axis=0) & ~queued.all(axis=0)).sum())
        if cell.fresnel:
            r = np.stack([FR.reflected_pixels(s["fresnel"], m, depth=depth) for s in samples])
            out["reflected in one sample and through in another"] = int((r.any(axis=0) & ~r.all(axis=0)).sum())
        if cell.gloss:
            # pixels whose primary hit is perturbed in two samples, under draws that differ (the key takes the sample)
            p0 = np.zeros((len(samples), m), dtype=bool)
            for j, s in enumerate(samples):
                for t in s["gloss"]:
                    if t["b"] == 0:
                        p0[j, t["pix"][(t["what"] & G.PERTURBED) != 0]] = True
            both = np.nonzero(p0[0] & p0[-1])[0]
            u = [G.ball(G.key(both % W, both // W, s["k"], SEED), 0)[0] for s in (samples[0], samples[-1])]
            out["perturbed by different draws in two samples"] = int((u[0] != u[1]).any(axis=1).sum()) if both.size else 0
    if cell.kinds:
        for label, code in (("triangle", TRIANGLE), ("sphere", SPHERE), ("plane", PLANE), ("cube", CUBE), ("sky", SKY)):
            out[f"primary hits: {label}"] = min(int((s["kind0"] == code).sum()) for s in samples)
        k0 = samples[0]["kind0"].reshape(H, W)
        out["pixels whose right neighbour is of another kind"] = int((k0[:, 1:] != k0[:, :-1]).sum())
        if cell.samples:
            k = np.stack([s["kind0"] for s in samples])
            out["pixels whose samples meet different kinds"] = int((k != k[0]).any(axis=0).sum())
    return out
