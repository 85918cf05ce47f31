"""Emissive surfaces (rt_scene_set_emission) for the restatement of the indirect passes: a wrapper and
nothing more. tests/indirect_paths_ref.indirect_paths takes `nearest` and `shade` callables; `emissive` wraps the pair
so that the colour of a hit gets + E[kind][index] in binary32, the (kind, index) taken from `nearest`. A miss, a
triangle and a kind without a table get + 0. The callables are indirect_paths_ref.castref_callables' or this module's
device_callables (indirect_paths_ref's, whose records keep `index` as well). numpy only."""
import numpy as np

import indirect_paths_ref as R

f32 = np.float32
SPHERE, PLANE, CUBE = 1, 2, 3                  # RT_HIT_*
KINDS = {"sphere": SPHERE, "plane": PLANE, "cube": CUBE}


def tables(**by_name):
    """{RT_HIT_*: float32 [n, 3]} from sphere=, plane=, cube= (None or empty: no table)."""
    out = {}
    for name, v in by_name.items():
        if v is not None and len(v):
            out[KINDS[name]] = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    return out


def lookup(E, kind, index):
    """e [m, 3] of hit records (kind [m], index [m]) under the tables E: the entry, or 0."""
    kind, index = np.asarray(kind).astype(np.int64), np.asarray(index).astype(np.int64)
    e = np.zeros((len(kind), 3), dtype=np.float32)
    for k, tab in E.items():
        m = kind == k
        e[m] = tab[index[m]]
    return e


def emissive(nearest, shade, E):
    """The pair (nearest, shade') with shade'(O, D) = shade(O, D).rgb + e of nearest(O, D)'s records, in binary32."""
    def shade_e(O, D):
        rgb = np.asarray(shade(O, D), dtype=np.float32)[:, :3]
        rec = nearest(O, D)
        with np.errstate(all="ignore"):
            return (rgb + lookup(E, rec["kind"], rec["index"])).astype(np.float32)
    return nearest, shade_e


def device_callables(sc, cull=True):
    """indirect_paths_ref.device_callables with `index` in nearest's records."""
    import torch
    _, shade = R.device_callables(sc, cull)

    def nearest(O, D):
        rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([O, D], axis=1), dtype=np.float32)).cuda()
        r = {k: v.cpu().numpy() for k, v in sc.trace_rays(rays, "nearest", cull=cull).items()}
        return {"t": r["t"], "kind": r["kind"], "index": r["index"], "tx": r["txy"][:, 0], "ty": r["txy"][:, 1],
                "normal": r["normal"]}
    return nearest, shade


def term_lookup(E, ids):
    """Scene.emission_term of an id guide [..., 2]: float32 [..., 4], rgb the entry of (kind, index), a = 0."""
    ids = np.asarray(ids)
    flat = ids.reshape(-1, 2)
    out = np.zeros((flat.shape[0], 4), dtype=np.float32)
    out[:, :3] = lookup(E, flat[:, 0], flat[:, 1])
    return out.reshape(ids.shape[:-1] + (4,))
