"""The diffuse paths of rt_scene_indirect_paths restated in numpy binary32 on top of indirect_ref: steps
(a) to (g) of include/rt_engine.h for every gather ray, then indirect_ref.indirect's own steps 4 to 6.

Two callables carry the casts: `nearest(O, D) -> records` (a dict of arrays: t, kind, tx, ty, normal -- castRay's hit
record) and `shade(O, D) -> rgb [m, 3]` (or rgba). They are query_ref.CastRef's (castref_callables) or the device's
trace_rays (device_callables). The texel of step (f) comes from the scene's texture arrays `tex` ([3][th, tw]) by
q_shade_hit's index expression. numpy has no FMA: every product and sum is rounded as the kernels' expressions are."""
import numpy as np

import indirect_ref as I

f32 = np.float32
PATH_SALT = 0x426f756e
GROUP = 4                      # RT_INDIRECT_GROUP
MAX_BOUNCES = 4                # RT_INDIRECT_MAX_BOUNCES


def path_key(key, b):
    """key_b from key_0 (uint64 arrays holding uint32 values): key_{b+1} = mix(key_b ^ 0x426f756e)."""
    key = np.asarray(key, dtype=np.uint64) & I.MASK
    for _ in range(b):
        key = I.mix(key ^ PATH_SALT)
    return key


def _f2i(v):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all="ignore"):
        r = np.where(np.isnan(v), 0.0, np.clip(np.trunc(v.astype(np.float64)), -2147483648.0, 2147483647.0))
    return r.astype(np.int64)


def texel(tex, tx, ty):
    """The texel q_shade_hit reads at texture coordinates tx, ty [m]: [m, 3]."""
    th, tw = tex[0].shape
    with np.errstate(all="ignore"):
        ci = _f2i((ty * f32(th)).astype(np.float32)) * tw + _f2i((tx * f32(tw)).astype(np.float32))
    ci = np.clip(ci, 0, tw * th - 1)
    return np.stack([np.ascontiguousarray(p, dtype=np.float32).reshape(-1)[ci] for p in tex], axis=1).astype(np.float32)


def next_ray(O, D, rec_t, rec_normal, key):
    """Step (g) for hits of ray(O, D) [m, 3] with records t [m], normal [m, 3] under keys [m]: ok [m] (the normal is
    not dead), and O, D, key of the next ray (rows where ok is False are not meaningful)."""
    n = np.ascontiguousarray(rec_normal, dtype=np.float32)
    with np.errstate(all="ignore"):
        nn = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(np.float32)
        ok = (nn != 0) & np.isfinite(nn)
        n = I._normalise(n)
        flip = I.dot(n, D) > 0
        n = np.where(flip[:, None], -n, n).astype(np.float32)
        P = (O + (D * np.asarray(rec_t, dtype=np.float32)[:, None]).astype(np.float32)).astype(np.float32)
        O2 = ((n * f32(0.00001)).astype(np.float32) + P).astype(np.float32)
    k2 = path_key(key, 1)
    D2 = I.direction(n, k2)[0] if len(n) else np.zeros((0, 3), dtype=np.float32)
    return ok, O2, D2, k2


def path(O, D, key, nearest, shade, tex, bounces):
    """c_j of the gather rays (O, D) [m, 3] under key_0 `key` [m]: L [m, 3], hits [m] (the surface hits each path
    shaded) and entered [bounces] (the paths whose cast b found a hit: the queue entering bounce b's shade pass)."""
    m = O.shape[0]
    L = np.zeros((m, 3), dtype=np.float32)
    T = np.ones((m, 3), dtype=np.float32)
    hits = np.zeros(m, dtype=np.int32)
    entered = [0] * bounces
    alive = np.arange(m)
    O, D, key = O.astype(np.float32), D.astype(np.float32), np.asarray(key, dtype=np.uint64)
    for b in range(bounces):
        if not len(alive):
            break
        term = np.asarray(shade(O, D), dtype=np.float32)[:, :3]
        rec = nearest(O, D)
        hit = np.asarray(rec["kind"]) >= 0
        entered[b] = int(hit.sum())
        hits[alive[hit]] += 1
        with np.errstate(all="ignore"):
            if b == 0:
                L[alive] = (f32(0) + term).astype(np.float32)
            else:
                L[alive] = (L[alive] + (T[alive] * term).astype(np.float32)).astype(np.float32)
        if b == bounces - 1:
            break
        a = texel(tex, np.asarray(rec["tx"], dtype=np.float32)[hit], np.asarray(rec["ty"], dtype=np.float32)[hit])
        with np.errstate(all="ignore"):
            T[alive[hit]] = a if b == 0 else (T[alive[hit]] * a).astype(np.float32)
        ok, O2, D2, k2 = next_ray(O[hit], D[hit], np.asarray(rec["t"])[hit], np.asarray(rec["normal"])[hit], key[hit])
        alive, O, D, key = alive[hit][ok], O2[ok], D2[ok], k2[ok]
    return L, hits, entered


def indirect_paths(width, depth, normal, ids, O, D, nearest, shade, tex, *, bounces=2, rays=1, ray_base=0, seed=0,
                   strength=1.0, albedo=None, rgba_in=None, details=False):
    """rgba [m, 4] and packed [m] of rt_scene_indirect_paths over flat buffers. With details a dict more: indirect_ref's,
    plus `hits` [rays][k] (per live pixel, the surface hits its ray j shaded) and `counts` (per group of GROUP rays a
    list with, per bounce, the paths that entered its shade pass: rt_debug_indirect_path_counts)."""
    assert 1 <= bounces <= MAX_BOUNCES
    live, n, start, _ = I.pixels(depth, normal, ids, O, D)
    idx = np.nonzero(live)[0]
    x, y = idx % width, idx // width
    state = {"j": 0}
    hits, entered = [], []

    def path_shade(Os, G):                    # indirect_ref.indirect asks for ray j = 0, 1, ... of all live pixels in turn
        j = state["j"]
        state["j"] += 1
        key = I.key(x, y, np.full(len(idx), ray_base + j), np.full(len(idx), seed))
        L, h, e = path(Os, G, key, nearest, shade, tex, bounces)
        hits.append(h)
        entered.append(e)
        return L

    out, packed, det = I.indirect(width, depth, normal, ids, O, D, path_shade, rays=rays, ray_base=ray_base, seed=seed,
                                  strength=strength, albedo=albedo, rgba_in=rgba_in, details=True)
    if not details:
        return out, packed
    if not len(idx):
        entered = [[0] * bounces for _ in range(rays)]
        hits = [np.zeros(0, dtype=np.int32) for _ in range(rays)]
    det["hits"] = hits
    det["counts"] = [[sum(entered[j][b] for j in range(j0, min(j0 + GROUP, rays))) for b in range(bounces)]
                     for j0 in range(0, rays, GROUP)]
    return out, packed, det


# ----------------------------------------------------------------------------- the callables
def castref_callables(ref):
    """nearest and shade over query_ref.CastRef; shade keeps its records, which nearest returns for the same rays."""
    last = {}

    def shade(O, D):
        rgba, _, rec = ref.shade(O, D)
        last["key"], last["rec"] = (O.tobytes(), D.tobytes()), rec
        return rgba

    def nearest(O, D):
        if last.get("key") == (O.tobytes(), D.tobytes()):
            return last["rec"]
        return ref.nearest(O, D)
    return nearest, shade


def device_callables(sc, cull=True):
    """nearest and shade over the device's own RT_QUERY_NEAREST and RT_QUERY_SHADE."""
    import torch

    def rays(O, D):
        return torch.from_numpy(np.ascontiguousarray(np.concatenate([O, D], axis=1), dtype=np.float32)).cuda()

    def shade(O, D):
        return sc.trace_rays(rays(O, D), "shade", cull=cull)["rgba"].cpu().numpy()

    def nearest(O, D):
        r = {k: v.cpu().numpy() for k, v in sc.trace_rays(rays(O, D), "nearest", cull=cull).items()}
        return {"t": r["t"], "kind": r["kind"], "tx": r["txy"][:, 0], "ty": r["txy"][:, 1], "normal": r["normal"]}
    return nearest, shade
