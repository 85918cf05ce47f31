"""Temporal accumulation over moving spheres and cubes with a history clamp (rt_scene_temporal_motion)
restated in numpy binary32, in the manner of temporal_ref.py: vectorised over the pixels, every intermediate a float32
array, only + - * /, compares and selections. Written from the definition; it shares no code with the kernels.

    temporal_motion(cur, prev, O, D, view, prev_view, prev_aspect, same_view, sphere_motion=..., cube_motion=...,
                    clamp=..., clamp_slack=..., clamp_history=..., ...) -> dict(rgba, moments, packed, ...)

The arguments are temporal_ref.temporal's; sphere_motion / cube_motion: None or [n, 3] / [n, 4] displacements."""
import numpy as np

from denoise_ref import luma, pack
from temporal_ref import _dot3, _floor

f32 = np.float32
RT_HIT_SPHERE, RT_HIT_CUBE = 1, 3
DEFAULTS = dict(max_history=32, depth_tolerance=0.02, normal_cos_min=0.9, clamp=1, clamp_slack=0.25, clamp_history=4)


def key(a):
    """The key of a float in the total order of the bit patterns: its bits, flipped entirely if the sign is set, else
    with the sign bit set; compared unsigned."""
    u = np.ascontiguousarray(a, dtype=f32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(f32)


def box(rgba, order=None):
    """(lo, hi) [H, W, 3]: per channel the minimum and maximum, in the order of the keys, of rgba over the 3 x 3
    pixels around each pixel that lie inside the buffer (reading with clamped coordinates gives the same set of
    values). order: the sequence in which the nine offsets are folded in (None: row by row)."""
    c = np.ascontiguousarray(rgba, dtype=f32)[..., :3]
    h, w = c.shape[:2]
    k = np.pad(key(c), ((1, 1), (1, 1), (0, 0)), mode="edge")
    offs = [(dy, dx) for dy in range(3) for dx in range(3)]
    if order is not None:
        offs = [offs[i] for i in order]
    lo = hi = None
    for dy, dx in offs:
        v = k[dy:dy + h, dx:dx + w]
        lo = v if lo is None else np.where(v < lo, v, lo)
        hi = v if hi is None else np.where(v > hi, v, hi)
    return unkey(lo), unkey(hi)


def displacement(ids, sphere_motion, cube_motion):
    """m [H, W, 3] of the object each pixel shows; planes, triangles and indices outside the tables: 0."""
    kind, index = ids[..., 0], ids[..., 1]
    m = np.zeros(kind.shape + (3,), dtype=f32)
    for k, tab in ((RT_HIT_SPHERE, sphere_motion), (RT_HIT_CUBE, cube_motion)):
        if tab is None or len(tab) == 0:
            continue
        tab = np.asarray(tab, dtype=f32)[:, :3]
        sel = (kind == k) & (index >= 0) & (index < tab.shape[0])
        m[sel] = tab[index[sel]]
    return m


def reproject_point(P, prev_view, prev_aspect, w, h):
    """temporal_ref.reproject from the world point on: (fx, fy, qq, ok)."""
    po = [f32(v) for v in prev_view[:3]]
    cp, sp, cy, sy = (f32(v) for v in prev_view[3:7])
    a = f32(prev_aspect)
    with np.errstate(all="ignore"):
        qx, qy, qz = ((P[k] - po[k]).astype(f32) for k in range(3))
        qq = (((qx * qx).astype(f32) + (qy * qy).astype(f32)).astype(f32) + (qz * qz).astype(f32)).astype(f32)
        vx = ((qx * cy).astype(f32) - (qz * sy).astype(f32)).astype(f32)
        z1 = ((qx * sy).astype(f32) + (qz * cy).astype(f32)).astype(f32)
        vy = ((qy * cp).astype(f32) + (z1 * sp).astype(f32)).astype(f32)
        vz = ((z1 * cp).astype(f32) - (qy * sp).astype(f32)).astype(f32)
        ok = vz > 0
        s = (f32(f32(1) / a) / vz).astype(f32)
        dx, dy = (vx * s).astype(f32), (vy * s).astype(f32)
        half = f32(f32(w) * f32(0.5))
        fx = ((((dx + f32(1)).astype(f32) / a).astype(f32) * half).astype(f32) - f32(0.5)).astype(f32)
        fy = ((((dy + f32(1)).astype(f32) / a).astype(f32) * half).astype(f32) - f32(0.5)).astype(f32)
        ok &= (fx >= -1) & (fx <= f32(w)) & (fy >= -1) & (fy <= f32(h))
    return fx, fy, qq, ok


def temporal_motion(cur, prev, O, D, view, prev_view, prev_aspect, same_view, sphere_motion=None, cube_motion=None,
                    clamp=True, clamp_slack=0.25, clamp_history=4, max_history=32, depth_tolerance=0.02,
                    normal_cos_min=0.9, want_moments=True, details=False):
    c4 = np.ascontiguousarray(cur["rgba"], dtype=f32)
    c = c4[..., :3]
    h, w = c.shape[:2]
    Y = luma(c)
    with np.errstate(all="ignore"):
        new_m = np.stack([Y, (Y * Y).astype(f32)], axis=-1)
    out = np.concatenate([c, np.ones((h, w, 1), dtype=f32)], axis=-1)
    mom = new_m.copy()
    has = np.zeros((h, w), dtype=bool)
    clamped = np.zeros((h, w), dtype=bool)
    static = np.ones((h, w), dtype=bool)
    if prev is not None:
        ids, t, N = cur["id"], cur["depth"].astype(f32), cur["normal"][..., :3].astype(f32)
        with np.errstate(all="ignore"):
            cand = (ids[..., 0] >= 0) & (t > 0) & (t < np.inf)
            tol, cos2 = f32(depth_tolerance), f32(f32(normal_cos_min) * f32(normal_cos_min))
            m = displacement(ids, sphere_motion, cube_motion)
            static = (m[..., 0] == 0) & (m[..., 1] == 0) & (m[..., 2] == 0)
            single = static if same_view else np.zeros((h, w), dtype=bool)     # the pixel itself, weight 1
            Oa = np.asarray(O, dtype=f32).reshape(h, w, 3)
            Da = np.asarray(D, dtype=f32).reshape(h, w, 3)
            P = [(Oa[..., k] + (Da[..., k] * t).astype(f32)).astype(f32) for k in range(3)]
            Pm = [(P[k] - m[..., k]).astype(f32) for k in range(3)]
            fx, fy, qq4, ok = reproject_point(Pm, prev_view, prev_aspect, w, h)
            cand &= single | ok
            qq = np.where(single, (t * t).astype(f32), qq4).astype(f32)
            four = cand & ~single
            fx = np.where(four, fx, f32(0)).astype(f32)
            fy = np.where(four, fy, f32(0)).astype(f32)
            x0, y0 = _floor(fx), _floor(fy)
            ax, ay = (fx - x0.astype(f32)).astype(f32), (fy - y0.astype(f32)).astype(f32)
            bx, by = (f32(1) - ax).astype(f32), (f32(1) - ay).astype(f32)
            yy, xx = np.mgrid[0:h, 0:w]
            tapdefs = [(single, xx, yy, np.ones((h, w), dtype=f32)),
                       (four, x0, y0, (bx * by).astype(f32)), (four, x0 + 1, y0, (ax * by).astype(f32)),
                       (four, x0, y0 + 1, (bx * ay).astype(f32)), (four, x0 + 1, y0 + 1, (ax * ay).astype(f32))]
            pm = prev.get("moments")
            use_m = want_moments and pm is not None
            S = {k: np.zeros((h, w), dtype=f32) for k in ("w", "r", "g", "b", "n", "m1", "m2")}
            nn = _dot3(N, N)
            for group, tx, ty, wt in tapdefs:
                inside = cand & group & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                cx, cy_ = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
                pid = prev["id"][cy_, cx]
                pt = prev["depth"][cy_, cx].astype(f32)
                pn = prev["normal"][cy_, cx, :3].astype(f32)
                pc = prev["rgba"][cy_, cx].astype(f32)
                good = inside & (pid[..., 0] == ids[..., 0]) & (pid[..., 1] == ids[..., 1])
                dd = np.abs(((pt * pt).astype(f32) - qq).astype(f32))
                good &= dd <= (tol * qq).astype(f32)
                dot = _dot3(N, pn)
                good &= dot > 0
                good &= (dot * dot).astype(f32) >= (cos2 * (nn * _dot3(pn, pn)).astype(f32)).astype(f32)
                vals = dict(r=pc[..., 0], g=pc[..., 1], b=pc[..., 2], n=pc[..., 3])
                if use_m:
                    pmq = pm[cy_, cx].astype(f32)
                    vals.update(m1=pmq[..., 0], m2=pmq[..., 1])
                S["w"] = np.where(good, (S["w"] + wt).astype(f32), S["w"])
                for k, v in vals.items():
                    S[k] = np.where(good, (S[k] + (wt * v).astype(f32)).astype(f32), S[k])
            has = cand & (S["w"] > 0)
            W = S["w"]
            H = [(S[k] / W).astype(f32) for k in ("r", "g", "b")]
            nh = (S["n"] / W).astype(f32)
            if clamp:
                lo, hi = box(c4)
                sl = f32(clamp_slack)
                for k in range(3):
                    e = ((hi[..., k] - lo[..., k]).astype(f32) * sl).astype(f32)
                    lo_, hi_ = (lo[..., k] - e).astype(f32), (hi[..., k] + e).astype(f32)
                    below = H[k] < lo_
                    above = ~below & (H[k] > hi_)
                    H[k] = np.where(below, lo_, np.where(above, hi_, H[k])).astype(f32)
                    clamped |= has & (below | above)
                nh = np.where(clamped & (nh > f32(clamp_history)), f32(clamp_history), nh).astype(f32)
            n = (nh + f32(1)).astype(f32)
            n = np.where(n < f32(max_history), n, f32(max_history)).astype(f32)
            al = (f32(1) / n).astype(f32)

            def blend(Hk, x):
                return (Hk + ((x - Hk).astype(f32) * al).astype(f32)).astype(f32)
            acc = np.stack([blend(H[0], c[..., 0]), blend(H[1], c[..., 1]), blend(H[2], c[..., 2]), n], axis=-1)
            out = np.where(has[..., None], acc, out).astype(f32)
            if use_m:
                am = np.stack([blend((S["m1"] / W).astype(f32), Y), blend((S["m2"] / W).astype(f32), (Y * Y).astype(f32))], axis=-1)
                mom = np.where(has[..., None], am, mom).astype(f32)
    res = dict(rgba=out, moments=mom if want_moments else None, packed=pack(out), depth=cur["depth"],
               normal=cur["normal"], id=cur["id"])
    if details:
        res["has_history"] = has
        res["clamped"] = clamped
        res["static"] = static
    return res
