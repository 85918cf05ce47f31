"""Temporal accumulation (rt_scene_temporal) restated in numpy binary32: vectorised over the pixels, a
Python loop over the four taps, every intermediate a float32 array (numpy rounds each float32 operation once, to
nearest even, as the device does with contraction off and correctly rounded division). Only + - * /, compares and
selections occur. Written from the definition; it shares no code with the kernels.

    temporal(cur, prev, O, D, view, prev_view, prev_aspect, same_view, ...) -> dict(rgba, moments, packed, ...)

cur = dict(rgba [H, W, 4], depth [H, W], normal [H, W, 4], id [H, W, 2]); prev = None (reset) or dict(rgba, depth,
normal, id, moments [H, W, 2] or None), where prev['rgba'] is a former result (accumulated colour, history length).
O, D: the current view's primary rays, [H * W, 3] or [H, W, 3] (Scene.primary_rays or Composer.primary); view /
prev_view: the seven terms of rt_view_terms (only prev_view's are used: the current view is in the rays); same_view:
the two views are the same bytes (cam and aspect), which the host decides."""
import numpy as np

from denoise_ref import luma, pack

f32 = np.float32
DEFAULTS = dict(max_history=32, depth_tolerance=0.02, normal_cos_min=0.9)


def _dot3(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(f32) + a[..., 2] * b[..., 2]).astype(f32)


def reproject(depth, O, D, prev_view, prev_aspect, w, h):
    """(fx, fy, qq, ok): where each pixel's world point lands in the previous view, the squared distance to the
    previous eye, and whether the geometry allows a history at all."""
    t = depth.astype(f32)
    O = np.asarray(O, dtype=f32).reshape(h, w, 3)
    D = np.asarray(D, dtype=f32).reshape(h, w, 3)
    po = [f32(v) for v in prev_view[:3]]
    cp, sp, cy, sy = (f32(v) for v in prev_view[3:7])
    a = f32(prev_aspect)
    with np.errstate(all="ignore"):
        P = [(O[..., k] + (D[..., k] * t).astype(f32)).astype(f32) for k in range(3)]
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


def _floor(f):
    """Truncation towards zero, corrected for negative values (f within [-1, 32768])."""
    i = np.trunc(f.astype(np.float64)).astype(np.int64)
    return np.where(i.astype(f32) > f, i - 1, i)


def temporal(cur, prev, O, D, view, prev_view, prev_aspect, same_view, max_history=32, depth_tolerance=0.02,
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
    taps = []
    if prev is not None:
        ids, t, N = cur["id"], cur["depth"].astype(f32), cur["normal"][..., :3].astype(f32)
        with np.errstate(all="ignore"):
            cand = (ids[..., 0] >= 0) & (t > 0) & (t < np.inf)
            tol, cos2 = f32(depth_tolerance), f32(f32(normal_cos_min) * f32(normal_cos_min))
            if same_view:
                qq = (t * t).astype(f32)
                yy, xx = np.mgrid[0:h, 0:w]
                tapdefs = [(xx, yy, np.ones((h, w), dtype=f32))]
            else:
                fx, fy, qq, ok = reproject(t, O, D, prev_view, prev_aspect, w, h)
                cand &= ok
                fx = np.where(cand, fx, f32(0)).astype(f32)
                fy = np.where(cand, fy, f32(0)).astype(f32)
                x0, y0 = _floor(fx), _floor(fy)
                ax, ay = (fx - x0.astype(f32)).astype(f32), (fy - y0.astype(f32)).astype(f32)
                bx, by = (f32(1) - ax).astype(f32), (f32(1) - ay).astype(f32)
                tapdefs = [(x0, y0, (bx * by).astype(f32)), (x0 + 1, y0, (ax * by).astype(f32)),
                           (x0, y0 + 1, (bx * ay).astype(f32)), (x0 + 1, y0 + 1, (ax * ay).astype(f32))]
            pm = prev.get("moments")
            use_m = want_moments and pm is not None
            S = {k: np.zeros((h, w), dtype=f32) for k in ("w", "r", "g", "b", "n", "m1", "m2")}
            nn = _dot3(N, N)
            for tx, ty, wt in tapdefs:
                inside = cand & (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
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
                taps.append((good, pc))
            has = cand & (S["w"] > 0)
            W = S["w"]
            n = ((S["n"] / W).astype(f32) + f32(1)).astype(f32)
            n = np.where(n < f32(max_history), n, f32(max_history)).astype(f32)
            al = (f32(1) / n).astype(f32)

            def blend(sumv, x):
                H = (sumv / W).astype(f32)
                return (H + ((x - H).astype(f32) * al).astype(f32)).astype(f32)
            acc = np.stack([blend(S["r"], c[..., 0]), blend(S["g"], c[..., 1]), blend(S["b"], c[..., 2]), n], axis=-1)
            out = np.where(has[..., None], acc, out).astype(f32)
            if use_m:
                am = np.stack([blend(S["m1"], Y), blend(S["m2"], (Y * Y).astype(f32))], axis=-1)
                mom = np.where(has[..., None], am, mom).astype(f32)
    res = dict(rgba=out, moments=mom if want_moments else None, packed=pack(out), depth=cur["depth"],
               normal=cur["normal"], id=cur["id"])
    if details:
        res["has_history"] = has
        res["taps"] = taps           # per tap: (counted [H, W], the tap's prev rgba [H, W, 4])
    return res
