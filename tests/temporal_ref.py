"""Temporal accumulation (rt_scene_temporal) restated in numpy binary32: vectorised over the pixels, a
Python loop over the four taps, every intermediate a float32 array (numpy rounds each float32 operation once, to
nearest even, as the device does with contraction off and correctly rounded division). Only + - * /, compares and
selections occur. Written from the definition; it shares no code with the kernels.

    temporal(cur, prev, O, D, view, prev_view, prev_aspect, same_view, ...) -> dict(rgba, moments, packed, ...)

cur = dict(rgba [H, W, 4], depth [H, W], normal [H, W, 4], id [H, W, 2]); prev = None (reset) or dict(rgba, depth,
normal, id, moments [H, W, 2] or None), where prev['rgba'] is a former result (accumulated colour, history length).
O, D: the current view's primary rays, [H * W, 3] or [H, W, 3] (Scene.primary_rays or Composer.primary); view /
prev_view: the seven terms of rt_view_terms (only prev_view's are used: the current view is in the rays); same_view:
the two views are the same bytes (cam and aspect), which the host decides. temporal is a thin entry onto `accumulate`,
which tmotion_ref.temporal_motion enters with a displacement per pixel and a colour box to clamp the history to."""
import numpy as np

from denoise_ref import luma, pack

f32 = np.float32
DEFAULTS = dict(max_history=32, depth_tolerance=0.02, normal_cos_min=0.9)


def _dot3(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(f32) + a[..., 2] * b[..., 2]).astype(f32)


def reproject_point(P, prev_view, prev_aspect, w, h):
    """(fx, fy, qq, ok) of the world points P (three [H, W] arrays): where each lands in the previous view, the squared
    distance to the previous eye, and whether the geometry allows a history at all."""
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


def world_points(depth, O, D, w, h):
    """P = O + D t of every pixel, as three [H, W] arrays."""
    t = depth.astype(f32)
    O = np.asarray(O, dtype=f32).reshape(h, w, 3)
    D = np.asarray(D, dtype=f32).reshape(h, w, 3)
    with np.errstate(all="ignore"):
        return [(O[..., k] + (D[..., k] * t).astype(f32)).astype(f32) for k in range(3)]


def reproject(depth, O, D, prev_view, prev_aspect, w, h):
    """reproject_point of each pixel's world point."""
    return reproject_point(world_points(depth, O, D, w, h), prev_view, prev_aspect, w, h)


def _floor(f):
    """Truncation towards zero, corrected for negative values (f within [-1, 32768])."""
    i = np.trunc(f.astype(np.float64)).astype(np.int64)
    return np.where(i.astype(f32) > f, i - 1, i)


def accumulate(cur, prev, O, D, prev_view, prev_aspect, same_view, m=None, clamp=None, max_history=32,
               depth_tolerance=0.02, normal_cos_min=0.9, want_moments=True):
    """The one accumulation behind temporal and tmotion_ref.temporal_motion: (result, details). m: None, or the
    displacement [H, W, 3] of the object each pixel shows, which its world point is moved back by; a pixel that did not
    move under the same view reads the history at itself with weight 1 (the single tap), every other pixel the four
    taps around where it lands. clamp: None, or (lo, hi, slack, clamp_history) with the colour box [H, W, 3] that the
    history's mean is brought into, shortening a clamped history. details: has_history, clamped, static [H, W] and
    taps, per tap taken (counted [H, W], the tap's prev rgba [H, W, 4])."""
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
    taps = []
    if prev is not None:
        ids, t, N = cur["id"], cur["depth"].astype(f32), cur["normal"][..., :3].astype(f32)
        with np.errstate(all="ignore"):
            cand = (ids[..., 0] >= 0) & (t > 0) & (t < np.inf)
            tol, cos2 = f32(depth_tolerance), f32(f32(normal_cos_min) * f32(normal_cos_min))
            if m is not None:
                static = (m[..., 0] == 0) & (m[..., 1] == 0) & (m[..., 2] == 0)
            single = static if same_view else np.zeros((h, w), dtype=bool)
            qq = (t * t).astype(f32)
            tapdefs = []
            if same_view:
                yy, xx = np.mgrid[0:h, 0:w]
                tapdefs.append((single, xx, yy, np.ones((h, w), dtype=f32)))
            if m is not None or not same_view:
                P = world_points(t, O, D, w, h)
                if m is not None:
                    P = [(P[k] - m[..., k]).astype(f32) for k in range(3)]
                fx, fy, qq4, ok = reproject_point(P, prev_view, prev_aspect, w, h)
                cand &= single | ok
                qq = np.where(single, qq, qq4).astype(f32)
                four = cand & ~single
                fx = np.where(four, fx, f32(0)).astype(f32)
                fy = np.where(four, fy, f32(0)).astype(f32)
                x0, y0 = _floor(fx), _floor(fy)
                ax, ay = (fx - x0.astype(f32)).astype(f32), (fy - y0.astype(f32)).astype(f32)
                bx, by = (f32(1) - ax).astype(f32), (f32(1) - ay).astype(f32)
                tapdefs += [(four, x0, y0, (bx * by).astype(f32)), (four, x0 + 1, y0, (ax * by).astype(f32)),
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
                taps.append((good, pc))
            has = cand & (S["w"] > 0)
            W = S["w"]
            H = [(S[k] / W).astype(f32) for k in ("r", "g", "b")]
            nh = (S["n"] / W).astype(f32)
            if clamp is not None:
                lo, hi, sl, clamp_history = clamp
                for k in range(3):
                    e = ((hi[..., k] - lo[..., k]).astype(f32) * f32(sl)).astype(f32)
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
    return res, dict(has_history=has, clamped=clamped, static=static, taps=taps)


def temporal(cur, prev, O, D, view, prev_view, prev_aspect, same_view, max_history=32, depth_tolerance=0.02,
             normal_cos_min=0.9, want_moments=True, details=False):
    res, d = accumulate(cur, prev, O, D, prev_view, prev_aspect, same_view, max_history=max_history,
                        depth_tolerance=depth_tolerance, normal_cos_min=normal_cos_min, want_moments=want_moments)
    if details:
        res.update(has_history=d["has_history"], taps=d["taps"])
    return res
