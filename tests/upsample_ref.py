"""Guided upsampling (rt_scene_upsample) restated in numpy binary32: vectorised over the hi pixels, a
Python loop over the four taps, every intermediate a float32 array (numpy rounds each float32 operation once, to
nearest even, as the device does with contraction off and correctly rounded division). Only + - * /, compares and
selections occur. Written from the definition; it shares no code with the kernels.

    upsample(hi, lo, base=None, select=None, normal_shift=5, sigma_depth=0.05, demodulate=True, details=False)
        -> dict(rgba float32 [H, W, 4], packed uint32 [H, W], source uint8 [H, W])

hi = dict(depth [H, W], normal [H, W, 4], id [H, W, 2], albedo [H, W, 4] when demodulating); lo = the same at
[h, w] plus rgba [h, w, 4]. base: None or float32 [H, W, 4]. select: None (no tables) or a dict with any of "sphere",
"plane", "cube", each a sequence with a non-zero entry per selected object."""
import numpy as np

from denoise_ref import pack

f32 = np.float32
RT_HIT_TRIANGLE, RT_HIT_SPHERE, RT_HIT_PLANE, RT_HIT_CUBE = 0, 1, 2, 3
TINY = f32(2.0 ** -10)
DEFAULTS = dict(normal_shift=5, sigma_depth=0.05, demodulate=True)
_KINDS = (("sphere", RT_HIT_SPHERE), ("plane", RT_HIT_PLANE), ("cube", RT_HIT_CUBE))


def _max(a, b):
    """a > b ? a : b (a NaN `a` gives b)."""
    return np.where(a > b, a, b).astype(f32)


def selected(ids, select):
    """Which hi pixels are upsampled."""
    kind, index = ids[..., 0], ids[..., 1]
    if select is None:
        return kind >= 0
    sel = np.zeros(kind.shape, dtype=bool)
    for name, k in _KINDS:
        t = np.asarray(select.get(name, ()) if select.get(name) is not None else ()).reshape(-1)
        if t.size == 0:
            continue
        ok = (kind == k) & (index >= 0) & (index < t.size)
        sel |= ok & (t[np.clip(index, 0, t.size - 1)] != 0)
    return sel


def positions(W, w):
    """(x0 int64 [W], ax float32 [W]) of the hi coordinates 0 .. W - 1 in a lo buffer of w."""
    s = f32(f32(w) / f32(W))
    f = (((np.arange(W).astype(f32) + f32(0.5)).astype(f32) * s).astype(f32) - f32(0.5)).astype(f32)
    i = np.trunc(f.astype(np.float64)).astype(np.int64)
    i = np.where(i.astype(f32) > f, i - 1, i)
    return i, (f - i.astype(f32)).astype(f32)


def upsample(hi, lo, base=None, select=None, normal_shift=5, sigma_depth=0.05, demodulate=True, details=False):
    ids = np.asarray(hi["id"])
    H, W = ids.shape[:2]
    lo_rgba = np.ascontiguousarray(lo["rgba"], dtype=f32)
    h, w = lo_rgba.shape[:2]
    sel = selected(ids, select)
    kind, index = ids[..., 0], ids[..., 1]
    z = np.asarray(hi["depth"], dtype=f32)
    N = np.asarray(hi["normal"], dtype=f32)[..., :3]
    x0, ax = positions(W, w)
    y0, ay = positions(H, h)
    X0, Y0 = np.broadcast_to(x0[None, :], (H, W)), np.broadcast_to(y0[:, None], (H, W))
    AX, AY = np.broadcast_to(ax[None, :], (H, W)), np.broadcast_to(ay[:, None], (H, W))
    one = f32(1)
    taps = []
    with np.errstate(all="ignore"):
        zden = (f32(sigma_depth) * _max(np.abs(z), TINY)).astype(f32)
        D = (zden * zden).astype(f32)
        S = np.zeros((H, W, 3), dtype=f32)
        Sw = np.zeros((H, W), dtype=f32)
        F = np.zeros((H, W, 3), dtype=f32)
        Fw = np.zeros((H, W), dtype=f32)
        for k in range(4):
            tx, ty = X0 + (k & 1), Y0 + (k >> 1)
            wx = AX if k & 1 else (one - AX).astype(f32)
            wy = AY if k & 2 else (one - AY).astype(f32)
            b = (wx * wy).astype(f32)
            inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            cx, cy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
            c = lo_rgba[cy, cx, :3]
            # the plain bilinear mean
            fok = inside & (b > 0)
            F = np.where(fok[..., None], (F + (b[..., None] * c).astype(f32)).astype(f32), F)
            Fw = np.where(fok, (Fw + b).astype(f32), Fw)
            # the guided mean
            qid = np.asarray(lo["id"])[cy, cx]
            ok = sel & inside & (qid[..., 0] == kind) & ((kind == RT_HIT_TRIANGLE) | (qid[..., 1] == index))
            Nq = np.asarray(lo["normal"], dtype=f32)[cy, cx, :3]
            dot = ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]).astype(f32) + N[..., 2] * Nq[..., 2]).astype(f32)
            m = _max(dot, f32(0))
            for _ in range(normal_shift):
                m = (m * m).astype(f32)
            d = (np.asarray(lo["depth"], dtype=f32)[cy, cx] - z).astype(f32)
            ez = (D / (D + (d * d).astype(f32)).astype(f32)).astype(f32)
            wq = ((b * m).astype(f32) * ez).astype(f32)
            ok &= (wq > 0) & (wq < np.inf)
            I = c
            if demodulate:
                I = (c / _max(np.asarray(lo["albedo"], dtype=f32)[cy, cx, :3], TINY)).astype(f32)
            S = np.where(ok[..., None], (S + (wq[..., None] * I).astype(f32)).astype(f32), S)
            Sw = np.where(ok, (Sw + wq).astype(f32), Sw)
            taps.append((ok, I, wq, b, fok))
        up = sel & (Sw > 0)
        C = (S / Sw[..., None]).astype(f32)
        if demodulate:
            C = (C * np.asarray(hi["albedo"], dtype=f32)[..., :3]).astype(f32)
        out = np.ones((H, W, 4), dtype=f32)
        if base is not None:
            out[...] = np.asarray(base, dtype=f32)
        else:
            out[..., :3] = (F / Fw[..., None]).astype(f32)
        out[up, :3] = C[up]
        out[up, 3] = one
    source = np.where(up, 1, np.where(sel, 2, 0)).astype(np.uint8)
    res = dict(rgba=out, packed=pack(out), source=source)
    if details:
        res.update(selected=sel, taps=taps, wsum=Sw)
    return res


def bilinear(lo_rgba, W, H):
    """The plain bilinear mean of every hi pixel (the pass without guides): float32 [H, W, 3]."""
    h, w = lo_rgba.shape[:2]
    ids = np.full((H, W, 2), -1, dtype=np.int32)
    hi = dict(id=ids, depth=np.zeros((H, W), dtype=f32), normal=np.zeros((H, W, 4), dtype=f32))
    lo = dict(rgba=lo_rgba, id=np.full((h, w, 2), -1, dtype=np.int32), depth=np.zeros((h, w), dtype=f32),
              normal=np.zeros((h, w, 4), dtype=f32))
    return upsample(hi, lo, demodulate=False)["rgba"][..., :3]
