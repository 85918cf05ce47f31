"""The variance-guided denoiser's semantics (rt_scene_denoise_variance) restated in numpy binary32, on
denoise_ref's helpers: vectorised over the pixels, Python loops over the taps, every intermediate a float32 array.
Only + - * /, compares and selections occur.

    denoise_variance(rgba, depth, normal, albedo, ids, moments=None, iterations=4, normal_shift=5, sigma_depth=0.05,
                     sigma_colour=4.0, sigma_floor=2^-6, min_history=4, spatial_boost=4.0, demodulate=True)
        -> (rgba_out float32 [H, W, 4], packed uint32 [H, W], variance float32 [H, W])

`rgba[..., 3]` is the history length n when `moments` ([H, W, 2], running means of luma and luma^2) is given."""
import numpy as np

import denoise_ref as R

f32 = np.float32
VMAX = f32(2.0 ** 40)
G3 = (f32(0.25), f32(0.5), f32(0.25))
DEFAULTS = dict(iterations=4, normal_shift=5, sigma_depth=0.05, sigma_colour=4.0, sigma_floor=2.0 ** -6, min_history=4,
                spatial_boost=4.0, demodulate=True)


def spatial_variance(I0, depth, normal, ids, normal_shift, sigma_depth, spatial_boost):
    """t * spatial_boost of every pixel from its 7 x 7 neighbourhood (before the clamp)."""
    h, w = depth.shape
    kind, index, N, z, zden2 = R._guides(depth, normal, ids, sigma_depth)
    with np.errstate(all="ignore"):
        Y = R.luma(I0)
        W = np.zeros((h, w), dtype=f32)
        s1 = np.zeros((h, w), dtype=f32)
        s2 = np.zeros((h, w), dtype=f32)
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                Yq = R._shifted(Y, dy, dx, 0)
                if dx == 0 and dy == 0:
                    wt = np.ones((h, w), dtype=f32)
                    ok = np.ones((h, w), dtype=bool)
                else:
                    ok, m, ez = R._geometry(N, z, zden2, kind, index, dy, dx, normal_shift)
                    wt = (m * ez).astype(f32)
                    ok &= (wt > 0) & (wt < np.inf)
                W = np.where(ok, (W + wt).astype(f32), W)
                s1 = np.where(ok, (s1 + (wt * Yq).astype(f32)).astype(f32), s1)
                s2 = np.where(ok, (s2 + (wt * (Yq * Yq).astype(f32)).astype(f32)).astype(f32), s2)
        mu1 = (s1 / W).astype(f32)
        mu2 = (s2 / W).astype(f32)
        t = (mu2 - (mu1 * mu1).astype(f32)).astype(f32)
        t = R._max(t, f32(0))
        return (t * f32(spatial_boost)).astype(f32)


def initial_variance(rgba, I0, depth, normal, albedo, ids, moments, normal_shift, sigma_depth, min_history,
                     spatial_boost, demodulate):
    """v_0 [H, W] (0 where the pixel is not valid) and the mask of the pixels whose v_0 is the temporal one."""
    valid = ids[..., 0] >= 0
    with np.errstate(all="ignore"):
        v = spatial_variance(I0, depth, normal, ids, normal_shift, sigma_depth, spatial_boost)
        temporal = np.zeros(valid.shape, dtype=bool)
        if moments is not None:
            m1, m2 = moments[..., 0].astype(f32), moments[..., 1].astype(f32)
            temporal = valid & (rgba[..., 3].astype(f32) >= f32(min_history))
            t = (m2 - (m1 * m1).astype(f32)).astype(f32)
            t = np.where(t > 0, t, f32(0)).astype(f32)
            if demodulate:
                a = R._max(R.luma(albedo.astype(f32)), R.TINY)
                t = (t / (a * a).astype(f32)).astype(f32)
            v = np.where(temporal, t, v)
        v = np.where(v < VMAX, v, VMAX).astype(f32)
    return np.where(valid, v, f32(0)).astype(f32), temporal


def mean3(v, valid):
    """The 3 x 3 mean of v over the adjacent valid pixels, weights g[dx] g[dy], g = {1, 2, 1} / 4."""
    h, w = v.shape
    with np.errstate(all="ignore"):
        sv = np.zeros((h, w), dtype=f32)
        sg = np.zeros((h, w), dtype=f32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                gg = f32(G3[dx + 1] * G3[dy + 1])
                ok = R._shifted(valid, dy, dx, False) if (dx or dy) else np.ones((h, w), dtype=bool)
                vq = R._shifted(v, dy, dx, 0)
                sv = np.where(ok, (sv + (gg * vq).astype(f32)).astype(f32), sv)
                sg = np.where(ok, (sg + gg).astype(f32), sg)
        return (sv / sg).astype(f32)


def iterate(I, v, depth, normal, ids, step, normal_shift, sigma_depth, sigma_colour, sigma_floor, want_taps=False):
    """One iteration: (I [H, W, 3], v [H, W]) -> (I', v'); pixels that are not valid keep I and have v' = 0."""
    h, w = depth.shape
    kind, index, N, z, zden2 = R._guides(depth, normal, ids, sigma_depth)
    valid = kind >= 0
    sc, sf = f32(sigma_colour), f32(sigma_floor)
    with np.errstate(all="ignore"):
        vbar = mean3(v, valid)
        S = ((f32(sc * sc) * vbar).astype(f32) + f32(sf * sf)).astype(f32)
        Yp = R.luma(I)
        acc = np.zeros((h, w, 3), dtype=f32)
        wsum = np.zeros((h, w), dtype=f32)
        vsum = np.zeros((h, w), dtype=f32)
        vmax = np.zeros((h, w), dtype=f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                Iq = R._shifted(I, oy, ox, 0)
                vq = R._shifted(v, oy, ox, 0)
                if dx == 0 and dy == 0:
                    wt = np.full((h, w), R.H5[2] * R.H5[2], dtype=f32)
                    ok = np.ones((h, w), dtype=bool)
                else:
                    ok, m, ez = R._geometry(N, z, zden2, kind, index, oy, ox, normal_shift)
                    wt = ((R.H5[dx + 2] * R.H5[dy + 2]) * m).astype(f32)
                    wt = (wt * ez).astype(f32)
                    dl = (R.luma(Iq) - Yp).astype(f32)
                    wt = (wt * (S / (S + (dl * dl).astype(f32)).astype(f32)).astype(f32)).astype(f32)
                    ok &= (wt > 0) & (wt < np.inf)
                acc = np.where(ok[..., None], (acc + (wt[..., None] * Iq).astype(f32)).astype(f32), acc)
                wsum = np.where(ok, (wsum + wt).astype(f32), wsum)
                vsum = np.where(ok, (vsum + ((wt * wt).astype(f32) * vq).astype(f32)).astype(f32), vsum)
                vmax = np.where(ok & (vq > vmax), vq, vmax)
        out = (acc / wsum[..., None]).astype(f32)
        vout = (vsum / (wsum * wsum).astype(f32)).astype(f32)
    I2 = np.where(valid[..., None], out, I).astype(f32)
    v2 = np.where(valid, vout, f32(0)).astype(f32)
    if want_taps:
        return I2, v2, vmax
    return I2, v2


def denoise_variance(rgba, depth, normal, albedo, ids, moments=None, iterations=4, normal_shift=5, sigma_depth=0.05,
                     sigma_colour=4.0, sigma_floor=2.0 ** -6, min_history=4, spatial_boost=4.0, demodulate=True,
                     want_irradiance=False):
    rgba = np.ascontiguousarray(rgba, dtype=f32)
    valid = ids[..., 0] >= 0
    I = R.demodulated(rgba, albedo) if demodulate else rgba[..., :3].copy()
    I0 = I.copy()
    v, temporal = initial_variance(rgba, I0, depth, normal, albedo, ids, moments, normal_shift, sigma_depth, min_history,
                                   spatial_boost, demodulate)
    v0 = v.copy()
    for i in range(iterations):
        I, v = iterate(I, v, depth, normal, ids, 1 << i, normal_shift, sigma_depth, sigma_colour, sigma_floor)
    with np.errstate(all="ignore"):
        C = (I * albedo[..., :3].astype(f32)).astype(f32) if demodulate else I
    out = rgba.copy()
    out[valid, :3] = C[valid]
    out[valid, 3] = f32(1)
    packed = R.pack(out)
    if want_irradiance:
        return out, packed, v, I0, I, v0, temporal
    return out, packed, v
