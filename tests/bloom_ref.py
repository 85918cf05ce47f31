"""The bloom pass (rt_scene_bloom) restated in numpy binary32: steps 1 to 6 of include/rt_engine.h. Every
intermediate is a float32 array (numpy rounds each float32 operation once, to nearest even, as the device does with
contraction off and correctly rounded division).

    bloom(rgba, state=None, levels=5, ...) -> dict(rgba, pixels, glow, B, t, lim)

`bloom_loops` is a second restatement written as plain loops over pixels and scalars, for the first to be held
against."""
import numpy as np

from denoise_ref import _max, luma, pack

f32 = np.float32
MAX_LEVELS = 8
DEFAULTS = dict(levels=5, threshold=1.0, limit=64.0, spread=0.75, strength=0.125)


def level_sizes(w, h, levels):
    """[(w_0, h_0), .. (w_L, h_L)]."""
    sizes = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        sizes.append((w, h))
    return sizes


def scale(state, threshold=1.0, limit=64.0):
    """Step 1: (t, lim)."""
    E = f32(1)
    if state is not None and f32(state[3]) == f32(1):
        E = f32(state[0])
    with np.errstate(all="ignore"):
        return f32(threshold) / E, f32(limit) / E


def bright(rgba, t, lim):
    """Step 2: Br as [H, W, 3]."""
    rgba = np.asarray(rgba, dtype=f32)
    with np.errstate(all="ignore"):
        l = luma(rgba)
        ok = (l > t) & (l < np.inf)
        s = ((l - t).astype(f32) / l).astype(f32)
        v = _max((rgba[..., :3] * s[..., None]).astype(f32), f32(0))
        v = np.where(v > lim, lim, v).astype(f32)
    return np.where(ok[..., None], v, f32(0)).astype(f32)


def down_taps(n_src):
    """The four source indices of every destination index along one axis: [4, n_dst]."""
    i = np.arange((n_src + 1) >> 1)
    return np.stack([np.clip(2 * i - 1, 0, n_src - 1), 2 * i, np.clip(2 * i + 1, 0, n_src - 1),
                     np.clip(2 * i + 2, 0, n_src - 1)])


def _tap(a, b, c, d):
    with np.errstate(all="ignore"):
        return (((a + d).astype(f32) + (f32(3) * (b + c).astype(f32)).astype(f32)).astype(f32) * f32(0.125)).astype(f32)


def down(S):
    """Step 3 on [hs, ws, C]."""
    S = np.asarray(S, dtype=f32)
    xs, ys = down_taps(S.shape[1]), down_taps(S.shape[0])
    H = _tap(S[:, xs[0]], S[:, xs[1]], S[:, xs[2]], S[:, xs[3]])
    return _tap(H[ys[0]], H[ys[1]], H[ys[2]], H[ys[3]])


def up_taps(n_dst, n_src):
    """(c, n): the nearer and the farther source index of every destination index along one axis."""
    i = np.arange(n_dst)
    c = i >> 1
    return c, np.clip(c + np.where(i & 1, 1, -1), 0, n_src - 1)


def _lerp(a, b):
    with np.errstate(all="ignore"):
        return ((f32(0.75) * a).astype(f32) + (f32(0.25) * b).astype(f32)).astype(f32)


def up(S, wd, hd):
    """Step 4: [hc, wc, C] to [hd, wd, C]."""
    S = np.asarray(S, dtype=f32)
    cx, nx = up_taps(wd, S.shape[1])
    cy, ny = up_taps(hd, S.shape[0])
    G = _lerp(S[:, cx], S[:, nx])
    return _lerp(G[cy], G[ny])


def bloom(rgba, state=None, levels=5, threshold=1.0, limit=64.0, spread=0.75, strength=0.125):
    """The whole call on a float32 [H, W, 4]. B: [B_1 .. B_L] as the downsamples left them."""
    rgba = np.asarray(rgba, dtype=f32)
    h, w = rgba.shape[:2]
    sizes = level_sizes(w, h, levels)
    t, lim = scale(state, threshold, limit)
    B = [down(bright(rgba, t, lim))]
    for _ in range(1, levels):
        B.append(down(B[-1]))
    assert [b.shape[:2] for b in B] == [(hk, wk) for wk, hk in sizes[1:]]
    A = B[-1]
    with np.errstate(all="ignore"):
        for k in range(levels - 2, -1, -1):                          # B[k] is level k + 1
            A = (B[k] + (f32(spread) * up(A, sizes[k + 1][0], sizes[k + 1][1])).astype(f32)).astype(f32)
        T = up(A, w, h)
        c = rgba[..., :3]
        o = np.where(T == f32(0), c, (c + (f32(strength) * T).astype(f32)).astype(f32)).astype(f32)
    out = np.concatenate([o, rgba[..., 3:]], axis=-1)                # alpha bit for bit: a copy
    glow = np.concatenate([T, np.zeros((h, w, 1), dtype=f32)], axis=-1)
    return dict(rgba=out, pixels=pack(o), glow=glow, B=B, t=t, lim=lim)


# ----------------------------------------------------------------------------- the same, pixel by pixel
def _clamp(i, n):
    return 0 if i < 0 else (n - 1 if i > n - 1 else i)


def _luma1(r, g, b):
    return f32(f32(f32(0.2126) * r + f32(0.7152) * g) + f32(0.0722) * b)


def _bright1(px, t, lim):
    r, g, b = f32(px[0]), f32(px[1]), f32(px[2])
    l = _luma1(r, g, b)
    if not (l > t) or not (l < f32(np.inf)):
        return [f32(0)] * 3
    s = f32(f32(l - t) / l)
    out = []
    for c in (r, g, b):
        v = f32(c * s)
        v = v if v > f32(0) else f32(0)
        out.append(lim if v > lim else v)
    return out


def _tap1(a, b, c, d):
    return f32(f32(f32(a + d) + f32(f32(3) * f32(b + c))) * f32(0.125))


def _down_loops(S, ws, hs):
    """S: S[y][x] = [3 scalars]."""
    wd, hd = (ws + 1) >> 1, (hs + 1) >> 1
    D = [[None] * wd for _ in range(hd)]
    for y in range(hd):
        ys = (_clamp(2 * y - 1, hs), 2 * y, _clamp(2 * y + 1, hs), _clamp(2 * y + 2, hs))
        for x in range(wd):
            xs = (_clamp(2 * x - 1, ws), 2 * x, _clamp(2 * x + 1, ws), _clamp(2 * x + 2, ws))
            px = []
            for ch in range(3):
                H = [_tap1(S[j][xs[0]][ch], S[j][xs[1]][ch], S[j][xs[2]][ch], S[j][xs[3]][ch]) for j in ys]
                px.append(_tap1(H[0], H[1], H[2], H[3]))
            D[y][x] = px
    return D


def _up1(S, wc, hc, x, y, ch):
    cx, cy = x >> 1, y >> 1
    nx, ny = _clamp(cx + (1 if x & 1 else -1), wc), _clamp(cy + (1 if y & 1 else -1), hc)
    G = [f32(f32(f32(0.75) * S[j][cx][ch]) + f32(f32(0.25) * S[j][nx][ch])) for j in (cy, ny)]
    return f32(f32(f32(0.75) * G[0]) + f32(f32(0.25) * G[1]))


def bloom_loops(rgba, state=None, levels=5, threshold=1.0, limit=64.0, spread=0.75, strength=0.125):
    """bloom()'s rgba and glow, by loops over pixels."""
    rgba = np.asarray(rgba, dtype=f32)
    h, w = rgba.shape[:2]
    sizes = level_sizes(w, h, levels)
    with np.errstate(all="ignore"):
        E = f32(1)
        if state is not None and f32(state[3]) == f32(1):
            E = f32(state[0])
        t, lim = f32(f32(threshold) / E), f32(f32(limit) / E)
        S = [[_bright1(rgba[y, x], t, lim) for x in range(w)] for y in range(h)]
        B = []
        for k in range(levels):
            S = _down_loops(S, sizes[k][0], sizes[k][1])
            B.append(S)
        A = B[-1]
        for k in range(levels - 2, -1, -1):
            wk, hk = sizes[k + 1]
            wc, hc = sizes[k + 2]
            A = [[[f32(B[k][y][x][ch] + f32(f32(spread) * _up1(A, wc, hc, x, y, ch))) for ch in range(3)]
                  for x in range(wk)] for y in range(hk)]
        out, glow = rgba.copy(), np.zeros_like(rgba)
        for y in range(h):
            for x in range(w):
                for ch in range(3):
                    T = _up1(A, sizes[1][0], sizes[1][1], x, y, ch)
                    glow[y, x, ch] = T
                    if not T == f32(0):
                        out[y, x, ch] = f32(rgba[y, x, ch] + f32(f32(strength) * T))
    return dict(rgba=out, glow=glow)


# ----------------------------------------------------------------------------- what the suites feed it
def hand_frame(w, h, seed=0, salt=True):
    """Log-normal luminances over 2^-10 .. 2^10 with a tint per channel; salted with what a frame can hold."""
    rng = np.random.default_rng(seed)
    l = np.exp2(np.clip(rng.normal(0, 4, (h, w, 1)), -10, 10))
    rgba = np.concatenate([l * rng.uniform(0.5, 1.5, (h, w, 3)), rng.uniform(-1, 2, (h, w, 1))], axis=-1).astype(f32)
    if salt:
        flat = rgba.reshape(-1, 4)
        n = flat.shape[0]
        for i, v in enumerate(np.array([0.0, -0.0, -0.75, 2.0 ** -140, 1e30, np.inf, -np.inf, np.nan], dtype=f32)):
            flat[(3 * i + 1) % n, i % 4] = v
            if n >= 16:
                flat[(5 * i + 7) % n, :3] = v
    return rgba
