"""The indirect pass (rt_scene_indirect) restated in numpy binary32: steps 1 to 6 of include/rt_engine.h.

Its own integer mixer, key, Marsaglia draw and composition; numpy has no FMA, so every product and sum is rounded as the
kernels' expressions are. The primary directions come from the caller (Scene.primary_rays on the device, the oracle's
rays on the CPU), and the colour of a gather ray from a callable `shade(O, D) -> rgb [m, 3]`: query_ref.CastRef.shade,
or Scene.trace_rays(..., "shade")."""
import numpy as np

f32 = np.float32
u32 = np.uint32
GOLD = 0x9e3779b9
SALT = 0x47497261
MASK = 0xffffffff


# ----------------------------------------------------------------------------- the hash
def mix(x):
    """The integer mixer, on uint64 arrays holding uint32 values (wrapping by the mask)."""
    x = np.asarray(x, dtype=np.uint64) & MASK
    x ^= x >> 16
    x = (x * 0x7feb352d) & MASK
    x ^= x >> 15
    x = (x * 0x846ca68b) & MASK
    x ^= x >> 16
    return x


def key(px, py, s, seed):
    px, py, s, seed = (np.asarray(v, dtype=np.uint64) for v in (px, py, s, seed))
    return mix(mix(mix(mix(seed) ^ s) ^ py) ^ px)


def draw(kg, t, a):
    """draw(t, a) under the mixed key kg: 24 bits as an exact binary32 value of [-1, 1)."""
    h = mix(kg + (GOLD * (t * 2 + a + 1)) % (1 << 32))
    return ((h >> 8).astype(np.float32) * f32(2.0 ** -23) - f32(1)).astype(np.float32)


def _normalise(v):
    """rf_normalise: a zero length leaves the vector as it is."""
    with np.errstate(all="ignore"):
        l = np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(np.float32)).astype(np.float32)
        nz = l != 0
        return np.where(nz[:, None], v / np.where(nz, l, f32(1))[:, None], v).astype(np.float32)


def dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).astype(np.float32)


def direction(n, k):
    """Step 3 for normals n [m, 3] and keys k [m]: G [m, 3], tries [m] (pairs drawn until one qualified, 0: none did)
    and the point u [m, 3] of the unit sphere."""
    n = np.ascontiguousarray(n, dtype=np.float32)
    m = n.shape[0]
    kg = mix(np.asarray(k, dtype=np.uint64) ^ SALT)
    u = np.zeros((m, 3), dtype=np.float32)
    tries = np.zeros(m, dtype=np.int32)
    open_ = np.ones(m, dtype=bool)
    for t in range(6):
        x1, x2 = draw(kg, t, 0), draw(kg, t, 1)
        s = (x1 * x1 + x2 * x2).astype(np.float32)
        take = open_ & (s < f32(1))
        with np.errstate(all="ignore"):
            r = np.sqrt((f32(1) - s).astype(np.float32)).astype(np.float32)
        cand = np.stack([(f32(2) * x1) * r, (f32(2) * x2) * r, f32(1) - f32(2) * s], axis=1).astype(np.float32)
        u[take] = cand[take]
        tries[take] = t + 1
        open_ &= ~take
    G = _normalise((n + u).astype(np.float32))
    with np.errstate(all="ignore"):
        keep = dot(G, n) > 0
    G = np.where(keep[:, None], G, n).astype(np.float32)
    return G, tries, u


# ----------------------------------------------------------------------------- the pass
def pack(c):
    """rgbToInt(f2i(c * 254) ...) of colours c [m, 3]."""
    v = (np.asarray(c, dtype=np.float32) * f32(254)).astype(np.float32)
    with np.errstate(all="ignore"):
        i = np.where(np.isnan(v), 0.0, np.clip(np.trunc(v.astype(np.float64)), -2147483648.0, 2147483647.0)).astype(np.int64)
    i = np.minimum(i, 255) & 0xff
    return ((i[:, 0] << 16) + (i[:, 1] << 8) + i[:, 2]).astype(np.uint32)


def pixels(depth, normal, ids, O, D):
    """Steps 1 and 2 over flat guides (depth [m], normal [m, 4], ids [m, 2]) with the primary rays O, D [m, 3]:
    live [m], n [m, 3], start [m, 3] (rows of dead pixels are not meaningful)."""
    depth = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)
    ng = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1, 4)[:, :3]
    kind = np.asarray(ids).reshape(-1, 2)[:, 0]
    with np.errstate(all="ignore"):
        nn = ((ng[:, 0] * ng[:, 0] + ng[:, 1] * ng[:, 1]) + ng[:, 2] * ng[:, 2]).astype(np.float32)
        live = (kind >= 0) & np.isfinite(depth) & (nn != 0) & np.isfinite(nn)
        P = (O + (D * depth[:, None]).astype(np.float32)).astype(np.float32)
        n = _normalise(ng)
        flip = dot(n, D) > 0
        n = np.where(flip[:, None], -n, n).astype(np.float32)
        start = ((n * f32(0.00001)).astype(np.float32) + P).astype(np.float32)
    return live, n, start, flip


def gather_rays(width, live, n, start, rays, ray_base, seed):
    """The gather rays of the live pixels: index [k] (flat pixel), and per ray j the directions G [rays][k, 3]."""
    idx = np.nonzero(live)[0]
    x, y = idx % width, idx // width
    Gs = []
    for j in range(rays):
        k = key(x, y, np.full(len(idx), ray_base + j), np.full(len(idx), seed))
        Gs.append(direction(n[idx], k)[0])
    return idx, Gs


def indirect(width, depth, normal, ids, O, D, shade, *, rays=1, ray_base=0, seed=0, strength=1.0, albedo=None,
             rgba_in=None, details=False):
    """rgba [m, 4] and packed [m] of the pass over flat buffers; shade(O, D) -> rgb [k, 3] (or rgba)."""
    live, n, start, flip = pixels(depth, normal, ids, O, D)
    m = live.shape[0]
    idx, Gs = gather_rays(width, live, n, start, rays, ray_base, seed)
    S = np.zeros((len(idx), 3), dtype=np.float32)
    cols = []
    for G in Gs:
        c = np.asarray(shade(start[idx], G), dtype=np.float32)[:, :3] if len(idx) else np.zeros((0, 3), dtype=np.float32)
        cols.append(c)
        S = (S + c).astype(np.float32)
    E = (S / f32(rays)).astype(np.float32)
    I = (f32(strength) * E).astype(np.float32)
    if albedo is not None:
        I = (I * np.ascontiguousarray(albedo, dtype=np.float32).reshape(-1, 4)[idx, :3]).astype(np.float32)
    out = np.zeros((m, 4), dtype=np.float32)
    out[:, 3] = 1
    if rgba_in is not None:
        out[:] = np.ascontiguousarray(rgba_in, dtype=np.float32).reshape(-1, 4)
        out[idx, :3] = (out[idx, :3] + I).astype(np.float32)
    else:
        out[idx, :3] = I
    packed = pack(out[:, :3])
    if details:
        return out, packed, dict(live=live, idx=idx, flip=flip, start=start, n=n, G=Gs, colours=cols)
    return out, packed
