"""The display transform (rt_scene_display) restated in numpy binary32 and Python integers: steps 1 to 5
of include/rt_engine.h. Every colour intermediate is a float32 array (numpy rounds each float32 operation once, to
nearest even, as the device does with contraction off and correctly rounded division); the histogram and its resolve
are integers; the sRGB codes come from the library's own table of thresholds (rt_display_transfer_table), so no pow
enters a comparison of bits.

    display(rgba, state=None, ids=None, table=None, meter="auto", ...) -> dict(rgba, pixels, state, histogram, E)

`state` is a float32 [4] (None: zeros) and is not written; the new one is returned. `resolve_sorted` is a second
restatement of the resolve that ranks the luminances instead of counting them."""
import numpy as np

from denoise_ref import _max, luma, pack

f32 = np.float32
BINS = 512
BIN0 = 1776
DEFAULTS = dict(meter="auto", exposure=1.0, key=0.18, min_exposure=2.0 ** -6, max_exposure=2.0 ** 6, meter_low=512,
                meter_high=973, adapt=1.0, meter_sky=False, curve="aces", white=4.0, transfer="srgb")


def table(rt):
    """The library's thresholds T[0 .. 255]."""
    import ctypes as C
    t = (C.c_float * 256)()
    assert rt.load_library().rt_display_transfer_table(t) == 0
    return np.array(t, dtype=f32)


def table_formula():
    """EOTF((v - 0.5) / 255) in binary64, T[0] = 0: what the library's table rounds to binary32."""
    c = (np.arange(256, dtype=np.float64) - 0.5) / 255.0
    t = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    t[0] = 0.0
    return t


def bins(l):
    """The bin of every luminance, -1 where it is not metered by its value (l <= 0, not finite)."""
    l = np.ascontiguousarray(l, dtype=f32)
    with np.errstate(invalid="ignore"):
        ok = (l > 0) & (l < np.inf)
    k = np.clip((l.view(np.uint32) >> 19).astype(np.int64) - BIN0, 0, BINS - 1)
    return np.where(ok, k, -1)


def histogram(rgba, ids=None, meter_sky=False):
    """Step 1: h[512] as Python-sized integers."""
    with np.errstate(all="ignore"):
        k = bins(luma(np.asarray(rgba, dtype=f32)))
    if ids is not None and not meter_sky:
        k = np.where(ids[..., 0] >= 0, k, -1)
    return np.bincount(k[k >= 0].ravel(), minlength=BINS).astype(np.int64)


def window(N, meter_low, meter_high):
    return (N * meter_low) >> 10, (N * meter_high + 1023) >> 10


def metered_luminance(h, meter_low=512, meter_high=973):
    """Lm of a histogram with N > 0 (integers throughout)."""
    N = int(h.sum())
    lo, hi = window(N, meter_low, meter_high)
    cum, s = 0, 0
    for k in range(BINS):
        c1 = cum + int(h[k])
        s += max(0, min(c1, hi) - max(cum, lo)) * k
        cum = c1
    m = (s * 256) // (hi - lo)
    return np.array([(BIN0 << 19) + (m << 11) + (1 << 18)], dtype=np.uint32).view(f32)[0]


def resolve(h, state, npx, exposure=1.0, key=0.18, min_exposure=2.0 ** -6, max_exposure=2.0 ** 6, meter_low=512,
            meter_high=973, adapt=1.0):
    """Step 2: the new state."""
    e0, valid0 = f32(state[0]), f32(state[3]) == f32(1)
    N = int(h.sum())
    if N == 0:
        return np.array([e0 if valid0 else f32(exposure), 0, 0, 1], dtype=f32)
    Lm = metered_luminance(h, meter_low, meter_high)
    with np.errstate(all="ignore"):
        et = f32(key) / Lm
        et = f32(min_exposure) if et < f32(min_exposure) else et
        et = f32(max_exposure) if et > f32(max_exposure) else et
        e = f32(e0 + f32(f32(et - e0) * f32(adapt))) if valid0 and f32(adapt) < f32(1) else et
        return np.array([e, Lm, f32(N) / f32(npx), 1], dtype=f32)


def resolve_sorted(l, meter_low=512, meter_high=973):
    """Lm from the metered luminances themselves: rank them, average the bins of ranks [lo, hi)."""
    k = np.sort(bins(np.asarray(l, dtype=f32)))
    k = k[k >= 0]
    lo, hi = window(len(k), meter_low, meter_high)
    m = (int(k[lo:hi].sum()) * 256) // (hi - lo)
    return np.array([(BIN0 << 19) + (m << 11) + (1 << 18)], dtype=np.uint32).view(f32)[0]


def _unit(o):
    o = _max(o, f32(0))
    return np.where(o > f32(1), f32(1), o).astype(f32)


def tone(rgb, E, curve="aces", white=4.0):
    """Steps 3 and 4 on [..., 3]."""
    with np.errstate(all="ignore"):
        c = (np.asarray(rgb, dtype=f32) * f32(E)).astype(f32)
        if curve == "clip":
            return c
        if curve == "reinhard":
            L = _max(luma(c), f32(0))
            w2 = f32(f32(white) * f32(white))
            s = ((f32(1) + (L / w2).astype(f32)).astype(f32) / (f32(1) + L).astype(f32)).astype(f32)
            return _unit((c * s[..., None]).astype(f32))
        x = _max(c, f32(0))
        x = np.where(x > f32(1024), f32(1024), x).astype(f32)
        num = (x * ((f32(2.51) * x).astype(f32) + f32(0.03)).astype(f32)).astype(f32)
        den = ((x * ((f32(2.43) * x).astype(f32) + f32(0.59)).astype(f32)).astype(f32) + f32(0.14)).astype(f32)
        return _unit((num / den).astype(f32))


def codes(o, T):
    """The number of v in 1 .. 255 with o >= T[v] (a NaN gives 0)."""
    o = np.asarray(o, dtype=f32)
    count = np.searchsorted(T[1:], o, side="right")               # T increases: the thresholds at or below o
    return np.where(np.isnan(o), 0, count).astype(np.uint32)


def pack_srgb(o, T):
    c = codes(o[..., :3], T)
    return ((c[..., 0] << 16) + (c[..., 1] << 8) + c[..., 2]).astype(np.uint32)


def display(rgba, state=None, ids=None, table=None, meter="auto", exposure=1.0, key=0.18, min_exposure=2.0 ** -6,
            max_exposure=2.0 ** 6, meter_low=512, meter_high=973, adapt=1.0, meter_sky=False, curve="aces", white=4.0,
            transfer="srgb"):
    """The whole call on a float32 [H, W, 4]. histogram: None where the call writes none (manual, or N == 0)."""
    rgba = np.asarray(rgba, dtype=f32)
    state = np.zeros(4, dtype=f32) if state is None else np.asarray(state, dtype=f32)
    h, new = None, None
    if meter == "manual":
        E = f32(exposure)
    else:
        h = histogram(rgba, ids, meter_sky)
        new = resolve(h, state, rgba.shape[0] * rgba.shape[1], exposure, key, min_exposure, max_exposure, meter_low,
                      meter_high, adapt)
        E = new[0] if meter == "auto" else (state[0] if state[3] == f32(1) else f32(exposure))
        if h.sum() == 0:
            h = None
    o = tone(rgba[..., :3], E, curve, white)
    out = np.concatenate([o, rgba[..., 3:]], axis=-1)                # alpha bit for bit: a copy
    pixels = pack(o) if transfer == "linear" else pack_srgb(o, table)
    return dict(rgba=out, pixels=pixels, state=new, histogram=h, E=E)
