"""Temporal accumulation over moving spheres and cubes with a history clamp (rt_scene_temporal_motion)
restated in numpy binary32, in the manner of temporal_ref.py: vectorised over the pixels, every intermediate a float32
array, only + - * /, compares and selections. Written from the definition; it shares no code with the kernels. The
accumulation itself is temporal_ref.accumulate; here are the displacement of a pixel and the colour box of the clamp.

    temporal_motion(cur, prev, O, D, view, prev_view, prev_aspect, same_view, sphere_motion=..., cube_motion=...,
                    clamp=..., clamp_slack=..., clamp_history=..., ...) -> dict(rgba, moments, packed, ...)

The arguments are temporal_ref.temporal's; sphere_motion / cube_motion: None or [n, 3] / [n, 4] displacements."""
import numpy as np

from temporal_ref import accumulate

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


def temporal_motion(cur, prev, O, D, view, prev_view, prev_aspect, same_view, sphere_motion=None, cube_motion=None,
                    clamp=True, clamp_slack=0.25, clamp_history=4, max_history=32, depth_tolerance=0.02,
                    normal_cos_min=0.9, want_moments=True, details=False):
    m = box_ = None
    if prev is not None:
        m = displacement(cur["id"], sphere_motion, cube_motion)
        if clamp:
            box_ = box(cur["rgba"]) + (clamp_slack, clamp_history)
    res, d = accumulate(cur, prev, O, D, prev_view, prev_aspect, same_view, m=m, clamp=box_, max_history=max_history,
                        depth_tolerance=depth_tolerance, normal_cos_min=normal_cos_min, want_moments=want_moments)
    if details:
        res.update(has_history=d["has_history"], clamped=d["clamped"], static=d["static"])
    return res
