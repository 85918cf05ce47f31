"""The numpy restatements of the post passes (denoise_ref, vdenoise_ref, temporal_ref, tmotion_ref, upsample_ref), bit
for bit: SHA-256 of every array they return, over seeded synthetic inputs, against tests/golden/post_refs_digest.json.
The restatements are what the device is compared with, so a refactor of them must not move one bit; this test is the
pin. The inputs are built to reach the branches that scenes rarely do: miss pixels (id.x = -1), a triangle id, a zero,
a negative and an infinite depth, a NaN and an infinite colour, a zero normal, history lengths on both sides of
min_history and clamp_history, a displacement index outside its table, and at 7 x 5 every 7 x 7 and step-8
neighbourhood leaving the buffer.

The golden file is written by hand, never by the test:

    python tests/test_post_refs_cpu.py --write [--refs DIR] [--out FILE]

--refs DIR takes the five restatements from DIR instead of tests/ (another revision's, to prove that two revisions
return the same bits)."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_refs_digest.json")
SHAPES = ((24, 16), (7, 5))                         # width x height
f32 = np.float32


def _refs():
    return {k: importlib.import_module(k) for k in ("denoise_ref", "vdenoise_ref", "temporal_ref", "tmotion_ref",
                                                    "upsample_ref")}


def _blocks(rng, h, w, lo, hi):
    """Integers in [lo, hi) that are constant over blocks of 3 rows x 4 columns, so that neighbours often agree."""
    coarse = rng.integers(lo, hi, size=((h + 2) // 3, (w + 3) // 4))
    return np.repeat(np.repeat(coarse, 3, axis=0), 4, axis=1)[:h, :w]


def guides(seed, w, h):
    """dict(rgba, depth, normal, albedo, id, moments) of one synthetic frame; rgba[..., 3] is a history length."""
    rng = np.random.default_rng(seed)
    kind = _blocks(rng, h, w, -1, 4).astype(np.int32)
    index = _blocks(rng, h, w, 0, 4).astype(np.int32)          # the motion tables have three rows: 3 is outside
    index[kind < 0] = -1
    kind[h // 2, w // 2], index[h // 2, w // 2] = 0, 7          # a triangle whose neighbours are other triangles
    kind[0, 0], index[0, 0] = -1, -1
    depth = (f32(4) + _blocks(rng, h, w, 0, 3).astype(f32) + rng.random((h, w), dtype=f32) * f32(0.2)).astype(f32)
    depth[kind < 0] = np.inf
    normal = np.zeros((h, w, 4), dtype=f32)
    n = _blocks(rng, h, w, 0, 3)
    normal[..., :3] = np.eye(3, dtype=f32)[n] + (rng.random((h, w, 3), dtype=f32) - f32(0.5)) * f32(0.3)
    albedo = np.ones((h, w, 4), dtype=f32)
    albedo[..., :3] = rng.random((h, w, 3), dtype=f32)
    rgba = rng.random((h, w, 4), dtype=f32)
    rgba[..., 3] = rng.integers(1, 40, size=(h, w)).astype(f32)  # on both sides of 4 (min_history, clamp_history) and 32
    y = rng.random((h, w), dtype=f32)
    moments = np.stack([y, (y * y + rng.random((h, w), dtype=f32) * f32(0.05)).astype(f32)], axis=-1).astype(f32)
    # the rare values, on hit pixels, each with hit neighbours
    hits = np.argwhere(kind > 0)
    pick = hits[rng.permutation(len(hits))[:8]]
    (a, b, c, d, e, g, i, j) = (tuple(p) for p in pick)
    depth[a] = 0
    depth[b] = -1.5
    depth[c] = np.inf
    rgba[d][0] = np.nan
    rgba[e][1] = np.inf
    normal[g] = 0
    albedo[i][:3] = 0
    rgba[j][3], rgba[a][3] = 3, 5
    return dict(rgba=rgba, depth=depth, normal=normal, albedo=albedo, id=np.stack([kind, index], axis=-1), moments=moments)


def rays(w, h, aspect):
    """(O, D, terms): the primary rays of an unrotated view at the origin, formed by inverting temporal_ref.reproject
    so that it lands their points on their own pixels, and the view's seven terms (eye, cos/sin pitch, cos/sin yaw)."""
    a = f32(aspect)
    half = f32(f32(w) * f32(0.5))
    x = ((((np.arange(w).astype(f32) + f32(0.5)) / half).astype(f32) * a).astype(f32) - f32(1)).astype(f32) * a
    y = ((((np.arange(h).astype(f32) + f32(0.5)) / half).astype(f32) * a).astype(f32) - f32(1)).astype(f32) * a
    D = np.ones((h, w, 3), dtype=f32)
    D[..., 0], D[..., 1] = x[None, :], y[:, None]
    D = (D / np.sqrt((D * D).sum(axis=-1, keepdims=True))).astype(f32)       # depth is the distance along a unit ray
    return np.zeros((h * w, 3), dtype=f32), D.reshape(-1, 3), (0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0)


def previous(cur, seed):
    """A history for `cur`: its guides with a few of them changed, another colour, lengths and moments."""
    rng = np.random.default_rng(seed)
    p = guides(seed, cur["depth"].shape[1], cur["depth"].shape[0])
    prev = dict(rgba=p["rgba"], moments=p["moments"], id=cur["id"].copy(), normal=cur["normal"].copy(),
                depth=(cur["depth"] * (f32(1) + (rng.random(cur["depth"].shape, dtype=f32) - f32(0.5)) * f32(0.03))).astype(f32))
    h, w = cur["depth"].shape
    prev["id"][h // 3, :, 1] += 1                                # a row of other objects
    prev["normal"][:, w // 3, :3] *= f32(-1)                     # a column that faces away
    return prev


def _put(out, name, value):
    if isinstance(value, np.ndarray):
        a = np.ascontiguousarray(value)
        out[name] = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()
    elif isinstance(value, (tuple, list)):
        out[name + "#"] = len(value)
        for i, v in enumerate(value):
            _put(out, f"{name}[{i}]", v)
    elif isinstance(value, dict):
        for k in sorted(value):
            _put(out, f"{name}.{k}", value[k])
    elif value is not None:
        out[name] = repr(value)


def digests():
    """{case: SHA-256 of dtype, shape and bytes} of every array the restatements return for the synthetic inputs."""
    R = _refs()
    out = {}
    for w, h in SHAPES:
        tag = f"{w}x{h}"
        cur = guides(1, w, h)
        g = (cur["rgba"], cur["depth"], cur["normal"], cur["albedo"], cur["id"])
        for name, kw in (("defaults", {}), ("colour", dict(sigma_colour=0.5, iterations=5)),
                         ("raw", dict(demodulate=False, normal_shift=2, sigma_depth=0.2))):
            _put(out, f"denoise/{tag}/{name}", R["denoise_ref"].denoise(*g, want_irradiance=True, **kw))
        for name, kw in (("spatial", {}), ("moments", dict(moments=cur["moments"])),
                         ("moments_raw", dict(moments=cur["moments"], demodulate=False, min_history=6, iterations=5))):
            _put(out, f"denoise_variance/{tag}/{name}", R["vdenoise_ref"].denoise_variance(*g, want_irradiance=True, **kw))
        aspect = 1.25
        O, D, terms = rays(w, h, aspect)
        prev = previous(cur, 2)
        other = (0.07, -0.03, 0.05, float(np.cos(0.01)), float(np.sin(0.01)), float(np.cos(0.02)), float(np.sin(0.02)))
        views = (("reset", None, terms, True), ("same", prev, terms, True), ("other", prev, other, False))
        for vname, hist, pterms, same in views:
            for wm in (True, False):
                r = R["temporal_ref"].temporal(cur, hist, O, D, terms, pterms, aspect, same, want_moments=wm, details=True)
                _put(out, f"temporal/{tag}/{vname}/moments{int(wm)}", r)
            if hist is not None:
                bare = dict(hist, moments=None)
                r = R["temporal_ref"].temporal(cur, bare, O, D, terms, pterms, aspect, same, max_history=8,
                                               depth_tolerance=0.1, normal_cos_min=0.5, details=True)
                _put(out, f"temporal/{tag}/{vname}/no_prev_moments", r)
        sph = np.array([[0.05, 0, 0], [0, 0, 0], [0, -0.04, 0.03]], dtype=f32)
        cub = np.array([[0, 0.06, 0, 9], [-0.05, 0.02, 0, 9], [0, 0, 0, 9]], dtype=f32)
        tables = (("none", {}), ("spheres", dict(sphere_motion=sph)), ("both", dict(sphere_motion=sph, cube_motion=cub)))
        for vname, hist, pterms, same in views:
            for tname, tkw in tables:
                for clamp in (True, False):
                    r = R["tmotion_ref"].temporal_motion(cur, hist, O, D, terms, pterms, aspect, same, clamp=clamp,
                                                        details=True, **tkw)
                    _put(out, f"temporal_motion/{tag}/{vname}/{tname}/clamp{int(clamp)}", r)
        r = R["tmotion_ref"].temporal_motion(cur, dict(prev, moments=None), O, D, terms, other, aspect, False,
                                             sphere_motion=sph, clamp_slack=0.0, clamp_history=20, max_history=24,
                                             want_moments=False, details=True)
        _put(out, f"temporal_motion/{tag}/other/spheres/tight", r)
        _put(out, f"tmotion_helpers/{tag}", dict(box=R["tmotion_ref"].box(cur["rgba"]),
                                                 displacement=R["tmotion_ref"].displacement(cur["id"], sph, cub),
                                                 reproject=R["temporal_ref"].reproject(cur["depth"], O, D, other, aspect, w, h)))
        lw, lh = (w + 1) // 2, (h + 1) // 2
        lo = {k: np.ascontiguousarray(v[::2, ::2]) for k, v in guides(1, w, h).items()}
        lo["rgba"] = guides(3, lw, lh)["rgba"]
        base = guides(4, w, h)["rgba"]
        select = dict(sphere=[1, 0, 1], cube=[0, 1], plane=[])
        for bname, b in (("nobase", None), ("base", base)):
            for sname, s in (("all", None), ("tables", select)):
                for dm in (True, False):
                    r = R["upsample_ref"].upsample(cur, lo, base=b, select=s, demodulate=dm, details=True)
                    _put(out, f"upsample/{tag}/{bname}/{sname}/demodulate{int(dm)}", r)
        _put(out, f"upsample/{tag}/bilinear", R["upsample_ref"].bilinear(lo["rgba"], w, h))
    return out


def test_the_restatements_return_the_pinned_bits():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = digests()
    assert sorted(got) == sorted(want)
    moved = [k for k in want if got[k] != want[k]]
    assert not moved, f"{len(moved)} of {len(want)} outputs moved, the first: {moved[:5]}"


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write the golden file (otherwise: compare with it)")
    ap.add_argument("--refs", help="directory to take the restatements from instead of tests/")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    if a.refs:
        sys.path.insert(0, os.path.abspath(a.refs))
    d = digests()
    if a.write:
        with open(a.out, "w") as f:
            f.write(json.dumps(d, indent=0, sort_keys=True) + "\n")
        print(f"wrote {len(d)} digests to {a.out}")
    else:
        with open(a.out) as f:
            print("same" if json.load(f) == d else "DIFFERENT")
