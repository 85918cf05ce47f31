"""Hand-made guides for the diffuse paths of rt_scene_indirect_paths, in the manner of
tests/indirect_guides.py, whose guide builder they use: every pixel's outcome at bounce 0 and at bounce 1 is known
beforehand, and the pixels are laid out so that the queue entering bounce 1 -- the second compaction -- shows chosen
wave patterns. numpy only.

The scene (scene_inputs): a camera at the origin looking along +z, every primary direction with D.z > 0; three planes
  A   z = -100 facing +z,     A'  z = -101 facing -z,     C   z = -300 facing +z,
one small sphere far off, the synthetic sky. A live pixel's normal guide is (0, 0, -1) in effect, so its gather rays
run towards -z; a hit's next ray runs into the half space of the hit plane's normal. A pixel is one of
  CONT  depth -200: the start lies between A' and C; the gather ray meets C, the next ray (+z) meets A', the one
        after that (-z) meets C again, and so on: a hit at every bounce;
  STOP  depth +5: the gather ray meets A; the next ray (+z) starts in front of A and A', and meets the sky;
  MISS  depth -2000: the start lies behind C; the gather ray meets the sky;
  DEAD  dead, by indirect_guides' reasons.
tests/test_indirect_paths_cpu.py holds all of this against query_ref.CastRef, and every mask against its claims.

The patterns are those of the slots' order. The cast pass appends a wave's hits to queue 0 as one run, in the order
the waves' atomics arrive: where every wave of the cast pass is full of hits (CONT and STOP pixels only, a pixel count
that is a multiple of 64) queue 0 is those waves, whole and aligned, in some order, and a wave of the bounce-0 pass
sees exactly one of the patterns below in its continuing lanes. At the sizes of a single wave the order is the slots'."""
import numpy as np

import indirect_guides as IG
import postpass as P
from scenes import Scn

f32 = np.float32
CONT, STOP, MISS, DEAD = 0, 1, 2, 3
WAVE = 64
MISS_DEPTH = -2000.0
RAYS = (1, 4, 5)
BOUNCES = 3
RAY_BASE, SEED = 3, 7
PATTERNS = ("lane 0 only", "lane 63 only", "alternating", "none between", "full")


def scene_inputs(rt, **kw):
    kw.setdefault("lights", [((20, 20, 20), 20, 1.0, 0.5, 0.25)])
    return Scn(rt, [(4000, 0, 3000, 1.0)], planes=[(0, 0, -100, 0, 0, 1), (0, 0, -101, 0, 0, -1), (0, 0, -300, 0, 0, 1)],
               cam=P.cam(rt, 0, 0, 0, 0, 0), **kw)


def guides(width, height, types, seed=1):
    """indirect_guides.guides for pixel types of this module (`kinds` keeps them): CONT takes its M pixel (depth -200),
    STOP its H pixel (depth +5), MISS an M pixel moved behind C."""
    types = np.asarray(types, dtype=np.int8)
    to_ig = np.array([IG.M, IG.H, IG.M, IG.D], dtype=np.int8)
    g = IG.guides(width, height, to_ig[types], seed)
    g.depth[types == MISS] = f32(MISS_DEPTH)
    g.kinds = types
    return g


def _wave(kind):
    w = np.full(WAVE, STOP, dtype=np.int8)
    if kind == "lane 0 only":
        w[0] = CONT
    elif kind == "lane 63 only":
        w[63] = CONT
    elif kind == "alternating":
        w[0::2] = CONT
    elif kind == "full":
        w[:] = CONT
    elif kind != "none":
        raise ValueError(kind)
    return w


def _cat(*kinds):
    return lambda npx: np.concatenate([_wave(k) for k in kinds])


def _mixed(npx):
    """1 500 pixels of every type, seeded: waves that are not full of hits, a partial last wave."""
    t = np.random.default_rng(8).choice(np.array([CONT, STOP, MISS, DEAD], dtype=np.int8), size=npx, p=[0.3, 0.3, 0.2, 0.2])
    t[npx - 1] = CONT
    return t


# (width, height) -> name -> (types(npx), the PATTERNS its waves show, the length of the queue entering bounce 1 at one ray)
MASKS = {
    (64, 4): {"edges": (_cat("lane 0 only", "none", "lane 63 only", "full"), {"lane 0 only", "lane 63 only", "none between", "full"}, 66),
              "fills": (_cat("alternating", "none", "alternating", "full"), {"alternating", "none between", "full"}, 128)},
    (1, 1): {"one": (lambda n: np.array([CONT], dtype=np.int8), set(), 1)},
    (3, 1): {"last": (lambda n: np.array([STOP, MISS, CONT], dtype=np.int8), set(), 1)},
    (63, 1): {"all": (lambda n: np.full(63, CONT, dtype=np.int8), set(), 63)},
    (65, 1): {"all": (lambda n: np.full(65, CONT, dtype=np.int8), {"full"}, 65)},    # the bounce-0 pass's tail wave has one live lane
    (50, 30): {"mixed": (_mixed, set(), None)},
}


def cases():
    return [(w, h, name) for (w, h), ms in MASKS.items() for name in ms]


def masked(width, height, name, seed=1):
    return guides(width, height, MASKS[(width, height)][name][0](width * height), seed)


def patterns(types):
    """The PATTERNS that the full waves of hits (CONT and STOP only) of one ray's slots show in their CONT lanes."""
    types = np.asarray(types)
    waves = [types[a:a + WAVE] for a in range(0, len(types) - WAVE + 1, WAVE)]
    full_hit = [bool(np.isin(w, (CONT, STOP)).all()) for w in waves]
    some = [bool((w == CONT).any()) for w in waves]
    found = set()
    for k, w in enumerate(waves):
        if not full_hit[k]:
            continue
        c = w == CONT
        if c[0] and c.sum() == 1:
            found.add("lane 0 only")
        if c[63] and c.sum() == 1:
            found.add("lane 63 only")
        if c[0::2].all() and not c[1::2].any() or c[1::2].all() and not c[0::2].any():
            found.add("alternating")
        if c.all():
            found.add("full")
        if not c.any() and 0 < k < len(waves) - 1 and some[k - 1] and some[k + 1]:
            found.add("none between")
    return found


def counts(types, rays, bounces):
    """rt_debug_indirect_path_counts for these guides: per group of rays, per bounce."""
    types = np.asarray(types)
    hit0, cont = int(np.isin(types, (CONT, STOP)).sum()), int((types == CONT).sum())
    return [[min(IG.GROUP, rays - j0) * (hit0 if b == 0 else cont) for b in range(bounces)] for j0 in range(0, rays, IG.GROUP)]


# ----------------------------------------------------------------------------- the ladder
def ladder_inputs(rt):
    """The scene under a constant sky s = 0.75, a constant texture a = 0.5 and lights of colour 0."""
    sky = [np.full((8, 16), 0.75, dtype=np.float32)] * 3
    tex = [np.full((8, 8), 0.5, dtype=np.float32)] * 3
    return scene_inputs(rt, sky=sky, tex=tex, lights=[((20, 20, 20), 20, 0.0, 0.0, 0.0)])


def ladder_check(rgb, det, bounces, s=0.75):
    """rgb [m, 3] of a call with one ray, strength 1, no albedo and no rgba_in against the details of the restatement:
    every live pixel is exactly s * 0.5^k with k its path's hit count, or exactly 0 when the budget ended the path at a
    hit. Returns the ks seen."""
    k = det["hits"][0]
    want = np.where(k >= bounces, f32(0), (f32(s) * np.power(f32(0.5), k.astype(np.float32))).astype(np.float32))
    got = np.ascontiguousarray(rgb, dtype=np.float32)[det["idx"]]
    bad = (P.bits(got) != P.bits(np.repeat(want[:, None], 3, axis=1))).any(axis=1)
    assert not bad.any(), (int(bad.sum()), det["idx"][bad][:8], got[bad][:2], want[bad][:2])
    return set(k.tolist())


# ----------------------------------------------------------------------------- the dark corner
CORNER = dict(w=16, h=8, rays=8, seed=3)


def corner_inputs(rt):
    """A black sky; a sphere (constructor radius 6.5: the radius is its square, 42.25) below the pixels' surface points,
    whose near side faces away from the one light, far down the -z axis; a plane above that faces the light. A gather ray
    that meets the sphere finds it dark, to the bit (the light lies behind the surface: max(dot, 0) = 0); its next ray
    meets the plane, which the light reaches everywhere but in the sphere's small shadow, or the black sky."""
    sky = [np.zeros((8, 16), dtype=np.float32)] * 3
    return Scn(rt, [(0, 0, -60, 6.5)], planes=[(0, 0, 200, 0, 0, -1)], cam=P.cam(rt, 0, 0, 0, 0, 0), sky=sky,
               lights=[((0, 0, -1000), 20, 1.0, 0.5, 0.25)])


def corner_guides():
    """Every pixel a surface point at depth +5 whose gather rays run towards -z (indirect_guides' H pixel)."""
    return IG.uniform(CORNER["w"], CORNER["h"], IG.H)


def corner_lit(det):
    """Of the restatement's details at bounces >= 2: the live pixels with a path that shaded two hits (the sphere, then
    the plane)."""
    return np.max(np.stack(det["hits"]), axis=0) >= 2
