"""Hand-made guides for the indirect pass (rt_scene_indirect): G-buffers whose every pixel has an outcome
known beforehand, laid out so that the cast pass's slots show chosen wave patterns. numpy only.

The scene (scene_inputs): a camera at the origin looking along +z, one plane behind it at z = -100 facing +z, one small
sphere far off at (4000, 0, 3000), the synthetic sky. Every primary direction of the view has D.z > 0. A pixel is one of
  H  depth +5, normal (0, 0, -1): no flip, every gather direction has G.z < 0 and meets the plane;
  M  depth -200, the same normal: the start lies behind the plane, every gather ray leaves it and meets the sky;
  D  dead, by one of DEAD_REASONS (the k-th dead pixel of a mask takes reason k % len).
The k-th live pixel of a mask takes LIVE_NORMALS[k % len] as its normal guide; each behaves as (0, 0, -1) does.
tests/test_indirect_guides_cpu.py holds all of this against indirect_ref.pixels and query_ref.CastRef, and every mask
against the wave patterns it claims."""
from types import SimpleNamespace

import numpy as np

import postpass as P
from scenes import Scn

f32 = np.float32
H, M, D = 0, 1, 2
GROUP = 4                      # RT_INDIRECT_GROUP: the rays of one cast pass
WAVE = 64
PLANE_KIND = 2                 # RT_HIT_PLANE, the plane's index is 0
INT_MIN = -(1 << 31)
NAN, INF = float("nan"), float("inf")

# (name, what differs from an H pixel): kind, depth or normal
DEAD_REASONS = (("kind -1", dict(kind=-1)), ("kind INT_MIN", dict(kind=INT_MIN)),
                ("depth nan", dict(depth=NAN)), ("depth +inf", dict(depth=INF)), ("depth -inf", dict(depth=-INF)),
                ("normal 0", dict(normal=(0.0, 0.0, 0.0))), ("normal -0", dict(normal=(-0.0, 0.0, -0.0))),
                ("normal nan", dict(normal=(0.0, NAN, -1.0))), ("normal inf", dict(normal=(INF, 0.0, -1.0))),
                ("nn overflows", dict(normal=(0.0, 0.0, -2e19))), ("nn underflows", dict(normal=(0.0, 0.0, -1e-23))))
# normal.xyzw of live pixels: unit, long, nn = 1e38, nn subnormal, flipped by step 2, a fourth component nobody reads
LIVE_NORMALS = ((0.0, 0.0, -1.0, 0.0), (0.0, 0.0, -3.0, 0.0), (0.0, 0.0, -1e19, 0.0), (0.0, 0.0, -1e-20, 0.0),
                (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, -1.0, NAN))
DEPTH = {H: 5.0, M: -200.0}

# the calls of tests/test_indirect_guides_gpu.py, which tests/test_indirect_guides_cpu.py classifies beforehand
RAYS = (1, 4, 5, 16)
RAY_BASE, SEED = 3, 7
STALE_SIZE, STALE_RAYS = (50, 30), (8, 3)

SIZES = ((50, 30), (64, 4), (3, 1), (1, 1), (1, 70), (70, 1))
CONDITIONS = ("lane 0 only", "lane 63 only", "alternating", "full H", "full M", "full D", "gap", "straddle", "tail")


def scene_inputs(rt):
    """The scene of the module's docstring as tests/scenes.py Scn."""
    return Scn(rt, [(4000, 0, 3000, 1.0)], planes=[(0, 0, -100, 0, 0, 1)], cam=P.cam(rt, 0, 0, 0, 0, 0),
               lights=[((20, 20, 20), 20, 1.0, 0.5, 0.25)])


def view_aspect(rt, width, height):
    """The aspect a width x height frame of these guides is viewed with. The reference's dy grows with height / width
    (kernel.cu:1625), so a 1 x 70 frame under the default aspect looks almost straight up and down in its outer rows
    (D.z = 0.007) and a depth of -200 no longer lies behind the plane; a frame taller than wide takes the default times
    width / height, which gives its rows the range a square frame's have."""
    return float(f32(rt.default_aspect() * min(1.0, width / height)))


# ----------------------------------------------------------------------------- masks
def _wave(kind):
    w = np.full(WAVE, M, dtype=np.int8)
    if kind == "lane 0 only":
        w[0] = H
        w[5:40:7] = D
    elif kind == "lane 63 only":
        w[63] = H
        w[3:60:9] = D
    elif kind == "alternating":
        w[0::2] = H
    elif kind == "dm":                       # dead and missing pixels, no hit
        w[0::3] = D
    elif kind == "hd":
        w[0::2] = H
        w[1::4] = D
    elif kind in ("H", "M", "D"):
        w[:] = {"H": H, "M": M, "D": D}[kind]
    else:
        raise ValueError(kind)
    return w


def _patterns(npx):
    """1 500 pixels: nine waves of patterns, seeded mixtures, then the 28 pixels of the last, partial wave."""
    rng = np.random.default_rng(5)
    t = rng.choice(np.array([H, M, D], dtype=np.int8), size=npx, p=[0.12, 0.4, 0.48])
    order = ["lane 0 only", "lane 63 only", "alternating", "H", "M", "D", "hd", "dm", "hd"]
    for k, kind in enumerate(order):
        t[k * WAVE:(k + 1) * WAVE] = _wave(kind)
    t[npx - 1] = H
    return t


def _edges(npx):
    return np.concatenate([_wave(k) for k in ("lane 0 only", "dm", "lane 63 only", "H")])


def _fills(npx):
    return np.concatenate([_wave(k) for k in ("alternating", "M", "D", "H")])


def _strip(npx):
    """70 pixels: a hit, every dead reason, then hits and misses in turn up to a hit in the last pixel."""
    t = np.array([H if k % 2 == 0 else M for k in range(npx)], dtype=np.int8)
    t[1:1 + len(DEAD_REASONS)] = D
    t[npx - 1] = H
    return t


ALL = set(CONDITIONS)
# (width, height) -> name -> (types(npx), {g: the conditions its slots must show for groups of g rays})
MASKS = {
    (50, 30): {"patterns": (_patterns, {1: ALL - {"straddle"}, GROUP: ALL})},
    (64, 4): {"edges": (_edges, {g: {"lane 0 only", "lane 63 only", "full H", "gap"} for g in (1, GROUP)}),
              "fills": (_fills, {g: {"alternating", "full M", "full D", "full H"} for g in (1, GROUP)})},
    (3, 1): {"hmh": (lambda n: np.array([H, M, H], dtype=np.int8), {1: {"tail"}, GROUP: {"tail", "straddle"}}),
             "mmh": (lambda n: np.array([M, M, H], dtype=np.int8), {1: {"tail"}, GROUP: {"tail"}})},
    (1, 1): {"h": (lambda n: np.array([H], dtype=np.int8), {1: {"tail"}, GROUP: {"tail", "straddle"}}),
             "m": (lambda n: np.array([M], dtype=np.int8), {1: set(), GROUP: set()})},
    (1, 70): {"strip": (_strip, {1: {"tail"}, GROUP: {"tail", "straddle"}})},
    (70, 1): {"strip": (_strip, {1: {"tail"}, GROUP: {"tail", "straddle"}})},
}


def cases():
    """(width, height, mask name) of every mask."""
    return [(w, h, name) for (w, h), ms in MASKS.items() for name in ms]


def conditions(types, g):
    """The CONDITIONS that the slots of a group of g rays show: slot i = j * npx + p, wave i // 64, a slot hits iff
    its pixel is H."""
    types = np.asarray(types)
    npx = len(types)
    n = g * npx
    slot = np.tile(types, g)
    ray = np.repeat(np.arange(g), npx)
    waves = [(slot[a:a + WAVE], ray[a:a + WAVE]) for a in range(0, n, WAVE)]
    has_h = [bool((t == H).any()) for t, _ in waves]
    found = set()
    for k, (t, r) in enumerate(waves):
        full = len(t) == WAVE
        hit = t == H
        if full and hit[0] and hit.sum() == 1:
            found.add("lane 0 only")
        if full and hit[63] and hit.sum() == 1:
            found.add("lane 63 only")
        if full and (np.array_equal(t[0::2], np.full(32, H)) and np.array_equal(t[1::2], np.full(32, M)) or
                     np.array_equal(t[0::2], np.full(32, M)) and np.array_equal(t[1::2], np.full(32, H))):
            found.add("alternating")
        for name, v in (("full H", H), ("full M", M), ("full D", D)):
            if full and (t == v).all():
                found.add(name)
        if not hit.any() and (t == D).any() and (t == M).any() and 0 < k < len(waves) - 1 and has_h[k - 1] and has_h[k + 1]:
            found.add("gap")
        for j in np.unique(r)[:-1]:
            if hit[r == j].any() and hit[r == j + 1].any():
                found.add("straddle")
    if n % WAVE and slot[n - 1] == H:
        found.add("tail")
    return found


# ----------------------------------------------------------------------------- guides
def guides(width, height, types, seed=1):
    """Flat guides of a width x height frame whose pixel p is of type types[p]: depth [m], normal [m, 4], id [m, 2],
    albedo [m, 4], rgba_in [m, 4]; `types`, `reason` (index into DEAD_REASONS, -1 for live pixels) and `live_normal`
    (index into LIVE_NORMALS, -1 for dead ones)."""
    types = np.asarray(types, dtype=np.int8)
    m = width * height
    assert types.shape == (m,)
    depth = np.empty(m, dtype=f32)
    normal = np.empty((m, 4), dtype=f32)
    ids = np.empty((m, 2), dtype=np.int32)
    reason = np.full(m, -1, dtype=np.int32)
    live_normal = np.full(m, -1, dtype=np.int32)
    n_dead = n_live = 0
    with np.errstate(all="ignore"):
        for p in range(m):
            if types[p] == D:
                r = n_dead % len(DEAD_REASONS)
                n_dead += 1
                how = DEAD_REASONS[r][1]
                reason[p] = r
                depth[p] = how.get("depth", DEPTH[H])
                normal[p] = (*how.get("normal", (0.0, 0.0, -1.0)), 0.0)
                ids[p] = (how.get("kind", PLANE_KIND), 0)
            else:
                k = n_live % len(LIVE_NORMALS)
                n_live += 1
                live_normal[p] = k
                depth[p] = DEPTH[int(types[p])]
                normal[p] = LIVE_NORMALS[k]
                ids[p] = (PLANE_KIND, 0) if types[p] == H else (1 + p % 3, p)
    rng = np.random.default_rng(seed)
    albedo = (f32(0.05) + f32(0.9) * rng.random((m, 4), dtype=f32)).astype(f32)
    rgba_in = rng.random((m, 4), dtype=f32)
    return SimpleNamespace(width=width, height=height, types=types, reason=reason, live_normal=live_normal, depth=depth,
                           normal=normal, id=ids, albedo=albedo, rgba_in=rgba_in)


def masked(width, height, name, seed=1):
    """The guides of mask `name` of MASKS[(width, height)]."""
    return guides(width, height, MASKS[(width, height)][name][0](width * height), seed)


def uniform(width, height, kind, seed=1):
    """Guides whose every pixel is of one type."""
    return guides(width, height, np.full(width * height, kind, dtype=np.int8), seed)
