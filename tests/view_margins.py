"""Scenes placed on the margins of the per-view candidate lists (the exactness-ledger row "a tile's
primary list taken from its block's view list"), in the style of tests/margins.py: each builder takes (rt, oracle, seed)
and returns a ViewMargin with a WITNESS.

Witnesses come from the reference's arithmetic and the HOST builder only, never from the device: primary rays from
oracle_primary_ray with the sample offsets of rt_sample_offset, hits from margins.quad (sphere::intersect in binary32)
and query_ref.CastRef, blocks, cones, flags and lists from rt.view_lists_host(..., want_beams=True); the unpadded
corner cone is the binary64 restatement of tests/test_view_lists_cpu.py, which that file holds against the host
builder. Every scene has 64 spheres or more (fillers behind the camera), so that it has eye cones and its culled
frames read the lists. tests/test_view_margins_cpu.py checks that every witness is non-empty and on its bound;
tests/test_view_margins_gpu.py renders the scenes with the lists on, off, brute force and through the oracle.
"""
import ctypes as C

import numpy as np

import margins as M
from margins import Margin, _unit, f32, inputs, quad, table

KCAP = 0.1                          # RT_CONE_KCAP (rt_tables.h): eye cones at or below this slope, the 3-D blocks above
PAD_REL, PAD_ABS = 4.0e-6, 8.0e-5   # RT_PAD_REL, RT_PAD_ABS (rt_device.h)
VIEW_OVERFLOW, VIEW_NOT_BUILT = 1, 2


class ViewMargin(Margin):
    """A Margin with the launch it is meant for: samples per pixel, the band of rows (y0, y1) that holds the witness
    (None: the whole frame) and the tile widths whose tiles nest in the view's blocks."""

    def __init__(self, *a, spp=1, band=None, tiles=(8,)):
        super().__init__(*a)
        self.spp, self.band, self.tiles = spp, band, tiles


# ---------------------------------------------------------------------------------------------- rays, blocks, cones
def camera(rt, cam):
    return rt.Camera(rt.Vec3(*[float(v) for v in cam[0]]), rt.Vec3(0, 0, 1), 0.0, float(cam[1]), float(cam[2]))


def frame_desc(rt, m):
    fd = rt.FrameDesc()
    fd.struct_size = C.sizeof(rt.FrameDesc)
    fd.width, fd.height = m.w, m.h
    fd.aspect = m.aspect
    fd.cam = camera(rt, m.cam)
    fd.opts.struct_size = C.sizeof(rt.LaunchOpts)
    fd.opts.cull = 1
    return fd


def offsets(rt, spp):
    lib = rt.load_library()
    out = []
    for k in range(spp):
        ox, oy = C.c_double(), C.c_double()
        assert lib.rt_sample_offset(k, spp, C.byref(ox), C.byref(oy)) == 0
        out.append((ox.value, oy.value))
    return out


def rays(oracle, cam, aspect, w, h, pixels, offs=((0.5, 0.5),)):
    """The oracle's primary rays of pixels x sample offsets -> O, D float32 [len(pixels) * len(offs), 3]."""
    lib = oracle.load()
    ocam = C.cast(C.pointer(cam), C.POINTER(oracle.OCamera))
    r = oracle.ORay()
    O = np.empty((len(pixels) * len(offs), 3), dtype=np.float32)
    D = np.empty_like(O)
    k = 0
    for (x, y) in pixels:
        for (ox, oy) in offs:
            lib.oracle_primary_ray(int(x), int(y), w, h, aspect, ocam, ox, oy, C.byref(r))
            O[k] = (r.Org.x, r.Org.y, r.Org.z)
            D[k] = (r.Dir.x, r.Dir.y, r.Dir.z)
            k += 1
    return O, D


def host_view(rt, m):
    """The host builder's summary, lists and beams of the margin's frame."""
    inp = inputs(rt, m)
    return rt.view_lists_host(inp.spheres, inp.n, frame_desc(rt, m), want_beams=True)


def block_of(v, x, y):
    sh = v["block_w"].bit_length() - 1
    return (y >> sh) * v["blocks_x"] + (x >> sh)


def block_rect(v, b, w, h):
    bw, bh, nbx = v["block_w"], v["block_h"], v["blocks_x"]
    bx, by = b % nbx, b // nbx
    return bx * bw, by * bh, min((bx + 1) * bw, w), min((by + 1) * bh, h)


def corner_cone(rt, m, rect):
    """The block's cone as DESIGN.md states it, in binary64: unit axis, padded slope (NaN where the padded sine
    reaches 1) and the UNPADDED sine of the corner directions at the pixel edges."""
    from test_view_lists_cpu import _numpy_block_cone
    with np.errstate(all="ignore"):
        return _numpy_block_cone(camera(rt, m.cam), f32(m.aspect), m.w, m.h, *rect)


def sin_dev(d, u):
    return float(np.linalg.norm(np.cross(np.asarray(d, dtype=np.float64), np.asarray(u, dtype=np.float64))))


def member_slack(beam, org, ent):
    """view_member_host (rt_tables.hip) restated in binary64 -> rad^2 1.0005 / d2 - 1: how far, relative, the squared
    distance of the centre from the block's axis stays below what the member test admits (reported, decides nothing)."""
    u, k = beam[:3].astype(np.float64), float(beam[3])
    v = ent[:3].astype(np.float64) - np.asarray(org, dtype=np.float64)
    vv, sa = float(v @ v), float(v @ u)
    d2 = max(vv - sa * sa, 0.0)
    rc = np.sqrt(float(ent[3]) + PAD_REL * vv + PAD_ABS) * 1.0001
    reach = sa + rc
    rad = k * max(reach, 0.0) + 1.0e-4 + rc
    return float(rad * rad * 1.0005 / d2 - 1.0) if d2 > 0 else float("inf")


def fillers(rng, org, fwd, k):
    """k small spheres 40 ... 80 units behind the ray origin (fwd: the centre pixel's direction): never seen, never on
    a list; a scene has eye cones, and its frames read view lists, from 64 spheres on."""
    org, fwd = np.asarray(org, dtype=np.float64), np.asarray(fwd, dtype=np.float64)
    return [(*(org - fwd * rng.uniform(40, 80) + _unit(rng) * 8.0), 0.1) for _ in range(k)]


def nearest(rt, oracle, m, O, D):
    import query_ref
    return query_ref.CastRef(oracle, inputs(rt, m)).nearest(O, D)


def _mix(rng, special, fill):
    """The special spheres at random list positions among the fillers -> spheres, positions of the special ones."""
    n = len(special) + len(fill)
    pos = sorted(int(p) for p in rng.choice(n, size=len(special), replace=False))
    out, fi = [None] * n, iter(fill)
    for p, s in zip(pos, special):
        out[p] = s
    return [s if s is not None else next(fi) for s in out], pos


# ---------------------------------------------------------------------------------------------- rows 1 and 2: the corner cone
PLACES = ("tl", "tr", "bl", "br", "l", "r", "t", "b")
# frame, which block (interior / at the frame's border on the witness's side / clipped by the frame), tiles that nest
CORNER_FRAMES = ((64, 48, "interior", (8,)), (64, 48, "border", (8,)), (60, 44, "clipped", (8,)), (52, 36, "clipped", (8,)),
                 (1920, 1080, "interior", (8, 16, 32, 64)), (1920, 1080, "clipped", (8, 16, 32, 64)))


def _pick_block(rng, v, kind, place):
    nbx, nby = v["blocks_x"], v["blocks_y"]
    if kind == "interior":
        return int(rng.integers(1, nbx - 1)), int(rng.integers(1, nby - 1))
    if kind == "clipped":        # 60 x 44, 52 x 36: the last column and row are 4 pixels; 1920 x 1080: the last row is 56
        if v["block_w"] * nbx == 1920:
            return int(rng.integers(1, nbx - 1)), nby - 1
        return (nbx - 1, nby - 1) if place in PLACES[:4] else (nbx - 1, int(rng.integers(0, nby))) if place in "lr" \
            else (int(rng.integers(0, nbx)), nby - 1)
    # border: the witness's side of the block is the frame's
    bx = 0 if "l" in place else nbx - 1 if "r" in place else int(rng.integers(0, nbx))
    by = 0 if "t" in place else nby - 1 if place in ("bl", "br", "b") else int(rng.integers(0, nby))
    return bx, by


def _place_pixel(place, rect):
    """The block's pixel at `place`, its neighbour towards the block's inside, and the offset's distance from the
    block's outer edge(s) there as a function of (ox, oy)."""
    x0, y0, x1, y1 = rect
    xm, ym = (x0 + x1) // 2, (y0 + y1) // 2
    x = x0 if "l" in place else x1 - 1 if "r" in place else xm
    y = y0 if "t" in place else y1 - 1 if place in ("bl", "br", "b") else ym
    ix = 1 if "l" in place else -1 if "r" in place else 0
    iy = 1 if "t" in place else -1 if place in ("bl", "br", "b") else 0

    def edge_dist(ox, oy):
        dx = ox if ix > 0 else 1 - ox if ix < 0 else 0.0
        dy = oy if iy > 0 else 1 - oy if iy < 0 else 0.0
        return dx + dy + (1e-3 * (abs(ox - 0.5) + abs(oy - 0.5)))      # ties: the sample nearest the pixel's middle
    return (x, y), (x + ix, y + iy), edge_dist


def _corner(rt, oracle, row, seed, frame, place, spp, base):
    """A sphere whose centre direction lies OUTSIDE the unpadded corner cone of a block and that the sample nearest the
    block's outer edge of the block's pixel at `place` still hits, grazing it from the neighbour's side."""
    w, h, kind, tiles = frame
    rng = np.random.default_rng(base + seed)
    offs = offsets(rt, spp)
    for attempt in range(40):
        aspect = float(f32(rng.uniform(0.75, 1.0) if w < 100 else rng.uniform(0.8, 1.2)))
        cam = (tuple(rng.uniform(-5, 5, 3)), float(rng.uniform(0, 360)), float(rng.uniform(-40, 40)))
        cs = camera(rt, cam)
        m0 = ViewMargin(row, seed, [(0.0, 0.0, 0.0, 0.1)] * 64, [], cam, aspect, w, h, {})
        v = rt.view_lists_host(inputs(rt, m0).spheres, 64, frame_desc(rt, m0), want_lists=False, want_beams=True)
        bx, by = _pick_block(rng, v, kind, place)
        b = by * v["blocks_x"] + bx
        rect = block_rect(v, b, w, h)
        beam = v["beams"][b].astype(np.float64)
        if beam[3] <= 0:
            continue
        u, _, s = corner_cone(rt, m0, rect)
        pix, inner, edge_dist = _place_pixel(place, rect)
        ks = int(np.argmin([edge_dist(ox, oy) for ox, oy in offs]))
        O, Dk = rays(oracle, cs, aspect, w, h, [pix, inner], [offs[ks]])
        org, d0 = O[0].astype(np.float64), Dk[0].astype(np.float64)
        out = d0 - Dk[1].astype(np.float64)
        out -= (out @ d0) * d0
        out /= np.linalg.norm(out)
        margin = (1e-3, 1e-2, 5e-2)[int(rng.integers(0, 3))]

        def cdir(alpha):
            return d0 * np.cos(alpha) + out * np.sin(alpha)
        lo, hi = 0.0, 1.2           # the smallest angle from the sample's ray at which the centre leaves the cone
        if sin_dev(cdir(hi), beam[:3]) < s * (1 + margin):
            continue
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if sin_dev(cdir(mid), beam[:3]) >= s * (1 + margin) else (mid, hi)
        alpha = hi
        L = float(rng.uniform(10, 40))
        fwd = rays(oracle, cs, aspect, w, h, [(w // 2, h // 2)])[1][0]
        back = [(*(org + rays(oracle, cs, aspect, w, h, [(int(rng.integers(0, w)), int(rng.integers(0, h)))])[1][0]
                   * rng.uniform(60, 100)), float(np.sqrt(rng.uniform(2, 5)))) for _ in range(3)]
        fill = fillers(rng, org, fwd, 62)
        for graze in (2e-3, 1e-2, 5e-2, 0.2, 0.5):
            R = L * np.sin(alpha) * (1 + graze)
            S = (*(org + cdir(alpha) * L), float(np.sqrt(R)))
            spheres, pos = _mix(rng, [S] + back, fill)
            m = ViewMargin(row, seed, spheres, [(tuple(_unit(rng) * 40), 15.0, 1.0, 0.9, 0.7), ((3.0, 30.0, -8.0), 8.0, 0.3, 0.5, 1.0)],
                           cam, aspect, w, h, {}, spp=spp, tiles=tiles,
                           band=None if h < 100 else (pix[1] // 16 * 16, min(pix[1] // 16 * 16 + 16, h)))
            m.witness = corner_witness(rt, oracle, m, pos[0], pix, b, place)
            wit = m.witness
            # (accepted on the reference's arithmetic alone; that the host builder lists the sphere is for the CPU
            # test to assert, so that a builder that drops it is shown the same scene and not a looser one)
            if wit["pixels"] and wit["dev"] > wit["sin_corner"] and (spp == 1 or not wit["centre_hits"]):
                return m
    raise AssertionError(f"{row}: no scene on the bound for seed {seed}")


def corner_witness(rt, oracle, m, si, pix, b, place):
    """The samples of pixel `pix` (of block b) whose closest hit, by the reference's arithmetic, is sphere si; where the
    sphere's centre lies against the block's corner cone and its padded cone; its standing in the host list of b."""
    offs = offsets(rt, m.spp)
    cs = camera(rt, m.cam)
    v = host_view(rt, m)
    assert block_of(v, *pix) == b
    rect = block_rect(v, b, m.w, m.h)
    _, edge_dist = _place_pixel(place, rect)[1:]
    O, D = rays(oracle, cs, m.aspect, m.w, m.h, [pix], offs + [(0.5, 0.5)])
    rec = nearest(rt, oracle, m, O, D)
    tab = table(m.spheres)
    own = (rec["kind"] == 1) & (rec["index"] == si) & quad(tab[si:si + 1], O, D)["hit"][:, 0]
    hit_samples = [k for k in range(m.spp) if own[k]]
    dist = [edge_dist(*o) for o in offs]
    beam = v["beams"][b]
    u, k_pred, s = corner_cone(rt, m, rect)
    count, flags, ent, pos, lbs = v["lists"][b]
    k = float(beam[3])
    return {"pixels": [pix] if hit_samples else [], "block": b, "rect": rect, "sphere": si, "place": place,
            "hit_samples": hit_samples, "nearest_samples": [i for i, d in enumerate(dist) if d - min(dist) < 0.01],
            "centre_hits": bool(own[m.spp]), "dev": sin_dev(tab[si, :3].astype(np.float64) - O[0].astype(np.float64), beam[:3])
            / float(np.linalg.norm(tab[si, :3].astype(np.float64) - O[0].astype(np.float64))),
            "sin_corner": float(s), "sin_padded": k / np.sqrt(1 + k * k), "k": k, "k_predicted": float(k_pred),
            "flags": int(flags), "on_list": si in pos.tolist(), "list_position": pos.tolist().index(si) if si in pos.tolist() else -1,
            "slack": member_slack(beam, O[0], tab[si]) if k > 0 else None,
            # the same against the cone without its pad: what is left were the x 1.01 + 1e-5 dropped
            "slack_unpadded": member_slack(np.array([*beam[:3], s / np.sqrt(1 - s * s)]), O[0], tab[si])}


def view_corner(rt, oracle, seed):
    """Row 1: one sample per pixel, the pixel's middle. Seeds run over the eight places (four corners, four edges) and
    the six frames of CORNER_FRAMES."""
    return _corner(rt, oracle, "view_corner", seed, CORNER_FRAMES[(seed // 8) % len(CORNER_FRAMES)], PLACES[seed % 8], 1, 1000)


def view_sample_edge(rt, oracle, seed):
    """Row 2: 4 and 16 samples per pixel; only samples nearest the block's outer pixel edge hit the sphere, the pixel's
    middle misses it (so no one-sample frame sees it in that block). Witness: which sample indices hit."""
    place = PLACES[seed % 8]
    spp = (4, 16)[(seed // 8) % 2]
    frame = CORNER_FRAMES[(seed + seed // 8 + 2 * (seed // 16)) % len(CORNER_FRAMES)]
    return _corner(rt, oracle, "view_sample_edge", seed, frame, place, spp, 2000)


# ---------------------------------------------------------------------------------------------- rows 3 and 4: flags, slopes
def _per_block_scene(rt, oracle, row, seed, w, h, aspect, cam, rng, extra=()):
    """One sphere on the ray of every block's middle pixel, a third of the block across, and fillers."""
    cs = camera(rt, cam)
    m0 = ViewMargin(row, seed, [(0.0, 0.0, 0.0, 0.1)] * 64, [], cam, aspect, w, h, {})
    v = rt.view_lists_host(inputs(rt, m0).spheres, 64, frame_desc(rt, m0), want_lists=False)
    vis = []
    for b in range(v["blocks"]):
        x0, y0, x1, y1 = block_rect(v, b, w, h)
        O, D = rays(oracle, cs, aspect, w, h, [((x0 + x1) // 2, (y0 + y1) // 2), (x0, y0)])
        L = float(rng.uniform(8, 30))
        R = L * float(np.linalg.norm(D[0].astype(np.float64) - D[1].astype(np.float64))) * 0.33
        vis.append((*(O[0].astype(np.float64) + D[0].astype(np.float64) * L), float(np.sqrt(R))))
    fwd = rays(oracle, cs, aspect, w, h, [(w // 2, h // 2)])[1][0]
    vis += list(extra)
    spheres, pos = _mix(rng, vis, fillers(rng, O[0], fwd, max(64 - len(vis), 16)))
    lights = [(tuple(_unit(rng) * 40), 15.0, 1.0, 0.9, 0.7), ((3.0, 30.0, -8.0), 8.0, 0.3, 0.5, 1.0)]
    return ViewMargin(row, seed, spheres, lights, cam, aspect, w, h, {}), pos


def _hit_pixels_by_block(rt, oracle, m, v):
    cs = camera(rt, m.cam)
    px = [(x, y) for y in range(m.h) for x in range(m.w)]
    O, D = rays(oracle, cs, m.aspect, m.w, m.h, px)
    rec = nearest(rt, oracle, m, O, D)
    out = {}
    for p in np.nonzero(rec["kind"] == 1)[0]:
        out.setdefault(block_of(v, *px[p]), []).append(px[p])
    return out


NOT_BUILT_FRAMES = ((16, 16, None), (32, 24, 1.3), (32, 24, 1.6), (16, 16, None), (28, 20, 1.45))


def view_not_built(rt, oracle, seed):
    """Row 3: frames whose blocks span too wide an angle for a cone (sin^2 >= 0.25): 16 x 16 at the default aspect, where
    EVERY block is RT_VIEW_NOT_BUILT, and small frames of a larger aspect where built and unbuilt blocks coexist.
    Witness: the per-block flags of the host builder, the flags predicted from the corner cone, and the pixels that hit
    a sphere inside an unbuilt block (and inside a built one)."""
    rng = np.random.default_rng(3000 + seed)
    w, h, aspect = NOT_BUILT_FRAMES[seed % len(NOT_BUILT_FRAMES)]
    aspect = float(rt.default_aspect() if aspect is None else f32(aspect))
    cam = ((4.0, 3.0, 10.0), 180.0, -20.0) if seed == 0 else (tuple(rng.uniform(-5, 5, 3)), float(rng.uniform(0, 360)), float(rng.uniform(-40, 40)))
    m, _ = _per_block_scene(rt, oracle, "view_not_built", seed, w, h, aspect, cam, rng)
    v = host_view(rt, m)
    flags = [l[1] for l in v["lists"]]
    pred = [VIEW_NOT_BUILT if not (corner_cone(rt, m, block_rect(v, b, w, h))[2] ** 2 < 0.25) else 0 for b in range(v["blocks"])]
    hits = _hit_pixels_by_block(rt, oracle, m, v)
    unbuilt = [p for b, px in hits.items() if flags[b] & VIEW_NOT_BUILT for p in px]
    built = [p for b, px in hits.items() if flags[b] == 0 for p in px]
    m.witness = {"pixels": unbuilt, "built_pixels": built, "flags": flags, "predicted": pred,
                 "not_built": v["not_built"], "blocks": v["blocks"], "all": seed % len(NOT_BUILT_FRAMES) in (0, 3)}
    return m


KCAP_FRAMES = ((64, 48, 0.88), (60, 44, None), (52, 36, 0.8), (64, 48, 0.9))


def view_kcap(rt, oracle, seed):
    """Row 4: a frame in which some blocks have a slope <= RT_CONE_KCAP (the builder culls them through the eye cones)
    and others a larger one (through the 3-D block table), spheres hit in both kinds. The two instantiations keep the
    same spheres except in a sliver: the eye cone of a sphere is padded for slopes up to KCAP, rc (1 + KCAP), where the
    member test of a block of slope k admits rc (1 + k). 31 copies of one large, distant sphere (so that one whole block
    of 16 of the eye-cone table holds nothing else) stand in that sliver of one block above KCAP.
    Witness: the slopes, the two sets of blocks, hit pixels in both, the sliver block and whether the host builder
    lists the sliver sphere there."""
    rng = np.random.default_rng(4000 + seed)
    w, h, aspect = KCAP_FRAMES[seed % len(KCAP_FRAMES)]
    aspect = float(rt.default_aspect() if aspect is None else f32(aspect))
    cam = (tuple(rng.uniform(-5, 5, 3)), float(rng.uniform(0, 360)), float(rng.uniform(-40, 40)))
    m0, _ = _per_block_scene(rt, oracle, "view_kcap", seed, w, h, aspect, cam, rng)
    v0 = host_view(rt, m0)
    k0 = v0["beams"][:, 3].astype(np.float64)
    bs = int(np.argmax(k0))                                   # the widest block
    u, k = v0["beams"][bs, :3].astype(np.float64), float(k0[bs])
    cs = camera(rt, cam)
    org = rays(oracle, cs, aspect, w, h, [(0, 0)])[0][0].astype(np.float64)
    side = np.cross(u, _unit(rng)); side /= np.linalg.norm(side)
    L, rho = 300.0, 0.4
    R = L * np.sin(rho)
    rc = np.sqrt(R * R + PAD_REL * L * L + PAD_ABS) * 1.0001
    # the widest angle from the block's axis the eye-cone instantiation keeps (cone_entry and the block's theta, rt_tables.hip)
    a_cone = np.arctan(1.001 * k) + np.arcsin((rc * 1.0001 * (1 + KCAP) + 1e-4) * 1.00025 * 1.001 / L) + 2.0e-3 + 1.0e-3
    # ... and the widest the member test of that block admits (bisection on view_member_host's restatement)
    beam = v0["beams"][bs]
    lo, hi = a_cone, a_cone + 0.2
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        c_mid = org + (u * np.cos(mid) + side * np.sin(mid)) * L
        lo, hi = (mid, hi) if member_slack(beam, org, np.array([*c_mid, R * R])) > 0 else (lo, mid)
    a_member = lo
    alpha = 0.5 * (a_cone + a_member)
    S = (*(org + (u * np.cos(alpha) + side * np.sin(alpha)) * L), float(np.sqrt(R)))
    rng = np.random.default_rng(4000 + seed)
    m, pos = _per_block_scene(rt, oracle, "view_kcap", seed, w, h, aspect, cam, rng, extra=[S] * 31)
    v = host_view(rt, m)
    ks = v["beams"][:, 3].astype(np.float64)
    pred = np.array([corner_cone(rt, m, block_rect(v, b, w, h))[1] for b in range(v["blocks"])])
    hits = _hit_pixels_by_block(rt, oracle, m, v)
    low = [b for b in range(v["blocks"]) if 0 < ks[b] <= KCAP]
    high = [b for b in range(v["blocks"]) if ks[b] > KCAP]
    copies = pos[-31:]
    listed = [c for c in copies if c in v["lists"][bs][3].tolist()]
    m.witness = {"pixels": [p for b in high for p in hits.get(b, [])], "low_pixels": [p for b in low for p in hits.get(b, [])],
                 "k": ks.tolist(), "k_predicted": pred.tolist(), "low": low, "high": high, "sliver_block": bs,
                 "sliver_listed": len(listed), "sliver": (float(a_cone), float(alpha), float(a_member)), "flags": [l[1] for l in v["lists"]]}
    return m


# ---------------------------------------------------------------------------------------------- row 5: the order of a view list
def _order_witness(rt, oracle, m, pair):
    """Pixels at which the near roots of the two spheres `pair` are equal or one ulp apart in the reference's float
    arithmetic, with different normals there; their blocks' host lists."""
    cs = camera(rt, m.cam)
    px = [(x, y) for y in range(m.h) for x in range(m.w)]
    O, D = rays(oracle, cs, m.aspect, m.w, m.h, px)
    tab = table(m.spheres)[list(pair)]
    q = quad(tab, O, D)
    with np.errstate(all="ignore"):
        tn = ((-q["B"] - np.sqrt(q["disc"]).astype(f32)) / (f32(2) * q["A"])).astype(f32)
    both = q["hit"].all(axis=1) & np.isfinite(tn).all(axis=1) & (np.sign(tn[:, 0]) == np.sign(tn[:, 1]))
    gap = np.abs(tn[:, 0].view(np.int32).astype(np.int64) - tn[:, 1].view(np.int32).astype(np.int64))
    sel = np.nonzero(both & (gap <= 1))[0]
    with np.errstate(all="ignore"):
        hp = (O[sel] + D[sel] * tn[sel, :1]).astype(f32)
    n0, n1 = hp - tab[0, :3], hp - tab[1, :3]
    differ = sum(bool(not np.array_equal(n0[i] / np.linalg.norm(n0[i]), n1[i] / np.linalg.norm(n1[i]))) for i in range(len(sel)))
    v = host_view(rt, m)
    blocks = sorted({block_of(v, *px[p]) for p in sel})
    on, bounds = True, []
    for b in blocks:
        count, flags, ent, pos, lbs = v["lists"][b]
        ok = flags == 0 and all(s in pos.tolist() for s in pair)
        on = on and ok
        if ok:
            bounds.append([float(lbs[pos.tolist().index(s)]) for s in pair])
    return {"pixels": [px[p] for p in sel], "ulp_gaps": [int(gap[p]) for p in sel], "normals_differ": int(differ),
            "negative": int((tn[sel] < 0).all(axis=1).sum()), "pair": tuple(pair), "blocks": blocks, "on_lists": on,
            "bounds": bounds, "flags": [l[1] for l in v["lists"]]}


def view_order(rt, oracle, seed):
    """Row 5: the front_to_back construction of tests/margins.py (two different spheres whose float near roots meet:
    crossing, internally tangent; seeds 0-7) with fillers, so that the frame reads a view list: the block-wide order and
    the early exit on a block-wide lower bound stand on their bound. The frame's middle, where the spheres meet, is a
    corner of four blocks. Seeds from 8 on put the camera INSIDE both spheres of an internally tangent pair, looking away
    from the point where they touch: the near roots that meet are negative, and so are the list's lower bounds."""
    rng = np.random.default_rng(5000 + seed)
    if seed < 8:
        m2 = M.front_to_back(rt, oracle, seed)
        pair_s, lights, cam, aspect, w, h = m2.spheres, m2.lights, m2.cam, m2.aspect, m2.w, m2.h
    else:
        w, h = 32, 24
        c = np.array([1.0, 2.0, 0.0]) + rng.uniform(-2, 2, 3)
        axis = _unit(rng)
        R = float(rng.uniform(0.3, 1.2))
        r2 = R * float(rng.uniform(0.3, 0.9))
        touch = c - axis * R
        depth = r2 * float(rng.uniform(0.5, 1.5))
        eye = touch + axis * depth
        pair_s = [(*c, float(f32(np.sqrt(R)))), (*(c - axis * (R - r2)), float(np.sqrt(r2)))]
        if (seed // 2) % 2:
            pair_s = pair_s[::-1]
        lights = [(tuple(_unit(rng) * rng.uniform(15, 40)), float(rng.uniform(5, 20)), *[float(x) for x in rng.uniform(0.3, 1, 3)])
                  for _ in range(int(rng.integers(1, 4)))]
        aspect = float(np.sqrt((2e-3, 2e-2)[seed % 2] / depth / 2.0))
        cam = M.aim(oracle, eye, eye + axis, aspect, w, h, rt)
    cs = camera(rt, cam)
    O, D = rays(oracle, cs, aspect, w, h, [(w // 2, h // 2)])
    spheres, pos = _mix(rng, list(pair_s), fillers(rng, O[0], D[0], 62))
    m = ViewMargin("view_order", seed, spheres, lights, cam, aspect, w, h, {})
    m.witness = _order_witness(rt, oracle, m, pos)
    m.witness["inside"] = seed >= 8
    return m


# ---------------------------------------------------------------------------------------------- device lists against host lists
def assert_lists_equal(dev, host, tab):
    """The device builder's lists (Scene.view_lists_info(want_lists=True)) against the host builder's
    (rt.view_lists_host) for the sphere table tab: the same summary, and per block the same count and flags, the same
    spheres, each with its own list position, front to back, with the same bounds up to the device's square root."""
    for k in ("block_w", "block_h", "blocks_x", "blocks_y", "blocks", "overflowed", "not_built", "longest"):
        assert dev[k] == host[k], (k, dev[k], host[k])
    for b, (d, hst) in enumerate(zip(dev["lists"], host["lists"])):
        assert d[0] == hst[0] and d[1] == hst[1], (b, d[:2], hst[:2])
        assert set(d[3].tolist()) == set(hst[3].tolist()), b                      # the same spheres
        assert np.array_equal(d[2], tab[d[3]]), b                                 # each with its own list position
        if d[0] > 1:
            assert (np.diff(d[4]) >= 0).all(), b                                  # front to back
            # the same order up to equal bounds: every sphere's bound agrees (the device's square root may differ
            # from sqrtf in the last place)
            hb = dict(zip(hst[3].tolist(), hst[4].tolist()))
            for p, lb in zip(d[3].tolist(), d[4].tolist()):
                assert abs(lb - hb[p]) <= 1e-5 * (1 + abs(lb)), (b, p, lb, hb[p])


# seeds of each builder the tests render; every one yields a non-empty witness (tests/test_view_margins_cpu.py)
BUILDERS = {
    "view_corner": (view_corner, list(range(48))),
    "view_sample_edge": (view_sample_edge, list(range(16))),
    "view_not_built": (view_not_built, list(range(5))),
    "view_kcap": (view_kcap, list(range(4))),
    "view_order": (view_order, list(range(12))),
}
