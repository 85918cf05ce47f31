"""The diffuse paths of rt_scene_indirect_paths without a device: the path key against its restatement
and its separation, the options' defaults and refusals, the exports and where the wrapper's methods sit; the hand-made
guides of tests/indirect_paths_guides.py against the composed reference (every pixel's outcome at every bounce, every
mask's patterns and counts); the ladder property of the restatement; and the dark-corner construction that
tests/test_indirect_paths_gpu.py runs on the device."""
import ctypes as C

import numpy as np
import pytest

import indirect_guides as IG
import indirect_paths_guides as PG
import indirect_paths_ref as R
import indirect_ref as I
import margins
import postpass as P
import query_ref as Q

f32 = np.float32
M = 100000


def _path_key(rt, k, b):
    lib = rt.load_library()
    k = np.ascontiguousarray(k, dtype=np.uint32)
    out = np.zeros_like(k)
    up = C.POINTER(C.c_uint)
    assert lib.rt_debug_indirect_path_key(k.ctypes.data_as(up), len(k), b, out.ctypes.data_as(up)) == 0
    return out


# ----------------------------------------------------------------------------- the key
def test_path_key_equals_the_restatement(rt):
    rng = np.random.default_rng(21)
    k = rng.integers(0, 1 << 32, M, dtype=np.uint64).astype(np.uint32)
    k[0], k[1] = 0, 0xffffffff
    keys = [_path_key(rt, k, b) for b in range(4)]
    assert np.array_equal(keys[0], k)                                   # b = 0 is the identity
    for b in range(4):
        assert np.array_equal(keys[b], R.path_key(k, b).astype(np.uint32)), b
    assert np.array_equal(keys[1], I.mix(k.astype(np.uint64) ^ 0x426f756e).astype(np.uint32))
    # pairwise distinct over b
    for a in range(4):
        for b in range(a + 1, 4):
            assert (keys[a][:10000] != keys[b][:10000]).all(), (a, b)
    # the first draw under key_1 is not the draw under key_0 more often than chance (24-bit draws: about M * 2^-24)
    d0 = I.draw(I.mix(keys[0].astype(np.uint64) ^ I.SALT), 0, 0)
    d1 = I.draw(I.mix(keys[1].astype(np.uint64) ^ I.SALT), 0, 0)
    assert (d0 == d1).sum() <= 3
    lib = rt.load_library()
    assert lib.rt_debug_indirect_path_key(None, 1, 0, None) == 1 and "path_key" in lib.rt_last_error().decode()


# ----------------------------------------------------------------------------- the options
def _desc(rt, lib):
    d = rt.IndirectDesc()
    lib.rt_indirect_desc_init(C.byref(d))
    d.width, d.height, d.aspect = 8, 4, 1.0
    d.cam = rt.default_camera()
    d.depth, d.normal, d.id, d.rgba_out = 0x10000, 0x20000, 0x30000, 0x40000
    return d


def test_opts_defaults_sizes_and_refusals(rt):
    lib = rt.load_library()
    o = rt.IndirectPathsOpts()
    lib.rt_indirect_paths_opts_init(C.byref(o))
    assert (o.struct_size, o.bounces) == (C.sizeof(rt.IndirectPathsOpts), 2) and C.sizeof(rt.IndirectPathsOpts) == 8
    assert rt.RT_INDIRECT_MAX_BOUNCES == 4
    s = rt.Scene()
    try:
        assert s.indirect_paths_opts().bounces == 2 and s.indirect_paths_opts(3).bounces == 3
        d = _desc(rt, lib)
        for bad in (0, 5, -1):
            assert s.indirect_paths_raw(d, s.indirect_paths_opts(bad)) == 1, bad
            assert "bounces" in lib.rt_last_error().decode()
        # in range (and NULL, the defaults): only the scene is missing, under this entry's name
        for o in (None, s.indirect_paths_opts(1), s.indirect_paths_opts(4)):
            assert s.indirect_paths_raw(d, o) == 1
            msg = lib.rt_last_error().decode()
            assert "sky" in msg and msg.startswith("rt_scene_indirect_paths:")
        # a shorter struct reads `bounces` as its default; 0 reads as this layout
        o = s.indirect_paths_opts(9)
        o.struct_size = rt.IndirectPathsOpts.bounces.offset
        assert s.indirect_paths_raw(d, o) == 1 and "sky" in lib.rt_last_error().decode()
        o.struct_size = 0
        assert s.indirect_paths_raw(d, o) == 1 and "bounces" in lib.rt_last_error().decode()
        o.bounces = 3
        assert s.indirect_paths_raw(d, o) == 1 and "sky" in lib.rt_last_error().decode()
        # the description's refusals are rt_scene_indirect's
        d.rays = 17
        assert s.indirect_paths_raw(d, None) == 1 and "rays" in lib.rt_last_error().decode()
        assert lib.rt_scene_indirect_paths(None, C.byref(d), None, None) == 1
        assert lib.rt_scene_indirect_paths(s.handle, None, None, None) == 1
        assert s.indirect_path_counts() == [] and s.indirect_paths_times() == []
        n = C.c_int(5)
        assert lib.rt_debug_indirect_path_counts(s.handle, None, 4, C.byref(n)) == 1
    finally:
        s.close()


def test_exports_layout_and_where_the_methods_sit(rt):
    lib = rt.load_library()
    for n in ("rt_indirect_paths_opts_init", "rt_scene_indirect_paths", "rt_debug_indirect_path_counts",
              "rt_debug_indirect_path_key"):
        assert hasattr(lib, n), n
    assert C.sizeof(rt.IndirectDesc) == 136
    names = list(vars(rt.Scene))
    last = names.index("indirect_times")
    for n in ("indirect_paths_opts", "indirect_paths_raw", "indirect_paths", "indirect_path_counts", "indirect_paths_times"):
        assert names.index(n) > last, n
    import inspect
    a, b = inspect.signature(rt.Scene.indirect).parameters, inspect.signature(rt.Scene.indirect_paths).parameters
    assert set(b) == set(a) | {"bounces"}
    for k in a:
        assert a[k].default == b[k].default and a[k].kind == b[k].kind, k
    s = rt.Scene()
    try:
        with pytest.raises(rt.RtError):
            s.indirect_paths({"aov": {}})
    finally:
        s.close()


# ----------------------------------------------------------------------------- the hand-made guides
@pytest.fixture(scope="module")
def world(rt, oracle):
    inp = PG.scene_inputs(rt)
    rays = {}

    def primary(w, h):
        if (w, h) not in rays:
            rays[(w, h)] = margins.primary_rays(oracle, inp.cam, IG.view_aspect(rt, w, h), w, h)
        return rays[(w, h)]
    return inp, Q.CastRef(oracle, inp), primary


@pytest.mark.parametrize("w,h,name", PG.cases())
def test_a_mask_shows_the_patterns_and_lengths_it_claims(w, h, name):
    make, claims, length = PG.MASKS[(w, h)][name]
    types = make(w * h)
    assert types.shape == (w * h,) and set(np.unique(types)) <= {PG.CONT, PG.STOP, PG.MISS, PG.DEAD}
    assert PG.patterns(types) == claims, name
    if length is not None:
        assert PG.counts(types, 1, 2)[0][1] == length
    assert PG.counts(types, 5, 3)[1] == [int(np.isin(types, (PG.CONT, PG.STOP)).sum())] + [int((types == PG.CONT).sum())] * 2


def test_the_masks_cover_every_pattern_and_length():
    claimed = set().union(*(c for ms in PG.MASKS.values() for _, c, _ in ms.values()))
    assert claimed == set(PG.PATTERNS)
    lengths = {l for ms in PG.MASKS.values() for _, _, l in ms.values() if l is not None}
    assert {1, 63, 65} <= lengths and any(l % 64 == 0 for l in lengths)
    # patterns() itself
    w = PG._wave
    assert PG.patterns(w("lane 0 only")) == {"lane 0 only"} and PG.patterns(w("lane 63 only")) == {"lane 63 only"}
    assert PG.patterns(w("alternating")) == {"alternating"} and PG.patterns(w("full")) == {"full"}
    assert PG.patterns(np.concatenate([w("full"), w("none"), w("full")])) == {"full", "none between"}
    assert PG.patterns(np.concatenate([w("full"), w("none")])) == {"full"}
    broken = w("lane 0 only")
    broken[7] = PG.MISS                                                  # not a full wave of hits: no claim
    assert PG.patterns(broken) == set()


@pytest.mark.parametrize("w,h,name", PG.cases())
def test_the_reference_gives_every_pixel_its_intended_outcome_at_every_bounce(world, w, h, name):
    inp, ref, primary = world
    g = PG.masked(w, h, name)
    O, Dir = primary(w, h)
    live, n, start, _ = I.pixels(g.depth, g.normal, g.id, O, Dir)
    assert np.array_equal(~live, g.kinds == PG.DEAD)
    rays = max(PG.RAYS) if w * h <= 256 else 2
    idx, Gs = I.gather_rays(w, live, n, start, rays, PG.RAY_BASE, PG.SEED)
    kinds = g.kinds[idx]
    x, y = idx % w, idx // w
    nearest, shade = R.castref_callables(ref)
    for j, G in enumerate(Gs):
        key = I.key(x, y, np.full(len(idx), PG.RAY_BASE + j), np.full(len(idx), PG.SEED))
        _, hits, entered = R.path(start[idx], G, key, nearest, shade, inp.tex, PG.BOUNCES)
        want = np.where(kinds == PG.CONT, PG.BOUNCES, np.where(kinds == PG.STOP, 1, 0))
        assert np.array_equal(hits, want), (j, idx[hits != want][:8])
        assert entered == [int((kinds != PG.MISS).sum())] + [int((kinds == PG.CONT).sum())] * (PG.BOUNCES - 1)


# ----------------------------------------------------------------------------- the ladder
def test_the_restatement_climbs_the_ladder(rt, oracle):
    inp = PG.ladder_inputs(rt)
    w, h = 50, 30
    g = PG.masked(w, h, "mixed")
    O, Dir = margins.primary_rays(oracle, inp.cam, IG.view_aspect(rt, w, h), w, h)
    nearest, shade = R.castref_callables(Q.CastRef(oracle, inp))
    for bounces in (1, 2, 3, 4):
        rgba, _, det = R.indirect_paths(w, g.depth, g.normal, g.id, O, Dir, nearest, shade, inp.tex, bounces=bounces,
                                        seed=5, details=True)
        ks = PG.ladder_check(rgba[:, :3], det, bounces)
        assert ks == ({0, 1} if bounces == 1 else {0, 1, bounces})      # MISS, STOP, and CONT up to the budget
        assert not rgba[~det["live"], :3].any()


# ----------------------------------------------------------------------------- the dark corner
def test_the_dark_corner_holds_for_the_restatement(rt, oracle):
    inp = PG.corner_inputs(rt)
    w, h = PG.CORNER["w"], PG.CORNER["h"]
    g = PG.corner_guides()
    O, Dir = margins.primary_rays(oracle, inp.cam, IG.view_aspect(rt, w, h), w, h)
    nearest, shade = R.castref_callables(Q.CastRef(oracle, inp))
    kw = dict(rays=PG.CORNER["rays"], seed=PG.CORNER["seed"], details=True)
    one, _, d1 = R.indirect_paths(w, g.depth, g.normal, g.id, O, Dir, nearest, shade, inp.tex, bounces=1, **kw)
    three, _, d3 = R.indirect_paths(w, g.depth, g.normal, g.id, O, Dir, nearest, shade, inp.tex, bounces=3, **kw)
    assert d1["live"].all()
    assert not one[:, :3].any()                                          # one bounce: every pixel is black
    twice = PG.corner_lit(d3)
    assert twice.sum() >= w * h // 2
    assert (three[twice, :3] > 0).all() and not three[~twice, :3].any()
