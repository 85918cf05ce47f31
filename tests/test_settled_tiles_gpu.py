"""Tile summaries of a resting view: the launch that records a tile's light verdicts also notes, in
one dword per tile, whether the tile is *settled* -- it has a primary record, at most four groups under at most eight
lights, and every (group, light) entry of its word says "adds nothing" -- and whether none of its valid pixels is a miss.
The reading launches send a settled tile straight to the write-back: 0 for its hit pixels, the sky texel on record for
the others. Every frame must stay the same bits as the oracle's; the read-back (Scene.tile_summaries) and the setter
(Scene.set_tile_summaries) show that the flag means what it says, is set wherever it may be, and is what the reader goes by.

The library takes at most eight lights (a ninth is refused by rt_scene_set_lights), which is also what a word holds: the
"more lights than a word holds" case cannot be launched, so the eight-light scene is rendered and the refusal asserted."""
import numpy as np
import pytest

import verdict_runs as R
from scenes import Inputs, Scn

pytestmark = pytest.mark.gpu

SIZES, layouts, rows_of = R.SIZES, R.layouts, R.rows_of
ONE = np.uint32(0x3f800000)   # 1.0f


@pytest.fixture(scope="module")
def refs(rt, gpu, oracle):
    return R.oracle_refs(rt, oracle)


def recorded(inp, w, h, want, launches=2, **kw):
    """A scene after `launches` launches of one view (2: the recording launch was the last)."""
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h, **kw), want, launches=launches)
    return sc


def summaries(rt, sc):
    """-> (settled, no_miss, groups) per tile, and the raw dwords."""
    t = sc.tile_summaries(want_tables=True)
    d = t["dwords"]
    assert int(((d & rt.RT_TILE_SETTLED) != 0).sum()) == t["settled"]
    assert int(((d & 3) == 3).sum()) == t["settled_no_miss"]
    return (d & rt.RT_TILE_SETTLED) != 0, (d & rt.RT_TILE_NO_MISS) != 0, (d >> rt.RT_TILE_GROUPS_SHIFT) & 0xff, d


def tiles_of(rt, img, tiles_y, tiles_x, fill):
    """[h, w] -> [tiles_y, tiles_x, 64] of 8 x 8 tiles; pixels outside the frame are `fill`."""
    h, w = img.shape
    return rt.pixels_to_tiles(np.pad(img, ((0, tiles_y * 8 - h), (0, tiles_x * 8 - w)), constant_values=fill), 8)


def ids_of(inp, w, h):
    """(kind, sphere) per pixel from a G-buffer launch on a scene of its own with the switch off."""
    import torch
    ref = inp.scene()
    ref.set_light_verdicts(0)
    ids = ref.render(w, h, aov=("id",))["aov"]["id"].cpu().numpy()
    torch.cuda.synchronize()
    return ids


def expected(rt, sc, inp, w, h, n_lights=3):
    """What the definition says of every 8 x 8 tile, from the words, the primary records and the G-buffer's ids:
    -> (settled, no miss among the valid pixels, groups, has a record, hit pixels [ty, tx, 64], valid pixels)."""
    words = sc.light_verdicts(want_words=True)["words"]
    prim = sc.primary_records(want_tables=True)
    ty, tx = words.shape
    ids = ids_of(inp, w, h)
    valid = tiles_of(rt, np.ones((h, w), dtype=bool), ty, tx, False)
    hit = tiles_of(rt, ids[..., 0] >= 0, ty, tx, False)
    sphere = tiles_of(rt, ids[..., 1], ty, tx, -1)
    has = (prim["positions"] != -2).any(axis=-1)
    codes = R.codes(words)
    groups = np.zeros((ty, tx), dtype=np.int64)
    settled = np.zeros((ty, tx), dtype=bool)
    for y in range(ty):
        for x in range(tx):
            groups[y, x] = len({int(i) for i in sphere[y, x][hit[y, x]]})   # spheres of distinct centres: a group each
            g = groups[y, x]
            settled[y, x] = has[y, x] and g <= R.GROUPS and bool((codes[y, x, :g, :n_lights] == R.NOTHING).all())
    return settled, ~(valid & ~hit).any(axis=-1), groups, has, hit, valid, prim


def check_meaning(rt, sc, inp, w, h, n_lights=3):
    got_settled, got_no_miss, got_groups, _ = summaries(rt, sc)
    settled, no_miss, groups, has, hit, valid, prim = expected(rt, sc, inp, w, h, n_lights)
    assert np.array_equal(got_settled, settled), (np.argwhere(got_settled != settled)[:4], int(settled.sum()), int(got_settled.sum()))
    assert np.array_equal(got_groups, np.minimum(groups, 255))
    # bit 1 against the G-buffer's misses for every tile, and against the records' own -1 where a tile has a record
    # (a tile without one resolves to -2 in every lane, which says nothing about its misses)
    assert np.array_equal(got_no_miss, no_miss), np.argwhere(got_no_miss != no_miss)[:4]
    with_record =~((prim["positions"] == -1) & valid).any(axis=-1)          # "no -1 among the tile's valid positions"
    assert np.array_equal(got_no_miss[has], with_record[has])
    return settled, no_miss, groups, has, hit, valid, prim


@pytest.mark.parametrize("n", sorted(SIZES))
@pytest.mark.parametrize("layout", sorted(layouts(90)))
def test_frames_at_rest(rt, refs, n, layout):
    w, h = SIZES[n]
    kw = layouts(h)[layout]
    inp, whole = refs[n]
    rows = rows_of(rt, h, kw)
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h, **kw), (whole[0][rows], whole[1][rows]), launches=4, what="%d %s" % (n, layout))
    t = sc.tile_summaries()
    assert t["state"] == 2 and (t["tiles_x"], t["tiles_y"]) == R.grid(w, h, kw), t
    print("%d %s: %d of %d tiles settled, %d of them without a miss" % (n, layout, t["settled"], t["tiles_x"] * t["tiles_y"], t["settled_no_miss"]))
    if layout == "tile8":
        assert t["settled"] >= 1


@pytest.mark.parametrize("tile,size", [(16, 256), (32, 512), (64, 1024)])
def test_wider_tiles_settle_too(rt, gpu, tile, size):
    """At 160 x 90 and 96 x 54 only the 8 x 8 tile nests in the view-list blocks, so the wider tiles above have no record
    and no flag. Here the frame is the smallest square whose blocks hold the tile, and the sample-loop kernels take the
    same path. The oracle is too slow at these sizes: the reference is the brute-force frame of a scene of its own."""
    inp = Inputs(rt, 256)
    ref = inp.scene()
    ref.set_light_verdicts(0)
    want = R.frame(ref, size, size, cull=False)
    sc = inp.scene()
    R.resting(sc, dict(width=size, height=size, tile=tile), want, launches=4, what="tile %d at %d" % (tile, size))
    t = sc.tile_summaries()
    print("tile %d at %d x %d: %d of %d tiles settled, %d of them without a miss" %
          (tile, size, size, t["settled"], t["tiles_x"] * t["tiles_y"], t["settled_no_miss"]))
    assert t["state"] == 2 and t["settled"] >= 1


def test_partial_tiles(rt, gpu, oracle):
    """100 columns and 54 rows: the last tile of every row has four columns outside the frame, the last row two rows."""
    inp = Inputs(rt, 256)
    w, h = 100, 54
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h), R.oracle_frame(oracle, inp, w, h), launches=4, what="100 x 54")
    settled = check_meaning(rt, sc, inp, w, h)[0]
    assert settled[:, -1].any() or settled[-1].any()   # a settled tile at the frame's edge


@pytest.mark.parametrize("n", sorted(SIZES))
def test_meaning_and_completeness(rt, refs, n):
    inp, want = refs[n]
    w, h = SIZES[n]
    sc = recorded(inp, w, h, want)
    assert sc.tile_summaries()["state"] == 1
    settled, no_miss, groups, has, _, _, _ = check_meaning(rt, sc, inp, w, h)
    print("%d x %d, %d spheres: %d of %d tiles settled (%d without a miss), %d with a record" %
          (w, h, n, int(settled.sum()), settled.size, int((settled & no_miss).sum()), int(has.sum())))
    assert settled.any() and (~settled).any()
    if n == 1024:   # (half of the oracle's tiles are all zero there: material for each kind)
        assert (settled & no_miss).any() and (settled & ~no_miss).any()


def test_settled_pixels(rt, refs):
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc = recorded(inp, w, h, want, launches=3)
    got = R.frame(sc, w, h)
    assert sc.tile_summaries()["state"] == 2
    settled, _, _, _, hit, valid, prim = check_meaning(rt, sc, inp, w, h)
    ty, tx = settled.shape
    rgba = np.stack([tiles_of(rt, got[0][..., c], ty, tx, 0) for c in range(4)], axis=-1)
    packed = tiles_of(rt, got[1], ty, tx, 0)
    entry, texel = rt.decode_primary_records(prim["dwords"])
    sky = np.stack([R._bits(p).reshape(-1) for p in inp.sky], axis=-1)
    h_m = settled[..., None] & hit
    m_m = settled[..., None] & valid & ~hit
    assert h_m.any() and m_m.any()
    assert (rgba[h_m] == np.array([0, 0, 0, ONE], dtype=np.uint32)).all() and (packed[h_m] == 0).all()
    assert (entry[m_m] == rt.RT_PRIMARY_MISS).all()
    assert np.array_equal(rgba[m_m][:, :3], sky[texel[m_m]]) and (rgba[m_m][:, 3] == ONE).all()


def changed_tiles(got, want, shape):
    diff = (got[0] != want[0]).any(axis=-1) | (got[1] != want[1])
    dd = np.zeros((shape[0] * 8, shape[1] * 8), dtype=bool)
    dd[:diff.shape[0], :diff.shape[1]] = diff
    return diff, dd.reshape(shape[0], 8, shape[1], 8).any(axis=(1, 3))


def test_reader_consumes_the_flag_and_only_where_it_is_set(rt, refs):
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc = recorded(inp, w, h, want, launches=3)
    settled, no_miss, _, has, hit, valid, prim = check_meaning(rt, sc, inp, w, h)
    d0 = summaries(rt, sc)[3].copy()
    ty, tx = settled.shape

    # every flag cleared: every tile takes the full path
    sc.set_tile_summaries(d0 & ~np.uint32(rt.RT_TILE_SETTLED))
    R.assert_same(R.frame(sc, w, h), want, "flags cleared")
    assert sc.tile_summaries()["state"] == 2 and sc.tile_summaries()["settled"] == 0

    # the flag set on every fifth tile with a record and a lit hit pixel: exactly those change, their hit pixels go black
    lit = tiles_of(rt, (want[0][..., :3] != 0).any(axis=-1), ty, tx, False) & hit
    cand = np.argwhere(has & ~settled & lit.any(axis=-1))[::5]
    assert len(cand) >= 1
    touched = np.zeros(settled.shape, dtype=bool)
    touched[cand[:, 0], cand[:, 1]] = True
    sc.set_tile_summaries(np.where(touched, d0 | np.uint32(rt.RT_TILE_SETTLED), d0))
    got = R.frame(sc, w, h)
    diff, changed = changed_tiles(got, want, settled.shape)
    assert np.array_equal(changed, touched), (int(changed.sum()), int(touched.sum()))
    rgba = np.stack([tiles_of(rt, got[0][..., c], ty, tx, 0) for c in range(4)], axis=-1)
    packed = tiles_of(rt, got[1], ty, tx, 0)
    black = touched[..., None] & hit
    assert (rgba[black] == np.array([0, 0, 0, ONE], dtype=np.uint32)).all() and (packed[black] == 0).all()
    assert not (tiles_of(rt, diff, ty, tx, False) & ~hit).any()           # their miss pixels keep their sky texel

    # the flags as recorded
    sc.set_tile_summaries(d0)
    R.assert_same(R.frame(sc, w, h), want, "flags restored")

    # a miss lane of a settled tile takes another in-range sky texel of another colour: that pixel changes, no other
    entry, texel = rt.decode_primary_records(prim["dwords"])
    sky = np.stack([R._bits(p).reshape(-1) for p in inp.sky], axis=-1)
    y, x = np.argwhere(settled & ~no_miss)[0]
    lane = int(np.argwhere(valid[y, x] & ~hit[y, x])[0, 0])
    old = int(texel[y, x, lane])
    new = next(c for c in ((old + k * 977 + 13) % sky.shape[0] for k in range(64)) if (sky[c] != sky[old]).any())
    dw = prim["dwords"].copy()
    dw[y, x, lane] = rt.encode_primary_records(np.uint32(rt.RT_PRIMARY_MISS), np.uint32(new))
    sc.set_primary_records(dw)
    got = R.frame(sc, w, h)
    diff, _ = changed_tiles(got, want, settled.shape)
    py, px = y * 8 + lane // 8, x * 8 + lane % 8
    assert diff[py, px] and int(diff.sum()) == 1, (int(diff.sum()), py, px)
    assert np.array_equal(got[0][py, px, :3], sky[new])

    # the entries (and texels) of hit lanes in settled tiles, poisoned with in-range values: never consulted
    dw = prim["dwords"].copy()
    ntex = inp.tex[0].size
    poison = settled[..., None] & hit
    assert poison.any()
    dw[poison] = rt.encode_primary_records(np.zeros(int(poison.sum()), dtype=np.uint32), (texel[poison] + 1) % ntex)
    sc.set_primary_records(dw)
    R.assert_same(R.frame(sc, w, h), want, "hit lanes of settled tiles poisoned")
    sc.set_primary_records(prim["dwords"])
    R.assert_same(R.frame(sc, w, h), want, "records restored")


def test_a_settled_tile_without_a_record_takes_the_full_path(rt, refs):
    """Through the setters only: a valid lane of a flagged tile says 0xfe -- the tile renders as the plain kernel does."""
    inp, want = refs[256]
    w, h = SIZES[256]
    sc = recorded(inp, w, h, want, launches=3)
    prim = sc.primary_records(want_tables=True)
    d0 = summaries(rt, sc)[3]
    dw = prim["dwords"].copy()
    dw[..., 0] = rt.encode_primary_records(np.uint32(rt.RT_PRIMARY_NONE), np.uint32(0))   # lane 0 is valid in every tile
    sc.set_primary_records(dw)
    sc.set_tile_summaries((d0 | np.uint32(rt.RT_TILE_SETTLED)) & ~np.uint32(rt.RT_TILE_NO_MISS))
    for k in range(2):
        R.assert_same(R.frame(sc, w, h), want, "every tile flagged, none with a record, launch %d" % k)


def test_more_groups_than_a_word_holds_are_never_flagged(rt, gpu):
    g = rt.generate_spheres(4096, 3)
    tiny = Scn(rt, [(g[i].orgin.x, g[i].orgin.y, g[i].orgin.z, 0.12) for i in range(4096)])
    w, h = SIZES[1024]
    ref = tiny.scene()
    ref.set_light_verdicts(0)
    off = R.frame(ref, w, h)
    R.assert_same(R.frame(ref, w, h, cull=False), off, "brute force")
    sc = tiny.scene()
    R.resting(sc, dict(width=w, height=h), off, launches=2)
    settled, _, groups, _, _, _, _ = check_meaning(rt, sc, tiny, w, h)
    assert (groups > R.GROUPS).any() and not settled[groups > R.GROUPS].any()
    for k in range(2):
        R.assert_same(R.frame(sc, w, h), off, "reading launch %d" % k)


def test_eight_lights_and_a_ninth_is_refused(rt, gpu):
    pos = [(20, 20, 20), (0, 20, -20), (0, 20, 0), (-20, 15, 5), (10, 25, -5), (25, 8, 0), (-5, 30, 12), (3, 18, 25), (8, 9, 10)]
    lights = [(p, 20, 0.2 + 0.1 * (i % 3), 0.1 * (i % 4), 0.15 * (i % 5)) for i, p in enumerate(pos)]
    inp = Inputs(rt, 256)
    sc0 = inp.scene()
    assert sc0.lib.rt_scene_set_lights(sc0.handle, Scn(rt, [], lights=lights).lights, 9) != 0   # no launch has nine
    inp.lights, inp.n_lights = Scn(rt, [], lights=lights[:8]).lights, 8
    w, h = SIZES[256]
    off = R.switched_off(inp, w, h)[0]
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h), off, launches=2)
    check_meaning(rt, sc, inp, w, h, n_lights=8)            # all eight codes of every group, or no flag
    for k in range(2):
        R.assert_same(R.frame(sc, w, h), off, "reading launch %d" % k)


def test_eight_spheres_have_no_record_and_no_flag(rt, gpu, oracle):
    inp = Inputs(rt, 8)
    w, h = 64, 48
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h), R.oracle_frame(oracle, inp, w, h), launches=4, what="8 spheres")
    t = sc.tile_summaries(want_tables=True)
    assert t["state"] == 2 and t["settled"] == 0 and not (t["dwords"] & rt.RT_TILE_SETTLED).any()


def test_a_non_finite_texel_does_not_settle_its_tile(rt, gpu):
    """Red is inf in every texel: 0 x inf is not 0, no lane may take a dark light for "adds nothing", and so no tile with a
    hit pixel is settled, whatever its lights. (The frame holds NaNs; a NaN matches a NaN.)"""
    inp = Inputs(rt, 256)
    inp.tex = [p.copy() for p in inp.tex]
    inp.tex[0][:] = np.inf
    w, h = SIZES[256]
    ref = inp.scene()
    ref.set_light_verdicts(0)
    off = R.frame(ref, w, h)
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h), off, launches=4, nan_equal=True, what="red = inf")
    settled, _, groups, has, hit, _, _ = check_meaning(rt, sc, inp, w, h)
    assert has.any() and hit.any() and not settled[hit.any(axis=-1)].any()
    assert settled.any()                                    # (the all-sky tiles still are)


def test_existing_read_backs_are_unchanged(rt, refs):
    """Words, tags, counts and primary records keep their offsets in front of the summaries: after a recording launch
    they equal those of a second scene built the same way, and rewriting the summaries leaves them as they were."""
    inp, want = refs[1024]
    w, h = SIZES[1024]

    def read(sc):
        c = sc.shadow_counts(want_tables=True)
        used = R.tagged_of(c["tags"])[0][..., :c["records"]]                 # (a record no tag points to is never written)
        return (sc.light_verdicts(want_words=True)["words"], c["tags"], np.where(used[..., None], c["counts"], 0),
                sc.primary_records(want_tables=True)["dwords"])

    a, b = recorded(inp, w, h, want), recorded(inp, w, h, want)
    ra, rb = read(a), read(b)
    for x, y in zip(ra, rb):
        assert np.array_equal(x, y)
    d = summaries(rt, a)[3]
    assert np.array_equal(d, summaries(rt, b)[3])
    a.set_tile_summaries(d ^ np.uint32(rt.RT_TILE_SETTLED))
    a.set_tile_summaries(d)
    for x, y in zip(read(a), ra):
        assert np.array_equal(x, y)
    assert np.array_equal(summaries(rt, a)[3], d)
    for k in range(2):
        R.assert_same(R.frame(a, w, h), want, "after the rewrites, launch %d" % k)
