"""Primary records of a resting view: the launch that records a tile's light verdicts also keeps,
per pixel, which entry of the tile's view list is the closest hit and which texel the pixel reads; the reading launches
evaluate that one entry instead of walking the list and fetch that texel instead of computing its index. Every frame
must stay the same bits as with the switch off, as the brute-force kernel's and as the oracle's; the read-back
(Scene.primary_records) and the setter (Scene.set_primary_records) show that the records mean what they say, are the
only thing read, and are read only where a tile has one."""
import ctypes as C

import numpy as np
import pytest

import verdict_runs as R
from scenes import Inputs, Scn

pytestmark = pytest.mark.gpu

SIZES, layouts, rows_of = R.SIZES, R.layouts, R.rows_of
LAYOUTS = ["tile8", "tile16", "tile32", "tile64", "band", "interleave"]


@pytest.fixture(scope="module")
def refs(rt, gpu, oracle):
    return R.oracle_refs(rt, oracle)


def at_rest(inp, w, h, want, what, launches=5, **kw):
    """Switch off = brute force = `want`; then plain, recording and reading launches on one scene, all = `want`.
    -> (the scene, its primary-record info after the last launch)."""
    _, info = R.switched_off(inp, w, h, want, what + ": ", read_back="primary_records", **kw)
    assert info["tiles_recorded"] == 0, info
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h, **kw), want, launches=launches, what=what)
    info = sc.primary_records()
    tiles = info["tiles_x"] * info["tiles_y"]
    print("%s: %d of %d tiles have a primary record (%.1f %%), %d hit and %d miss pixels in them" %
          (what, info["tiles_recorded"], tiles, 100.0 * info["tiles_recorded"] / tiles, info["hit_pixels"], info["miss_pixels"]))
    assert info["state"] == 2 and (info["tiles_x"], info["tiles_y"]) == R.grid(w, h, kw), info
    return sc, info


@pytest.mark.parametrize("n", sorted(SIZES))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_frames_at_rest(rt, refs, n, layout):
    w, h = SIZES[n]
    kw = layouts(h)[layout]
    inp, whole = refs[n]
    rows = rows_of(rt, h, kw)
    _, info = at_rest(inp, w, h, (whole[0][rows], whole[1][rows]), "%d %s" % (n, layout), **kw)
    if layout == "tile8":                                  # the product's layout nests in the view-list blocks
        assert info["tiles_recorded"] >= 1 and info["hit_pixels"] >= 1
    assert info["tile_w"] == (kw.get("tile") or 8)


@pytest.mark.parametrize("tile,size", [(16, 256), (32, 512), (64, 1024)])
def test_wider_tiles_with_a_record(rt, gpu, tile, size):
    """At 160 x 90 and 96 x 54 the view-list blocks are 8 x 8 pixels and only the 8 x 8 tile nests in them, so the wider
    tiles above take the 0xfe path. Here the frame is the smallest square whose blocks hold the tile (blocks of 16, 32
    and 64 pixels from 256, 512 and 1024 pixels a side), and the sample-loop kernels read records too. The oracle is too
    slow at these sizes: the reference frame is the brute-force kernel's on a scene of its own with the switch off."""
    inp = Inputs(rt, 256)
    ref = inp.scene()
    ref.set_light_verdicts(0)
    want = R.frame(ref, size, size, cull=False)
    sc = inp.scene()
    R.resting(sc, dict(width=size, height=size, tile=tile), want, launches=4, what="tile %d at %d" % (tile, size))
    info = sc.primary_records()
    print("tile %d at %d x %d: %d of %d tiles have a record" % (tile, size, size, info["tiles_recorded"], info["tiles_x"] * info["tiles_y"]))
    assert info["state"] == 2 and info["tile_w"] == tile and info["tiles_recorded"] >= 1 and info["hit_pixels"] >= 1


def _edge(rt, oracle, inp, w, h, what, **kw):
    return at_rest(inp, w, h, R.oracle_frame(oracle, inp, w, h), what, launches=4, **kw)


def test_eight_spheres_have_no_record(rt, gpu, oracle):
    """No eye cones below 64 spheres, so no view lists: every tile says 0xfe and every reader walks as before."""
    sc, info = _edge(rt, oracle, Inputs(rt, 8), 64, 48, "8 spheres")
    assert info["tiles_recorded"] == 0 and info["hit_pixels"] == 0 and info["miss_pixels"] == 0
    t = sc.primary_records(want_tables=True)
    assert ((t["dwords"] & 0xff) == rt.RT_PRIMARY_NONE).all() and (t["positions"] == -2).all()


def test_no_spheres_all_sky(rt, gpu, oracle):
    _edge(rt, oracle, Scn(rt, []), 64, 48, "0 spheres")


def test_partial_tiles(rt, gpu, oracle):
    """100 columns: the last tile of every row of tiles has four columns outside the frame."""
    sc, info = _edge(rt, oracle, Inputs(rt, 256), 100, 54, "100 x 54")
    assert info["tiles_recorded"] >= 1
    t = sc.primary_records(want_tables=True)
    pos = rt.tiles_to_pixels(t["positions"], 8)
    assert (pos[:, 100:] == -2).all() and (pos[54:] == -2).all()   # lanes outside the frame resolve to nothing


def test_camera_inside_a_sphere(rt, gpu, oracle):
    """A sphere of the list around the camera: negative-t hits, which the walk's gate lets through and the reader's must."""
    inp = Inputs(rt, 256)
    rt.load_library().rt_sphere_init(C.byref(inp.spheres[5]), 4.0, 3.0, 9.5, 2.0)
    sc, info = _edge(rt, oracle, inp, 96, 54, "camera inside sphere 5")
    assert info["tiles_recorded"] >= 1 and info["hit_pixels"] >= 1


def test_two_identical_spheres(rt, gpu, oracle):
    """The tie rule: of two identical spheres the lower table position holds the hit, in the record too."""
    inp = Inputs(rt, 256)
    lib = rt.load_library()
    for i in (3, 200):
        lib.rt_sphere_init(C.byref(inp.spheres[i]), 4.0, 2.0, 5.0, 0.9)
    sc, info = _edge(rt, oracle, inp, 96, 54, "spheres 3 and 200 identical")
    t = sc.primary_records(want_tables=True)
    assert (t["positions"] == 3).any() and not (t["positions"] == 200).any()


def test_update_in_three_bands(rt, gpu, oracle):
    lib = rt.load_library()
    with R.App(rt, 256, 13, 64, 528) as app:
        want = R.oracle_frame(oracle, app.inp, 64, 528)[1]
        states = []
        for k in range(5):
            got, state = app.update()
            assert np.array_equal(got, want), (k, state, int((got != want).sum()))
            states.append(state)
        assert states == [0, 1, 2, 2, 2], states
        info = rt.PrimaryRecordsInfo()
        assert lib.rt_debug_primary_records(lib.rt_debug_shim_scene(), C.byref(info), None, None, 0) == 0, lib.rt_last_error()
        print("last band: %d of %d x %d tiles with a primary record" % (info.tiles_recorded, info.tiles_x, info.tiles_y))
        assert info.state == 2


def recorded(inp, w, h, want, launches=2, **kw):
    """A scene after `launches` launches of one view (2: the recording launch was the last), and its records."""
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h, **kw), want, launches=launches)
    return sc, sc.primary_records(want_tables=True)


def test_meaning_of_the_records(rt, refs):
    """The records against a G-buffer launch of the same view on a scene with the switch off: the entry resolves to the
    pixel's hit id, the texel to the pixel's albedo."""
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc, t = recorded(inp, w, h, want)
    assert t["state"] == 1
    tiles = t["tiles_x"] * t["tiles_y"]
    print("160 x 90, 1024 spheres, tile 8: %d of %d tiles have a record (%.1f %%); %d hit, %d miss pixels" %
          (t["tiles_recorded"], tiles, 100.0 * t["tiles_recorded"] / tiles, t["hit_pixels"], t["miss_pixels"]))
    assert t["tiles_recorded"] >= 1 and t["hit_pixels"] >= 1 and t["miss_pixels"] >= 1   # (against a vacuous pass)
    ref = inp.scene()
    ref.set_light_verdicts(0)
    import torch
    g = ref.render(w, h, aov=("id", "albedo"))
    torch.cuda.synchronize()
    ids = g["aov"]["id"].cpu().numpy()
    albedo = R._bits(g["aov"]["albedo"].cpu().numpy())
    pos = rt.tiles_to_pixels(t["positions"], 8)[:h, :w]
    entry, texel = rt.decode_primary_records(rt.tiles_to_pixels(t["dwords"], 8)[:h, :w])
    has = pos != -2
    hit, miss = has & (pos >= 0), has & (pos == -1)
    assert int(hit.sum()) == t["hit_pixels"] and int(miss.sum()) == t["miss_pixels"]
    assert (entry[hit] < 64).all() and (entry[miss] == rt.RT_PRIMARY_MISS).all()
    assert np.array_equal(pos[hit], ids[..., 1][hit]) and (ids[..., 0][hit] == 1).all()
    assert (ids[..., 1][miss] == -1).all() and (ids[..., 0][miss] == -1).all()
    tex = np.stack([R._bits(p).reshape(-1) for p in inp.tex], axis=-1)
    sky = np.stack([R._bits(p).reshape(-1) for p in inp.sky], axis=-1)
    assert texel[hit].max() < tex.shape[0] and texel[miss].max() < sky.shape[0]
    assert np.array_equal(tex[texel[hit]], albedo[hit][:, :3])
    assert np.array_equal(sky[texel[miss]], albedo[miss][:, :3])


def test_reader_consumes_the_records_and_only_where_it_should(rt, refs):
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc, t = recorded(inp, w, h, want, launches=3)
    lists = sc.view_lists_info(want_lists=True)
    bw, bh, nbx = lists["block_w"], lists["block_h"], lists["blocks_x"]
    dw = t["dwords"].copy()
    entry, texel = rt.decode_primary_records(dw)
    has = (t["positions"] != -2).any(axis=-1)                # tiles with a record
    hit = t["positions"] >= 0
    ntex = inp.tex[0].size
    tex = np.stack([R._bits(p).reshape(-1) for p in inp.tex], axis=-1)
    touched = np.zeros(has.shape, dtype=bool)

    def to_tiles(img, fill):
        return rt.pixels_to_tiles(np.pad(img, ((0, t["tiles_y"] * 8 - h), (0, t["tiles_x"] * 8 - w)), constant_values=fill), 8)

    # Every fifth tile with a hit pixel that is lit in red: its hit pixels take the next entry of their own list (the same
    # one where the list has one entry) and a texel of another red, both in range. A lit pixel's red is a sum of texel
    # red times light, so such a tile changes whichever way its pixels' new entries turn out; a tile whose hit pixels
    # are all dark would not show a texel (and is not chosen). (The stand-in texture's blue has two values only.)
    lit = to_tiles(want[0][..., 0] != 0, False) & hit
    cand = np.argwhere(has & lit.any(axis=-1))[::5]
    assert len(cand) >= 1
    for ty, tx in cand:
        count = lists["lists"][(ty * 8 // bh) * nbx + (tx * 8 // bw)][0]
        assert count >= 1 and (entry[ty, tx][hit[ty, tx]] < count).all()
        e2 = (entry[ty, tx].astype(np.int64) + 1) % count
        for off in (ntex // 2 + 7, ntex // 3 + 11, ntex // 5 + 13, 12345):
            x2 = (texel[ty, tx] + off) % ntex
            if (tex[x2][hit[ty, tx], 0] != tex[texel[ty, tx]][hit[ty, tx], 0]).all():
                break
        else:
            pytest.fail("no texel of another red for tile %d, %d" % (ty, tx))
        new = rt.encode_primary_records(e2, x2)
        dw[ty, tx] = np.where(hit[ty, tx], new, dw[ty, tx])
        touched[ty, tx] = True
    sc.set_primary_records(dw)
    got = R.frame(sc, w, h)
    assert sc.primary_records()["state"] == 2
    diff = (got[0] != want[0]).any(axis=-1) | (got[1] != want[1])
    inside = np.kron(touched, np.ones((8, 8), dtype=bool))[:h, :w]
    assert (diff & inside).any()                             # the records reach the pixels ...
    assert not (diff & ~inside).any()                        # ... of the tiles touched, and of no others
    dd = np.zeros((touched.shape[0] * 8, touched.shape[1] * 8), dtype=bool)
    dd[:h, :w] = diff
    changed = dd.reshape(touched.shape[0], 8, touched.shape[1], 8).any(axis=(1, 3))
    assert np.array_equal(changed, touched), (int(changed.sum()), int(touched.sum()))   # exactly the tiles touched
    sc.set_primary_records(t["dwords"])
    R.assert_same(R.frame(sc, w, h), want, "original records back")
    # lanes outside the frame (in-range values there too): never consulted
    poisoned = t["dwords"].copy()
    outside = to_tiles(np.zeros((h, w), dtype=bool), True)
    assert outside.any()
    poisoned[outside] = rt.encode_primary_records(np.uint32(0), np.uint32(1))
    sc.set_primary_records(poisoned)
    R.assert_same(R.frame(sc, w, h), want, "lanes outside the frame poisoned")


def test_poisoned_records_of_tiles_without_one(rt, gpu, oracle):
    """The 8-sphere scene, and tiles of 64 x 1 at 96 x 54: where a tile says 0xfe in one valid lane, nothing else of it is read."""
    for inp, w, h, kw in ((Inputs(rt, 8), 64, 48, dict()), (Inputs(rt, 256), 96, 54, dict(tile=64))):
        want = R.oracle_frame(oracle, inp, w, h)
        sc, t = recorded(inp, w, h, want, launches=3, **kw)
        none = (t["positions"] == -2).all(axis=-1) & ((t["dwords"] & 0xff) == rt.RT_PRIMARY_NONE).any(axis=-1)
        if not none.any():
            print("%d spheres %s: every tile has a record" % (inp.n, kw))
            continue
        dw = t["dwords"].copy()
        keep = dw[none][:, :1].copy()
        dw[none] = rt.encode_primary_records(np.uint32(0), np.uint32(2))   # in range; one valid lane keeps its 0xfe
        first = np.argwhere(none)
        for (ty, tx), k in zip(first, keep):
            dw[ty, tx, 0] = k[0]
        sc.set_primary_records(dw)
        for k in range(2):
            R.assert_same(R.frame(sc, w, h, **kw), want, "%d spheres %s: poisoned, launch %d" % (inp.n, kw, k))
        assert sc.primary_records()["tiles_recorded"] == t["tiles_recorded"]


def test_view_list_evicted_between_record_and_read(rt, gpu, oracle):
    """View A rests (0 1 2); four other views get one launch each; A comes back three times. Every launch is the
    oracle's frame, whatever became of A's table and of its view list."""
    inp = Inputs(rt, 256)
    w, h = 96, 54
    cams = [inp.cam] + [rt.Camera(rt.Vec3(4.0 + 0.25 * k, 3.0, 10.0 - 0.5 * k), rt.Vec3(0, 0, 1), 0.0, 180.0 - 3.0 * k, -20.0)
                        for k in range(1, 5)]
    wants = []
    for cam in cams:
        inp.cam = cam
        wants.append(R.oracle_frame(oracle, inp, w, h))
    inp.cam = cams[0]
    sc = inp.scene()
    states = []
    for k, v in enumerate([0, 0, 0, 1, 2, 3, 4, 0, 0, 0]):
        R.assert_same(R.frame(sc, w, h, cam=cams[v]), wants[v], "launch %d, view %d" % (k, v))
        states.append(sc.primary_records()["state"])
    print("states over A A A B C D E A A A:", states)
    assert states[:3] == [0, 1, 2]


def test_switch_off(rt, refs):
    inp, want = refs[256]
    w, h = SIZES[256]
    sc = inp.scene()
    sc.set_light_verdicts(0)
    for k in range(4):
        R.assert_same(R.frame(sc, w, h), want, "launch %d" % k)
        info = sc.primary_records(want_tables=True)
        assert info["state"] == 0 and info["slot"] == -1 and "dwords" not in info


def test_verdict_and_shadow_count_read_backs_are_unchanged(rt, refs):
    """The words, the tags and the shadow-count records keep their offsets in front of the primary records: their
    read-backs after a recording launch equal those of a second scene's, and rewriting the primary records leaves them."""
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc, t = recorded(inp, w, h, want)
    words = sc.light_verdicts(want_words=True)
    counts = sc.shadow_counts(want_tables=True)
    assert words["state"] == 1 and words["unwritten"] == 0 and (words["tiles_x"], words["tiles_y"]) == (20, 12)
    assert counts["records"] >= 1 and counts["tagged"] >= 1
    sc.set_primary_records(t["dwords"])
    again_w, again_c = sc.light_verdicts(want_words=True), sc.shadow_counts(want_tables=True)
    assert np.array_equal(words["words"], again_w["words"])
    assert np.array_equal(counts["tags"], again_c["tags"]) and np.array_equal(counts["counts"], again_c["counts"])
    sc.set_shadow_counts(tags=counts["tags"], counts=counts["counts"])
    assert np.array_equal(sc.primary_records(want_tables=True)["dwords"], t["dwords"])
    for k in range(2):
        R.assert_same(R.frame(sc, w, h), want, "after the rewrites, launch %d" % k)
