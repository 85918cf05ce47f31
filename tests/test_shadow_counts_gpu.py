"""Shadow counts of a resting view: the launch that records a tile's light verdicts also keeps,
for up to `records` of the lights it walked to the end (code 0: neither dark nor clear), every lane's number of unshadowed
samples; the reading launches take the count from the record in place of the occluder search and the ten samples. Every
frame must stay the same bits as with the switch off, as the brute-force kernel's and as the oracle's; the read-back
(Scene.shadow_counts) and the setter (Scene.set_shadow_counts) show that the records exist, are well formed, are the
only thing read, and are really read."""
import ctypes as C

import numpy as np
import pytest

import verdict_runs as R
from scenes import Inputs, Scn

pytestmark = pytest.mark.gpu

SIZES, layouts, rows_of, tagged_of = R.SIZES, R.layouts, R.rows_of, R.tagged_of


@pytest.fixture(scope="module")
def refs(rt, gpu, oracle):
    return R.oracle_refs(rt, oracle)


@pytest.mark.parametrize("n", sorted(SIZES))
@pytest.mark.parametrize("layout", ["tile8", "tile16", "tile32", "tile64", "band", "interleave"])
def test_frames_at_rest(rt, refs, n, layout):
    w, h = SIZES[n]
    kw = layouts(h)[layout]
    inp, whole = refs[n]
    rows = rows_of(rt, h, kw)
    want = (whole[0][rows], whole[1][rows])
    R.switched_off(inp, w, h, want, read_back="shadow_counts", **kw)
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h, **kw), want, launches=5, what="%d %s" % (n, layout))
    info = sc.shadow_counts()
    tiles = info["tiles_x"] * info["tiles_y"]
    print("%d spheres, %s: %d of %d tiles have a record (%.1f %%), %d records" %
          (n, layout, info["tiles_tagged"], tiles, 100.0 * info["tiles_tagged"] / tiles, info["tagged"]))
    assert info["state"] == 2 and (info["tiles_x"], info["tiles_y"]) == R.grid(w, h, kw)
    assert info["tagged"] >= 1 and info["records"] >= 1   # (against a vacuous pass)


def rest(inp, w, h, want, launches=3, **kw):
    sc = inp.scene()
    words = R.resting(sc, dict(width=w, height=h, **kw), want, launches=launches)
    return sc, words, sc.shadow_counts(want_tables=True)


def test_read_back_invariants_and_poisoned_free_records(refs):
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc, words, t = rest(inp, w, h, want)
    used, grp, li = tagged_of(t["tags"])
    recs = t["records"]
    assert not used[..., recs:].any()                       # bytes beyond the records stay 0
    assert used.any()
    codes = R.codes(words)
    for ty, tx, r in zip(*np.nonzero(used)):
        assert grp[ty, tx, r] < R.GROUPS and codes[ty, tx, grp[ty, tx, r], li[ty, tx, r]] == 0, (ty, tx, r)
        mine = t["tags"][ty, tx][used[ty, tx]]
        assert len(set(mine.tolist())) == len(mine), (ty, tx)   # no (group, light) twice
    assert t["counts"][used[..., :recs]].max() <= 10            # every lane of a record in use: 0..10 samples
    assert (t["counts"][used[..., :recs]] > 0).any()
    # free records are never read: poison them, the frames stay
    poisoned = t["counts"].copy()
    poisoned[~used[..., :recs]] = 0xee
    sc.set_shadow_counts(counts=poisoned)
    for k in range(2):
        R.assert_same(R.frame(sc, w, h), want, "poisoned free records, launch %d" % k)
        assert sc.shadow_counts()["state"] == 2


def test_reader_consumes_the_records(refs):
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc, _, t = rest(inp, w, h, want)
    used, _, _ = tagged_of(t["tags"])
    used = used[..., :t["records"]]
    flipped = t["counts"].copy()
    flipped[used] = 10 - flipped[used]
    sc.set_shadow_counts(counts=flipped)
    got = R.frame(sc, w, h)
    assert sc.shadow_counts()["state"] == 2
    diff = (got[0] != want[0]).any(axis=-1) | (got[1] != want[1])
    assert diff.any()                                        # the counts reach the pixels ...
    tile_has = used.any(axis=-1)
    inside = np.kron(tile_has, np.ones((8, 8), dtype=bool))[:h, :w]
    assert not (diff & ~inside).any()                        # ... of the tiles with a record, and no others
    sc.set_shadow_counts(counts=t["counts"])
    R.assert_same(R.frame(sc, w, h), want, "original counts back")


def test_capacity(rt, gpu):
    """More walked lights in a tile than it has records, and more groups than a word has: the surplus has no tag."""
    pos = [(20, 20, 20), (0, 20, -20), (0, 20, 0), (-20, 15, 5), (10, 25, -5), (25, 8, 0), (-5, 30, 12), (3, 18, 25)]
    lights = [(p, 20, 0.2 + 0.1 * (i % 3), 0.1 * (i % 4), 0.15 * (i % 5)) for i, p in enumerate(pos)]
    inp = Inputs(rt, 256)
    inp.lights, inp.n_lights = Scn(rt, [], lights=lights).lights, 8
    w, h = 160, 90
    ref = inp.scene()
    ref.set_light_verdicts(0)
    want = R.frame(ref, w, h, cull=False)
    sc, words, t = rest(inp, w, h, want, launches=4)
    used, grp, li = tagged_of(t["tags"])
    recs = t["records"]
    c0 = R.codes(words)[..., 0, :]                           # the first group exists wherever the word is not 0
    walked = ((c0 == 0).sum(axis=-1) * (words != 0))         # its code-0 lights: every one of them was walked
    assert (walked > recs).any(), int(walked.max())
    full = used[..., :recs].all(axis=-1)
    assert full[walked > recs].all() and not used[..., recs:].any()
    # more than four groups in a tile: groups beyond the fourth carry no tag
    g = rt.generate_spheres(4096, 3)
    tiny = Scn(rt, [(g[i].orgin.x, g[i].orgin.y, g[i].orgin.z, 0.12) for i in range(4096)])
    ref = tiny.scene()
    ref.set_light_verdicts(0)
    want = R.frame(ref, w, h, cull=False)
    sc, words, t = rest(tiny, w, h, want, launches=4)
    used, grp, li = tagged_of(t["tags"])
    assert used.any() and (grp[used] < R.GROUPS).all()
    cd = R.codes(words)
    assert (cd[..., 3, :] != 0).any()                        # tiles with at least four groups exist (test_light_verdicts: some have more)


def test_invalidation(rt, gpu):
    inp = Inputs(rt, 1024)
    sc = inp.scene()
    size = [160, 90]

    def settle(tag):
        fresh = inp.scene()
        fresh.set_light_verdicts(0)
        want = R.frame(fresh, *size)
        R.assert_same(R.frame(fresh, *size, cull=False), want, tag + ": fresh scene against brute force")
        states = []
        for k in range(4):
            R.assert_same(R.frame(sc, *size), want, "%s, launch %d" % (tag, k))
            states.append(sc.light_verdicts()["state"])
        assert states == [0, 1, 2, 2], (tag, states)
        assert sc.shadow_counts()["tagged"] >= 1, tag

    settle("start")
    inp.lights = R.copy_lights(rt, inp.lights, 3)
    inp.lights[0].pos.x = 14.0
    sc.set_lights(inp.lights, 3)
    settle("a light moved")
    inp.spheres = rt.generate_spheres(1024, 1)
    rt.load_library().rt_sphere_init(C.byref(inp.spheres[5]), 4.0, 3.0, 6.0, 0.9)
    sc.set_spheres(inp.spheres, 1024)
    settle("a sphere changed")
    inp.tex = [p.copy() for p in inp.tex]
    inp.tex[0][:, ::2] *= np.float32(0.5)
    sc.set_texture(inp.tex)
    settle("texture changed")
    size[:] = [96, 54]
    settle("frame size changed")


def test_two_views_alternating(rt, gpu):
    inp = Inputs(rt, 256)
    cams = [inp.cam, rt.Camera(rt.Vec3(4.5, 3, 10), rt.Vec3(0, 0, 1), 0.0, 171.0, -20.0)]
    ref = inp.scene()
    ref.set_light_verdicts(0)
    wants = [R.frame(ref, 96, 54, cam=c, cull=False) for c in cams]
    sc = inp.scene()
    states = []
    for k in range(10):
        R.assert_same(R.frame(sc, 96, 54, cam=cams[k % 2]), wants[k % 2], "launch %d" % k)
        states.append(sc.light_verdicts()["state"])
        if states[-1] == 2:
            assert sc.shadow_counts()["state"] == 2
    assert states[-2:] == [2, 2], states                     # both views end reading


def test_tagged_all_sums_the_tables_of_both_views(rt, refs):
    """The read-back walks the scene's tables once: `tagged` is the last launch's table, `tagged_all` every table's. With
    one view at rest the two agree; once a second view has settled beside it, `tagged_all` is the sum of what `tagged`
    said right after each view's own launches."""
    inp, want = refs[256]
    w, h = SIZES[256]
    sc = inp.scene()
    R.resting(sc, dict(width=w, height=h), want, launches=3)
    a = sc.shadow_counts()
    assert a["state"] == 2 and a["tagged"] >= 1 and a["tagged_all"] == a["tagged"], a
    cam = rt.Camera(rt.Vec3(4.5, 3, 10), rt.Vec3(0, 0, 1), 0.0, 171.0, -20.0)
    ref = inp.scene()
    ref.set_light_verdicts(0)
    R.resting(sc, dict(width=w, height=h, cam=cam), R.frame(ref, w, h, cam=cam, cull=False), launches=3, what="second view")
    b = sc.shadow_counts()
    assert b["state"] == 2 and b["slot"] != a["slot"], (a, b)
    assert b["tagged_all"] >= b["tagged"] and b["tagged_all"] == a["tagged"] + b["tagged"], (a, b)


def test_two_streams_after_the_recording_launch(refs):
    import torch
    inp, want = refs[1024]
    w, h = SIZES[1024]
    sc = inp.scene()
    for k in range(2):
        R.assert_same(R.frame(sc, w, h), want, "launch %d" % k)
    assert sc.light_verdicts()["state"] == 1
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for k in range(6):
        with torch.cuda.stream(streams[k % 2]):
            outs.append(sc.render(w, h, stream=streams[k % 2]))
    torch.cuda.synchronize()
    assert sc.light_verdicts()["state"] == 2 and sc.shadow_counts()["tagged"] >= 1
    for k, o in enumerate(outs):
        R.assert_same((R._bits(o["rgba"].cpu().numpy()), o["packed"].cpu().numpy().view(np.uint32)), want, "in flight %d" % k)


def test_update_in_three_bands(rt, gpu, oracle):
    lib = rt.load_library()
    with R.App(rt, 256, 11, 64, 528) as app:
        want = R.oracle_frame(oracle, app.inp, 64, 528)[1]
        states = []
        for k in range(5):
            got, state = app.update()
            assert np.array_equal(got, want), (k, state, int((got != want).sum()))
            states.append(state)
        assert states == [0, 1, 2, 2, 2], states
        info = rt.ShadowCountsInfo()
        assert lib.rt_debug_shadow_counts(lib.rt_debug_shim_scene(), C.byref(info), None, None, 0) == 0, lib.rt_last_error()
        # (the read-back is that of the frame's last launch, the third band; the three bands' tables together hold the records)
        print("last band: %d records in %d x %d tiles; all bands: %d" % (info.tagged, info.tiles_x, info.tiles_y, info.tagged_all))
        assert info.state == 2 and info.tagged_all >= 1


def test_moving_camera_records_nothing(rt, gpu):
    inp = Inputs(rt, 256)
    sc = inp.scene()
    ref = inp.scene()
    ref.set_light_verdicts(0)
    for k in range(5):
        cam = rt.default_camera()
        cam.Org.z = 10.0 + 0.0625 * k
        R.assert_same(R.frame(sc, 96, 54, cam=cam), R.frame(ref, 96, 54, cam=cam, cull=False), "launch %d" % k)
        assert sc.light_verdicts()["state"] == 0
        info = sc.shadow_counts()
        assert info["state"] == 0 and info["tagged"] == 0
