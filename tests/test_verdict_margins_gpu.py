"""The margin scenes of tests/margins.py and tests/view_margins.py as RESTING views: each frame
four times on one long-lived scene, so that the kernel that records light verdicts (MODE 7) and the one that reads them
(MODE 6) meet the scenes placed on the culling bounds whose decisions they record and reuse -- the facing test, the full
occluder, the pre-pass's `dark`, the all-clear test. Every launch must give the oracle's frame, bit for bit in float4
and packed words. The device's table is read only to show that the reading paths ran (the summary test) and, for the
facing_away row, to hold the meaning of its words against the reference's arithmetic."""
import numpy as np
import pytest

import margins as M
import verdict_runs as R
import view_margins as V
from scenes import Scn

pytestmark = pytest.mark.gpu

CASES = [(name, seed) for name, (_, seeds) in M.BUILDERS.items() for seed in seeds]
VIEW_CASES = [(name, seed) for name, (_, seeds) in V.BUILDERS.items() for seed in seeds]
LIGHT_ROWS = ("shadow_rounding", "t_threshold", "shortcut_sure", "shortcut_behind", "prepass_guard", "full_occluder",
              "list_ball", "facing_away")

# the ledger row a builder's scenes belong to, where that is not its own name: full_occluder's sweep stays within 1e-2 of
# the edge, where the kernel's conservative test of the whole beam never holds (no table of its 80 scenes has any code);
# full_occluder_inside holds the scenes of the same row in which it does
FAMILY = {"full_occluder_inside": "full_occluder"}

SEEN = {}     # (family, seed) -> {"nothing", "clear", "multi"} of the case's tables, or None: the case failed


def _build(mod, name, seed):
    """The margin scene, built once per process: the cache is the one the margin tests themselves use."""
    from test_margins_gpu import _margin as margin
    from test_view_margins_gpu import _margin as view_margin
    return (margin if mod is M else view_margin)(name, seed)


def _scn(rt, m):
    return Scn(rt, m.spheres, lights=m.lights, cam=V.camera(rt, m.cam), aspect=m.aspect)


def _multi_group_tiles(scene, sc, m, band):
    """Tiles (8 x 8) of the frame whose pixels hit two or more different spheres: two or more groups."""
    import torch
    y0, y1 = band or (0, 0)
    ids = scene.render(m.w, m.h, y0=y0, y1=y1, cam=sc.cam, aspect=m.aspect, aov=("id",))["aov"]["id"].cpu().numpy()
    torch.cuda.synchronize()
    n = 0
    for ty in range(0, ids.shape[0], 8):
        for tx in range(0, ids.shape[1], 8):
            t = ids[ty:ty + 8, tx:tx + 8].reshape(-1, 2)
            n += len({int(i) for k, i in t if k >= 0}) >= 2
    return n


def _rest(rt, oracle, key, m, tiles, band=None):
    """The margin's frame at every tile shape, each as a resting view of one scene; -> the words recorded at each."""
    SEEN[key] = None
    sc = _scn(rt, m)
    y0, y1 = band or (0, 0)
    want = R.oracle_frame(oracle, sc, m.w, m.h, y0, y1)
    scene = sc.scene()
    words = {}
    for tile in tiles:
        kw = dict(width=m.w, height=m.h, y0=y0, y1=y1, cam=sc.cam, aspect=m.aspect, tile=tile)
        words[tile] = R.resting(scene, kw, want, what="%s seed %d tile %d" % (key[0], key[1], tile))
    c = np.concatenate([R.codes(w).reshape(-1) for w in words.values()])
    SEEN[key] = {"nothing": int((c == R.NOTHING).sum()), "clear": int((c == R.CLEAR).sum()),
                 "multi": _multi_group_tiles(scene, sc, m, band) if key[0] in ("front_to_back", "view_order") else 0}
    return sc, scene, want, words


@pytest.mark.parametrize("name,seed", [c for c in CASES if c[0] != "facing_away"])
def test_margin_scene_at_rest_equals_oracle(rt, gpu, oracle, name, seed):
    _rest(rt, oracle, (name, seed), _build(M, name, seed), (8, 16))


@pytest.mark.parametrize("name,seed", VIEW_CASES)
def test_view_margin_scene_at_rest_equals_oracle(rt, gpu, oracle, name, seed):
    m = _build(V, name, seed)
    if m.spp == 1:
        _rest(rt, oracle, (name, seed), m, m.tiles, m.band)
        return
    # verdicts are for one-sample launches: a multi-sample margin never takes a table
    sc = _scn(rt, m)
    scene = sc.scene()
    y0, y1 = m.band or (0, 0)
    frames = []
    for k in range(3):
        frames.append(R.frame(scene, m.w, m.h, y0=y0, y1=y1, spp=m.spp, cam=sc.cam, aspect=m.aspect, tile=m.tiles[0]))
        assert scene.light_verdicts()["state"] == 0, (name, seed, k)
    R.assert_same(frames[1], frames[0], "second launch")
    R.assert_same(frames[2], frames[0], "third launch")


def _with_light0(rt, sc, **fields):
    lights = (rt.Light * sc.n_lights)()
    for i in range(sc.n_lights):
        l = sc.lights[i]
        lights[i] = rt.Light(rt.Vec3(l.pos.x, l.pos.y, l.pos.z), l.size, l.r, l.g, l.b)
    for k, v in fields.items():
        setattr(lights[0], k, v)
    return lights


def _settle(rt, oracle, sc, scene, kw, tag):
    """Three more frames of a warmed-up scene whose inputs just changed (`sc` holds the new ones): each equals a fresh
    scene's frame and the brute-force frame bit for bit, and the oracle's (NaNs as they come if the oracle's NaN bit
    patterns are the device's, else NaN matched with NaN: the assertion message says which). -> the new table."""
    fresh = sc.scene()
    fresh.set_light_verdicts(0)
    w, h = kw["width"], kw["height"]
    opts = {k: v for k, v in kw.items() if k not in ("width", "height")}
    want = R.frame(fresh, w, h, **opts)
    R.assert_same(R.frame(fresh, w, h, cull=False, **opts), want, tag + ": brute force against a fresh scene")
    orc = R.oracle_frame(oracle, sc, w, h)
    nan_bits_agree = R.differing(want, orc) == (0, 0)
    R.assert_same(want, orc, tag + ": fresh scene against the oracle, NaN bits %s" % ("as they are" if nan_bits_agree else "matched as NaN"),
                  nan_equal=not nan_bits_agree)
    states, words = [], None
    for k in range(3):
        R.assert_same(R.frame(scene, w, h, **opts), want, "%s: launch %d after the change" % (tag, k))
        info = scene.light_verdicts(want_words=True)
        states.append(info["state"])
        if info["state"] == 1:
            assert info["unwritten"] == 0
            words = info["words"]
    assert states == [0, 1, 2], (tag, states)
    return words


@pytest.mark.parametrize("seed", M.BUILDERS["facing_away"][1])
def test_facing_away_words_mean_what_the_reference_says(rt, gpu, oracle, seed):
    """The first of the three "adds nothing" exits (normal.toL < -1e-4 for every lane of the group). Frames as for every
    margin; and the words: a tile whose 64 pixels all lie 1e-5 below the bound (by the reference's start and normal in
    binary64) carries code 1 for light 0; a tile wholly 1e-5 above it does not -- the light is unshadowed (witness
    `open`), so neither a full occluder nor `dark` can give that code. Then the same warmed-up scene with a non-finite
    light colour, and with a non-finite texel under the patch: no lane may take 0 x inf for 0, so no code 1 for light 0."""
    m = _build(M, "facing_away", seed)
    wit = m.witness
    sc, scene, want, words = _rest(rt, oracle, ("facing_away", seed), m, (8, 16))
    c = R.codes(words[8])
    assert wit["away_tiles"] and wit["lit_tiles"] and wit["open"]
    for tx, ty in wit["away_tiles"]:
        assert c[ty, tx, 0, 0] == R.NOTHING, ("away", seed, tx, ty, c[ty, tx, 0])
    for tx, ty in wit["lit_tiles"]:
        assert c[ty, tx, 0, 0] != R.NOTHING, ("lit", seed, tx, ty, c[ty, tx, 0])
    kw = dict(width=m.w, height=m.h, cam=sc.cam, aspect=m.aspect, tile=8)

    # light 0's blue is inf: L.fin == 0, no lane is zero_ok, none of the three exits may be taken for light 0
    sc.lights = _with_light0(rt, sc, b=float("inf"))
    scene.set_lights(sc.lights, sc.n_lights)
    c = R.codes(_settle(rt, oracle, sc, scene, kw, "light 0 blue = inf"))
    assert not (c[:, :, :, 0] == R.NOTHING).any(), (seed, np.argwhere(c[:, :, :, 0] == R.NOTHING)[:4])

    # the light finite again, one texel under the patch not: frames only
    sc.lights = _with_light0(rt, sc, b=float(m.lights[0][4]))
    scene.set_lights(sc.lights, sc.n_lights)
    texel = wit["texel"]                     # the one most pixels of the patch read, by the reference's arithmetic
    assert wit["texel_pixels"] >= 64
    sc.tex = [p.copy() for p in sc.tex]
    sc.tex[seed % 3][texel] = np.inf
    scene.set_texture(sc.tex)
    _settle(rt, oracle, sc, scene, kw, "texel %s = inf" % (texel,))


def test_the_reading_paths_ran(rt, gpu, oracle):
    """Over the cases above (run here if they have not been): every light-row family has a table with a code 1, some table
    holds a code 2, and a front_to_back or view_order scene has a tile of two or more groups -- so the frames above were
    not all rendered with tables that skip nothing. (Measured: the 80 scenes of full_occluder's sweep record no code at
    all, 0 entries of either kind; the four full_occluder_inside scenes of the same row record 87 entries of code 1.)"""
    for name, seed in CASES:
        if (name, seed) not in SEEN and name != "facing_away":
            try:
                _rest(rt, oracle, (name, seed), _build(M, name, seed), (8, 16))
            except AssertionError:
                pass
    for name, seed in VIEW_CASES:
        if (name, seed) not in SEEN:
            m = _build(V, name, seed)
            if m.spp == 1:
                try:
                    _rest(rt, oracle, (name, seed), m, m.tiles, m.band)
                except AssertionError:
                    pass
    for seed in M.BUILDERS["facing_away"][1]:
        if ("facing_away", seed) not in SEEN:
            try:
                _rest(rt, oracle, ("facing_away", seed), _build(M, "facing_away", seed), (8, 16))
            except AssertionError:
                pass
    fam = {}
    for (name, _), s in SEEN.items():
        f = fam.setdefault(FAMILY.get(name, name), {"cases": 0, "failed": 0, "with_nothing": 0, "nothing": 0, "clear": 0, "multi": 0})
        f["cases"] += 1
        if s is None:
            f["failed"] += 1
            continue
        f["with_nothing"] += s["nothing"] > 0
        for k in ("nothing", "clear", "multi"):
            f[k] += s[k]
    for name in sorted(fam):
        print(name, fam[name])
    for name in LIGHT_ROWS:
        assert fam[name]["with_nothing"] >= 1, (name, fam[name])
    assert sum(f["clear"] for f in fam.values()) >= 1
    assert fam["front_to_back"]["multi"] + fam["view_order"]["multi"] >= 1
