"""The compact reading launch of a resting view: once a table has a run list and the list's counts
have reached the host, a reading launch starts one workgroup per tile that still computes and one per run of R settled
tiles. The frame must be the full grid's, bit for bit, in every layout and tile shape; the geometry and the list must be
what the numpy model (tests/compact_ref.py) derives from the read-back summaries and records. Every launch here is
followed by a device synchronise (verdict_runs.frame), so the launches of a view go: plain, recording, reading with the
full grid (the list is built), compact from the fourth on."""
import numpy as np
import pytest

import compact_ref as M
import verdict_runs as R
from scenes import Inputs

pytestmark = pytest.mark.gpu

W, H, N = 160, 90, 1024
RUN = 64  # RT_COMPACT_RUN, the default
EDGE = 8  # the run length of the boundary cases (160 x 90 has fewer than 65 streamable tiles to keep)


@pytest.fixture(autouse=True)
def every_share_goes_compact(monkeypatch):
    """The library keeps the full grid where less than a quarter of the tiles would be streamed; the small frames here
    have fewer, and the boundary cases none at all: scenes made by Inputs.scene go compact at any share."""
    plain = Inputs.scene

    def scene(self):
        sc = plain(self)
        sc.set_compact_run(64, 1, 0)
        return sc
    monkeypatch.setattr(Inputs, "scene", scene)


@pytest.fixture(scope="module")
def refs(rt, gpu, oracle):
    inp = Inputs(rt, N)
    return inp, R.oracle_frame(oracle, inp, W, H)


def rested(inp, want, launches=4, compact=1, **kw):
    sc = inp.scene()
    sc.set_compact_launch(compact)
    for k in range(launches):
        R.assert_same(R.frame(sc, W, H, **kw), want, "launch %d" % k)
    return sc


@pytest.mark.parametrize("layout", sorted(R.layouts(H)))
def test_frames_equal_in_every_layout(rt, refs, layout):
    """Twelve launches of one view (re-sorts at 2, 4 and 8 rebuild the list), each the oracle's bits; the switch off
    gives the same and never a compact launch; the plain kernel (light verdicts off) is verdict_runs.switched_off's."""
    inp, whole = refs
    kw = R.layouts(H)[layout]
    rows = R.rows_of(rt, H, kw)
    want = (whole[0][rows], whole[1][rows])
    sc = inp.scene()
    seen = []
    for k in range(12):
        R.assert_same(R.frame(sc, W, H, **kw), want, "%s launch %d" % (layout, k))
        seen.append(sc.compact_launch())
    assert [i["compact"] for i in seen[:3]] == [0, 0, 0] and all(i["compact"] == 1 for i in seen[3:]), [i["compact"] for i in seen]
    last = seen[-1]
    tx, ty = R.grid(W, H, kw)
    assert last["n_unsettled"] + last["n_streamed"] == tx * ty and last["run"] == RUN
    assert last["workgroups"] == M.workgroups(last["n_unsettled"], last["n_streamed"], RUN)
    assert last["rebuilds"] >= 3, last            # after the recording launch and after the re-sorts at 4 and 8
    off = rested(inp, want, launches=5, compact=0, **kw)
    info = off.compact_launch()
    assert (info["compact"], info["workgroups"], info["rebuilds"]) == (0, 0, 0), info
    R.switched_off(inp, W, H, want=want, what=layout + " ", **kw)


@pytest.mark.parametrize("tile,size", [(16, 256), (32, 512), (64, 1024)])
def test_wider_tiles_stream_too(rt, gpu, tile, size):
    """The smallest squares whose view-list blocks hold the tile (test_settled_tiles_gpu): settled tiles exist there."""
    inp = Inputs(rt, 256)
    ref = inp.scene()
    ref.set_light_verdicts(0)
    want = R.frame(ref, size, size, cull=False)
    sc = inp.scene()
    for k in range(5):
        R.assert_same(R.frame(sc, size, size, tile=tile), want, "tile %d launch %d" % (tile, k))
    info = sc.compact_launch()
    assert info["compact"] == 1 and info["n_streamed"] >= 1, info


@pytest.mark.parametrize("kw", [dict(want_rgba=False), dict(want_packed24=True), dict(tile_order=0)], ids=["no_rgba", "packed24", "grid_order"])
def test_other_outputs_and_orders(rt, refs, kw):
    inp, want = refs
    kw = dict(kw)
    order = kw.pop("tile_order", 1)
    import torch
    on, off = inp.scene(), inp.scene()
    off.set_compact_launch(0)
    for sc in (on, off):
        sc.set_tile_order(order)
    for k in range(5):
        a, b = on.render(W, H, **kw), off.render(W, H, **kw)
        torch.cuda.synchronize()
        for key in ("packed", "rgba", "packed24"):
            if a.get(key) is not None:
                assert np.array_equal(a[key].cpu().numpy().view(np.uint32), b[key].cpu().numpy().view(np.uint32)), (key, k)
        assert np.array_equal(a["packed"].cpu().numpy().view(np.uint32), want[1]), k
    assert on.compact_launch()["compact"] == 1 and off.compact_launch()["compact"] == 0


def model_of(rt, sc, order=None):
    s = sc.tile_summaries(want_tables=True)["dwords"]
    p = sc.primary_records(want_tables=True)["dwords"]
    ty, tx = s.shape
    mask = M.streamable(s, p, M.valid_lanes(W, H, 8, ty, tx))
    return M.run_list(M.grid_order(ty, tx) if order is None else order, mask), mask


def test_geometry_and_list_against_the_model(rt, refs):
    inp, want = refs
    for order in (0, 1):
        sc = inp.scene()
        sc.set_tile_order(order)
        for k in range(4):
            R.assert_same(R.frame(sc, W, H), want, "launch %d" % k)
        info = sc.compact_launch(want_list=True)
        (lst, n_u, n_s), mask = model_of(rt, sc)
        assert info["compact"] == 1 and info["list_built"] == 1
        assert (info["n_unsettled"], info["n_streamed"]) == (n_u, n_s) == (info["list_n_unsettled"], info["list_n_streamed"]), (info, n_u, n_s)
        assert n_s >= 2 and n_u >= 1
        assert info["workgroups"] == M.workgroups(n_u, n_s, RUN)
        got = info["list"]
        assert sorted(got.tolist()) == M.grid_order(*mask.shape).tolist()         # a permutation of the tiles
        built_from = sc.compact_order(got.size)
        if order == 0:
            assert np.array_equal(built_from, M.grid_order(*mask.shape))
            assert np.array_equal(got, lst)                                       # grid order: the model's list itself
        else:   # the sorted order, read back: the list is the model's partition of it, element by element
            assert np.array_equal(got, M.run_list(built_from, mask)[0])


def doctored(rt, inp, want, keep, compact, ahead):
    """A rested scene whose summaries keep RT_TILE_SETTLED on the first `keep` streamable tiles only (-1: every tile is
    said to be settled without a miss lane), and its next two frames."""
    sc = inp.scene()
    sc.set_compact_launch(compact)
    sc.set_compact_run(EDGE, ahead)
    for k in range(4):
        R.assert_same(R.frame(sc, W, H), want, "launch %d" % k)
    d = sc.tile_summaries(want_tables=True)["dwords"].copy()
    if keep < 0:
        d[:] = rt.RT_TILE_SETTLED | rt.RT_TILE_NO_MISS
    else:
        (_, _, _), mask = model_of(rt, sc)
        idx = np.argwhere(mask)
        assert len(idx) > keep
        d[~mask] &= ~np.uint32(rt.RT_TILE_SETTLED)
        for y, x in idx[keep:]:
            d[y, x] &= ~np.uint32(rt.RT_TILE_SETTLED)
    before = sc.compact_launch()["rebuilds"]
    sc.set_tile_summaries(d)
    frames = [R.frame(sc, W, H), R.frame(sc, W, H)]
    return sc, frames, before


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("keep", [0, 1, EDGE - 1, EDGE, EDGE + 1, -1])
def test_run_boundaries(rt, refs, keep, ahead):
    """n_streamed = 0, 1, R - 1, R, R + 1 and T (then n_unsettled = 0) through the setter, R = 8, the runs behind and ahead; the expected frame is the full
    grid's over the same doctored table. The setter makes the list stale: the rebuild count goes up, the first frame
    after it keeps the full grid, the second is compact with the new counts."""
    inp, want = refs
    on, got, before = doctored(rt, inp, want, keep, 1, ahead)
    _, exp, _ = doctored(rt, inp, want, keep, 0, ahead)
    for g, e in zip(got, exp):
        R.assert_same(g, e, "keep %d" % keep)
    if keep >= 0:
        R.assert_same(got[1], want, "keep %d against the oracle" % keep)
    info = on.compact_launch()
    tiles = info["tiles_x"] * info["tiles_y"]
    assert info["compact"] == 1 and info["rebuilds"] == before + 1, (info, before)
    assert info["n_streamed"] == (tiles if keep < 0 else keep) and info["n_unsettled"] == tiles - info["n_streamed"], info
    assert info["workgroups"] == M.workgroups(info["n_unsettled"], info["n_streamed"], EDGE) and info["ahead"] == ahead


def test_a_settled_tile_without_a_record_keeps_its_wave(rt, refs):
    inp, want = refs
    sc = rested(inp, want)
    s = sc.tile_summaries(want_tables=True)["dwords"]
    p = sc.primary_records(want_tables=True)["dwords"].copy()
    cand = np.argwhere(((s & 3) == rt.RT_TILE_SETTLED))      # settled, with miss lanes
    assert len(cand) >= 1
    y, x = cand[0]
    p[y, x, 0] = (p[y, x, 0] & ~np.uint32(0xff)) | np.uint32(M.PRIMARY_NONE)
    before = sc.compact_launch()["rebuilds"]
    sc.set_primary_records(p)
    R.frame(sc, W, H)
    R.assert_same(R.frame(sc, W, H), want, "a settled tile whose record says none")
    info = sc.compact_launch(want_list=True)
    assert info["compact"] == 1 and info["rebuilds"] == before + 1
    assert ((int(y) << 16) | int(x)) in info["list"][:info["n_unsettled"]].tolist()
