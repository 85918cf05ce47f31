"""The compact reading launch, the cases beside tests/test_compact_launch_gpu.py: every tile
shape in every layout with the streamed path running, the list against the order it was built from, element by
element, the outputs' coverage and guards (tests/arena.py), sample ranges that accumulate, frames in flight on two
streams across a rebuild and across a slot eviction, the runs ahead of the one-wave tiles, and the settled-tiles
suite with the switch either way."""
import numpy as np
import pytest

import compact_ref as M
import test_settled_tiles_gpu as S
import verdict_runs as R
from arena import run_twice, same_bytes
from scenes import Inputs

pytestmark = pytest.mark.gpu

RUN = 8      # run length of the coverage cases: several runs, and a last one that is not full, at these sizes
SQUARE = {8: 160, 16: 256, 32: 512, 64: 1024}     # the smallest squares whose view-list blocks hold the tile
LAYOUTS = {"whole": lambda s: dict(), "band": lambda s: dict(y0=16, y1=s - 22), "interleave": lambda s: dict(interleave=(3, 1, 16))}


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
def inp256(rt, gpu):
    return Inputs(rt, 256)


@pytest.fixture(scope="module")
def refs(rt, gpu, oracle):
    return R.oracle_refs(rt, oracle)


def rest(sc, w, h, launches=4, **kw):
    out = None
    for _ in range(launches):
        out = R.frame(sc, w, h, **kw)
    return out


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("tile", sorted(SQUARE))
def test_every_tile_shape_in_every_layout(rt, inp256, tile, layout):
    """The reference is the brute-force frame of a scene of its own with light verdicts off (the oracle is too slow at
    these sizes); the band ends inside a tile row of every shape but 64 x 1, and the streamed path must have run."""
    size = SQUARE[tile]
    kw = dict(LAYOUTS[layout](size), tile=tile)
    ref = inp256.scene()
    ref.set_light_verdicts(0)
    want = R.frame(ref, size, size, cull=False, **kw)
    on, off = inp256.scene(), inp256.scene()
    off.set_compact_launch(0)
    for k in range(5):
        R.assert_same(R.frame(on, size, size, **kw), want, "tile %d %s launch %d" % (tile, layout, k))
        R.assert_same(R.frame(off, size, size, **kw), want, "tile %d %s launch %d, switch off" % (tile, layout, k))
    info = on.compact_launch()
    assert info["compact"] == 1 and info["n_streamed"] >= 1 and info["n_unsettled"] >= 1, info
    assert (info["tiles_x"], info["tiles_y"]) == R.grid(size, size, kw)
    assert off.compact_launch()["compact"] == 0


@pytest.mark.parametrize("launches", [4, 6, 10])
def test_list_is_a_stable_partition_of_the_sorted_order(rt, refs, launches):
    """Tile order on (the default): after 4, 6 and 10 launches the list was built from the orders sorted at launch 2, 4
    and 8. Element by element it is the model's partition of that order, read back."""
    inp, want = refs[1024]
    w, h = R.SIZES[1024]
    sc = inp.scene()
    for k in range(launches):
        R.assert_same(R.frame(sc, w, h), want, "launch %d" % k)
    info = sc.compact_launch(want_list=True)
    assert info["compact"] == 1
    order = sc.compact_order(info["tiles_x"] * info["tiles_y"])
    assert sorted(order.tolist()) == M.grid_order(info["tiles_y"], info["tiles_x"]).tolist()
    assert not np.array_equal(order, M.grid_order(info["tiles_y"], info["tiles_x"]))          # a sorted order, not grid order
    s = sc.tile_summaries(want_tables=True)["dwords"]
    p = sc.primary_records(want_tables=True)["dwords"]
    lst, n_u, n_s = M.run_list(order, M.streamable(s, p, M.valid_lanes(w, h, 8, *s.shape)))
    assert (info["n_unsettled"], info["n_streamed"]) == (n_u, n_s)
    assert np.array_equal(info["list"], lst)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("w,h,kw", [(100, 54, dict()), (160, 90, dict(y0=16, y1=72)), (160, 74, dict(interleave=(3, 1, 16)))],
                         ids=["partial_tiles", "band", "interleave"])
def test_coverage_and_guards(rt, inp256, w, h, kw, ahead):
    """A compact launch into guard | payload | guard arenas of two patterns (a sentinel and a NaN): every element of
    rgba, packed and packed24 written, the same bytes both times and the wrapper's with the switch off, no guard touched
    -- so no lane beyond the frame's edge or the band's end stored anything."""
    rows = len(R.rows_of(rt, h, kw))
    sc = inp256.scene()
    sc.set_compact_run(RUN, ahead)
    rest(sc, w, h, **kw)
    outs = {"pixels": dict(nbytes=4 * w * rows, align=4), "rgba": dict(nbytes=16 * w * rows, align=16), "packed24": dict(nbytes=3 * w * rows, align=4)}

    def call(p):
        sc.render_raw(sc.frame_desc(w, h, pixels=p["pixels"], rgba=p["rgba"], packed24=p["packed24"], **kw), _stream())
        assert sc.compact_launch()["compact"] == 1 and sc.compact_launch()["ahead"] == ahead
    got = run_twice(call, outs)
    off = inp256.scene()
    off.set_compact_launch(0)
    out = off.render(w, h, want_packed24=True, **kw)
    for k, name in (("pixels", "packed"), ("rgba", "rgba"), ("packed24", "packed24")):
        same_bytes(got[k], out[name], k)
    # rgba = NULL: the packed words alone, the float4 arena not handed to the call stays all pattern
    outs2 = {"pixels": dict(nbytes=4 * w * rows, align=4), "rgba": dict(nbytes=16 * w * rows, align=16, written=False)}

    def call2(p):
        sc.render_raw(sc.frame_desc(w, h, pixels=p["pixels"], rgba=0, **kw), _stream())
        assert sc.compact_launch()["compact"] == 1
    same_bytes(run_twice(call2, outs2)["pixels"], out["packed"], "packed without rgba")


def test_sample_ranges_accumulate(rt, inp256):
    """Four one-sample launches of a four-sample frame, each its own resting view (sample_base is in the key), the last
    three adding to the float4 frame: after the views have come to rest every pass is compact, and the frame is the
    four-sample launch's."""
    import torch
    w, h = 160, 90
    sc = inp256.scene()
    want = sc.render(w, h, spp=4)
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    packed = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    compact = []
    for rnd in range(5):
        for k in range(4):
            fd = sc.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), spp=1, sample_base=k, sample_total=4,
                               accumulate=k > 0, resolve=0 if k == 3 else -1)
            sc.render_raw(fd, _stream())
            torch.cuda.synchronize()
            compact.append(sc.compact_launch()["compact"])
        assert np.array_equal(rgba.cpu().numpy().view(np.uint32), want["rgba"].cpu().numpy().view(np.uint32)), rnd
        assert np.array_equal(packed.cpu().numpy(), want["packed"].cpu().numpy()), rnd
    assert compact[-4:] == [1, 1, 1, 1], compact


def test_four_samples_in_one_launch_are_out_of_scope(rt, inp256):
    sc = inp256.scene()
    a = [sc.render(96, 54, spp=4) for _ in range(4)]
    assert sc.compact_launch()["compact"] == 0 and sc.compact_launch()["rebuilds"] == 0
    assert np.array_equal(a[0]["packed"].cpu().numpy(), a[3]["packed"].cpu().numpy())


def _in_flight(rt, inp, views, rounds, want):
    """`rounds` passes over `views` (render kwargs), frame k on stream k & 1, no host wait inside a pass: every frame
    equals want[view] bit for bit. -> the scene."""
    import torch
    sc = inp.scene()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    k = 0
    for rnd in range(rounds):
        outs = []
        for v, kw in enumerate(views):
            with torch.cuda.stream(streams[k & 1]):
                outs.append((v, sc.render(kw["w"], kw["h"], stream=streams[k & 1], **{a: b for a, b in kw.items() if a not in "wh"})))
            k += 1
        torch.cuda.synchronize()
        for v, o in outs:
            got = (o["rgba"].cpu().numpy().view(np.uint32), o["packed"].cpu().numpy().view(np.uint32))
            R.assert_same(got, want[v], "round %d view %d" % (rnd, v))
    return sc


def test_two_streams_across_rebuilds(rt, refs):
    """One view, sixteen frames in flight per pass on two streams: the re-sorts at 2, 4, 8, 16, 32 and 64 rebuild the
    list between compact launches of the other stream."""
    inp, want = refs[1024]
    w, h = R.SIZES[1024]
    sc = _in_flight(rt, inp, [dict(w=w, h=h)] * 16, 5, [want] * 16)
    info = sc.compact_launch()
    assert info["compact"] == 1 and info["rebuilds"] >= 5, info


def test_two_streams_across_evictions(rt, refs):
    """Five layouts against four slots, in a cycle, on two streams: every table is evicted and re-recorded before it is
    read, or read compact by one stream while the other records over its neighbour; the frames are the serial ones."""
    inp, whole = refs[1024]
    w, h = R.SIZES[1024]
    views = [dict(w=w, h=h), dict(w=w, h=h, y0=0, y1=32), dict(w=w, h=h, y0=32, y1=64), dict(w=w, h=h, y0=64, y1=90), dict(w=w, h=h, y0=8, y1=80)]
    want = [(whole[0][v.get("y0", 0):v.get("y1", h)], whole[1][v.get("y0", 0):v.get("y1", h)]) for v in views]
    _in_flight(rt, inp, views, 6, want)
    # four of them fit the slots and come to rest
    sc = _in_flight(rt, inp, views[:4], 6, want[:4])
    assert sc.compact_launch()["compact"] == 1


@pytest.mark.parametrize("compact", [0, 1])
def test_settled_tiles_suite_either_way(rt, refs, oracle, gpu, monkeypatch, compact):
    """The settled-tiles cases that read a table, with every scene they make switched one way."""
    plain = Inputs.scene

    def scene(self):
        sc = plain(self)
        sc.set_compact_launch(compact)
        return sc
    monkeypatch.setattr(Inputs, "scene", scene)
    for n in sorted(S.SIZES):
        for layout in sorted(S.layouts(90)):
            S.test_frames_at_rest(rt, refs, n, layout)
        S.test_meaning_and_completeness(rt, refs, n)
    S.test_partial_tiles(rt, gpu, oracle)
    S.test_settled_pixels(rt, refs)
    S.test_reader_consumes_the_flag_and_only_where_it_is_set(rt, refs)
    S.test_a_settled_tile_without_a_record_takes_the_full_path(rt, refs)


def test_a_grid_of_more_than_262144_tiles(rt, gpu):
    """7680 x 4320: 518 400 tiles, 2 025 blocks of 256 for the list builder -- its one-workgroup sum then takes more than
    one block per thread. Counts and list against the model; the frame against the full grid's."""
    import torch
    w, h = 7680, 4320
    inp = Inputs(rt, 1024)
    on, off = inp.scene(), inp.scene()
    off.set_compact_launch(0)
    for k in range(4):
        a = on.render(w, h)
        torch.cuda.synchronize()
    b = None
    for k in range(3):
        b = off.render(w, h)
        torch.cuda.synchronize()
    assert torch.equal(a["packed"], b["packed"]) and torch.equal(a["rgba"].view(torch.int32), b["rgba"].view(torch.int32))
    info = on.compact_launch(want_list=True)
    assert info["compact"] == 1 and info["tiles_x"] * info["tiles_y"] == 518400
    order = on.compact_order(518400)
    s = on.tile_summaries(want_tables=True)["dwords"]
    p = on.primary_records(want_tables=True)["dwords"]
    lst, n_u, n_s = M.run_list(order, M.streamable(s, p, M.valid_lanes(w, h, 8, *s.shape)))
    assert (info["n_unsettled"], info["n_streamed"]) == (n_u, n_s) and n_s > 262144 // 2
    assert np.array_equal(info["list"], lst)


def test_few_streamable_tiles_keep_the_full_grid(rt, refs):
    """The threshold (the library's default is a quarter of the tiles): 160 x 90 with 1024 spheres streams just under
    half of its tiles. At a threshold of 50 % its reading launches keep the full grid and build one list only; at 0 the
    same scene goes compact."""
    inp, want = refs[1024]
    w, h = R.SIZES[1024]
    sc = inp.scene()
    sc.set_compact_run(64, 1, 50)
    for k in range(8):
        R.assert_same(R.frame(sc, w, h), want, "launch %d" % k)
    info = sc.compact_launch()
    assert info["list_built"] == 1 and 0 < 2 * info["list_n_streamed"] < info["tiles_x"] * info["tiles_y"], info
    assert info["compact"] == 0 and info["rebuilds"] == 1, info
    sc.set_compact_run(64, 1, 0)
    R.assert_same(R.frame(sc, w, h), want, "threshold 0")
    assert sc.compact_launch()["compact"] == 1
