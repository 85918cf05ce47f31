"""The view-list margin scenes of tests/view_margins.py are ON the bounds they name (host computation only: runs
without a GPU): the witness is non-empty, its sphere stands on its block's host list although its centre lies outside
the block's unpadded corner cone, and the flags and slopes predicted from the block geometry are the ones the host
builder reports -- so that a generator that drifts off its margin fails here and not silently in
tests/test_view_margins_gpu.py."""
import functools

import numpy as np
import pytest

import view_margins as V

CASES = [(name, seed) for name, (_, seeds) in V.BUILDERS.items() for seed in seeds]


@functools.lru_cache(maxsize=None)
def _margin(name, seed):
    import oracle_py
    import rt_amd
    return V.BUILDERS[name][0](rt_amd.load(), oracle_py, seed)


@pytest.mark.parametrize("name,seed", CASES)
def test_witness_is_on_its_bound(rt, oracle, name, seed):
    m = _margin(name, seed)
    w = m.witness
    assert len(m.spheres) >= 64                                   # eye cones: the culled frame reads view lists
    assert w["pixels"], (name, seed)
    assert all(0 <= x < m.w and 0 <= y < m.h for x, y in w["pixels"])
    if m.band:
        assert m.band[0] % 8 == 0 and all(m.band[0] <= y < m.band[1] for _, y in w["pixels"])
    if name in ("view_corner", "view_sample_edge"):
        assert w["flags"] == 0 and w["on_list"] and w["list_position"] >= 0
        assert w["dev"] > w["sin_corner"]                         # the centre: outside the unpadded corner cone
        assert abs(w["k"] - w["k_predicted"]) <= 1e-5 * (1 + w["k"])
        assert w["slack"] > 0
        x0, y0, x1, y1 = w["rect"]
        (x, y), place = w["pixels"][0], w["place"]
        assert x == (x0 if "l" in place else x1 - 1 if "r" in place else (x0 + x1) // 2)
        assert y == (y0 if "t" in place else y1 - 1 if place in ("bl", "br", "b") else (y0 + y1) // 2)
        if name == "view_sample_edge":
            assert m.spp in (4, 16) and not w["centre_hits"]      # the pixel's middle misses the sphere
            assert w["hit_samples"] and set(w["hit_samples"]) <= set(w["nearest_samples"]), w
    elif name == "view_not_built":
        assert w["flags"] == w["predicted"] and w["not_built"] == sum(1 for f in w["flags"] if f & V.VIEW_NOT_BUILT)
        if w["all"]:
            assert w["not_built"] == w["blocks"]
        else:
            assert 0 < w["not_built"] < w["blocks"] and w["built_pixels"]
    elif name == "view_kcap":
        k, kp = np.array(w["k"]), np.array(w["k_predicted"])
        assert not any(w["flags"]) and (np.abs(k - kp) <= 1e-5 * (1 + kp)).all()
        assert (np.abs(kp - V.KCAP) > 1e-4).all()                 # no block on the threshold itself
        assert w["low"] == [b for b in range(len(kp)) if kp[b] <= V.KCAP] and w["low"] and w["high"]
        assert w["low_pixels"]
        assert w["sliver_block"] in w["high"] and w["sliver_listed"] == 31
        a_cone, alpha, a_member = w["sliver"]
        assert a_cone + 1e-3 < alpha < a_member - 1e-3, w["sliver"]   # well inside the sliver, on both sides
    elif name == "view_order":
        assert max(w["ulp_gaps"]) <= 1 and w["normals_differ"] > 0 and w["on_lists"] and w["bounds"]
        if w["inside"]:
            assert w["negative"] == len(w["pixels"]) and all(b < 0 for bb in w["bounds"] for b in bb)


def test_corner_rows_cover_places_blocks_and_frames():
    """Rows 1 and 2 over their seeds: every place at 8-pixel and at 64-pixel blocks, interior, border and clipped
    blocks; row 2 every place at 4 and at 16 samples."""
    seen = {(V.PLACES[s % 8], V.CORNER_FRAMES[(s // 8) % len(V.CORNER_FRAMES)][:3]) for s in V.BUILDERS["view_corner"][1]}
    assert seen == {(p, f[:3]) for p in V.PLACES for f in V.CORNER_FRAMES}
    assert {(V.PLACES[s % 8], (4, 16)[(s // 8) % 2]) for s in V.BUILDERS["view_sample_edge"][1]} == {(p, n) for p in V.PLACES for n in (4, 16)}


def test_measured_slack_of_the_corner_rows(rt, oracle):
    """What the witnesses measure (printed; the ledger row of DESIGN.md quotes it): by how much the witness spheres'
    centres exceed the corner cone, and the smallest relative slack the member test leaves them, per block size."""
    for name in ("view_corner", "view_sample_edge"):
        for big in (False, True):
            ws = [_margin(name, s) for s in V.BUILDERS[name][1]]
            ws = [m.witness for m in ws if (m.w > 100) == big]
            ex = [w["dev"] / w["sin_corner"] - 1 for w in ws]
            pad = [w["sin_padded"] / w["sin_corner"] - 1 for w in ws]
            print("%s, %d-pixel blocks: %d scenes, centre beyond the corner cone by %.2g ... %.2g relative (the pad: %.2g ... %.2g), "
                  "member slack %.3g ... %.3g, without the cone's pad %.3g ... %.3g"
                  % (name, 64 if big else 8, len(ws), min(ex), max(ex), min(pad), max(pad), min(w["slack"] for w in ws),
                     max(w["slack"] for w in ws), min(w["slack_unpadded"] for w in ws), max(w["slack_unpadded"] for w in ws)))
            assert min(ex) > 0
