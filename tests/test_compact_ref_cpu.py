"""The numpy model of the compact launch's run list (tests/compact_ref.py) against a plain loop over the order."""
import numpy as np

import compact_ref as M


def slow_list(order, summaries, primary, valid):
    keep, stream = [], []
    for e in order:
        ty, tx = int(e) >> 16, int(e) & 0xffff
        s = int(summaries[ty, tx])
        ok = bool(s & 1) and (bool(s & 2) or not any(valid[ty, tx, l] and (int(primary[ty, tx, l]) & 0xff) == 0xfe for l in range(64)))
        (stream if ok else keep).append(int(e))
    return keep + stream, len(keep), len(stream)


def test_model_is_a_stable_partition():
    rng = np.random.default_rng(5)
    ty, tx = 7, 13
    summaries = rng.integers(0, 4, size=(ty, tx)).astype(np.uint32) | (rng.integers(0, 5, size=(ty, tx)).astype(np.uint32) << 8)
    primary = rng.choice(np.array([0, 3, 0xff, 0xfe], dtype=np.uint32), size=(ty, tx, 64), p=[0.5, 0.3, 0.19, 0.01]) | np.uint32(0x1200)
    valid = M.valid_lanes(100, 54, 8, ty, tx)
    assert valid[:, -1, 4:8].sum() == 0 and valid[-1, :, 48:].sum() == 0 and valid[0, 0].all()
    for order in (M.grid_order(ty, tx), rng.permutation(M.grid_order(ty, tx))):
        got = M.run_list(order, M.streamable(summaries, primary, valid))
        want = slow_list(order, summaries, primary, valid)
        assert got[0].tolist() == want[0] and got[1:] == want[1:]
        assert sorted(got[0].tolist()) == sorted(order.tolist()) and 0 < got[2] < ty * tx


def test_a_record_outside_the_frame_does_not_count():
    summaries = np.full((1, 2), 1, dtype=np.uint32)              # settled, with miss lanes
    primary = np.full((1, 2, 64), 0xff, dtype=np.uint32)
    primary[0, 1, 7] = 0xfe                                       # column 15 of a frame 12 wide: outside
    primary[0, 0, 9] = 0xfe                                       # inside
    valid = M.valid_lanes(12, 8, 8, 1, 2)
    lst, n_u, n_s = M.run_list(M.grid_order(1, 2), M.streamable(summaries, primary, valid))
    assert (lst.tolist(), n_u, n_s) == ([0, 1], 1, 1)


def test_workgroups():
    assert [M.workgroups(5, n, 8) for n in (0, 1, 7, 8, 9)] == [5, 6, 6, 6, 7]
    assert M.workgroups(0, 91, 8) == 12
