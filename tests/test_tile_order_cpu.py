"""tests/tile_order_ref.py on its own (no GPU): the restatement the device's tile order is compared with must itself
keep the contract of csrc/rt_tables.h."""
import numpy as np
import pytest

import tile_order_ref as ref


def test_bucket_fixed_points():
    assert int(ref.bucket(0)) == 0 and int(ref.bucket(1)) == 0
    assert int(ref.bucket(2)) == 8 and int(ref.bucket(3)) == 12          # eight buckets per octave
    assert int(ref.bucket(0xffffffff)) == 255                           # rounds up to 2^32: clamped
    assert int(ref.bucket(0xffffffff - 128)) == 255                     # the largest that rounds down
    assert int(ref.bucket((1 << 24) + 1)) == int(ref.bucket(1 << 24)) == 24 * 8


def test_bucket_is_monotone():
    rng = np.random.default_rng(7)
    c = np.concatenate((np.arange(1 << 16, dtype=np.uint32), ref.edge_values(),
                        np.floor(np.exp2(rng.uniform(0, 32, 1 << 18))).astype(np.uint32)))
    c.sort()
    b = ref.bucket(c)
    assert (np.diff(b) >= 0).all()
    assert b.min() == 0 and b.max() == 255


def test_bucket_steps_are_steps():
    steps = np.array(ref.bucket_steps(), dtype=np.uint32)
    assert (ref.bucket(steps) > ref.bucket(steps - 1)).all()
    # integer durations reach every bucket from 8 x log2(8) on, and 1, 2, 4 of the eight in the octaves of 1, 2 and 4
    assert len(steps) + 1 == 1 + 2 + 4 + 8 * 29
    assert np.unique(ref.bucket(ref.edge_values())).size == len(steps) + 1


def test_keys_and_sizes_of_a_small_grid():
    cost = np.arange(17 * 33, dtype=np.uint32).reshape(33, 17)          # 2 x 3 blocks
    key = ref.keys(cost, 17, 33)
    assert key.tolist() == [cost[:16, :16].max(), cost[:16, 16].max(), cost[16:32, :16].max(), cost[16:32, 16].max(),
                            cost[32, :16].max(), cost[32, 16]]
    assert ref.block_sizes(17, 33).tolist() == [256, 16, 256, 16, 16, 1]


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_perm_of_a_legal_order_is_a_permutation(shape):
    tiles_x, tiles_y = shape
    nbx, nby = ref.blocks_of(tiles_x, tiles_y)
    assert nbx * nby <= ref.MAX_BLOCKS and max(shape) <= 0xffff
    tiles = np.sort(ref.all_tiles(tiles_x, tiles_y))
    cases = ref.cost_cases(tiles_x, tiles_y)
    for name in ("zero", "log_uniform", "many_buckets", "bucket_edges"):
        key = ref.keys(cases[name], tiles_x, tiles_y)
        start = ref.start_from_keys(key, tiles_x, tiles_y)
        ref.check_start(key, start, tiles_x, tiles_y)
        perm = ref.perm_from_start(start, tiles_x, tiles_y)
        assert np.array_equal(np.sort(perm), tiles), name
        # tiles row-major inside their block: the first tile of the order is the first block's upper left corner
        first = int(np.argmin(start))
        assert perm[0] == ((first // nbx * 16) << 16 | first % nbx * 16), name


def test_check_start_rejects_illegal_orders():
    tiles_x, tiles_y = 33, 47
    key = ref.keys(ref.cost_cases(tiles_x, tiles_y)["log_uniform"], tiles_x, tiles_y)
    start = ref.start_from_keys(key, tiles_x, tiles_y)
    order = np.argsort(start)
    swapped = start.copy()          # two full blocks of different buckets change places
    full = [b for b in order if ref.block_sizes(tiles_x, tiles_y)[b] == 256]
    a, b = full[0], full[-1]
    assert ref.bucket(key[a]) != ref.bucket(key[b])
    swapped[a], swapped[b] = start[b], start[a]
    with pytest.raises(AssertionError):
        ref.check_start(key, swapped, tiles_x, tiles_y)
    doubled = start.copy()
    doubled[order[1]] = doubled[order[0]]
    with pytest.raises(AssertionError):
        ref.check_start(key, doubled, tiles_x, tiles_y)


def test_refused_shapes_are_outside_the_limits():
    for tiles_x, tiles_y in ref.REFUSED:
        nbx, nby = ref.blocks_of(tiles_x, tiles_y)
        assert max(tiles_x, tiles_y) > 0xffff or nbx * nby > ref.MAX_BLOCKS


def test_the_cost_cases_are_what_they_are_named():
    """So that a change to the cases cannot quietly empty one."""
    key = lambda shape, name: ref.keys(ref.cost_cases(*shape)[name], *shape)
    assert np.unique(ref.bucket(key((640, 480), "many_buckets"))).size == 239   # every bucket an integer duration reaches
    one = key((640, 480), "one_bucket")
    assert np.unique(ref.bucket(one)).size == 1 and np.unique(one).size > 500
    assert key((33, 47), "one_tile_in_last_block").tolist() == [0] * 8 + [5000]
    assert np.isin(ref.edge_values(), key((1024, 1024), "bucket_edges")).all()
    for shape in ref.SHAPES:                                                    # the four named values wherever they fit
        if np.prod(ref.blocks_of(*shape)) >= 4:
            assert np.isin(ref.SPECIAL, key(shape, "bucket_edges")).all(), shape


@pytest.mark.parametrize("via_configs", (False, True))
def test_debug_entry_refuses_before_it_touches_a_device(rt, via_configs):
    """rt_debug_tile_order checks the grid with the library's own limits first: no GPU is needed to be refused."""
    for tiles_x, tiles_y in ref.REFUSED:
        rc, key, start, perm = rt.debug_tile_order(np.ones(tiles_x * tiles_y, dtype=np.uint32), tiles_x, tiles_y, via_configs)
        assert rc == 2, (tiles_x, tiles_y)                       # RT_ERR_UNSUPPORTED
        assert all((a == 0xffffffff).all() for a in (key, start, perm))
    for tiles_x, tiles_y in ((0, 4), (4, 0), (-1, 4)):
        rc, *_ = rt.debug_tile_order(np.zeros(0, dtype=np.uint32), tiles_x, tiles_y, via_configs)
        assert rc == 1, (tiles_x, tiles_y)                       # RT_ERR_INVALID
