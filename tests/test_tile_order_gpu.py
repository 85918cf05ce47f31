"""The three tile-order kernels (rt_tile_order_launch, csrc/rt_tables.hip) against tests/tile_order_ref.py, through
rt_debug_tile_order: exact, at the grids and durations of tile_order_ref.SHAPES / cost_cases. Both launch geometries --
rt_tile_order_launch's own and the one a frame graph builds its kernel nodes from -- run every case."""
import functools

import numpy as np
import pytest

import tile_order_ref as ref

pytestmark = pytest.mark.gpu

RT_OK, RT_ERR_UNSUPPORTED = 0, 2


@functools.lru_cache(maxsize=None)
def _cases(tiles_x, tiles_y):
    """name -> (durations, their keys): computed once per grid, shared by both launch geometries, never written."""
    out = {}
    for name, cost in ref.cost_cases(tiles_x, tiles_y).items():
        key = ref.keys(cost, tiles_x, tiles_y)
        cost.setflags(write=False)
        key.setflags(write=False)
        out[name] = (cost, key)
    return out


@pytest.mark.parametrize("via_configs", (False, True), ids=("launch", "graph_configs"))
@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_order_against_host_restatement(rt, gpu, shape, via_configs):
    tiles_x, tiles_y = shape
    tiles = np.sort(ref.all_tiles(tiles_x, tiles_y))
    for name, (cost, want_key) in _cases(tiles_x, tiles_y).items():
        rc, key, start, perm = rt.debug_tile_order(cost, tiles_x, tiles_y, via_configs)
        assert rc == RT_OK, (name, rt.load_library().rt_last_error())
        assert np.array_equal(key, want_key), name
        ref.check_start(key, start, tiles_x, tiles_y)
        assert np.array_equal(perm, ref.perm_from_start(start, tiles_x, tiles_y)), name
        assert np.array_equal(np.sort(perm), tiles), name          # independently: a permutation of the tiles


@pytest.mark.parametrize("via_configs", (False, True), ids=("launch", "graph_configs"))
@pytest.mark.parametrize("shape", ref.REFUSED, ids=lambda s: f"{s[0]}x{s[1]}")
def test_grids_beyond_the_limits_are_refused(rt, gpu, shape, via_configs):
    tiles_x, tiles_y = shape
    cost = np.ones(tiles_x * tiles_y, dtype=np.uint32)
    rc, key, start, perm = rt.debug_tile_order(cost, tiles_x, tiles_y, via_configs)
    assert rc == RT_ERR_UNSUPPORTED
    for a in (key, start, perm):                                   # nothing written
        assert (a == 0xffffffff).all()
