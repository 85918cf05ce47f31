"""A numpy model of the run list of a compact reading launch: a stable partition of the launch's
order -- tile_perm, or grid order -- into the tiles that keep a wave of their own and, behind them, the streamable
ones. A tile is streamable iff it is settled and either has no miss lane (RT_TILE_NO_MISS) or has no valid lane whose
primary record says RT_PRIMARY_NONE."""
import numpy as np

SETTLED, NO_MISS, PRIMARY_NONE = 1, 2, 0xfe   # RT_TILE_SETTLED, RT_TILE_NO_MISS, RT_PRIMARY_NONE


def grid_order(tiles_y, tiles_x):
    ty, tx = np.divmod(np.arange(tiles_y * tiles_x, dtype=np.uint32), np.uint32(tiles_x))
    return (ty << np.uint32(16)) | tx


def valid_lanes(width, rows, tile_w, tiles_y, tiles_x):
    """bool [tiles_y, tiles_x, 64]: the lanes inside a contiguous launch of `rows` rows (lane = row in tile * tile_w + column)."""
    th = 64 // tile_w
    lane = np.arange(64)
    px = np.arange(tiles_x)[None, :, None] * tile_w + (lane % tile_w)[None, None, :]
    ly = np.arange(tiles_y)[:, None, None] * th + (lane // tile_w)[None, None, :]
    return (px < width) & (ly < rows)


def streamable(summaries, primary, valid):
    """bool [tiles_y, tiles_x] from the summaries uint32 [ty, tx], the primary records uint32 [ty, tx, 64] and the valid lanes."""
    settled = (summaries & SETTLED) != 0
    no_miss = (summaries & NO_MISS) != 0
    none = (((primary & 0xff) == PRIMARY_NONE) & valid).any(axis=-1)
    return settled & (no_miss | ~none)


def run_list(order, stream_mask):
    """-> (list, n_unsettled, n_streamed): `order` uint32 [(ty << 16) | tx], stream_mask bool [ty, tx]."""
    order = np.asarray(order, dtype=np.uint32)
    s = stream_mask[order >> 16, order & 0xffff]
    return np.concatenate([order[~s], order[s]]), int((~s).sum()), int(s.sum())


def workgroups(n_unsettled, n_streamed, run):
    return n_unsettled + (n_streamed + run - 1) // run
