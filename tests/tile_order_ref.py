"""The tile order of a launch (rt_scene_set_tile_order) restated in numpy from its contract in csrc/rt_tables.h, not from
the kernels: blocks of 16 x 16 tiles, the block with the longest tile first, tiles row-major inside a block,
perm[] = (tile_y << 16) | tile_x; always a permutation of the tiles, whatever the durations hold.

"Longest first" is by bucket: eight buckets per octave of the duration -- the exponent and the first three mantissa bits
of the duration as a binary32 -- counted from the bucket of 1 and clamped to 0 .. 255. The order of the blocks inside one
bucket is not defined (the device ranks them with atomics), so `check_start` states the property every legal order has
and `perm_from_start` derives the one perm[] that belongs to a given order."""
import numpy as np

BLOCK = 16
MAX_BLOCKS = 4096
BUCKETS = 256

# (tiles_x, tiles_y) and what each is there for
SHAPES = (
    (1, 1),            # smallest grid
    (16, 16),          # exactly one block
    (17, 1), (1, 17),  # a one-tile edge block
    (15, 31), (33, 47),  # partial blocks on both edges
    (80, 45),          # 640 x 360 at tile 8
    (480, 270),        # 3840 x 2160 at tile 8
    (640, 480),        # 1200 blocks: more than one step of a 1024-thread workgroup
    (1024, 1024),      # exactly MAX_BLOCKS
    (65535, 1), (1, 65535),  # MAX_BLOCKS in a line, coordinates at 0xffff
)
REFUSED = ((65536, 1), (1040, 1024))   # a coordinate above 0xffff; 65 x 64 blocks


def blocks_of(tiles_x, tiles_y):
    return -(-tiles_x // BLOCK), -(-tiles_y // BLOCK)


def bucket(c):
    """Bucket of a duration (uint32, scalar or array): 0 for 0 and 1, 255 at most."""
    c = np.asarray(c, dtype=np.uint32)
    b = (c.astype(np.float32).view(np.uint32) >> 20).astype(np.int64) - (127 << 3)
    return np.clip(b, 0, BUCKETS - 1)


def keys(cost, tiles_x, tiles_y):
    """The longest tile of every block, blocks row-major."""
    nbx, nby = blocks_of(tiles_x, tiles_y)
    padded = np.zeros((nby * BLOCK, nbx * BLOCK), dtype=np.uint32)
    padded[:tiles_y, :tiles_x] = np.asarray(cost, dtype=np.uint32).reshape(tiles_y, tiles_x)
    return padded.reshape(nby, BLOCK, nbx, BLOCK).max(axis=(1, 3)).reshape(-1)


def block_sizes(tiles_x, tiles_y):
    """Tiles of every block (blocks at the right and lower edge are smaller), blocks row-major."""
    nbx, nby = blocks_of(tiles_x, tiles_y)
    w = np.minimum(BLOCK, tiles_x - BLOCK * np.arange(nbx, dtype=np.int64))
    h = np.minimum(BLOCK, tiles_y - BLOCK * np.arange(nby, dtype=np.int64))
    return (h[:, None] * w[None, :]).reshape(-1)


def check_start(key, start, tiles_x, tiles_y):
    """Raises AssertionError unless `start` is a legal order of the blocks for `key`: ranked by start, the blocks'
    buckets do not increase, and each block starts where the tiles of the blocks before it end."""
    key = np.asarray(key, dtype=np.uint32)
    start = np.asarray(start, dtype=np.uint32).astype(np.int64)
    sizes = block_sizes(tiles_x, tiles_y)
    assert key.shape == start.shape == sizes.shape, (key.shape, start.shape, sizes.shape)
    order = np.argsort(start, kind="stable")
    want = np.concatenate(([0], np.cumsum(sizes[order])[:-1]))
    bad = np.nonzero(start[order] != want)[0]
    assert bad.size == 0, (f"{bad.size} blocks do not start where the blocks before them end; first at rank {bad[0]}: "
                           f"block {order[bad[0]]} starts at {start[order[bad[0]]]}, the tiles before it end at {want[bad[0]]}")
    b = bucket(key)[order]
    up = np.nonzero(b[1:] > b[:-1])[0]
    assert up.size == 0, (f"{up.size} blocks come after a block of a lower bucket; first at rank {up[0] + 1}: "
                          f"bucket {b[up[0] + 1]} after {b[up[0]]}")


def start_from_keys(key, tiles_x, tiles_y):
    """One legal order: the blocks of a bucket in block order."""
    order = np.argsort(-bucket(key), kind="stable")
    sizes = block_sizes(tiles_x, tiles_y)
    start = np.empty(order.size, dtype=np.uint32)
    start[order] = np.concatenate(([0], np.cumsum(sizes[order])[:-1]))
    return start


def all_tiles(tiles_x, tiles_y):
    """(tile_y << 16) | tile_x of every tile, row-major."""
    ty, tx = np.divmod(np.arange(tiles_x * tiles_y, dtype=np.int64), tiles_x)
    return ((ty << 16) | tx).astype(np.uint32)


def perm_from_start(start, tiles_x, tiles_y):
    """perm[] for the blocks' starting places; 0xffffffff where no tile lands."""
    nbx, _ = blocks_of(tiles_x, tiles_y)
    n = tiles_x * tiles_y
    ty, tx = np.divmod(np.arange(n, dtype=np.int64), tiles_x)
    bx, by = tx // BLOCK, ty // BLOCK
    bw = np.minimum(BLOCK, tiles_x - bx * BLOCK)
    at = np.asarray(start, dtype=np.uint32).astype(np.int64)[by * nbx + bx] + (ty % BLOCK) * bw + tx % BLOCK
    if at.min() < 0 or at.max() >= n:
        raise ValueError("start[] puts a tile outside the order")
    perm = np.full(n, 0xffffffff, dtype=np.uint32)
    perm[at] = ((ty << 16) | tx).astype(np.uint32)
    return perm


def bucket_steps():
    """Every duration at which `bucket` steps (found by bisection on `bucket` itself, which is monotone)."""
    steps = []
    for k in range(1, BUCKETS):
        lo, hi = 0, 0xffffffff          # smallest c with bucket(c) >= k
        if int(bucket(hi)) < k:
            break
        while lo < hi:
            mid = (lo + hi) // 2
            if int(bucket(mid)) >= k:
                hi = mid
            else:
                lo = mid + 1
        if not steps or steps[-1] != lo:
            steps.append(lo)
    return steps


SPECIAL = (0xffffffff, (1 << 24) + 1, 1, 0)


def edge_values():
    """The steps of `bucket` and the value below each, plus 0, 1, 2^24 + 1 (rounds in the conversion to binary32) and
    0xffffffff (rounds up to 2^32: bucket 256 before the clamp)."""
    vals = set(SPECIAL)
    for s in bucket_steps():
        vals.update((s, s - 1))
    return np.array(sorted(vals), dtype=np.uint32)


def cost_cases(tiles_x, tiles_y, seed=2024):
    """name -> durations (uint32 [tiles_x * tiles_y], row-major) for one grid."""
    n = tiles_x * tiles_y
    nbx, nby = blocks_of(tiles_x, tiles_y)
    nb = nbx * nby
    rng = np.random.default_rng(seed + 65537 * tiles_x + tiles_y)
    ty, tx = np.divmod(np.arange(n, dtype=np.int64), tiles_x)
    block = (ty // BLOCK) * nbx + tx // BLOCK          # the block of every tile
    # one tile per block, anywhere in it
    pick = np.zeros(nb, dtype=np.int64)
    shuffled = rng.permutation(n)
    pick[block[shuffled]] = shuffled
    cases = {}
    cases["zero"] = np.zeros(n, dtype=np.uint32)
    cases["equal"] = np.full(n, 48271, dtype=np.uint32)
    cases["ramp"] = (np.arange(n, dtype=np.uint64) * 0xffffffff // max(n - 1, 1)).astype(np.uint32)
    cases["log_uniform"] = np.clip(np.floor(np.exp2(rng.uniform(0.0, 32.0, n))), 1, 0xffffffff).astype(np.uint32)
    last = np.zeros(n, dtype=np.uint32)
    last[n - 1] = 5000                                  # the last tile lies in the last (partial) block
    cases["one_tile_in_last_block"] = last
    # every block's key in one bucket (exponent 20, mantissa bits 000), the keys themselves different
    cases["one_bucket"] = rng.integers(1 << 20, (1 << 20) + (1 << 17), n, dtype=np.uint32)
    # as many buckets as durations can reach, dealt to the blocks: one tile per block carries its value
    steps = np.array([1] + bucket_steps(), dtype=np.uint32)
    many = np.zeros(n, dtype=np.uint32)
    many[pick] = steps[rng.permutation(nb) % steps.size]
    cases["many_buckets"] = many
    # the four named values first, so that every grid of four blocks or more has them; then the steps, from a place
    # that differs from grid to grid
    special = np.array(SPECIAL, dtype=np.uint32)
    rest = edge_values()
    rest = np.roll(rest[~np.isin(rest, special)], -int(rng.integers(rest.size)))
    edges = np.concatenate((special, rest))
    e = np.zeros(n, dtype=np.uint32)
    e[pick] = edges[np.arange(nb) % edges.size]
    cases["bucket_edges"] = e
    return cases
