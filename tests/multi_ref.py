"""A plain model of the multi-device exchange (include/rt_engine.h, rt_multi_* and rt_assemble_rows24), in integer
numpy and with no GPU: which rows a rank owns, how its rows lie in the root's receive buffer, and how the root reads a
frame back out of it.

The frame's rows are dealt in blocks of 16 rows round-robin: rank r of n owns blocks r, r + n, r + 2n, ... and keeps
them one after the other, in that order (its local rows); the last block of a frame may be short. A rank sends its
local rows as 3 bytes per pixel, B, G, R: the 0x00RRGGBB word without its zero byte, least significant byte first.
The root's receive buffer is n slots of `slot_rows` rows of `width * 3` bytes; slot r holds rank r's local rows from
its first byte on, and whatever follows them in the slot belongs to nobody."""
import numpy as np

BLOCK = 16


def deal(height, n):
    """Per rank, the frame rows it owns, in local-row order."""
    blocks = [list(range(y, min(y + BLOCK, height))) for y in range(0, height, BLOCK)]
    return [[y for blk in blocks[rank::n] for y in blk] for rank in range(n)]


def slot_rows(height, n):
    """Rows of a receive slot: the largest share, in whole blocks."""
    return max((len(rows) + BLOCK - 1) // BLOCK for rows in deal(height, n)) * BLOCK


def pack24(words):
    """0x00RRGGBB words [rows, w] -> uint8 [rows, w * 3]: B, G, R per pixel."""
    words = np.asarray(words, dtype=np.uint32)
    rows, w = words.shape
    out = np.empty((rows, w, 3), dtype=np.uint8)
    out[..., 0] = words % 256               # B
    out[..., 1] = words // 256 % 256        # G
    out[..., 2] = words // 65536 % 256      # R
    return out.reshape(rows, w * 3)


def fill_slots(frame_words, n, slot_rows, poison):
    """The receive buffer (uint8 [n, slot_rows, w * 3]) after every rank's rows of `frame_words` [h, w] arrived: `poison`
    in every byte that no rank owns."""
    frame_words = np.asarray(frame_words, dtype=np.uint32)
    h, w = frame_words.shape
    recv = np.full((n, slot_rows, w * 3), poison, dtype=np.uint8)
    for rank, rows in enumerate(deal(h, n)):
        if rows:
            recv[rank, :len(rows)] = pack24(frame_words[rows])
    return recv


def assemble(recv_bytes, w, h, n, slot_rows, channels=(0, 1, 2), stride=None, rank_of=None):
    """Words [h, w] read from the receive buffer: frame row y comes from slot (y // 16) % n at local row
    (y // 16 // n) * 16 + y % 16, and a pixel's word is b0 | b1 << 8 | b2 << 16. The keyword arguments exist for
    the tests that break the model on purpose: the order the three bytes are read in, the rows from one slot to the
    next, and the rule that gives a block its slot."""
    stride = slot_rows if stride is None else stride
    rank_of = (lambda blk: blk % n) if rank_of is None else rank_of
    flat = np.ascontiguousarray(recv_bytes, dtype=np.uint8).reshape(-1)
    out = np.empty((h, w), dtype=np.uint32)
    for y in range(h):
        blk = y // BLOCK
        lrow = (blk // n) * BLOCK + y % BLOCK
        first = (rank_of(blk) * stride + lrow) * w * 3
        px = flat[first:first + w * 3].reshape(w, 3).astype(np.uint32)
        out[y] = px[:, channels[0]] + px[:, channels[1]] * 256 + px[:, channels[2]] * 65536
    return out


def distinct_words(w, h, seed):
    """A frame [h, w] of 0x00RRGGBB words for feeding the exchange by hand: the words are pairwise distinct, the
    three bytes of every word differ from each other, and no pixel shares a byte at the same place with its left or
    upper neighbour -- a swapped channel, a neighbour's byte or another row's word cannot pass for the right one."""
    rng = np.random.default_rng(seed)
    count = w * h
    assert count <= 200 * 199 * 198
    seen, words = set(), np.empty(count, dtype=np.uint32)
    for i in range(count):
        left = words[i - 1] if i % w else None
        up = words[i - w] if i >= w else None
        while True:
            b, g, r = (int(v) for v in rng.permutation(256)[:3])      # three different bytes
            word = b | g << 8 | r << 16
            if word in seen:
                continue
            if any(nb is not None and any((int(nb) >> s & 255) == (word >> s & 255) for s in (0, 8, 16)) for nb in (left, up)):
                continue
            break
        seen.add(word)
        words[i] = word
    return words.reshape(h, w)
