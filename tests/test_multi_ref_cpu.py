"""tests/multi_ref.py, the plain model of the multi-device exchange that tests/test_multi_gpu.py holds the device to:
its row deal against rt.interleaved_rows, its two directions against each other, and that it notices being wrong."""
import numpy as np
import pytest

import multi_ref

HEIGHTS = (1, 15, 16, 17, 33, 90, 100)
RANKS = (1, 2, 3, 5, 8)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_deal_is_the_interleaved_rows_and_a_partition(rt, h, n):
    dealt = multi_ref.deal(h, n)
    assert len(dealt) == n
    for rank in range(n):
        assert dealt[rank] == rt.interleaved_rows(h, rank, n, 16), (h, n, rank)
    assert sorted(y for rows in dealt for y in rows) == list(range(h))


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_slot_rows_is_the_largest_share_in_whole_blocks(h, n):
    blocks = (h + 15) // 16
    assert multi_ref.slot_rows(h, n) == ((blocks + n - 1) // n) * 16
    assert multi_ref.slot_rows(h, n) >= max(len(rows) for rows in multi_ref.deal(h, n))


@pytest.mark.parametrize("w", (4, 36))
@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("h", HEIGHTS)
def test_assemble_undoes_fill_slots(h, n, w):
    frame = multi_ref.distinct_words(w, h, seed=h * 100 + n)
    assert len(np.unique(frame)) == w * h and int(frame.max()) < 1 << 24
    sr = multi_ref.slot_rows(h, n)
    recv = multi_ref.fill_slots(frame, n, sr, 0xA5)
    assert recv.shape == (n, sr, w * 3) and recv.dtype == np.uint8
    assert np.array_equal(multi_ref.assemble(recv, w, h, n, sr), frame)
    # exactly the owned bytes were written: h rows of w * 3 bytes, everything else is still poison
    owned = np.zeros(recv.shape, dtype=bool)
    for rank, rows in enumerate(multi_ref.deal(h, n)):
        owned[rank, :len(rows)] = True
    assert int(owned.sum()) == h * w * 3 and (recv[~owned] == 0xA5).all()
    # a taller slot than needed changes nothing
    recv = multi_ref.fill_slots(frame, n, sr + 16, 0xA5)
    assert np.array_equal(multi_ref.assemble(recv, w, h, n, sr + 16), frame)


def test_pack24_is_blue_green_red():
    got = multi_ref.pack24(np.array([[0x00112233, 0x00A0B0C0]], dtype=np.uint32))
    assert got.tolist() == [[0x33, 0x22, 0x11, 0xC0, 0xB0, 0xA0]]


BROKEN = {
    "bytes read as R, G, B": dict(channels=(2, 1, 0)),
    "slot stride of slot_rows - 16": dict(stride=multi_ref.slot_rows(17, 2) - 16),
    "rank taken as blk // n": dict(rank_of=lambda blk: blk // 2),
}


@pytest.mark.parametrize("name", sorted(BROKEN))
def test_the_model_notices_being_wrong(name):
    """4 x 17 on two ranks (a whole block for the first, a one-row block for the second): each broken variant of
    assemble() changes the result."""
    w, h, n = 4, 17, 2
    sr = multi_ref.slot_rows(h, n)
    frame = multi_ref.distinct_words(w, h, seed=7)
    recv = multi_ref.fill_slots(frame, n, sr, 0xA5)
    assert np.array_equal(multi_ref.assemble(recv, w, h, n, sr), frame)
    wrong = multi_ref.assemble(recv, w, h, n, sr, **BROKEN[name])
    assert not np.array_equal(wrong, frame), name
