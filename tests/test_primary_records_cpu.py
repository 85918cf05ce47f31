"""The numpy side of the primary records: a record's fields, and the order of a tile's lanes."""
import numpy as np
import pytest


@pytest.mark.parametrize("tile_w", [8, 16, 32, 64])
def test_lane_order_round_trip(rt, tile_w):
    th = 64 // tile_w
    ty, tx = 3, 2
    a = np.arange(ty * tx * 64, dtype=np.int32).reshape(ty, tx, 64)
    p = rt.tiles_to_pixels(a, tile_w)
    assert p.shape == (ty * th, tx * tile_w)
    for y, x in ((0, 0), (th - 1, tile_w - 1), (th, tile_w), (ty * th - 1, tx * tile_w - 1)):
        lane = (y % th) * tile_w + x % tile_w           # the kernel's lane / TW and lane % TW
        assert p[y, x] == a[y // th, x // tile_w, lane]
    assert np.array_equal(rt.pixels_to_tiles(p, tile_w), a)


def test_record_fields(rt):
    d =np.array([0x000000fe, 0x000000ff, 0x00000003, 0xffffff3f, 0x0001_0000 | 7], dtype=np.uint32)
    entry, texel = rt.decode_primary_records(d)
    assert entry.tolist() == [rt.RT_PRIMARY_NONE, rt.RT_PRIMARY_MISS, 3, 63, 7]
    assert texel.tolist() == [0, 0, 0, (1 << 24) - 1, 256]
    assert np.array_equal(rt.encode_primary_records(entry, texel), d)
