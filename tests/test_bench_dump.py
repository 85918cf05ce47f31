"""bench.py --dump-outputs: what it writes is float32/float64, 64 MB at most, and the frame it was given -- whole
where an array fits its share, otherwise at a seeded sample of pixels that is the same from run to run."""
import os

import numpy as np
import torch

import bench


def _frame(h, w):
    g = torch.Generator().manual_seed(0)
    packed = torch.randint(0, 1 << 24, (h, w), dtype=torch.int32, generator=g)     # 0x00RRGGBB words
    return packed, torch.rand((h, w, 4), generator=g)


def test_dump_of_the_c3_frame(tmp_path):
    packed, rgba = _frame(2160, 3840)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"packed": packed, "rgba": rgba})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["packed.npy", "rgba.npy", "rgba_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, b), f
    assert np.array_equal(np.load(tmp_path / "a" / "packed.npy").astype(np.int64), packed.numpy())
    idx = np.load(tmp_path / "a" / "rgba_index.npy").astype(np.int64)
    assert len(idx) > 10 ** 6 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rgba.npy"), rgba.reshape(-1, 4).numpy()[idx])


def test_dump_of_a_small_frame_is_whole(tmp_path):
    packed, rgba = _frame(90, 160)
    bench.dump_outputs(str(tmp_path), {"packed": packed, "rgba": rgba})
    assert sorted(os.listdir(tmp_path)) == ["packed.npy", "rgba.npy"]
    assert np.array_equal(np.load(tmp_path / "packed.npy").astype(np.int64), packed.numpy())
    assert np.array_equal(np.load(tmp_path / "rgba.npy"), rgba.numpy())
