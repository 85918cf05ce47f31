"""tests/arena.py on host memory (no GPU): the harness the output-coverage tests rest on notices what it is there for."""
import ctypes as C

import numpy as np
import pytest

import arena

DATA = np.arange(67 * 45 * 3, dtype=np.uint8)          # 3 bytes per pixel: no multiple of a word per row
OUTS = dict(x=dict(nbytes=DATA.size, align=4), y=dict(nbytes=64, align=16, written=False))


def _write_all(p):
    C.memmove(p["x"], DATA.ctypes.data, DATA.size)


def test_a_complete_write_passes():
    got = arena.run_twice(_write_all, OUTS, device="cpu")
    arena.same_bytes(got["x"], DATA)
    with pytest.raises(AssertionError, match="differ from the wrapper"):
        arena.same_bytes(got["x"], DATA[::-1].copy())


@pytest.mark.parametrize("what,call", [
    ("differ between the two patterns", lambda p: C.memmove(p["x"], DATA.ctypes.data, DATA.size - 1)),     # one byte short
    ("guard", lambda p: (_write_all(p), C.memset(p["x"] + DATA.size, 0, 1))),                              # one byte over
    ("guard", lambda p: (_write_all(p), C.memset(p["x"] - 1, 0, 1))),                                      # one byte before
    ("must not touch", lambda p: (_write_all(p), C.memset(p["y"] + 5, 0, 1))),
], ids=["short", "over", "before", "untouched"])
def test_what_goes_wrong_is_noticed(what, call):
    with pytest.raises(AssertionError, match=what):
        arena.run_twice(call, OUTS, device="cpu")


def test_no_byte_of_the_two_patterns_agrees():
    a, b = (np.frombuffer(np.uint32(p).tobytes(), dtype=np.uint8) for p in arena.PATTERNS)
    assert (a != b).all()
    assert np.isnan(np.uint32(arena.PATTERNS[1]).view(np.float32))


@pytest.mark.parametrize("align", [4, 8, 16])
def test_alignment_is_the_required_one_and_no_better(align):
    a = arena.Arena(100, align, arena.PATTERNS[1], device="cpu")
    assert a.ptr % align == 0 and a.ptr % (2 * align) != 0
    assert a.offset >= arena.GUARD and 4 * a.buf.numel() - a.offset - a.nbytes >= arena.GUARD


def test_a_prefilled_payload_keeps_its_contents():
    fill = bytes(range(16))
    got = arena.run_twice(lambda p: None, dict(x=dict(nbytes=16, align=8, prefill=fill)), device="cpu")
    assert bytes(got["x"]) == fill
