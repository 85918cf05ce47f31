"""Output buffers that show what a launch wrote: guard | payload | guard in one device allocation filled with one
32-bit pattern, the payload at the alignment its interface requires and no better.

The wrappers of the package allocate outputs with torch.empty, and the caching allocator hands a freed block back to
the next request of the same size: the second of two paths that are compared usually renders into the first one's frame,
so equal results do not show that every element was written. Here every call runs twice, into arenas of two different
patterns. An element the call leaves out differs between the two runs, a write outside the payload breaks a guard, and
the second pattern is a NaN as a float: a kernel that reads its output where it must overwrite spoils its result."""
import numpy as np

GUARD = 4096                                  # bytes on either side, at least
PATTERNS = (0x5a5a5a5a, 0x7fc5a5a5)           # the second: a quiet NaN as binary32


class Arena:
    """nbytes of payload at an address that is a multiple of `align` (4, 8 or 16) but not of 2 * align.
    prefill (bytes-like, optional): what the payload holds before the call instead of the pattern. device "cpu": host
    memory, for the harness's own tests."""

    def __init__(self, nbytes, align, pattern, prefill=None, pinned=False, device="cuda"):
        import torch
        assert align in (4, 8, 16) and nbytes > 0
        self.nbytes, self.align, self.pattern = int(nbytes), align, pattern
        total = GUARD + 2 * align + self.nbytes + GUARD
        words = (total + 3) // 4
        signed = pattern - (1 << 32) if pattern >= 1 << 31 else pattern
        if pinned:
            self.buf = torch.full((words,), signed, dtype=torch.int32).pin_memory()
        else:
            self.buf = torch.full((words,), signed, dtype=torch.int32, device=device)
        base = self.buf.data_ptr()
        assert base % 4 == 0
        ptr = base + GUARD
        ptr += (align - ptr % (2 * align)) % (2 * align)          # ptr = align (mod 2 * align)
        assert ptr % align == 0 and ptr % (2 * align) == align
        self.offset = ptr - base
        self.ptr = ptr
        assert self.offset >= GUARD and 4 * words - self.offset - self.nbytes >= GUARD
        if prefill is not None:
            fill = np.frombuffer(bytes(prefill), dtype=np.uint8)
            assert fill.size == self.nbytes
            self.bytes_view()[self.offset:self.offset + self.nbytes] = torch.from_numpy(fill.copy()).to(self.buf.device)

    def bytes_view(self):
        import torch
        return self.buf.view(torch.uint8)

    def _expected(self):
        return np.tile(np.frombuffer(np.uint32(self.pattern).tobytes(), dtype=np.uint8), self.buf.numel())

    def read(self):
        """(payload bytes, whether both guards still hold the pattern); the caller has waited for the device."""
        got = self.bytes_view().cpu().numpy()
        want = self._expected()
        lo, hi = self.offset, self.offset + self.nbytes
        intact = np.array_equal(got[:lo], want[:lo]) and np.array_equal(got[hi:], want[hi:])
        return got[lo:hi].copy(), intact

    def untouched(self, payload):
        want = self._expected()[self.offset:self.offset + self.nbytes]
        return np.array_equal(payload, want)


def _wait():
    import torch
    if torch.cuda.is_available():
        torch.cuda.synchronize()


class Run:
    """One run of an operation into arenas of one pattern. outputs: name -> dict(nbytes=, align=, written= (True: the
    call must write all of it; False: it must not touch it), prefill= (optional bytes, instead of the pattern),
    pinned= (optional: pinned host memory)). ptrs[name]: where the operation writes."""

    def __init__(self, outputs, pattern, device="cuda"):
        self.outputs, self.pattern = outputs, pattern
        self.arenas = {k: Arena(o["nbytes"], o["align"], pattern, o.get("prefill"), o.get("pinned", False), device)
                       for k, o in outputs.items()}
        self.ptrs = {k: a.ptr for k, a in self.arenas.items()}
        _wait()

    def collect(self):
        """Waits for the device; asserts that every guard is intact and every output the call must not touch still all
        pattern; returns name -> payload bytes (uint8)."""
        _wait()
        got = {}
        for k, a in self.arenas.items():
            payload, intact = a.read()
            assert intact, f"{k}: a guard word was overwritten (pattern {self.pattern:#x})"
            if not self.outputs[k].get("written", True):
                assert a.untouched(payload), f"{k}: written, but the call must not touch it (pattern {self.pattern:#x})"
            got[k] = payload
        return got


def assert_pair(outputs, first, second, what=""):
    """The payloads of two runs with different patterns: every output the call must write is the same bytes in both."""
    for k, o in outputs.items():
        if o.get("written", True):
            a, b = first[k], second[k]
            diff = np.nonzero(a != b)[0]
            assert diff.size == 0, (f"{what} {k}: {diff.size} bytes differ between the two patterns (not written, or computed "
                                    f"from the buffer's old contents); first at byte {diff[0]} of {a.size}")


def run_twice(call, outputs, what="", device="cuda"):
    """call(ptrs) runs an operation whose outputs are the device pointers ptrs[name]: once per pattern, each into fresh
    arenas. Returns name -> payload bytes."""
    got = []
    for pattern in PATTERNS:
        run = Run(outputs, pattern, device)
        call(run.ptrs)
        got.append(run.collect())
    assert_pair(outputs, got[0], got[1], what)
    return got[0]


def as_bytes(t):
    """A tensor or array as the bytes it holds."""
    if hasattr(t, "detach"):
        t = t.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(t).view(np.uint8).reshape(-1)


def same_bytes(got, want, what=""):
    want = as_bytes(want)
    assert got.size == want.size, (what, got.size, want.size)
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, f"{what}: {diff.size} bytes differ from the wrapper's result; first at byte {diff[0]} of {got.size}"
