"""hipEvent timing for the post-pass bench tools (bench_denoise, bench_vdenoise, bench_temporal, bench_tmotion,
bench_upsample): clocks settled first (tools/_settle.py), then the median over `reps` repetitions of `iters` calls.
The traffic floors are a float4 copy kernel (rt_debug_copy16) moving the bytes a pass must move at least."""
import statistics

import torch

from _settle import settle


def timed(step, iters):
    """Enqueues `iters` calls of step between two events; the events, to be read after a synchronise."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    return e0, e1


def time_ms(step, iters, reps):
    """Median ms per call of one step."""
    settle(step, torch.cuda.synchronize, window=max(1, iters))
    runs = []
    for _ in range(reps):
        e0, e1 = timed(step, iters)
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / iters)
    return statistics.median(runs)


def interleaved_ms(steps, iters, reps):
    """({name: median ms per call}, {name: host ms per call of the pre-roll's last window}): every repetition times
    each of `steps` once, one after the other, so that a clock change hits all of them."""
    pre = {k: settle(s, torch.cuda.synchronize, window=max(1, iters))[-1] * 1e3 for k, s in steps.items()}
    runs = {k: [] for k in steps}
    for _ in range(reps):
        ev = {k: timed(s, iters) for k, s in steps.items()}
        torch.cuda.synchronize()
        for k, (e0, e1) in ev.items():
            runs[k].append(e0.elapsed_time(e1) / iters)
    return {k: statistics.median(v) for k, v in runs.items()}, pre


def copier(lib, nbytes, st):
    """A step that moves nbytes in all (half read, half written) in 16-byte words on stream `st`."""
    n16 = nbytes // 2 // 16
    src = torch.empty(n16 * 4, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    return lambda: lib.rt_debug_copy16(src.data_ptr(), dst.data_ptr(), n16, st)


def copy_floor(lib, nbytes, iters, reps, st):
    """Median ms of that copy."""
    return time_ms(copier(lib, nbytes, st), iters, reps)
