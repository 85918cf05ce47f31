#!/usr/bin/env python3
"""The bloom pass (rt_scene_bloom) on one MI355X, at 3840x2160 and 960x540, on the frame of high dynamic
range that tools/bench_display.py forms (a rendered frame of the 1024-sphere scene, every 16th sphere emissive, the
colour times 4): with the default settings and with `levels` 1 and 8 the product (variant 0) against the yardstick
(variant 1) and a float4 copy kernel moving the bytes the call must move, all alternating within every repetition, with
rgba_out and pixels both written. The bytes: per pixel of the frame 16 read and 20 written by the combine and 16 read by
the first downsample; per texel of level k 16 written by its downsample, 16 read by the next one, 16 read and 16 written
by the step that makes A_k of B_k, and 16 read by the step below it.
Clocks settled first (tools/_settle.py), hipEvent timing, the median of --reps repetitions of --iters calls.
Prints one JSON line and writes it to --out. --existing FILE: a JSON object recorded beside this run (the parent's
bench.py, sweeps of a tuning build), merged into the result key by key.

  python3 tools/bench_bloom.py [--iters 20] [--reps 7] [--out profiles/bloom_c3.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import rt_amd
from _timing import copier, interleaved_ms

SETTINGS = {"default": 5, "levels1": 1, "levels8": 8}


def bytes_moved(W, H, levels):
    """What one call must move at least, in bytes."""
    n = [W * H]
    for _ in range(levels):
        W, H = (W + 1) >> 1, (H + 1) >> 1
        n.append(W * H)
    total = n[0] * (16 + 20 + 16)
    for k in range(1, levels + 1):
        total += 16 * n[k]                      # B_k written
        if k < levels:
            total += 16 * n[k]                  # read by the next downsample
            total += 32 * n[k]                  # B_k read, A_k written
        total += 16 * n[k]                      # A_k (A_L = B_L) read by the step below it
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--existing", default="")
    ap.add_argument("--product-only", action="store_true", help="variant 0 and the copy only (tuning sweeps)")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    n = 1024
    scene = rt.Scene.default(n)
    tab = np.zeros((n, 3), dtype=np.float32)
    tab[::16] = (12.0, 10.0, 6.0)
    scene.set_emission("sphere", tab)
    st = torch.cuda.current_stream().cuda_stream
    out = {"iters": a.iters, "reps": a.reps, "spheres": n,
           "statistic": "median over reps of hipEvent ms per call (settled clocks); variants 0 and 1 and the copy alternate "
                        "within every repetition",
           "variants": "0: the product (LDS-staged tiles); 1: the yardstick (a thread per output pixel, 16 and 4 taps from "
                       "global memory)"}
    if a.note:
        out["note"] = a.note
    variants = (0,) if a.product_only else (0, 1)
    for W, H in ((3840, 2160), (960, 540)):
        frame = scene.render(W, H, aov=("id",))
        rgba = (frame["rgba"] * 4 + scene.emission_term(frame)).contiguous()
        res = torch.empty_like(rgba)
        packed = torch.empty((H, W), dtype=torch.int32, device="cuda")
        glow = torch.empty_like(rgba)
        r = {}

        def step_of(levels, variant, want_glow=False):
            d = scene.bloom_desc(W, H, rgba_in=rgba.data_ptr(), rgba_out=res.data_ptr(), pixels=packed.data_ptr(),
                                 glow_out=glow.data_ptr() if want_glow else 0, levels=levels, variant=variant)

            def step():
                if scene.bloom_raw(d, st) != 0:
                    raise rt.RtError("rt_scene_bloom failed")
            return step
        steps = {}
        for name, levels in SETTINGS.items():
            for v in variants:
                steps[f"{name}_variant{v}"] = step_of(levels, v)
            steps[f"{name}_copy"] = copier(scene.lib, bytes_moved(W, H, levels), st)
        ms, _ = interleaved_ms(steps, a.iters, a.reps)
        r["ms"] = ms
        r["bytes_moved"] = {name: bytes_moved(W, H, levels) for name, levels in SETTINGS.items()}
        for name in SETTINGS:
            if not a.product_only:
                r[f"{name}_variant1_over_variant0"] = ms[f"{name}_variant1"] / ms[f"{name}_variant0"]
            r[f"{name}_over_copy"] = ms[f"{name}_variant0"] / ms[f"{name}_copy"]
        scene.set_bloom_timing(True)
        for name, levels in SETTINGS.items():
            for v in variants:
                step_of(levels, v)()
                r[f"{name}_variant{v}_launches_ms"] = scene.bloom_times()
        scene.set_bloom_timing(False)
        step_of(5, 0, want_glow=True)()
        torch.cuda.synchronize()
        r["share_above_threshold"] = float((rgba[..., :3] * rgba.new_tensor([0.2126, 0.7152, 0.0722])).sum(-1).gt(1).float().mean())
        r["share_with_glow"] = float((glow[..., :3] != 0).any(dim=-1).float().mean())
        out[f"{W}x{H}"] = r
    scene.close()
    out["device"] = torch.cuda.get_device_name(0)
    if a.existing:
        with open(a.existing) as f:
            out.update(json.load(f))
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
