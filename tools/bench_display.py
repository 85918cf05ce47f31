#!/usr/bin/env python3
"""The display transform (rt_scene_display) on one MI355X, at 3840x2160 and 960x540, on a rendered frame
of the 1024-sphere scene brought to a high dynamic range (every 16th sphere emissive, the colour times 4) with its id
guide: per metering mode (AUTO: metering, resolve, apply; LAGGED: one fused pass, resolve; MANUAL: apply) the product
(variant 0) against the yardstick (variant 1), alternating within every repetition, with rgba_out and pixels both
written, ACES and the sRGB pack; a meter-only call; and a float4 copy kernel moving the bytes an apply-only call moves
(per pixel 16 read, 20 written), timed in the same session.
Clocks settled first (tools/_settle.py), hipEvent timing, the median of --reps repetitions of --iters calls.
Prints one JSON line and writes it to --out. --existing FILE: a JSON object recorded beside this run (the parent's bench.py, sweeps of a tuning build), merged
into the result key by key.

  python3 tools/bench_display.py [--iters 20] [--reps 7] [--out profiles/display_c3.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import rt_amd
from _timing import copier, interleaved_ms

METERS = {"auto": 1, "lagged": 2, "manual": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--existing", default="")
    ap.add_argument("--product-only", action="store_true", help="variant 0 and the copy only (tuning sweeps)")
    ap.add_argument("--note", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display_c3.json"))
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
           "variants": "0: the product (a strided kernel, the histogram and the thresholds in LDS, a 512-thread resolve); "
                       "1: the yardstick (a thread per pixel, global atomics, 255 compares per channel, a serial resolve)"}
    if a.note:
        out["note"] = a.note
    for W, H in ((3840, 2160), (960, 540)):
        frame = scene.render(W, H, aov=("id",))
        rgba = (frame["rgba"] * 4 + scene.emission_term(frame)).contiguous()
        ids = frame["aov"]["id"]
        res = torch.empty_like(rgba)
        packed = torch.empty((H, W), dtype=torch.int32, device="cuda")
        state = torch.zeros(4, dtype=torch.float32, device="cuda")
        hist = torch.zeros(rt.RT_DISPLAY_BINS, dtype=torch.int32, device="cuda")
        r = {}

        def step_of(meter, variant, outputs=True):
            d = scene.display_desc(W, H, rgba_in=rgba.data_ptr(), id=ids.data_ptr(), rgba_out=res.data_ptr() if outputs else 0,
                                   pixels=packed.data_ptr() if outputs else 0, state=state.data_ptr(),
                                   histogram_out=hist.data_ptr(), meter=meter, adapt=0.5, variant=variant)

            def step():
                if scene.display_raw(d, st) != 0:
                    raise rt.RtError("rt_scene_display failed")
            return step
        variants = (0,) if a.product_only else (0, 1)
        steps = {f"{name}_variant{v}": step_of(m, v) for name, m in METERS.items() for v in variants}
        for v in variants:
            steps[f"meter_only_variant{v}"] = step_of(1, v, outputs=False)
        steps["copy"] = copier(scene.lib, W * H * 36, st)
        ms, _ = interleaved_ms(steps, a.iters, a.reps)
        r["ms"] = ms
        for name in list(METERS) + ["meter_only"]:
            if not a.product_only:
                r[f"{name}_variant1_over_variant0"] = ms[f"{name}_variant1"] / ms[f"{name}_variant0"]
        r["manual_over_copy"] = ms["manual_variant0"] / ms["copy"]
        r["auto_over_lagged"] = ms["auto_variant0"] / ms["lagged_variant0"]
        r["lagged_over_manual"] = ms["lagged_variant0"] / ms["manual_variant0"]
        torch.cuda.synchronize()
        r["metered_share"] = float(state[2])
        r["exposure"] = float(state[0])
        r["bins_in_use"] = int((hist != 0).sum())
        r["largest_bin_share"] = float(hist.max()) / max(1, int(hist.sum()))
        r["share_above_one"] = float((rgba[..., :3] > 1).any(dim=-1).float().mean())
        scene.set_display_timing(True)
        for name, m in METERS.items():
            step_of(m, 0)()
            r[f"{name}_launches_ms"] = scene.display_times()
        scene.set_display_timing(False)
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
