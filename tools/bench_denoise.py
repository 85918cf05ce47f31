#!/usr/bin/env python3
"""The denoiser (rt_scene_denoise) on one MI355X, at C3 (3840x2160, 1024 spheres) and at 960x540: the
whole call and every launch of it (pack, each iteration), for the product kernels (variant 0), the plain yardstick
(variant 1) and the product kernels without LDS staging (variant 2), at the defaults and at iterations 1 ... 6. Beside
them, in the same process: the frame with all four guides and the 4-spp frame minus the 1-spp frame (what a caller
would pay to supersample instead), and a traffic floor -- a float4 copy kernel moving the bytes the design must move
(per pixel: pack 60 read + 36 written, an iteration 36 read + 16 written, the last one 52 read + 20 written).
Clocks settled first (tools/_settle.py), hipEvent timing, the median of --reps repetitions of --iters calls.
Prints one JSON line and writes it to --out.

  python3 tools/bench_denoise.py [--iters 20] [--reps 7] [--out profiles/denoise_c3.json]
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch
import rt_amd
from _timing import copy_floor, time_ms

ALL = ("depth", "normal", "id", "albedo")
PACK_BYTES, ITER_BYTES, LAST_BYTES = 96, 52, 72      # per pixel, read + written


def denoise_cases(rt, scene, w, h, iters, reps):
    st = torch.cuda.current_stream().cuda_stream
    frame = scene.render(w, h, aov=ALL)
    out = torch.empty_like(frame["rgba"])
    packed = torch.empty_like(frame["packed"])
    a = frame["aov"]
    res = {}
    for n in (4, 1, 2, 3, 5, 6):
        for variant in (0, 1, 2):
            d = scene.denoise_desc(w, h, rgba_in=frame["rgba"].data_ptr(), depth=a["depth"].data_ptr(),
                                   normal=a["normal"].data_ptr(), albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(),
                                   rgba_out=out.data_ptr(), pixels=packed.data_ptr(), iterations=n, variant=variant)

            def step(d=d):
                if scene.denoise_raw(d, st) != 0:
                    raise rt.RtError("rt_scene_denoise failed")
            r = {"call_ms": time_ms(step, iters, reps)}
            scene.set_denoise_timing(True)
            per = []
            for _ in range(reps):
                step()
                per.append(scene.denoise_times())
            scene.set_denoise_timing(False)
            r["launch_ms"] = [statistics.median(col) for col in zip(*per)]
            r["launches"] = (["pack"] if variant != 1 else []) + [f"step{1 << i}" for i in range(n)]
            res[f"iterations{n}_variant{variant}"] = r
    npx = w * h
    floor = {"pack_ms": copy_floor(scene.lib, npx * PACK_BYTES, iters, reps, st),
             "iteration_ms": copy_floor(scene.lib, npx * ITER_BYTES, iters, reps, st),
             "last_iteration_ms": copy_floor(scene.lib, npx * LAST_BYTES, iters, reps, st)}
    floor["default_call_ms"] = floor["pack_ms"] + 3 * floor["iteration_ms"] + floor["last_iteration_ms"]
    res["traffic_floor"] = floor
    d4 = res["iterations4_variant0"]
    res["default_call_over_floor"] = d4["call_ms"] / floor["default_call_ms"]
    res["launch_over_floor_iterations6_variant0"] = [
        t / (floor["pack_ms"] if i == 0 else floor["last_iteration_ms"] if i == 6 else floor["iteration_ms"])
        for i, t in enumerate(res["iterations6_variant0"]["launch_ms"])]
    res["variant1_over_variant0"] = {str(n): res[f"iterations{n}_variant1"]["call_ms"] / res[f"iterations{n}_variant0"]["call_ms"]
                                     for n in range(1, 7)}
    res["variant2_over_variant0"] = {str(n): res[f"iterations{n}_variant2"]["call_ms"] / res[f"iterations{n}_variant0"]["call_ms"]
                                     for n in range(1, 7)}
    return res


def frame_cases(rt, scene, w, h, iters, reps):
    st = torch.cuda.current_stream().cuda_stream
    pk = torch.empty((h, w), dtype=torch.int32, device="cuda")
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    bufs = {"depth": torch.empty((h, w), dtype=torch.float32, device="cuda"),
            "normal": torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
            "id": torch.empty((h, w, 2), dtype=torch.int32, device="cuda"),
            "albedo": torch.empty((h, w, 4), dtype=torch.float32, device="cuda")}
    res = {}
    for tag, kw in (("frame_1spp_ms", {}), ("frame_1spp_all4_guides_ms", {f"aov_{k}": v.data_ptr() for k, v in bufs.items()}),
                    ("frame_4spp_ms", {"spp": 4})):
        fd = scene.frame_desc(w, h, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), **kw)
        res[tag] = time_ms(lambda fd=fd: scene.render_raw(fd, st), iters, reps)
    res["three_more_samples_ms"] = res["frame_4spp_ms"] - res["frame_1spp_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    out = {"iters": a.iters, "reps": a.reps,
           "statistic": "median over reps of hipEvent ms per call (settled clocks); launch_ms: median over reps of the "
                        "hipEvent time of each launch of one call (rt_scene_denoise_times)",
           "variants": "0: the product kernels; 1: one thread per pixel, every tap from the caller's arrays; "
                       "2: the product kernels without LDS staging",
           "traffic_floor_bytes_per_pixel": {"pack": PACK_BYTES, "iteration": ITER_BYTES, "last_iteration": LAST_BYTES}}
    scene = rt.Scene.default(1024)
    for w, h in ((3840, 2160), (960, 540)):
        r = frame_cases(rt, scene, w, h, a.iters, a.reps)
        r.update(denoise_cases(rt, scene, w, h, a.iters, a.reps))
        r["default_call_over_three_more_samples"] = r["iterations4_variant0"]["call_ms"] / r["three_more_samples_ms"]
        out[f"n1024_{w}x{h}"] = r
    scene.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
