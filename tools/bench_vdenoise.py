#!/usr/bin/env python3
"""The variance-guided denoiser (rt_scene_denoise_variance) on one MI355X, at C3 (3840x2160, 1024
spheres) and at 960x540, on the history of tools/bench_temporal.py's moving camera (five views along a line, walked
there and back): the whole call and every launch of it (pack, spatial estimate, each iteration) for the product
kernels (variant 0), the plain yardstick (variant 1) and the product kernels with the other step-16 kernel (variant 2),
with the moments and with moments = NULL, at iterations 1 ... 6. Beside them, interleaved within every repetition so
that a clock change hits all of them: rt_scene_denoise at the same iteration count with sigma_colour = 2^-6 (the
yardstick the new call is a ratio of), and a traffic floor -- a float4 copy kernel moving the bytes each launch must
move at least (per pixel: pack 68 read + 40 written, the spatial estimate 40 read + 4 written, an iteration 40 read +
20 written, the last one 56 read + 24 written). Clocks settled first (tools/_settle.py), hipEvent timing, the median of
--reps repetitions of --iters calls. Prints one JSON line and writes it to --out.

  python3 tools/bench_vdenoise.py [--iters 20] [--reps 7] [--out profiles/vdenoise_c3.json]
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch
import rt_amd
from _timing import copier, interleaved_ms

ALL = ("depth", "normal", "id", "albedo")
PACK_BYTES, SPATIAL_BYTES, ITER_BYTES, LAST_BYTES = 108, 44, 60, 80      # per pixel, read + written


def moving_history(rt, scene, w, h, step_len):
    """The last frame of bench_temporal's walk (all four guides) and the history accumulated along it."""
    aspect = rt.default_aspect()
    views = []
    for i in range(5):
        cam = rt.default_camera()
        cam.Org.x += step_len * i
        cam.Camyaw += 0.05 * i
        views.append(cam)
    hist, frame = None, None
    for k in [0, 1, 2, 3, 4, 3, 2, 1]:
        frame = scene.render(w, h, cam=views[k], aspect=aspect, aov=ALL)
        hist = scene.temporal(frame, hist, cam=views[k], aspect=aspect)
    torch.cuda.synchronize()
    return frame, hist


def cases(rt, scene, w, h, iters, reps, step_len):
    st = torch.cuda.current_stream().cuda_stream
    frame, hist = moving_history(rt, scene, w, h, step_len)
    a = frame["aov"]
    out = torch.empty_like(frame["rgba"])
    packed = torch.empty_like(frame["packed"])
    var = torch.empty_like(a["depth"])
    common = dict(depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(), albedo=a["albedo"].data_ptr(),
                  id=a["id"].data_ptr(), rgba_out=out.data_ptr(), pixels=packed.data_ptr())

    def vd_step(n, variant, moments):
        d = scene.vdenoise_desc(w, h, rgba_in=(hist if moments else frame)["rgba"].data_ptr(),
                                moments=hist["moments"].data_ptr() if moments else 0, variance_out=var.data_ptr(),
                                iterations=n, variant=variant, **common)

        def step():
            if scene.denoise_variance_raw(d, st) != 0:
                raise rt.RtError("rt_scene_denoise_variance failed")
        return step

    def dn_step(n):
        d = scene.denoise_desc(w, h, rgba_in=hist["rgba"].data_ptr(), iterations=n, sigma_colour=2.0 ** -6, **common)

        def step():
            if scene.denoise_raw(d, st) != 0:
                raise rt.RtError("rt_scene_denoise failed")
        return step

    def launches(step, times, on):
        on(True)
        per = []
        for _ in range(reps):
            step()
            per.append(times())
        on(False)
        return [statistics.median(col) for col in zip(*per)]

    res = {}
    for n in (4, 1, 2, 3, 5, 6):
        steps = {"variant0_moments": vd_step(n, 0, True), "variant1_moments": vd_step(n, 1, True),
                 "variant2_moments": vd_step(n, 2, True), "variant0_null": vd_step(n, 0, False),
                 "variant1_null": vd_step(n, 1, False), "rt_scene_denoise": dn_step(n)}
        r = {"call_ms": interleaved_ms(steps, iters, reps)[0], "launch_ms": {}}
        for k, s in steps.items():
            if k == "rt_scene_denoise":
                r["launch_ms"][k] = launches(s, scene.denoise_times, scene.set_denoise_timing)
            else:
                r["launch_ms"][k] = launches(s, scene.vdenoise_times, scene.set_vdenoise_timing)
        c = r["call_ms"]
        r["variant1_over_variant0"] = {"moments": c["variant1_moments"] / c["variant0_moments"],
                                       "null": c["variant1_null"] / c["variant0_null"]}
        r["variant0_over_rt_scene_denoise"] = {"moments": c["variant0_moments"] / c["rt_scene_denoise"],
                                               "null": c["variant0_null"] / c["rt_scene_denoise"]}
        # per launch: iteration i of the new call over iteration i of rt_scene_denoise (pack over pack first)
        v0, dn = r["launch_ms"]["variant0_moments"], r["launch_ms"]["rt_scene_denoise"]
        r["launch_over_rt_scene_denoise"] = [v0[0] / dn[0]] + [v0[2 + i] / dn[1 + i] for i in range(n)]
        res[f"iterations{n}"] = r
    res["launches"] = {"variants 0 and 2": ["pack", "spatial"] + [f"step{1 << i}" for i in range(6)],
                       "variant 1": ["initial variance"] + [f"step{1 << i}" for i in range(6)],
                       "rt_scene_denoise": ["pack"] + [f"step{1 << i}" for i in range(6)]}
    floors = {"pack_ms": PACK_BYTES, "spatial_dense_ms": SPATIAL_BYTES, "iteration_ms": ITER_BYTES, "last_iteration_ms": LAST_BYTES}
    res["traffic_floor"], _ = interleaved_ms({k: copier(scene.lib, w * h * b, st) for k, b in floors.items()}, iters, reps)
    r6 = res["iterations6"]["launch_ms"]
    res["step16"] = {"variant0_ms": r6["variant0_moments"][6], "variant2_ms": r6["variant2_moments"][6]}
    res["spatial_pass_ms"] = {"sparse (moving camera, moments)": r6["variant0_moments"][1], "dense (moments = NULL)": r6["variant0_null"][1]}
    hit = a["id"][..., 0] >= 0
    n_hist = hist["rgba"][..., 3]
    res["hit_share"] = float(hit.float().mean())
    res["short_history_share_of_hits"] = float(((n_hist < 4) & hit).float().sum() / hit.float().sum())
    res["step_len"] = step_len
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", type=float, default=0.02, help="camera translation per frame (scene units)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vdenoise_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    out = {"iters": a.iters, "reps": a.reps,
           "statistic": "median over reps of hipEvent ms per call (settled clocks); within a repetition the contenders are "
                        "timed one after the other; launch_ms: median over reps of the hipEvent time of each launch of one "
                        "call (rt_scene_vdenoise_times / rt_scene_denoise_times)",
           "variants": "0: the product kernels; 1: one thread per pixel, every tap from the caller's arrays; 2: the product "
                       "kernels with the other step-16 kernel; rt_scene_denoise: variant 0 of it, sigma_colour = 2^-6",
           "traffic_floor_bytes_per_pixel": {"pack": PACK_BYTES, "spatial_dense": SPATIAL_BYTES, "iteration": ITER_BYTES,
                                             "last_iteration": LAST_BYTES}}
    scene = rt.Scene.default(1024)
    for w, h in ((3840, 2160), (960, 540)):
        out[f"n1024_{w}x{h}"] = cases(rt, scene, w, h, a.iters, a.reps, a.step)
    scene.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
