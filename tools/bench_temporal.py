#!/usr/bin/env python3
"""Temporal accumulation (rt_scene_temporal) on one MI355X, at C3 (3840x2160, 1024 spheres) and at
960x540, with the camera moved by a small step per frame (five views along a line, walked there and back, each
frame's history reprojected from the view before it): the device time of a call for the product kernel (variant 0)
and for the plain yardstick (variant 1), with and without the moments, and beside them a traffic floor -- a float4
copy kernel moving the bytes the pass must move at least (per pixel: 44 of current inputs, 44 of previous colour and
guides read once, 8 of previous moments, 28 written). A standing camera (the single-tap path) and `reset` are timed
too. The three contenders are interleaved call by call group within every repetition, so that a clock change hits
all of them. Clocks settled first (tools/_settle.py), hipEvent timing, the median of --reps repetitions of --iters
calls. Prints one JSON line and writes it to --out.

  python3 tools/bench_temporal.py [--iters 20] [--reps 7] [--out profiles/temporal_c3.json]
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch
import rt_amd
from _timing import copier, interleaved_ms

GUIDES = ("depth", "normal", "id")
CUR_BYTES, PREV_BYTES, MOMENT_BYTES, OUT_BYTES = 44, 44, 8, 20      # per pixel; + 8 of moments written


def cases(rt, scene, w, h, iters, reps, step_len):
    st = torch.cuda.current_stream().cuda_stream
    aspect = rt.default_aspect()
    views = []
    for i in range(5):
        cam = rt.default_camera()
        cam.Org.x += step_len * i
        cam.Camyaw += 0.05 * i
        views.append((cam, scene.render(w, h, cam=cam, aspect=aspect, aov=GUIDES)))
    walk = [0, 1, 2, 3, 4, 3, 2, 1]
    hist = [scene.temporal(views[0][1], None, cam=views[0][0], aspect=aspect) for _ in range(2)]
    torch.cuda.synchronize()

    def descs(variant, moments, standing=False, reset=False):
        ds = []
        for k in range(len(walk)):
            cam, f = views[0] if standing else views[walk[k]]
            pcam, pf = views[0] if standing else views[walk[k - 1]]
            src, dst = hist[k & 1], hist[(k + 1) & 1]
            ds.append(scene.temporal_desc(
                w, h, cam=cam, aspect=aspect, prev_cam=pcam, prev_aspect=aspect, rgba_in=f["rgba"].data_ptr(),
                depth=f["aov"]["depth"].data_ptr(), normal=f["aov"]["normal"].data_ptr(), id=f["aov"]["id"].data_ptr(),
                prev_rgba=src["rgba"].data_ptr(), prev_depth=pf["aov"]["depth"].data_ptr(),
                prev_normal=pf["aov"]["normal"].data_ptr(), prev_id=pf["aov"]["id"].data_ptr(),
                prev_moments=src["moments"].data_ptr() if moments else 0, rgba_out=dst["rgba"].data_ptr(),
                moments_out=dst["moments"].data_ptr() if moments else 0, pixels=dst["packed"].data_ptr(), reset=reset,
                variant=variant))
        return ds

    def stepper(ds):
        state = {"k": 0}

        def step():
            if scene.temporal_raw(ds[state["k"] % len(ds)], st) != 0:
                raise rt.RtError("rt_scene_temporal failed")
            state["k"] += 1
        return step

    full = CUR_BYTES + PREV_BYTES + MOMENT_BYTES + OUT_BYTES + 8
    bare = CUR_BYTES + PREV_BYTES + OUT_BYTES
    floor = {"moving": full, "moving_no_moments": bare, "standing": full, "reset": 16 + OUT_BYTES + 8}
    kw = {"moving": dict(), "moving_no_moments": dict(), "standing": dict(standing=True), "reset": dict(reset=True)}
    res = {}
    for k, bytes_per_px in floor.items():
        moments = k != "moving_no_moments"
        res[k], _ = interleaved_ms({"variant0_ms": stepper(descs(0, moments, **kw[k])),
                                    "variant1_ms": stepper(descs(1, moments, **kw[k])),
                                    "copy_floor_ms": copier(scene.lib, w * h * bytes_per_px, st)}, iters, reps)
    res["traffic_floor_bytes_per_pixel"] = floor
    for k in floor:
        r = res[k]
        r["variant1_over_variant0"] = r["variant1_ms"] / r["variant0_ms"]
        r["variant0_over_floor"] = r["variant0_ms"] / r["copy_floor_ms"]
    # the device time of single launches, as the scene reports it
    scene.set_temporal_timing(True)
    for variant in (0, 1):
        step = stepper(descs(variant, True))
        per = []
        for _ in range(max(reps, 8)):
            step()
            per += scene.temporal_times()
        res["moving"][f"variant{variant}_launch_ms"] = statistics.median(per)
    scene.set_temporal_timing(False)
    hit = (views[1][1]["aov"]["id"][..., 0] >= 0)
    n = hist[0]["rgba"][..., 3]
    res["hit_share"] = float(hit.float().mean())
    res["step_len"] = step_len
    res["history_len_mean_on_hits"] = float(n[views[walk[-1]][1]["aov"]["id"][..., 0] >= 0].mean())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", type=float, default=0.02, help="camera translation per frame (scene units)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    out = {"iters": a.iters, "reps": a.reps,
           "statistic": "median over reps of hipEvent ms per call (settled clocks); within a repetition variant 0, variant 1 "
                        "and the copy are timed one after the other; launch_ms: median of rt_scene_temporal_times",
           "variants": "0: the product kernel (64 x 4 tiles in row-major order, the right tap column from the next lane); "
                       "1: one thread per pixel in grid order, every tap from the caller's arrays; with a standing camera "
                       "or reset variant 0 is variant 1's kernel"}
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
