#!/usr/bin/env python3
"""The indirect pass (rt_scene_indirect) on one MI355X, at C3 (3840x2160, 1024 spheres, the bench camera)
and at 1920x1080, with 1 and 4 rays per pixel: the whole call of variant 0 and of variant 1, timed alternately for
--rounds rounds of --iters calls each (hipEvents, clocks settled first by tools/_settle.py), every pass of one call
(rt_scene_indirect_times), the queue lengths and the share of dead pixels. For scale, in the same process:
trace_rays(shade) of the same view's primary rays, and the frame with its four guides. Prints one JSON line and writes
it to --out (an existing "existing_paths" entry of that file is kept: tools/bench_reflect.py and bench.py fill it).

  python3 tools/bench_indirect.py [--iters 2] [--rounds 5] [--out profiles/indirect_c3.json]

With --bounces N the diffuse paths instead (rt_scene_indirect_paths): one ray per pixel at both sizes,
bounces 1 .. N, the two variants alternating as above, every launch of one call, the queue length entering each bounce;
and bounces = 1 through the new entry against rt_scene_indirect, alternating. The default --out is then
profiles/indirect_paths_c3.json.

  python3 tools/bench_indirect.py --bounces 3
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch
import rt_amd
from _settle import settle
from _timing import time_ms, timed

ALL = ("depth", "normal", "id", "albedo")


def indirect_cases(rt, scene, w, h, iters, rounds):
    st = torch.cuda.current_stream().cuda_stream
    frame = scene.render(w, h, aov=ALL)
    a = frame["aov"]
    out = torch.empty_like(frame["rgba"])
    packed = torch.empty_like(frame["packed"])
    dead = float((a["id"][..., 0] < 0).float().mean())
    res = {"dead_pixel_share": dead, "live_pixels": int((a["id"][..., 0] >= 0).sum())}
    for rays in (1, 4):
        steps = {}
        for variant in (0, 1):
            d = scene.indirect_desc(w, h, depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(), id=a["id"].data_ptr(),
                                    albedo=a["albedo"].data_ptr(), rgba_in=frame["rgba"].data_ptr(), rgba_out=out.data_ptr(),
                                    pixels=packed.data_ptr(), rays=rays, variant=variant)

            def step(d=d):
                if scene.indirect_raw(d, st) != 0:
                    raise rt.RtError("rt_scene_indirect failed")
            steps[variant] = step
        for s in steps.values():
            settle(s, torch.cuda.synchronize, window=iters, max_windows=8)
        runs = {0: [], 1: []}
        for _ in range(rounds):
            for variant in (0, 1):
                e0, e1 = timed(steps[variant], iters)
                torch.cuda.synchronize()
                runs[variant].append(e0.elapsed_time(e1) / iters)
        r = {}
        scene.set_indirect_timing(True)
        for variant in (0, 1):
            steps[variant]()
            r[f"variant{variant}"] = {"call_ms_rounds": runs[variant], "call_ms_median": statistics.median(runs[variant]),
                                      "call_ms_min": min(runs[variant]), "pass_ms": scene.indirect_times(),
                                      "queue": scene.indirect_counts()}
        scene.set_indirect_timing(False)
        r["passes"] = "variant 0: per group of at most 4 rays cast, shade, resolve; variant 1: the kernel"
        r["variant0_median_below_variant1_min"] = r["variant0"]["call_ms_median"] < r["variant1"]["call_ms_min"]
        r["variant1_over_variant0"] = r["variant1"]["call_ms_median"] / r["variant0"]["call_ms_median"]
        res[f"rays{rays}"] = r
    # for scale: SHADE of the view's own primary rays, and the frame with its guides
    rays_t = scene.primary_rays(w, h).reshape(-1, 6)
    rgba = torch.empty((w * h, 4), dtype=torch.float32, device="cuda")
    q = scene.query("shade", w * h, rays=rays_t.data_ptr(), rgba=rgba.data_ptr())
    res["trace_rays_shade_primary_ms"] = time_ms(lambda: scene.trace_rays_raw(q, st), iters, rounds)
    bufs = {k: torch.empty_like(v) for k, v in a.items()}
    fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), rgba=out.data_ptr(), **{f"aov_{k}": v.data_ptr() for k, v in bufs.items()})
    res["frame_all4_guides_ms"] = time_ms(lambda: scene.render_raw(fd, st), 20, rounds)
    return res


def _stats(runs):
    return {"call_ms_rounds": runs, "call_ms_median": statistics.median(runs), "call_ms_min": min(runs), "call_ms_max": max(runs)}


def paths_cases(rt, scene, w, h, max_bounces, iters, rounds):
    st = torch.cuda.current_stream().cuda_stream
    frame = scene.render(w, h, aov=ALL)
    a = frame["aov"]
    out = torch.empty_like(frame["rgba"])
    packed = torch.empty_like(frame["packed"])
    res = {"live_pixels": int((a["id"][..., 0] >= 0).sum())}

    def desc(variant):
        return scene.indirect_desc(w, h, depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(), id=a["id"].data_ptr(),
                                   albedo=a["albedo"].data_ptr(), rgba_in=frame["rgba"].data_ptr(), rgba_out=out.data_ptr(),
                                   pixels=packed.data_ptr(), rays=1, variant=variant)

    def alternate(steps):
        for s in steps.values():
            settle(s, torch.cuda.synchronize, window=iters, max_windows=8)
        runs = {k: [] for k in steps}
        for _ in range(rounds):
            for k, s in steps.items():
                e0, e1 = timed(s, iters)
                torch.cuda.synchronize()
                runs[k].append(e0.elapsed_time(e1) / iters)
        return runs

    for bounces in range(1, max_bounces + 1):
        o = scene.indirect_paths_opts(bounces)
        steps = {}
        for variant in (0, 1):
            def step(d=desc(variant)):
                if scene.indirect_paths_raw(d, o, st) != 0:
                    raise rt.RtError("rt_scene_indirect_paths failed")
            steps[variant] = step
        runs = alternate(steps)
        r = {}
        scene.set_indirect_timing(True)
        for variant in (0, 1):
            steps[variant]()
            r[f"variant{variant}"] = {**_stats(runs[variant]), "launch_ms": scene.indirect_paths_times(),
                                      "queue": scene.indirect_path_counts() if bounces > 1 else [scene.indirect_counts()]}
        scene.set_indirect_timing(False)
        r["variant0_median_below_variant1_min"] = r["variant0"]["call_ms_median"] < r["variant1"]["call_ms_min"]
        r["variant1_median_below_variant0_min"] = r["variant1"]["call_ms_median"] < r["variant0"]["call_ms_min"]
        res[f"bounces{bounces}"] = r
    # bounces = 1 through the new entry against rt_scene_indirect: the same launches
    o1, d0 = scene.indirect_paths_opts(1), desc(0)

    def old():
        if scene.indirect_raw(d0, st) != 0:
            raise rt.RtError("rt_scene_indirect failed")

    def new():
        if scene.indirect_paths_raw(d0, o1, st) != 0:
            raise rt.RtError("rt_scene_indirect_paths failed")
    runs = alternate({"rt_scene_indirect": old, "rt_scene_indirect_paths": new})
    e = {k: _stats(v) for k, v in runs.items()}
    a_, b_ = e["rt_scene_indirect"], e["rt_scene_indirect_paths"]
    e["medians_inside_each_others_range"] = (b_["call_ms_min"] <= a_["call_ms_median"] <= b_["call_ms_max"] and
                                             a_["call_ms_min"] <= b_["call_ms_median"] <= a_["call_ms_max"])
    res["one_bounce_entries"] = e
    return res


def paths_main(rt, a):
    out = {"iters": a.iters, "rounds": a.rounds, "rays": 1,
           "statistic": "call_ms_rounds: hipEvent ms per call of --iters calls, the two variants alternating per round "
                        "(settled clocks); launch_ms: the hipEvent time of each launch of one call "
                        "(rt_scene_indirect_times); queue: per group, the entries that entered each bounce's shade pass",
           "variants": "0: the product (wavefront: cast, one shade-and-continue pass per bounce, resolve); "
                       "1: the plain one-thread-per-pixel yardstick"}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "existing_paths" in old:
            out["existing_paths"] = old["existing_paths"]
    scene = rt.Scene.default(1024)
    for w, h in ((3840, 2160), (1920, 1080)):
        out[f"n1024_{w}x{h}"] = paths_cases(rt, scene, w, h, a.bounces, a.iters, a.rounds)
    scene.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bounces", type=int, default=0, help="N: time the diffuse paths with bounces 1 .. N instead")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rt = rt_amd.load()
    if a.bounces:
        a.out = a.out or os.path.join(ROOT, "profiles", "indirect_paths_c3.json")
        return paths_main(rt, a)
    a.out = a.out or os.path.join(ROOT, "profiles", "indirect_c3.json")
    out = {"iters": a.iters, "rounds": a.rounds,
           "statistic": "call_ms_rounds: hipEvent ms per call of --iters calls, the two variants alternating per round "
                        "(settled clocks); pass_ms: the hipEvent time of each launch of one call (rt_scene_indirect_times)",
           "variants": "0: the product (wavefront passes: cast, shade over the compacted queue, resolve); "
                       "1: the plain one-thread-per-pixel yardstick"}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if "existing_paths" in old:
            out["existing_paths"] = old["existing_paths"]
    scene = rt.Scene.default(1024)
    for w, h in ((3840, 2160), (1920, 1080)):
        out[f"n1024_{w}x{h}"] = indirect_cases(rt, scene, w, h, a.iters, a.rounds)
    scene.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
