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

With --emit K emissive surfaces (rt_scene_set_emission): every K-th sphere of a second, otherwise equal
scene emits; the product (variant 0) at one ray per pixel and bounces 1 and 2 at both sizes, the scene without tables and
the scene with them alternating as above, with the queue lengths of both. The default --out is then
profiles/indirect_emit_c3.json (its "parent_ab" and "existing_paths" entries are kept).

  python3 tools/bench_indirect.py --emit 16
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch
import rt_amd
from _settle import settle
from _timing import time_ms, timed

ALL = ("depth", "normal", "id", "albedo")
CALL = "call_ms_rounds: hipEvent ms per call of --iters calls, the two variants alternating per round (settled clocks); "


class View:
    """A frame of `scene` with its guides, the outputs of the calls on it, and the steps that make one call."""

    def __init__(self, rt, scene, w, h):
        self.rt, self.scene, self.w, self.h = rt, scene, w, h
        self.st = torch.cuda.current_stream().cuda_stream
        self.frame = scene.render(w, h, aov=ALL)
        self.aov = self.frame["aov"]
        self.out = torch.empty_like(self.frame["rgba"])
        self.packed = torch.empty_like(self.frame["packed"])
        self.live = int((self.aov["id"][..., 0] >= 0).sum())

    def step(self, rays, variant, bounces=None):
        """One call of variant `variant`: rt_scene_indirect, or with `bounces` rt_scene_indirect_paths."""
        a, scene, st = self.aov, self.scene, self.st
        d = scene.indirect_desc(self.w, self.h, depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(), id=a["id"].data_ptr(),
                                albedo=a["albedo"].data_ptr(), rgba_in=self.frame["rgba"].data_ptr(), rgba_out=self.out.data_ptr(),
                                pixels=self.packed.data_ptr(), rays=rays, variant=variant)
        o = scene.indirect_paths_opts(bounces) if bounces else None
        name = "rt_scene_indirect_paths" if bounces else "rt_scene_indirect"

        def step():
            if (scene.indirect_paths_raw(d, o, st) if bounces else scene.indirect_raw(d, st)) != 0:
                raise self.rt.RtError(name + " failed")
        return step


def alternate(steps, iters, rounds):
    """ms per call of every step of `steps`: settled, then `rounds` rounds of `iters` calls each, the steps in turn."""
    for s in steps.values():
        settle(s, torch.cuda.synchronize, window=iters, max_windows=8)
    runs = {k: [] for k in steps}
    for _ in range(rounds):
        for k, s in steps.items():
            e0, e1 = timed(s, iters)
            torch.cuda.synchronize()
            runs[k].append(e0.elapsed_time(e1) / iters)
    return runs


def _stats(runs, with_max=True):
    s = {"call_ms_rounds": runs, "call_ms_median": statistics.median(runs), "call_ms_min": min(runs)}
    if with_max:
        s["call_ms_max"] = max(runs)
    return s


def indirect_cases(v, iters, rounds):
    scene, a = v.scene, v.aov
    res = {"dead_pixel_share": float((a["id"][..., 0] < 0).float().mean()), "live_pixels": v.live}
    for rays in (1, 4):
        steps = {variant: v.step(rays, variant) for variant in (0, 1)}
        runs = alternate(steps, iters, rounds)
        r = {}
        scene.set_indirect_timing(True)
        for variant in (0, 1):
            steps[variant]()
            r[f"variant{variant}"] = {**_stats(runs[variant], with_max=False), "pass_ms": scene.indirect_times(),
                                      "queue": scene.indirect_counts()}
        scene.set_indirect_timing(False)
        r["passes"] = "variant 0: per group of at most 4 rays cast, shade, resolve; variant 1: the kernel"
        r["variant0_median_below_variant1_min"] = r["variant0"]["call_ms_median"] < r["variant1"]["call_ms_min"]
        r["variant1_over_variant0"] = r["variant1"]["call_ms_median"] / r["variant0"]["call_ms_median"]
        res[f"rays{rays}"] = r
    # for scale: SHADE of the view's own primary rays, and the frame with its guides
    w, h = v.w, v.h
    rays_t = scene.primary_rays(w, h).reshape(-1, 6)
    rgba = torch.empty((w * h, 4), dtype=torch.float32, device="cuda")
    q = scene.query("shade", w * h, rays=rays_t.data_ptr(), rgba=rgba.data_ptr())
    res["trace_rays_shade_primary_ms"] = time_ms(lambda: scene.trace_rays_raw(q, v.st), iters, rounds)
    bufs = {k: torch.empty_like(t) for k, t in a.items()}
    fd = scene.frame_desc(w, h, pixels=v.packed.data_ptr(), rgba=v.out.data_ptr(), **{f"aov_{k}": t.data_ptr() for k, t in bufs.items()})
    res["frame_all4_guides_ms"] = time_ms(lambda: scene.render_raw(fd, v.st), 20, rounds)
    return res


def paths_cases(v, max_bounces, iters, rounds):
    scene = v.scene
    res = {"live_pixels": v.live}
    for bounces in range(1, max_bounces + 1):
        steps = {variant: v.step(1, variant, bounces) for variant in (0, 1)}
        runs = alternate(steps, iters, rounds)
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
    runs = alternate({"rt_scene_indirect": v.step(1, 0), "rt_scene_indirect_paths": v.step(1, 0, 1)}, iters, rounds)
    e = {k: _stats(r) for k, r in runs.items()}
    a_, b_ = e["rt_scene_indirect"], e["rt_scene_indirect_paths"]
    e["medians_inside_each_others_range"] = (b_["call_ms_min"] <= a_["call_ms_median"] <= b_["call_ms_max"] and
                                             a_["call_ms_min"] <= b_["call_ms_median"] <= a_["call_ms_max"])
    res["one_bounce_entries"] = e
    return res


def emit_cases(views, iters, rounds):
    """views: {"no_tables": View, "tables": View} of two scenes that differ in the emission tables alone."""
    res = {"live_pixels": views["no_tables"].live}
    for bounces in (1, 2):
        steps = {k: v.step(1, 0, bounces) for k, v in views.items()}
        runs = alternate(steps, iters, rounds)
        r = {}
        for k, v in views.items():
            steps[k]()
            r[k] = {**_stats(runs[k]), "queue": v.scene.indirect_path_counts() if bounces > 1 else [v.scene.indirect_counts()]}
        a_, b_ = r["no_tables"], r["tables"]
        r["tables_over_no_tables"] = b_["call_ms_median"] / a_["call_ms_median"]
        r["tables_median_inside_no_tables_range"] = a_["call_ms_min"] <= b_["call_ms_median"] <= a_["call_ms_max"]
        r["same_queues"] = a_["queue"] == b_["queue"]
        res[f"bounces{bounces}"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bounces", type=int, default=0, help="N: time the diffuse paths with bounces 1 .. N instead")
    ap.add_argument("--emit", type=int, default=0, help="K: time the product with every K-th sphere emissive against no tables")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rt = rt_amd.load()
    out = {"iters": a.iters, "rounds": a.rounds}
    if a.emit:
        a.out = a.out or os.path.join(ROOT, "profiles", "indirect_emit_c3.json")
        out.update({"rays": 1, "emit_every": a.emit, "variant": 0,
                    "statistic": CALL.replace("the two variants", "the scene without tables and the scene with them") +
                                 "queue: per group, the entries that entered each bounce's shade pass"})
    elif a.bounces:
        a.out = a.out or os.path.join(ROOT, "profiles", "indirect_paths_c3.json")
        out.update({"rays": 1,
                    "statistic": CALL + "launch_ms: the hipEvent time of each launch of one call (rt_scene_indirect_times); "
                                 "queue: per group, the entries that entered each bounce's shade pass",
                    "variants": "0: the product (wavefront: cast, one shade-and-continue pass per bounce, resolve); "
                                "1: the plain one-thread-per-pixel yardstick"})
    else:
        a.out = a.out or os.path.join(ROOT, "profiles", "indirect_c3.json")
        out.update({"statistic": CALL + "pass_ms: the hipEvent time of each launch of one call (rt_scene_indirect_times)",
                    "variants": "0: the product (wavefront passes: cast, shade over the compacted queue, resolve); "
                                "1: the plain one-thread-per-pixel yardstick"})
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        for k in ("existing_paths", "parent_ab"):
            if k in old:
                out[k] = old[k]
    scene = rt.Scene.default(1024)
    lit = None
    if a.emit:
        import numpy as np
        lit = rt.Scene.default(1024)
        e = np.zeros((1024, 3), dtype=np.float32)
        e[::a.emit] = (1.0, 0.75, 0.5)
        lit.set_emission("sphere", e)
    for w, h in ((3840, 2160), (1920, 1080)):
        v = View(rt, scene, w, h)
        if a.emit:
            out[f"n1024_{w}x{h}"] = emit_cases({"no_tables": v, "tables": View(rt, lit, w, h)}, a.iters, a.rounds)
        else:
            out[f"n1024_{w}x{h}"] = paths_cases(v, a.bounces, a.iters, a.rounds) if a.bounces else indirect_cases(v, a.iters, a.rounds)
    scene.close()
    if lit is not None:
        lit.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
