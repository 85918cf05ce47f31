#!/usr/bin/env python3
"""Reflective frame at C3 (3840x2160, 1024 spheres, k = 0.5 on every fourth sphere, reflect_depth 3) on one MI355X:
ms per frame (BVH and brute-force variants), the time of every pass (hipEvents), the queue length per bounce, the
BVH build time, and the same frame with reflect_depth = 0. Prints one JSON line.

--floor: the whole-scene scope (rt_scene_set_reflect_scope) on C3's spheres plus the reference's plane
(kernel.cu:1187) with k = 0.3: the same figures for the all-kinds passes. --out also writes the JSON to a file.

--spp N (N > 1): the supersampled frame (rt_scene_set_reflect_samples) instead. Three ways to N samples
per pixel, timed in this process and interleaved round by round: `merged` (one call with spp = N), `progressive` (N
one-sample accumulate calls: the same pipeline fed a sample at a time) and `one_sample_x_n` (N times the one-sample
reflective frame); per round ms per N samples, then median, min and max over the rounds, the time of every pass and the
queue lengths of each, and the shader clock read while merged frames are in flight. The default of 1 runs exactly as
described above.

--rough RHO (RHO > 0): glossy mirrors (rt_scene_set_roughness): that roughness on the mirrors the tool
creates -- every fourth sphere and, with --floor, the plane. Combines with --floor and --spp; 0 sets no table.

  python3 tools/bench_reflect.py [--iters 20] [--depth 3] [--floor] [--rough RHO] [--spp N --rounds 5] [--out FILE]
"""
import argparse, ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import torch
import rt_amd
from _settle import settle


def time_frames(scene, fd, iters):
    st = torch.cuda.current_stream()
    settle(lambda: scene.render_raw(fd, st.cuda_stream), torch.cuda.synchronize, window=5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        scene.render_raw(fd, st.cuda_stream)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def time_calls(scene, fds, iters):
    """hipEvent ms per run of all of `fds`, over `iters` runs (no pre-roll: the caller has settled the clocks)."""
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        for fd in fds:
            scene.render_raw(fd, st.cuda_stream)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def passes_of(scene, fds, depth):
    """Per-pass ms and queue lengths summed over one timed run of `fds`."""
    st = torch.cuda.current_stream()
    names = ["frame_kernel", "primary"] + [f"bounce{b}" for b in range(1, depth + 1)]
    ms, queue = [0.0] * len(names), [0] * depth
    scene.set_reflect_timing(True)
    for fd in fds:
        scene.render_raw(fd, st.cuda_stream)
        stats = scene.reflect_stats()
        ms = [a + b for a, b in zip(ms, stats["pass_ms"])]
        queue = [a + b for a, b in zip(queue, stats["queue"])]
    scene.set_reflect_timing(False)
    return {"pass_ms": dict(zip(names, ms)), "queue_per_bounce": queue}


def supersampled(a, rt, scene, w, h, out):
    from bench import read_clocks
    n = a.spp
    scene.set_reflect_samples("many")
    rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    pk = torch.empty((h, w), dtype=torch.int32, device="cuda")
    kw = dict(pixels=pk.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=a.depth)
    variants = {
        "merged": [scene.frame_desc(w, h, spp=n, **kw)],
        "progressive": [scene.frame_desc(w, h, spp=1, sample_base=k, sample_total=n, accumulate=k > 0,
                                         resolve=0 if k == n - 1 else -1, **kw) for k in range(n)],
        "one_sample_x_n": [scene.frame_desc(w, h, **kw)] * n,
    }
    st = torch.cuda.current_stream()
    settle(lambda: scene.render_raw(variants["merged"][0], st.cuda_stream), torch.cuda.synchronize, window=3)
    rounds = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fds in variants.items():
            rounds[name].append(time_calls(scene, fds, a.iters))
    for _ in range(3):
        scene.render_raw(variants["merged"][0], st.cuda_stream)
    out["clocks_under_merged"] = read_clocks(fast_only=True)
    torch.cuda.synchronize()
    out["spp"], out["rounds"] = n, a.rounds
    out["statistic"] = "hipEvent ms per N samples per pixel; per round, then median / min / max over the rounds"
    for name, fds in variants.items():
        v = sorted(rounds[name])
        out[name] = {"rounds_ms": rounds[name], "median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1],
                     **passes_of(scene, fds, a.depth)}
    out["merged_over_progressive"] = out["merged"]["median_ms"] / out["progressive"]["median_ms"]
    out["merged_over_one_sample_x_n"] = out["merged"]["median_ms"] / out["one_sample_x_n"]["median_ms"]
    out["clocks_end"] = read_clocks()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--floor", action="store_true", help="add the reference's plane (k = 0.3) under the scene scope")
    ap.add_argument("--spp", type=int, default=1, help="> 1: the supersampled frame, three ways (see above)")
    ap.add_argument("--rough", type=float, default=0.0, help="> 0: this roughness on the mirrors (see above)")
    ap.add_argument("--rounds", type=int, default=5, help="with --spp: rounds of the interleaved comparison")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    rt = rt_amd.load()
    w, h, n = 3840, 2160, 1024
    scene = rt.Scene.default(n)
    scene.set_materials([0.5 if i % 4 == 0 else 0.0 for i in range(n)])
    if a.floor:
        planes = (rt.Plane * 1)()
        rt.load_library().rt_plane_init(ctypes.byref(planes[0]), 0.0, -4.0, 0.0, 0.0, 1.0, 0.0)
        scene.set_planes(planes, 1)
        scene.set_plane_materials([0.3])
        scene.set_reflect_scope("scene")
    if a.rough > 0:
        scene.set_roughness("sphere", [a.rough if i % 4 == 0 else 0.0 for i in range(n)])
        if a.floor:
            scene.set_roughness("plane", [a.rough])
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    pk = torch.empty((h, w), dtype=torch.int32, device="cuda")
    out = {"config": f"{w}x{h}_n{n}_k0.5_every4th_depth{a.depth}" + ("_floor_k0.3_scope_scene" if a.floor else "") +
           (f"_rough{a.rough:g}" if a.rough > 0 else ""),
           "iters": a.iters}
    if a.spp > 1:
        out["config"] += f"_spp{a.spp}"
        del rgba, pk
        supersampled(a, rt, scene, w, h, out)
        out["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(out))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
        return
    fd0 = scene.frame_desc(w, h, pixels=pk.data_ptr(), rgba=rgba.data_ptr())
    out["plain_ms"] = time_frames(scene, fd0, a.iters)
    fd = scene.frame_desc(w, h, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=a.depth)
    out["reflect_ms"] = time_frames(scene, fd, a.iters)
    fdb = scene.frame_desc(w, h, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=a.depth, cull=False)
    out["reflect_brute_ms"] = time_frames(scene, fdb, max(2, a.iters // 10))
    out["bvh_speedup_vs_brute"] = out["reflect_brute_ms"] / out["reflect_ms"]
    scene.set_reflect_timing(True)
    scene.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    stats = scene.reflect_stats()
    names = ["frame_kernel", "primary"] + [f"bounce{b}" for b in range(1, a.depth + 1)]
    out["pass_ms"] = dict(zip(names, stats["pass_ms"] or []))
    out["queue_per_bounce"] = stats["queue"]
    out["bvh"] = {k: stats[k] for k in ("bvh_build_ms", "bvh_nodes", "bvh_depth", "bvh_leaves")}
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
