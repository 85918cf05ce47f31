#!/usr/bin/env python3
"""Reflective frame at C3 (3840x2160, 1024 spheres, k = 0.5 on every fourth sphere, reflect_depth 3) on one MI355X:
ms per frame (BVH and brute-force variants), the time of every pass (hipEvents), the queue length per bounce, the
BVH build time, and the same frame with reflect_depth = 0. Prints one JSON line.

--floor: the whole-scene scope (rt_scene_set_reflect_scope) on C3's spheres plus the reference's plane
(kernel.cu:1187) with k = 0.3: the same figures for the all-kinds passes. --out also writes the JSON to a file.

  python3 tools/bench_reflect.py [--iters 20] [--depth 3] [--floor] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--floor", action="store_true", help="add the reference's plane (k = 0.3) under the scene scope")
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
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    pk = torch.empty((h, w), dtype=torch.int32, device="cuda")
    out = {"config": f"{w}x{h}_n{n}_k0.5_every4th_depth{a.depth}" + ("_floor_k0.3_scope_scene" if a.floor else ""),
           "iters": a.iters}
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
