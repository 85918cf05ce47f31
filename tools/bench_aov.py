#!/usr/bin/env python3
"""G-buffer outputs of the frame (rt_frame_desc.aov_*) on one MI355X: the plain frame, depth only,
depth + id and all four guides, against the route they replace (rt_scene_primary_rays + rt_scene_trace_rays NEAREST,
which writes a 64-byte rt_hit per pixel), at C3 (3840x2160, 1024 spheres) and at 960x540, and the 960x540 mesh scene
plain and with all four. Clocks settled first (tools/_settle.py), hipEvent timing, the median of --reps repetitions of
--iters launches. Prints one JSON line and writes it to --out.

  python3 tools/bench_aov.py [--iters 20] [--reps 7] [--out profiles/aov_c3.json]
"""
import argparse, ctypes, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch
import rt_amd
from _settle import settle

SETS = {"plain": (), "depth": ("depth",), "depth_id": ("depth", "id"), "all4": ("depth", "normal", "id", "albedo")}


def time_ms(step, iters, reps):
    settle(step, torch.cuda.synchronize, window=max(1, iters))
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / iters)
    return statistics.median(runs)


def aov_buffers(w, h):
    return {"depth": torch.empty((h, w), dtype=torch.float32, device="cuda"),
            "normal": torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
            "id": torch.empty((h, w, 2), dtype=torch.int32, device="cuda"),
            "albedo": torch.empty((h, w, 4), dtype=torch.float32, device="cuda")}


def frame_cases(rt, scene, w, h, iters, reps, cam=None, aspect=None, sets=SETS):
    st = torch.cuda.current_stream().cuda_stream
    pk = torch.empty((h, w), dtype=torch.int32, device="cuda")
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    bufs = aov_buffers(w, h)
    res = {}
    for tag, names in sets.items():
        fd = scene.frame_desc(w, h, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), cam=cam, aspect=aspect,
                              **{f"aov_{k}": bufs[k].data_ptr() for k in names})
        res[f"{tag}_ms"] = time_ms(lambda fd=fd: scene.render_raw(fd, st), iters, reps)
    return res


def query_route(rt, scene, w, h, iters, reps, cam=None, aspect=None):
    """primary_rays + NEAREST per frame: what a caller had to run for the same guides before."""
    st = torch.cuda.current_stream().cuda_stream
    rays = torch.empty((h * w, 6), dtype=torch.float32, device="cuda")
    hits = torch.empty((h * w, 16), dtype=torch.int32, device="cuda")
    fd = scene.frame_desc(w, h, cam=cam, aspect=aspect)
    q = scene.query("nearest", h * w, rays=rays.data_ptr(), hits=hits.data_ptr(), cull=1)
    lib = scene.lib

    def step():
        rc = lib.rt_scene_primary_rays(scene.handle, ctypes.byref(fd), rays.data_ptr(), st)
        rc = rc or scene.trace_rays_raw(q, st)
        if rc != 0:
            raise rt.RtError(f"query route: status {rc}")
    return time_ms(step, iters, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aov_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    out = {"iters": a.iters, "reps": a.reps, "statistic": "median over reps of hipEvent ms per frame (settled clocks)",
           "outputs": "every frame writes pixels and rgba; the sets add these guides: " +
                      ", ".join(f"{k} = {list(v)}" for k, v in SETS.items())}
    scene = rt.Scene.default(1024)
    for w, h in ((3840, 2160), (960, 540)):
        r = frame_cases(rt, scene, w, h, a.iters, a.reps)
        r["primary_rays_plus_nearest_ms"] = query_route(rt, scene, w, h, a.iters, a.reps)
        r["all4_added_ms"] = r["all4_ms"] - r["plain_ms"]
        r["depth_id_added_ms"] = r["depth_id_ms"] - r["plain_ms"]
        r["query_route_over_all4"] = r["primary_rays_plus_nearest_ms"] / r["all4_ms"]
        r["query_route_added_over_all4_added"] = (r["primary_rays_plus_nearest_ms"] / r["all4_added_ms"]
                                                  if r["all4_added_ms"] > 0 else None)
        out[f"n1024_{w}x{h}"] = r
    scene.close()

    import meshes
    from scenes import Inputs
    inp = Inputs(rt, 64)
    ms = inp.scene()
    ms.set_mesh(rt.mesh_from_obj_text(meshes.uv_sphere_obj()))
    out["mesh_960x540_n64_uv_sphere"] = frame_cases(rt, ms, 960, 540, a.iters, a.reps, cam=inp.cam, aspect=inp.aspect,
                                                    sets={"plain": (), "all4": SETS["all4"]})
    ms.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
