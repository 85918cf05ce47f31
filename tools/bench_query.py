#!/usr/bin/env python3
"""Ray queries (rt_scene_trace_rays) on one MI355X: NEAREST and SHADE of C3's primary rays (3840x2160, 1024 spheres),
OCCLUDED of as many random rays, each through the sphere BVH and through the whole lists, and NEAREST / SHADE of the
960x540 mesh scene's primary rays; the C3 frame kernel beside them. Clocks settled first (untimed pre-roll), hipEvent
timing, the median of --reps repetitions of --iters launches. Prints one JSON line and writes it to --out.

  python3 tools/bench_query.py [--iters 5] [--reps 5] [--out profiles/query_c3.json]
"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import rt_amd
from _settle import settle


def time_ms(step, iters, reps, settle_first=True):
    if settle_first:
        settle(step, torch.cuda.synchronize, window=max(1, iters))
    else:   # the whole-list variants run for seconds: one untimed launch
        step()
        torch.cuda.synchronize()
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


def query_step(scene, rt, mode, rays, cull, bufs):
    n = rays.shape[0]
    q = scene.query(mode, n, rays=rays.data_ptr(), cull=cull, hits=bufs["hits"].data_ptr(),
                    occluded=bufs["occ"].data_ptr(), rgba=bufs["rgba"].data_ptr(), packed=bufs["packed"].data_ptr())
    st = torch.cuda.current_stream().cuda_stream

    def step():
        rc = scene.trace_rays_raw(q, st)
        if rc != 0:
            raise rt_amd.load().RtError(f"rt_scene_trace_rays: status {rc}")
    return step


def buffers(n):
    return {"hits": torch.empty((n, 16), dtype=torch.int32, device="cuda"),
            "occ": torch.empty(n, dtype=torch.int32, device="cuda"),
            "rgba": torch.empty((n, 4), dtype=torch.float32, device="cuda"),
            "packed": torch.empty(n, dtype=torch.int32, device="cuda")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    out = {"iters": a.iters, "reps": a.reps, "statistic": "median over reps of hipEvent ms per launch"}

    w, h, n = 3840, 2160, 1024
    scene = rt.Scene.default(n)
    rays = scene.primary_rays(w, h).reshape(-1, 6)
    bufs = buffers(rays.shape[0])
    pk = torch.empty((h, w), dtype=torch.int32, device="cuda")
    rgba = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
    fd = scene.frame_desc(w, h, pixels=pk.data_ptr(), rgba=rgba.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    c3 = {"rays": int(rays.shape[0]), "frame_kernel_ms": time_ms(lambda: scene.render_raw(fd, st), 20, a.reps)}
    for mode in ("nearest", "shade"):
        for cull, tag in ((1, "bvh"), (0, "brute")):
            c3[f"{mode}_{tag}_ms"] = time_ms(query_step(scene, rt, mode, rays, cull, bufs), a.iters if cull else 1,
                                             a.reps if cull else 3, settle_first=bool(cull))
    rng = np.random.default_rng(1)
    m = rays.shape[0]
    O = rng.uniform(-30, 30, (m, 3)).astype(np.float32)
    D = rng.standard_normal((m, 3)).astype(np.float32)
    D /= np.sqrt((D * D).sum(axis=1, keepdims=True))
    rnd = torch.from_numpy(np.concatenate([O, D], axis=1).astype(np.float32)).cuda()
    for cull, tag in ((1, "bvh"), (0, "brute")):
        c3[f"occluded_random_{tag}_ms"] = time_ms(query_step(scene, rt, "occluded", rnd, cull, bufs),
                                                  a.iters if cull else 1, a.reps if cull else 3, settle_first=bool(cull))
    for mode in ("nearest", "shade", "occluded_random"):
        c3[f"{mode}_bvh_speedup_vs_brute"] = c3[f"{mode}_brute_ms"] / c3[f"{mode}_bvh_ms"]
    out["c3_3840x2160_n1024"] = c3
    scene.close()

    import meshes
    from scenes import Inputs
    inp = Inputs(rt, 64)
    ms = inp.scene()
    ms.set_mesh(rt.mesh_from_obj_text(meshes.uv_sphere_obj()))
    mw, mh = 960, 540
    mrays = ms.primary_rays(mw, mh, cam=inp.cam, aspect=inp.aspect).reshape(-1, 6)
    mb = buffers(mrays.shape[0])
    mesh = {"rays": int(mrays.shape[0])}
    for mode in ("nearest", "shade"):
        mesh[f"{mode}_ms"] = time_ms(query_step(ms, rt, mode, mrays, 1, mb), a.iters, a.reps)
    out["mesh_960x540_n64_uv_sphere"] = mesh
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
