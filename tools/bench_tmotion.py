#!/usr/bin/env python3
"""Temporal accumulation over moving objects (rt_scene_temporal_motion) on one MI355X, at C3 (3840x2160,
1024 spheres) and at 960x540, with the slowly moving camera of tools/bench_temporal.py (five views along a line, walked
there and back) and every 16th sphere displaced a little per frame. Interleaved in one session, call group by call
group within every repetition, so that a clock change hits all of them:

  temporal_v0      rt_scene_temporal, variant 0: the pass without motion or clamp (the baseline)
  motion_v0 / _v1  the new entry with the displacement tables and the clamp on: the product kernel / the yardstick
  noclamp_v0       the new entry with the tables and the clamp off
  zero_v0          the new entry with tables of zeros and the clamp on
  copy_floor       a float4 copy of the bytes the pass must move at least (the pass reads no new per-pixel array:
                   bench_temporal.py's 124 bytes per pixel)

Clocks settled first (tools/_settle.py; the pre-roll's last window is recorded per contender), hipEvent timing, the
median of --reps repetitions of --iters calls. Prints one JSON line and writes it to --out.

  python3 tools/bench_tmotion.py [--iters 20] [--reps 7] [--out profiles/tmotion_c3.json]
"""
import argparse, ctypes as C, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import rt_amd
from _timing import copier, interleaved_ms

GUIDES = ("depth", "normal", "id")
BYTES = 44 + 44 + 8 + 20 + 8            # current inputs, previous colour and guides, previous moments, outputs
MOVE = (0.01, 0.005, -0.01)             # per frame, every 16th sphere


def cases(rt, scene, w, h, iters, reps, step_len):
    st = torch.cuda.current_stream().cuda_stream
    aspect = rt.default_aspect()
    n = scene.n_spheres
    base = (rt.Sphere * n)()
    C.memmove(base, scene.spheres, C.sizeof(base))
    views = []
    for i in range(5):
        cam = rt.default_camera()
        cam.Org.x += step_len * i
        cam.Camyaw += 0.05 * i
        cur = (rt.Sphere * n)()
        C.memmove(cur, base, C.sizeof(base))
        for j in range(0, n, 16):
            o = cur[j].orgin
            o.x, o.y, o.z = o.x + MOVE[0] * i, o.y + MOVE[1] * i, o.z + MOVE[2] * i
        scene.set_spheres(cur, n)
        pos = np.array([[s.orgin.x, s.orgin.y, s.orgin.z] for s in cur], dtype=np.float32)
        views.append((cam, scene.render(w, h, cam=cam, aspect=aspect, aov=GUIDES), pos))
    walk = [0, 1, 2, 3, 4, 3, 2, 1]
    hist = [scene.temporal(views[0][1], None, cam=views[0][0], aspect=aspect) for _ in range(2)]
    tabs = []
    for k in range(len(walk)):
        m = np.zeros((n, 4), dtype=np.float32)
        m[:, :3] = views[walk[k]][2] - views[walk[k - 1]][2]
        tabs.append(torch.from_numpy(m).cuda())
    zeros = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def descs(entry, variant, clamp=True, zero=False):
        ds = []
        for k in range(len(walk)):
            cam, f, _ = views[walk[k]]
            pcam, pf, _ = views[walk[k - 1]]
            src, dst = hist[k & 1], hist[(k + 1) & 1]
            args = dict(cam=cam, aspect=aspect, prev_cam=pcam, prev_aspect=aspect, rgba_in=f["rgba"].data_ptr(),
                        depth=f["aov"]["depth"].data_ptr(), normal=f["aov"]["normal"].data_ptr(), id=f["aov"]["id"].data_ptr(),
                        prev_rgba=src["rgba"].data_ptr(), prev_depth=pf["aov"]["depth"].data_ptr(),
                        prev_normal=pf["aov"]["normal"].data_ptr(), prev_id=pf["aov"]["id"].data_ptr(),
                        prev_moments=src["moments"].data_ptr(), rgba_out=dst["rgba"].data_ptr(),
                        moments_out=dst["moments"].data_ptr(), pixels=dst["packed"].data_ptr(), variant=variant)
            if entry == "temporal":
                ds.append(scene.temporal_desc(w, h, **args))
            else:
                tab = zeros if zero else tabs[k]
                ds.append(scene.temporal_motion_desc(w, h, sphere_motion=tab.data_ptr(), n_sphere_motion=n, clamp=clamp, **args))
        return ds

    def stepper(entry, ds):
        state = {"k": 0}
        call = scene.temporal_raw if entry == "temporal" else scene.temporal_motion_raw

        def step():
            if call(ds[state["k"] % len(ds)], st) != 0:
                raise rt.RtError("the temporal call failed")
            state["k"] += 1
        return step

    steps = {"temporal_v0_ms": stepper("temporal", descs("temporal", 0)),
             "motion_v0_ms": stepper("motion", descs("motion", 0)),
             "motion_v1_ms": stepper("motion", descs("motion", 1)),
             "noclamp_v0_ms": stepper("motion", descs("motion", 0, clamp=False)),
             "zero_v0_ms": stepper("motion", descs("motion", 0, zero=True)),
             "copy_floor_ms": copier(scene.lib, w * h * BYTES, st)}
    res, pre = interleaved_ms(steps, iters, reps)
    res["preroll_last_window_host_ms"] = pre
    res["motion_v0_over_temporal_v0"] = res["motion_v0_ms"] / res["temporal_v0_ms"]
    res["noclamp_v0_over_temporal_v0"] = res["noclamp_v0_ms"] / res["temporal_v0_ms"]
    res["zero_v0_over_temporal_v0"] = res["zero_v0_ms"] / res["temporal_v0_ms"]
    res["motion_v1_over_motion_v0"] = res["motion_v1_ms"] / res["motion_v0_ms"]
    res["motion_v0_over_floor"] = res["motion_v0_ms"] / res["copy_floor_ms"]
    res["traffic_floor_bytes_per_pixel"] = BYTES
    # what the displacements buy: the movers' pixels that keep a history, with the tables and without
    scene.set_temporal_timing(True)
    for name, ds in (("motion_v0", descs("motion", 0)), ("motion_v1", descs("motion", 1))):
        step = stepper("motion", ds)
        per = []
        for _ in range(max(reps, 8)):
            step()
            per += scene.temporal_times()
        res[f"{name}_launch_ms"] = statistics.median(per)
    scene.set_temporal_timing(False)
    ids = views[1][1]["aov"]["id"]
    mover = (ids[..., 0] == 1) & (ids[..., 1] % 16 == 0)
    h0 = scene.temporal(views[0][1], None, cam=views[0][0], aspect=aspect)
    with_m = scene.temporal_motion(views[1][1], h0, cam=views[1][0], aspect=aspect, sphere_motion=tabs[1])
    without = scene.temporal(views[1][1], h0, cam=views[1][0], aspect=aspect)
    res["mover_pixel_share"] = float(mover.float().mean())
    res["mover_history_share_with_tables"] = float((with_m["rgba"][..., 3][mover] > 1).float().mean())
    res["mover_history_share_without"] = float((without["rgba"][..., 3][mover] > 1).float().mean())
    res["step_len"], res["sphere_move_per_frame"] = step_len, list(MOVE)
    scene.set_spheres(base, n)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", type=float, default=0.02, help="camera translation per frame (scene units)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tmotion_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    out = {"iters": a.iters, "reps": a.reps,
           "statistic": "median over reps of hipEvent ms per call (settled clocks); within a repetition the contenders are "
                        "timed one after the other; launch_ms: median of rt_scene_temporal_times",
           "contenders": "temporal_v0: rt_scene_temporal variant 0 (no motion, no clamp); motion_v0 / motion_v1: "
                         "rt_scene_temporal_motion with the tables and the clamp, product kernel / yardstick; noclamp_v0: "
                         "tables, clamp off; zero_v0: tables of zeros, clamp on; copy_floor: float4 copy of the pass's bytes"}
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
