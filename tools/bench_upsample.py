#!/usr/bin/env python3
"""Guided upsampling (rt_scene_upsample) on one MI355X, at C3 (3840x2160, 1024 spheres) with k = 0.5 on
every fourth sphere and reflect_depth 3: the full-resolution reflective frame against the render_upscaled pipeline at
factors 2 and 4, split into its three launches (the plain frame with guides, the reflective frame at reduced
resolution, the upsample); and the upsample launch alone -- the product kernel (variant 0, one thread per pixel), the
lane-exchange kernel of the exact 2 x ratio (variant 1) and a float4 copy kernel moving the bytes the pass moves at
that share of mirror pixels (per hi pixel: id 8 read; not upsampled: base 16 read, 21 written; upsampled: depth and
normal 20 read, 21 written; per lo pixel next to an upsampled one: 44 read).
Clocks settled first (tools/_settle.py), hipEvent timing, the median of --reps repetitions of --iters calls.
Prints one JSON line and writes it to --out.

  python3 tools/bench_upsample.py [--iters 20] [--reps 7] [--out profiles/upsample_c3.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")]
import torch
import rt_amd
from _timing import copy_floor, time_ms

GUIDES = ("depth", "normal", "id")


def frame_bufs(w, h):
    return {"pixels": torch.empty((h, w), dtype=torch.int32, device="cuda"),
            "rgba": torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
            "depth": torch.empty((h, w), dtype=torch.float32, device="cuda"),
            "normal": torch.empty((h, w, 4), dtype=torch.float32, device="cuda"),
            "id": torch.empty((h, w, 2), dtype=torch.int32, device="cuda")}


def frame_desc(scene, w, h, b, **kw):
    return scene.frame_desc(w, h, pixels=b["pixels"].data_ptr(), rgba=b["rgba"].data_ptr(),
                            **{f"aov_{k}": b[k].data_ptr() for k in GUIDES}, **kw)


def moved_bytes(source, factor):
    """Bytes the pass must move for this `source` map (uint8 [H, W]) at an integer factor."""
    sel = source != 0
    H, W = sel.shape
    h, w = H // factor, W // factor
    quads = sel[:h * factor, :w * factor].reshape(h, factor, w, factor).any(dim=3).any(dim=1)
    near = torch.nn.functional.max_pool2d(quads[None, None].float(), 3, stride=1, padding=1)[0, 0] > 0
    n_sel, n_px = int(sel.sum()), H * W
    return (n_px - n_sel) * (8 + 16 + 21) + n_sel * (8 + 20 + 21) + int(near.sum()) * 44


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_c3.json"))
    a = ap.parse_args()
    rt = rt_amd.load()
    n, W, H = 1024, 3840, 2160
    scene = rt.Scene.default(n)
    scene.set_materials([0.5 if i % 4 == 0 else 0.0 for i in range(n)])
    st = torch.cuda.current_stream().cuda_stream
    out = {"iters": a.iters, "reps": a.reps, "reflect_depth": a.depth, "spheres": n, "size": [W, H],
           "statistic": "median over reps of hipEvent ms per call (settled clocks)",
           "variants": "0: the product kernel, one thread per pixel, every tap from the caller's arrays; 1: at factor 2 a lane per "
                       "2 x 2 quad with the neighbouring lo columns from the neighbouring lanes, else the same kernel"}
    hi = frame_bufs(W, H)
    fd_plain = frame_desc(scene, W, H, hi)
    fd_full = frame_desc(scene, W, H, frame_bufs(W, H), reflect_depth=a.depth)
    out["plain_frame_3_guides_ms"] = time_ms(lambda: scene.render_raw(fd_plain, st), a.iters, a.reps)
    out["reflective_frame_full_ms"] = time_ms(lambda: scene.render_raw(fd_full, st), a.iters, a.reps)
    select = scene.upsample_select()["sphere"]
    table = torch.tensor(select, dtype=torch.uint8, device="cuda")
    res_out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    packed = torch.empty((H, W), dtype=torch.int32, device="cuda")
    source = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    for factor in (2, 4):
        w, h = W // factor, H // factor
        lo = frame_bufs(w, h)
        fd_lo = frame_desc(scene, w, h, lo, reflect_depth=a.depth)
        r = {"lo_size": [w, h]}
        r["reflective_frame_lo_ms"] = time_ms(lambda: scene.render_raw(fd_lo, st), a.iters, a.reps)
        descs = {}
        for variant in (0, 1):
            descs[variant] = scene.upsample_desc(
                W, H, w, h, rgba_lo=lo["rgba"].data_ptr(), depth_lo=lo["depth"].data_ptr(), normal_lo=lo["normal"].data_ptr(),
                id_lo=lo["id"].data_ptr(), depth=hi["depth"].data_ptr(), normal=hi["normal"].data_ptr(), id=hi["id"].data_ptr(),
                base=hi["rgba"].data_ptr(), rgba_out=res_out.data_ptr(), pixels=packed.data_ptr(), source=source.data_ptr(),
                sphere_select=table.data_ptr(), n_sphere_select=n, use_tables=True, demodulate=False, variant=variant)

            def step(d=descs[variant]):
                if scene.upsample_raw(d, st) != 0:
                    raise rt.RtError("rt_scene_upsample failed")
            r[f"upsample_variant{variant}_ms"] = time_ms(step, a.iters, a.reps)

        def pipeline():
            scene.render_raw(fd_plain, st)
            scene.render_raw(fd_lo, st)
            scene.upsample_raw(descs[0], st)
        r["pipeline_ms"] = time_ms(pipeline, a.iters, a.reps)
        torch.cuda.synchronize()
        r["selected_share"] = float((source != 0).float().mean())
        r["upsampled_share"] = float((source == 1).float().mean())
        r["selected_without_a_tap"] = int((source == 2).sum())
        r["moved_bytes"] = moved_bytes(source, factor)
        r["copy_floor_ms"] = copy_floor(scene.lib, r["moved_bytes"], a.iters, a.reps, st)
        r["variant0_over_copy"] = r["upsample_variant0_ms"] / r["copy_floor_ms"]
        r["variant1_over_variant0"] = r["upsample_variant1_ms"] / r["upsample_variant0_ms"]
        r["pipeline_over_full_frame"] = r["pipeline_ms"] / out["reflective_frame_full_ms"]
        out[f"factor{factor}"] = r
    scene.close()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
