#!/usr/bin/env python3
"""Refractive frames at C3 (3840x2160, 1024 spheres, reflect_depth 3) on one MI355X, three material configurations:
  glass   tau = 0.9, ior = 1.5 on every fourth sphere (i % 4 == 0)
  mirror  k = 0.5 on the same spheres (tools/bench_reflect.py's configuration)
  mix     the glass of `glass`, and k = 0.5 on the spheres half way between them (i % 4 == 2)
For each: ms per frame (BVH and brute force), the time of every pass (hipEvents), the queue length per bounce, and the
shader clock read while frames are in flight. With --ab-root DIR (a checkout of another commit with its library built),
the mirror configuration is also timed alternately in fresh processes of that tree and of this one, --ab-rounds times
each, so that the two libraries see the same machine state. Prints one JSON line (and writes it to --out).

--fresnel: Fresnel glass (rt_scene_set_glass_model) instead: the glass configuration under the plain model,
under the Fresnel model, and under the Fresnel model with roughness 0.1 on the glass spheres -- ms per frame, the time
of every pass and the queue lengths of each. With --ab-root the configuration timed alternately is then the glass one
under the plain model (rt_scene_set_materials_ex and render_raw only: what the other tree has as well).

  python3 tools/bench_refract.py [--iters 20] [--depth 3] [--fresnel] [--ab-root DIR --ab-rounds 5] [--out file.json]
"""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

W, H, N = 3840, 2160, 1024


def materials(kind, n=N):
    k = [0.0] * n
    tau = [0.0] * n
    ior = [0.0] * n
    for i in range(n):
        if i % 4 == 0:
            if kind == "mirror":
                k[i] = 0.5
            else:
                tau[i], ior[i] = 0.9, 1.5
        elif i % 4 == 2 and kind == "mix":
            k[i] = 0.5
    return k, tau, ior


def time_frames(torch, settle, scene, fd, iters):
    st = torch.cuda.current_stream()
    settle(lambda: scene.render_raw(fd, st.cuda_stream), torch.cuda.synchronize, window=5)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        scene.render_raw(fd, st.cuda_stream)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def mirror_child(root, iters, depth, kind="mirror"):
    """Time the mirror configuration with the package of `root` (only set_materials and render_raw: the API every
    commit since reflections has), or (--fresnel) the glass one (set_materials_ex). Prints {"ms": ...}."""
    sys.path[:0] = [root, os.path.join(ROOT, "tools")]
    import torch
    import rt_amd
    from _settle import settle
    rt = rt_amd.load()
    scene = rt.Scene.default(N)
    if kind == "mirror":
        scene.set_materials(materials("mirror")[0])
    else:
        scene.set_materials_ex(*materials(kind))
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    pk = torch.empty((H, W), dtype=torch.int32, device="cuda")
    fd = scene.frame_desc(W, H, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=depth)
    print(json.dumps({"ms": time_frames(torch, settle, scene, fd, iters), "lib": rt.LIB_PATH}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--fresnel", action="store_true", help="the glass configuration under the Fresnel model (see above)")
    ap.add_argument("--ab-root", default="")
    ap.add_argument("--ab-rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--mirror-child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.mirror_child:
        mirror_child(a.mirror_child, a.iters, a.depth, "glass" if a.fresnel else "mirror")
        return
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
    import torch
    import rt_amd
    from _settle import settle
    from bench import read_clocks
    rt = rt_amd.load()
    scene = rt.Scene.default(N)
    rgba = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    pk = torch.empty((H, W), dtype=torch.int32, device="cuda")
    out = {"config": f"{W}x{H}_n{N}_depth{a.depth}", "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    fd0 = scene.frame_desc(W, H, pixels=pk.data_ptr(), rgba=rgba.data_ptr())
    out["plain_ms"] = time_frames(torch, settle, scene, fd0, a.iters)
    fd = scene.frame_desc(W, H, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=a.depth)
    fdb = scene.frame_desc(W, H, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), reflect_depth=a.depth, cull=False)
    names = ["frame_kernel", "primary"] + [f"bounce{b}" for b in range(1, a.depth + 1)]
    # (--fresnel: the glass configuration three times over -- model, roughness on the glass spheres)
    cases = ([("glass_plain", "glass", "plain", 0.0), ("glass_fresnel", "glass", "fresnel", 0.0),
              ("glass_fresnel_rough0.1", "glass", "fresnel", 0.1)] if a.fresnel
             else [(kind, kind, None, 0.0) for kind in ("glass", "mirror", "mix")])
    for name, kind, model, rho in cases:
        k, tau, ior = materials(kind)
        if kind == "mirror":
            scene.set_materials(k)
        else:
            scene.set_materials_ex(k, tau, ior)
        if model is not None:
            scene.set_glass_model(model)
            scene.set_roughness("sphere", [rho if t > 0 else 0.0 for t in tau] if rho > 0 else None)
        r = {"ms": time_frames(torch, settle, scene, fd, a.iters)}
        # the clock under this workload: read while a window of frames is in flight
        for _ in range(5):
            scene.render_raw(fd, torch.cuda.current_stream().cuda_stream)
        r["clocks"] = read_clocks(fast_only=True)
        torch.cuda.synchronize()
        r["brute_ms"] = time_frames(torch, settle, scene, fdb, max(2, a.iters // 10))
        r["bvh_speedup_vs_brute"] = r["brute_ms"] / r["ms"]
        scene.set_reflect_timing(True)
        scene.render_raw(fd, torch.cuda.current_stream().cuda_stream)
        stats = scene.reflect_stats()
        scene.set_reflect_timing(False)
        r["pass_ms"] = dict(zip(names, stats["pass_ms"] or []))
        r["queue_per_bounce"] = stats["queue"]
        out[name] = r
    out["clocks_end"] = read_clocks()
    if a.ab_root:
        del scene, rgba, pk
        torch.cuda.empty_cache()
        ab = {"parent_root": os.path.basename(os.path.abspath(a.ab_root)), "parent_ms": [], "this_ms": []}
        for _ in range(a.ab_rounds):
            for key, root in (("parent_ms", os.path.abspath(a.ab_root)), ("this_ms", ROOT)):
                env = dict(os.environ)
                env.pop("RT_ENGINE_LIB", None)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mirror-child", root, "--iters",
                                    str(a.iters), "--depth", str(a.depth)] + (["--fresnel"] if a.fresnel else []), capture_output=True, text=True, env=env,
                                   timeout=600)
                if p.returncode != 0:
                    raise SystemExit(f"mirror child for {root} failed ({p.returncode}): {p.stderr[-2000:]}")
                ab[key].append(json.loads(p.stdout.strip().splitlines()[-1])["ms"])
        for key in ("parent_ms", "this_ms"):
            v = sorted(ab[key])
            ab[key.replace("_ms", "_median_ms")] = v[len(v) // 2]
            ab[key.replace("_ms", "_spread_ms")] = v[-1] - v[0]
        ab["this_over_parent"] = ab["this_median_ms"] / ab["parent_median_ms"]
        out["glass_plain_ab" if a.fresnel else "mirror_ab"] = ab
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
