#!/usr/bin/env python3
"""What the geometry of the resting-view reader's launch costs before it computes anything: one-wave
workgroups with the reader's block size, LDS bytes and 72 registers (rt_debug_launch_floor), timed with device events
after a pre-roll, the rounds interleaved.

  (a) empty workgroups: the full grid, the unsettled tiles plus runs of 16 settled ones, the unsettled tiles alone
  (b) the same with one scalar load per workgroup, waited for
  (c) the frame's float4 and packed word stored in 8 x 8 tile shape, one tile per workgroup and R tiles per workgroup
  (d) a linear float4 fill of the same bytes: the ceiling

  python3 tools/launch_floor_probe.py [--width 3840 --height 2160 --unsettled 41529] > profiles/compact_launch_floor.json
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rt_amd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--unsettled", type=int, default=41529, help="tiles that keep a wave of their own (C3: 129 600 - 88 071)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--preroll", type=int, default=400)
    a = ap.parse_args()
    rt = rt_amd.load()
    lib = rt.load_library()
    tiles = ((a.width + 7) // 8) * ((a.height + 7) // 8)
    streamed = tiles - a.unsettled
    grids = [("full_grid", tiles), ("unsettled_plus_runs_of_16", a.unsettled + (streamed + 15) // 16), ("unsettled_only", a.unsettled)]
    names, cfgs = [], []
    for what, label in ((0, "a_empty"), (1, "b_scalar_load")):
        for g, n in grids:
            names.append("%s/%s/%d" % (label, g, n))
            cfgs.append((what, n, 1))
    for run in (1, 4, 8, 16, 32):
        names.append("c_tile_stores/run_%d/%d" % (run, (tiles + run - 1) // run))
        cfgs.append((2, (tiles + run - 1) // run, run))
    names.append("d_linear_fill")
    cfgs.append((3, 1, 1))
    flat = np.ascontiguousarray(np.array(cfgs, dtype=np.int32).reshape(-1))
    ms = np.zeros((len(cfgs), a.rounds), dtype=np.float32)
    rc = lib.rt_debug_launch_floor(a.width, a.height, flat.ctypes.data_as(C.POINTER(C.c_int)), len(cfgs), a.rounds, a.reps, a.preroll,
                                   ms.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise SystemExit("rt_debug_launch_floor: %d %s" % (rc, lib.rt_last_error().decode()))
    frame_bytes = a.width * a.height * 20
    out = {"what": "launch floor of the resting-view reader's geometry: one-wave workgroups, the reader's LDS bytes, 72 registers; "
                   "%d x %d, %d tiles of 8 x 8, %d of them unsettled; microseconds per launch, %d launches per timing, "
                   "%d interleaved rounds after %d fills" % (a.width, a.height, tiles, a.unsettled, a.reps, a.rounds, a.preroll),
           "frame_bytes": frame_bytes, "rows": {}}
    for name, row in zip(names, ms):
        us = [float(x) * 1000.0 for x in row]
        e = {"us": [round(x, 2) for x in us], "median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
        if name[0] in "cd":
            e["median_tb_per_s"] = round(frame_bytes / (float(np.median(us)) * 1e-6) / 1e12, 3)
        out["rows"][name] = e
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
