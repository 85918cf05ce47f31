#!/usr/bin/env python3
"""How many tiles of a resting view are settled, counted from the read-backs that do not need the
tile summaries: the light verdicts' words, the primary records and the group count per tile from a G-buffer `id` launch.
A tile is settled iff it has a primary record, at most 4 groups, and every (group, light) code it has is 1. Where the
library has tile summaries, the kernel's own flags are counted beside it and must agree.

  python3 tools/settled_tiles_count.py [--width 3840 --height 2160 --spheres 1024] > profiles/settled_tiles_before.json
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import rt_amd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--spheres", type=int, default=1024)
    a = ap.parse_args()
    rt = rt_amd.load()
    w, h = a.width, a.height
    sc = rt.Scene.default(a.spheres)
    for _ in range(2):                          # plain, then the recording launch
        sc.render(w, h)
    torch.cuda.synchronize()
    words = sc.light_verdicts(want_words=True)
    prim = sc.primary_records(want_tables=True)
    assert words["state"] == 1 and prim["state"] == 1, (words["state"], prim["state"])
    ty, tx = words["words"].shape
    ref = rt.Scene.default(a.spheres)
    ref.set_light_verdicts(0)
    ids = ref.render(w, h, aov=("id",))["aov"]["id"].cpu().numpy()
    torch.cuda.synchronize()

    def tiles(img, fill):
        return rt.pixels_to_tiles(np.pad(img, ((0, ty * 8 - h), (0, tx * 8 - w)), constant_values=fill), 8)

    valid = tiles(np.ones((h, w), dtype=bool), False)
    hit = tiles(ids[..., 0] >= 0, False)
    s = np.sort(tiles(np.where(ids[..., 0] >= 0, ids[..., 1], -1), -1), axis=-1)
    groups = ((s[..., 1:] != s[..., :-1]) & (s[..., 1:] >= 0)).sum(axis=-1) + (s[..., 0] >= 0)
    has = (prim["positions"] != -2).any(axis=-1)
    n_lights = 3
    sh = np.array([[16 * g + 2 * li for li in range(n_lights)] for g in range(4)], dtype=np.uint64)
    codes = (words["words"][..., None, None] >> sh) & np.uint64(3)                       # [ty, tx, 4, lights]
    exists = np.arange(4)[None, None, :, None] < groups[..., None, None]
    settled = has & (groups <= 4) & ((codes == 1) | ~exists).all(axis=(-1, -2))
    miss = (valid & ~hit).any(axis=-1)
    contributing = ((codes != 1) & exists).any(axis=-2).sum(axis=-1)                     # lights some group still evaluates
    out = {"what": "tiles of a resting view that no light reaches, counted from the words, the primary records and a "
                   "G-buffer id launch (8 x 8 tiles, %d x %d, %d spheres, default camera and lights)" % (w, h, a.spheres),
           "tiles": int(settled.size), "with_a_record": int(has.sum()), "more_than_4_groups": int((groups > 4).sum()),
           "more_than_1_group": int((groups > 1).sum()), "without_a_hit": int((groups == 0).sum()),
           "settled": int(settled.sum()), "settled_no_miss_lane": int((settled & ~miss).sum()),
           "settled_has_miss_lanes": int((settled & miss).sum()),
           "settled_share": float(settled.mean()),
           "tiles_by_lights_still_evaluated": [int((contributing == k).sum()) for k in range(n_lights + 1)]}
    if hasattr(sc, "tile_summaries"):
        d = sc.tile_summaries(want_tables=True)["dwords"]
        flagged = (d & rt.RT_TILE_SETTLED) != 0
        out["kernel_flags"] = {"settled": int(flagged.sum()), "settled_no_miss_lane": int((flagged & ((d & rt.RT_TILE_NO_MISS) != 0)).sum()),
                               "agree_with_the_count": bool(np.array_equal(flagged, settled))}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
