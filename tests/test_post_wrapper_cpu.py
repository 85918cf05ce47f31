"""The post-pass section of rt.Scene as a caller sees it without a device, against tests/golden/post_wrapper_api.json:
the signature of every public method from denoise_desc to denoise_times, and every field of what the five descriptor
builders return for three kinds of call -- all defaults, every optional given, the flags given as False (and, for the
temporal pair, a camera without a previous one). A refactor of the section must move none of it; this test is the pin.

The golden file is written by hand, never by the test:

    python tests/test_post_wrapper_cpu.py --write"""
import ctypes as C
import inspect
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_wrapper_api.json")
FIRST, LAST = "denoise_desc", "denoise_times"
BUILDERS = {"denoise_desc": (640, 360), "vdenoise_desc": (640, 360), "temporal_desc": (640, 360),
            "temporal_motion_desc": (640, 360), "upsample_desc": (640, 360, 320, 180)}
FLAGS = ("demodulate", "reset", "use_tables", "clamp")
GIVEN = dict(iterations=3, normal_shift=2, sigma_depth=0.125, sigma_colour=0.75, sigma_floor=0.03125, min_history=6,
             spatial_boost=2.5, variant=1, max_history=9, depth_tolerance=0.0625, normal_cos_min=0.5, clamp_slack=0.375,
             clamp_history=7, aspect=1.25, prev_aspect=1.75)


def _load():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import rt_amd
    return rt_amd.load()


def public_methods(rt):
    names = list(vars(rt.Scene))
    return [n for n in names[names.index(FIRST):names.index(LAST) + 1] if not n.startswith("_")]


def fields(d):
    """Every field of a descriptor: numbers as they are, a camera as the hex of its bytes."""
    out = {}
    for k, _ in d._fields_:
        v = getattr(d, k)
        out[k] = bytes(v).hex() if isinstance(v, C.Structure) else v
    return out


def calls(rt, name):
    """{call: keyword arguments} for the builder `name`."""
    params = inspect.signature(getattr(rt.Scene, name)).parameters
    if name == "temporal_motion_desc":           # **kw: temporal_desc's
        params = {**params, **inspect.signature(rt.Scene.temporal_desc).parameters}
    keys = [k for k, p in params.items() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    every = {}
    for i, k in enumerate(keys):
        if k in FLAGS:
            every[k] = True
        elif k in ("cam", "prev_cam"):
            every[k] = rt.Camera(rt.Vec3(1, 2, 3) if k == "cam" else rt.Vec3(-4, 5, 6), rt.Vec3(0, 0, 1), 0.5, 170.0, -15.0)
        else:
            every[k] = GIVEN.get(k, 0x1000 * (i + 1))          # a pointer or a count: left as the integer passed in
    out = {"defaults": {}, "every_optional": every, "flags_false": {k: False for k in keys if k in FLAGS}}
    if "cam" in keys:
        out["cam_only"] = {"cam": every["cam"], "aspect": 1.25}
    return out


def snapshot(rt):
    scene = rt.Scene()
    try:
        descs = {name: {call: fields(getattr(scene, name)(*size, **kw)) for call, kw in calls(rt, name).items()}
                 for name, size in BUILDERS.items()}
    finally:
        scene.close()
    return {"signatures": {n: str(inspect.signature(getattr(rt.Scene, n))) for n in public_methods(rt)}, "descs": descs}


def test_the_post_pass_section_keeps_its_signatures_and_descriptors(rt):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(snapshot(rt)))
    assert list(got["signatures"]) == list(want["signatures"])
    assert got["signatures"] == want["signatures"]
    for name in BUILDERS:
        for call in want["descs"][name]:
            assert got["descs"][name][call] == want["descs"][name][call], (name, call)
    assert got["descs"] == want["descs"]


def test_temporal_motion_desc_carries_temporal_desc_unchanged(rt):
    scene = rt.Scene()
    try:
        for call, kw in calls(rt, "temporal_desc").items():
            t, m = fields(scene.temporal_desc(640, 360, **kw)), fields(scene.temporal_motion_desc(640, 360, **kw))
            assert m["struct_size"] == C.sizeof(rt.TMotionDesc) and t["struct_size"] == C.sizeof(rt.TemporalDesc)
            assert {k: m[k] for k in t if k != "struct_size"} == {k: v for k, v in t.items() if k != "struct_size"}, call
            assert list(m)[:len(t)] == list(t)
    finally:
        scene.close()


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="write the golden file (otherwise: compare with it)")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    snap = json.loads(json.dumps(snapshot(_load())))
    if a.write:
        with open(a.out, "w") as f:
            f.write(json.dumps(snap, indent=1) + "\n")
        print(f"wrote {len(snap['signatures'])} signatures and {sum(len(v) for v in snap['descs'].values())} descriptors")
    else:
        with open(a.out) as f:
            print("same" if json.load(f) == snap else "DIFFERENT")
