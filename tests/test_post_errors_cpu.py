"""The refusals of the post passes, pinned: the return code and the whole text of rt_last_error() of a fixed walk of
calls against tests/golden/post_errors.json, which `python tests/test_post_errors_cpu.py --write` records. The per-pass
_cpu suites check that a refusal names its field; this pins the wording, the order of the checks and the numbers in the
parenthesis, for all nine entries and the fourteen timing functions.

The walk holds refusals only. The scene is host only and the pointers are made up (fixed numbers, so that nothing in a
text can depend on where a buffer happens to lie): every description here is refused before anything is enqueued, and
none that passes the checks may be added, since where a device is visible it would be launched on those pointers. A
host-only scene has no sky, which is what refuses an indirect description whose own fields are all in range; the
"no texture" refusal behind it needs a sky, so a device, and is not in the walk. rt_scene_denoise does not check its
buffers for overlaps, so it has no overlap cases."""
import ctypes as C
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_errors.json")
NAN, INF = float("nan"), float("inf")
BASE = 0x10000000                      # the made-up buffers: one every 4 KiB from here (16 x 8 pixels: at most 2 KiB each)
RT_ERR_INVALID = 1


class at:
    """The made-up address of a description's buffer, plus an offset."""
    def __init__(self, name, off=0):
        self.name, self.off = name, off

    def __repr__(self):
        return f"@{self.name}{self.off:+d}" if self.off else f"@{self.name}"


class size_of:
    """A struct_size that ends before the named field."""
    def __init__(self, field):
        self.field = field

    def __repr__(self):
        return f"up to {self.field}"


# entry -> (description type, its init, the buffers in the order they are laid out, other fields of the base description)
_CAM = object()
ENTRIES = {
    "rt_scene_denoise": ("DenoiseDesc", "rt_denoise_desc_init",
                         ("rgba_in", "depth", "normal", "albedo", "id", "rgba_out", "pixels"), dict(width=16, height=8)),
    "rt_scene_denoise_variance": ("VDenoiseDesc", "rt_vdenoise_desc_init",
                                  ("rgba_in", "depth", "normal", "albedo", "id", "rgba_out", "pixels", "moments", "variance_out"),
                                  dict(width=16, height=8)),
    "rt_scene_temporal": ("TemporalDesc", "rt_temporal_desc_init",
                          ("rgba_in", "depth", "normal", "id", "prev_rgba", "prev_depth", "prev_normal", "prev_id",
                           "prev_moments", "rgba_out", "moments_out", "pixels"),
                          dict(width=16, height=8, aspect=1.5, prev_aspect=1.5, cam=_CAM, prev_cam=_CAM)),
    "rt_scene_temporal_motion": ("TMotionDesc", "rt_tmotion_desc_init",
                                 ("rgba_in", "depth", "normal", "id", "prev_rgba", "prev_depth", "prev_normal", "prev_id",
                                  "prev_moments", "rgba_out", "moments_out", "pixels", "sphere_motion", "cube_motion"),
                                 dict(width=16, height=8, aspect=1.5, prev_aspect=1.5, cam=_CAM, prev_cam=_CAM,
                                      n_sphere_motion=64, n_cube_motion=8)),
    "rt_scene_upsample": ("UpsampleDesc", "rt_upsample_desc_init",
                          ("rgba_lo", "depth_lo", "normal_lo", "albedo_lo", "id_lo", "depth", "normal", "albedo", "id", "base",
                           "rgba_out", "pixels", "source", "sphere_select", "plane_select", "cube_select"),
                          dict(width=16, height=8, lo_width=8, lo_height=4, n_sphere_select=16, n_plane_select=4,
                               n_cube_select=4, use_tables=1)),
    "rt_scene_display": ("DisplayDesc", "rt_display_desc_init",
                         ("rgba_in", "id", "rgba_out", "pixels", "state", "histogram_out"), dict(width=16, height=8)),
    "rt_scene_bloom": ("BloomDesc", "rt_bloom_desc_init", ("rgba_in", "state", "rgba_out", "pixels", "glow_out"),
                       dict(width=16, height=8)),
    "rt_scene_indirect": ("IndirectDesc", "rt_indirect_desc_init",
                          ("depth", "normal", "id", "albedo", "rgba_in", "rgba_out", "pixels"),
                          dict(width=16, height=8, aspect=1.0, cam=_CAM)),
}
ENTRIES["rt_scene_indirect_paths"] = ENTRIES["rt_scene_indirect"]
TIMED = ("denoise", "vdenoise", "temporal", "upsample", "display", "bloom", "indirect")


def _common_atrous():
    return [dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20), dict(height=32769),
            dict(rgba_in=0), dict(depth=0), dict(normal=0), dict(id=0), dict(rgba_out=0), dict(albedo=0),
            dict(rgba_in=at("rgba_in", 4)), dict(rgba_in=at("rgba_in", 8)), dict(normal=at("normal", 8)),
            dict(albedo=at("albedo", 4)), dict(rgba_out=at("rgba_out", 12)), dict(id=at("id", 4)), dict(depth=at("depth", 2)),
            dict(pixels=at("pixels", 1)),
            dict(iterations=0), dict(iterations=7), dict(iterations=-1), dict(normal_shift=-1), dict(normal_shift=9),
            dict(sigma_depth=0.0), dict(sigma_depth=-0.05), dict(sigma_depth=NAN), dict(sigma_depth=INF),
            dict(sigma_colour=NAN), dict(sigma_colour=INF), dict(variant=-1), dict(variant=3),
            # the order of the checks: the size before a pointer before an alignment before a range
            dict(width=0, rgba_in=0), dict(rgba_in=0, iterations=0), dict(depth=at("depth", 2), iterations=0),
            dict(iterations=0, variant=3), dict(struct_size=size_of("iterations")), dict(struct_size=size_of("rgba_out")),
            dict(struct_size=4)]


def _common_temporal():
    return [dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20), dict(height=32769),
            dict(rgba_in=0), dict(depth=0), dict(normal=0), dict(id=0), dict(rgba_out=0),
            dict(prev_rgba=0), dict(prev_depth=0), dict(prev_normal=0), dict(prev_id=0), dict(prev_moments=0),
            dict(rgba_in=at("rgba_in", 4)), dict(rgba_in=at("rgba_in", 8)), dict(normal=at("normal", 8)),
            dict(rgba_out=at("rgba_out", 12)), dict(prev_rgba=at("prev_rgba", 4)), dict(prev_normal=at("prev_normal", 8)),
            dict(id=at("id", 4)), dict(prev_id=at("prev_id", 4)), dict(prev_moments=at("prev_moments", 4)),
            dict(moments_out=at("moments_out", 4)), dict(depth=at("depth", 2)), dict(prev_depth=at("prev_depth", 1)),
            dict(pixels=at("pixels", 1)),
            dict(max_history=0), dict(max_history=257), dict(max_history=-1), dict(variant=-1), dict(variant=2),
            dict(depth_tolerance=0.0), dict(depth_tolerance=-0.02), dict(depth_tolerance=NAN), dict(depth_tolerance=INF),
            dict(normal_cos_min=-0.1), dict(normal_cos_min=1.5), dict(normal_cos_min=NAN), dict(normal_cos_min=INF),
            dict(aspect=0.0), dict(aspect=NAN), dict(aspect=INF), dict(prev_aspect=0.0), dict(prev_aspect=-1.5),
            dict(prev_aspect=NAN),
            # an output on an input (no alias is allowed: the pass gathers), an output on an output
            dict(rgba_out=at("rgba_in")), dict(rgba_out=at("rgba_in", 16)), dict(rgba_out=at("prev_rgba", 2032)),
            dict(rgba_out=at("prev_rgba", -2032)), dict(rgba_out=at("normal")), dict(rgba_out=at("depth")),
            dict(moments_out=at("prev_moments")), dict(moments_out=at("id", 8)), dict(pixels=at("depth")),
            dict(pixels=at("prev_id", 1020)), dict(pixels=at("rgba_out", 16)), dict(moments_out=at("rgba_out")),
            # reset lifts the need for prev_*, not for the current buffers
            dict(reset=1, depth=0), dict(reset=1, rgba_out=at("rgba_in")), dict(reset=1, prev_aspect=0.0, aspect=0.0),
            dict(width=0, rgba_in=0), dict(rgba_in=0, max_history=0), dict(max_history=0, variant=2),
            dict(struct_size=size_of("max_history")), dict(struct_size=size_of("rgba_in")), dict(struct_size=4)]


def _cases():
    c = {}
    c["rt_scene_denoise"] = _common_atrous()
    c["rt_scene_denoise_variance"] = _common_atrous() + [
        dict(moments=at("moments", 4)), dict(variance_out=at("variance_out", 2)),
        dict(sigma_colour=-1.0), dict(sigma_colour=2.0 ** 21),
        dict(sigma_floor=0.0), dict(sigma_floor=-1.0), dict(sigma_floor=NAN), dict(sigma_floor=INF),
        dict(min_history=0), dict(min_history=257), dict(min_history=-4),
        dict(spatial_boost=-1.0), dict(spatial_boost=NAN), dict(spatial_boost=INF),
        # an output on an input, an output on an output, rgba_out inside rgba_in but not rgba_in itself
        dict(pixels=at("rgba_in")), dict(variance_out=at("depth")), dict(rgba_out=at("normal")), dict(rgba_out=at("moments")),
        dict(variance_out=at("pixels")), dict(pixels=at("rgba_out")), dict(rgba_out=at("rgba_in", 16)),
        dict(rgba_out=at("rgba_in", -16)), dict(variance_out=at("moments", 64)),
        dict(struct_size=size_of("sigma_floor")), dict(struct_size=size_of("min_history")),
        dict(struct_size=size_of("sigma_depth"))]
    c["rt_scene_temporal"] = _common_temporal()
    c["rt_scene_temporal_motion"] = _common_temporal() + [
        dict(n_sphere_motion=-1), dict(n_cube_motion=-1), dict(n_sphere_motion=-(1 << 31)),
        dict(sphere_motion=0), dict(cube_motion=0), dict(sphere_motion=0, n_sphere_motion=1),
        dict(sphere_motion=at("sphere_motion", 4)), dict(sphere_motion=at("sphere_motion", 8)),
        dict(cube_motion=at("cube_motion", 12)), dict(cube_motion=at("cube_motion", 1)),
        dict(clamp_slack=-0.01), dict(clamp_slack=16.5), dict(clamp_slack=NAN), dict(clamp_slack=INF), dict(clamp_slack=-INF),
        dict(clamp_history=0), dict(clamp_history=257), dict(clamp_history=-4),
        dict(rgba_out=at("sphere_motion")), dict(rgba_out=at("sphere_motion", 1008)), dict(rgba_out=at("sphere_motion", -2032)),
        dict(moments_out=at("cube_motion")), dict(moments_out=at("cube_motion", 120)), dict(pixels=at("cube_motion", 64)),
        dict(pixels=at("sphere_motion", 1020)),
        dict(clamp=0, clamp_slack=-1.0), dict(reset=1, rgba_out=at("sphere_motion")),
        dict(struct_size=size_of("clamp_history")), dict(struct_size=size_of("sphere_motion"))]
    c["rt_scene_upsample"] = [
        dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20), dict(height=32769),
        dict(lo_width=0), dict(lo_height=0), dict(lo_width=-2), dict(lo_height=-8),
        dict(lo_width=17), dict(lo_height=9), dict(width=32769, lo_width=32769),
        dict(rgba_lo=0), dict(depth_lo=0), dict(normal_lo=0), dict(id_lo=0), dict(depth=0), dict(normal=0),
        dict(id=0), dict(rgba_out=0), dict(albedo=0), dict(albedo_lo=0),
        dict(rgba_lo=at("rgba_lo", 4)), dict(normal_lo=at("normal_lo", 8)), dict(albedo_lo=at("albedo_lo", 8)),
        dict(normal=at("normal", 4)), dict(albedo=at("albedo", 12)), dict(base=at("base", 8)),
        dict(rgba_out=at("rgba_out", 8)), dict(id=at("id", 4)), dict(id_lo=at("id_lo", 4)),
        dict(depth=at("depth", 2)), dict(depth_lo=at("depth_lo", 1)), dict(pixels=at("pixels", 2)),
        dict(normal_shift=-1), dict(normal_shift=9), dict(variant=-1), dict(variant=2),
        dict(sigma_depth=0.0), dict(sigma_depth=-0.05), dict(sigma_depth=NAN), dict(sigma_depth=INF),
        dict(n_sphere_select=-1), dict(n_plane_select=-1), dict(n_cube_select=-5),
        dict(sphere_select=0), dict(plane_select=0), dict(cube_select=0),
        # an output on an input, an output on an output, rgba_out inside `base` but not `base` itself
        dict(rgba_out=at("rgba_lo")), dict(rgba_out=at("normal")), dict(rgba_out=at("depth")),
        dict(rgba_out=at("base", 16)), dict(rgba_out=at("base", -16)), dict(rgba_out=at("id", 1008)),
        dict(pixels=at("depth")), dict(pixels=at("id_lo", 252)), dict(pixels=at("rgba_out", 16)),
        dict(source=at("rgba_out", 2047)), dict(source=at("pixels")), dict(source=at("sphere_select", 15)),
        dict(source=at("depth_lo", 127)), dict(pixels=at("cube_select")),
        dict(width=0, rgba_lo=0), dict(rgba_lo=0, normal_shift=9), dict(normal_shift=9, variant=2),
        dict(struct_size=size_of("sigma_depth")), dict(struct_size=size_of("rgba_out")), dict(struct_size=4)]
    q = at
    c["rt_scene_display"] = [
        dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20), dict(height=32769),
        dict(meter=-1), dict(meter=3), dict(curve=-1), dict(curve=3), dict(transfer=-1), dict(transfer=2),
        dict(variant=-1), dict(variant=2),
        dict(rgba_in=0), dict(state=0), dict(state=0, meter=2), dict(meter=0, rgba_out=0, pixels=0),
        dict(rgba_in=q("rgba_in", 4)), dict(rgba_in=q("rgba_in", 8)), dict(rgba_out=q("rgba_out", 8)),
        dict(state=q("state", 4)), dict(state=q("state", 8)), dict(id=q("id", 4)), dict(pixels=q("pixels", 2)),
        dict(histogram_out=q("histogram_out", 1)),
        dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=NAN), dict(exposure=INF),
        dict(key=0.0), dict(key=-0.18), dict(key=NAN), dict(key=INF),
        dict(min_exposure=0.0), dict(min_exposure=NAN), dict(min_exposure=INF), dict(min_exposure=-1.0),
        dict(max_exposure=0.0), dict(max_exposure=NAN), dict(max_exposure=INF), dict(min_exposure=2.0, max_exposure=1.0),
        dict(meter_low=-1), dict(meter_low=973), dict(meter_low=1000), dict(meter_high=1025),
        dict(meter_low=1024, meter_high=1024),
        dict(adapt=0.0), dict(adapt=-0.5), dict(adapt=1.5), dict(adapt=NAN),
        dict(white=0.0), dict(white=-4.0), dict(white=NAN), dict(white=INF),
        # an output on an input, an output on an output, rgba_out inside rgba_in but not rgba_in itself
        dict(rgba_out=q("rgba_in", 16)), dict(rgba_out=q("rgba_in", -16)), dict(rgba_out=q("id")), dict(pixels=q("rgba_in")),
        dict(pixels=q("id", 1020)), dict(state=q("rgba_in", 2032)), dict(state=q("id")),
        dict(histogram_out=q("rgba_in", 2044)), dict(histogram_out=q("id", -2044)),
        dict(pixels=q("rgba_out", 2044)), dict(state=q("rgba_out")), dict(state=q("pixels", 496)),
        dict(histogram_out=q("pixels", -2044)), dict(histogram_out=q("state", -2032)), dict(state=q("histogram_out", 2032)),
        dict(meter=0, pixels=q("rgba_out")), dict(meter=0, pixels=q("rgba_in", 2044)),
        dict(width=0, meter=3), dict(meter=3, rgba_in=0), dict(rgba_in=q("rgba_in", 4), exposure=0.0),
        dict(struct_size=size_of("exposure")), dict(struct_size=size_of("white")), dict(struct_size=size_of("adapt")),
        dict(struct_size=size_of("meter_high")), dict(struct_size=size_of("state")), dict(struct_size=4)]
    c["rt_scene_bloom"] = [
        dict(width=0), dict(height=0), dict(width=-3), dict(height=-1), dict(width=1 << 20), dict(height=32769),
        dict(levels=0), dict(levels=-1), dict(levels=9), dict(variant=-1), dict(variant=2),
        dict(rgba_in=0), dict(rgba_out=0, pixels=0, glow_out=0),
        dict(rgba_in=q("rgba_in", 4)), dict(rgba_in=q("rgba_in", 8)), dict(state=q("state", 4)), dict(state=q("state", 8)),
        dict(rgba_out=q("rgba_out", 8)), dict(pixels=q("pixels", 2)), dict(glow_out=q("glow_out", 4)),
        dict(glow_out=q("glow_out", 8)),
        dict(threshold=-1.0), dict(threshold=NAN), dict(threshold=INF),
        dict(limit=0.0), dict(limit=-1.0), dict(limit=NAN), dict(limit=INF),
        dict(spread=-0.25), dict(spread=4.5), dict(spread=NAN), dict(spread=INF),
        dict(strength=-0.125), dict(strength=NAN), dict(strength=INF),
        # an output on an input, an output on an output, rgba_out inside rgba_in but not rgba_in itself
        dict(rgba_out=q("rgba_in", 16)), dict(rgba_out=q("rgba_in", -16)), dict(rgba_out=q("state")),
        dict(rgba_out=q("state", -2032)), dict(pixels=q("rgba_in")), dict(pixels=q("rgba_in", 2044)),
        dict(pixels=q("state", 12)), dict(glow_out=q("rgba_in")), dict(glow_out=q("rgba_in", -2032)),
        dict(glow_out=q("state")), dict(pixels=q("rgba_out", 2044)), dict(glow_out=q("rgba_out")),
        dict(glow_out=q("rgba_out", 2032)), dict(glow_out=q("pixels", -2032)), dict(rgba_out=0, glow_out=q("pixels")),
        dict(width=0, levels=0), dict(levels=0, rgba_in=0), dict(rgba_in=q("rgba_in", 4), limit=0.0),
        dict(struct_size=size_of("levels")), dict(struct_size=size_of("threshold")), dict(struct_size=size_of("limit")),
        dict(struct_size=size_of("rgba_out")), dict(struct_size=size_of("rgba_out"), levels=5),
        dict(struct_size=size_of("rgba_in")), dict(struct_size=4)]
    indirect = [
        dict(width=0), dict(width=32769), dict(height=-1), dict(height=32769),
        dict(aspect=0.0), dict(aspect=-1.0), dict(aspect=NAN), dict(aspect=INF),
        dict(depth=0), dict(normal=0), dict(id=0), dict(rgba_out=0),
        dict(depth=q("depth", 2)), dict(normal=q("normal", 8)), dict(id=q("id", 4)), dict(albedo=q("albedo", 8)),
        dict(rgba_in=q("rgba_in", 4)), dict(rgba_out=q("rgba_out", 8)), dict(pixels=q("pixels", 1)),
        dict(rays=0), dict(rays=17), dict(ray_base=-1), dict(ray_base=(1 << 24) - 3, rays=4), dict(cull=2), dict(cull=-2),
        dict(variant=2), dict(variant=-1), dict(strength=-0.5), dict(strength=NAN), dict(strength=INF),
        # an output on an input, an output on an output, rgba_out inside rgba_in but not rgba_in itself
        dict(rgba_out=q("normal")), dict(pixels=q("depth")), dict(rgba_out=q("rgba_in", 16)), dict(rgba_out=q("rgba_in", -16)),
        dict(pixels=q("rgba_out")), dict(rgba_out=q("albedo")), dict(pixels=q("id", 1020)),
        # every field in range: the scene has no sky
        dict(), dict(rgba_out=q("rgba_in")), dict(albedo=0, rgba_in=0, pixels=0), dict(ray_base=(1 << 24) - 4, rays=4),
        dict(variant=1), dict(width=32768, height=32768, variant=1, rays=16),
        dict(width=0, depth=0), dict(depth=0, rays=0), dict(rays=0, variant=2),
        dict(struct_size=size_of("rays")), dict(struct_size=size_of("depth")), dict(struct_size=4)]
    c["rt_scene_indirect"] = indirect
    # (opts, description fields): "default" passes NULL options; else (struct_size, bounces), struct_size None: the type's
    c["rt_scene_indirect_paths"] = ([dict(opts=(None, b)) for b in (0, 5, -1, 1 << 20)]
                                    + [dict(opts=(0, 9)), dict(opts=(0, 0)), dict(opts=(4, 9)), dict(opts=(4, 0)),
                                       dict(opts=(8, 5)), dict(opts=(64, 5)), dict(opts=(None, 0), width=0)]
                                    + [dict(opts=o, **kw) for o in ("default", (None, 1), (None, 4)) for kw in indirect])
    return c


def walk_table():
    """(label, entry, arguments): arguments "null scene" / "null description", or the fields that differ from the base."""
    rows = []
    for entry, cases in _cases().items():
        rows.append((f"{entry} null scene", entry, "null scene"))
        rows.append((f"{entry} null description", entry, "null description"))
        rows.append((f"{entry} null scene and description", entry, "null both"))
        rows += [(f"{entry} {kw!r}", entry, kw) for kw in cases]
    for t in TIMED:
        rows += [(f"rt_scene_set_{t}_timing null scene", f"rt_scene_set_{t}_timing", (None, 1)),
                 (f"rt_scene_{t}_times before any call", f"rt_scene_{t}_times", ("scene", "ms", 4, "n")),
                 (f"rt_scene_set_{t}_timing on", f"rt_scene_set_{t}_timing", ("scene", 1)),
                 (f"rt_scene_{t}_times with timing on", f"rt_scene_{t}_times", ("scene", "ms", 4, "n")),
                 (f"rt_scene_{t}_times null scene", f"rt_scene_{t}_times", (None, "ms", 4, "n")),
                 (f"rt_scene_{t}_times null ms", f"rt_scene_{t}_times", ("scene", None, 4, "n")),
                 (f"rt_scene_{t}_times null n", f"rt_scene_{t}_times", ("scene", "ms", 4, None)),
                 (f"rt_scene_{t}_times cap -1", f"rt_scene_{t}_times", ("scene", "ms", -1, "n")),
                 (f"rt_scene_{t}_times cap 0", f"rt_scene_{t}_times", ("scene", "ms", 0, "n")),
                 (f"rt_scene_set_{t}_timing off", f"rt_scene_set_{t}_timing", ("scene", 0))]
    return rows


def _desc(rt, lib, entry, kw):
    tname, init, buffers, base = ENTRIES[entry]
    T = getattr(rt, tname)
    d = T()
    getattr(lib, init)(C.byref(d))
    where = {k: BASE + 4096 * i for i, k in enumerate(buffers)}
    for k, v in {**where, **base, **kw}.items():
        if k == "opts":
            continue
        if v is _CAM:
            v = rt.default_camera()
        elif isinstance(v, at):
            v = where[v.name] + v.off
        elif isinstance(v, size_of):
            v = getattr(T, v.field).offset
        setattr(d, k, v)
    return d


def _opts(rt, lib, spec):
    if spec == "default":
        return None
    o = rt.IndirectPathsOpts()
    lib.rt_indirect_paths_opts_init(C.byref(o))
    size, o.bounces = spec
    if size is not None:
        o.struct_size = size
    return C.byref(o)


def walk(rt):
    """[{call, rc, error}] of the table on one fresh host-only scene. It ends at the first pass entry that is not
    refused: nothing may follow a description that got past the checks."""
    lib = rt.load_library()
    scene = lib.rt_scene_create()          # host only: no sky, no lists
    out = []
    try:
        for label, entry, args in walk_table():
            fn = getattr(lib, entry)
            if entry in ENTRIES:
                kw = {} if isinstance(args, str) else args
                d = None if args in ("null description", "null both") else C.byref(_desc(rt, lib, entry, kw))
                s = None if args in ("null scene", "null both") else scene
                if entry == "rt_scene_indirect_paths":
                    rc = fn(s, d, _opts(rt, lib, kw.get("opts", "default")), None)
                else:
                    rc = fn(s, d, None)
            else:
                ms, n = (C.c_float * 4)(), C.c_int(7)
                given = {"scene": scene, "ms": ms, "n": C.byref(n)}
                rc = fn(*[given.get(a, a) if isinstance(a, str) else a for a in args])
            out.append({"call": label, "rc": int(rc), "error": lib.rt_last_error().decode("utf-8", errors="replace")})
            if entry in ENTRIES and rc != RT_ERR_INVALID:
                break
    finally:
        lib.rt_scene_destroy(scene)
    return out


def _dump(rows):
    return json.dumps(rows, indent=1, ensure_ascii=True) + "\n"


def test_the_refusals_are_the_recorded_ones(rt):
    with open(GOLDEN) as f:
        want = json.load(f)
    # the golden is of this table, and no pass entry in it was accepted
    assert [r["call"] for r in want] == [label for label, _, _ in walk_table()]
    for (label, entry, _), w in zip(walk_table(), want):
        if entry in ENTRIES:
            assert w["rc"] == RT_ERR_INVALID and w["error"].startswith(entry + ": "), label
    got = walk(rt)
    for g, w in zip(got, want):
        assert (g["rc"], g["error"]) == (w["rc"], w["error"]), g["call"]
    assert len(got) == len(want)
    # the timing functions: a switch on a scene is accepted, every other call in the walk reports 0 intervals or is refused
    assert {r["rc"] for r in want} == {0, 1}
    by = {r["call"]: r for r in want}
    # the paired entries word these differently
    assert "id 8-byte, depth and pixels 4-byte" in by["rt_scene_denoise {'id': @id+4}"]["error"]
    assert "id and moments 8-byte" in by["rt_scene_denoise_variance {'id': @id+4}"]["error"]
    assert "min_history" not in by["rt_scene_denoise {'width': 0}"]["error"]
    assert "min_history 4" in by["rt_scene_denoise_variance {'width': 0}"]["error"]
    assert by["rt_scene_temporal {'width': 0}"]["error"].startswith("rt_scene_temporal: ")
    assert by["rt_scene_temporal_motion {'width': 0}"]["error"].startswith("rt_scene_temporal_motion: ")
    assert "no sky" in by["rt_scene_indirect {}"]["error"]
    assert "no sky" in by["rt_scene_indirect_paths {'opts': (None, 4)}"]["error"]
    assert "bounces" in by["rt_scene_indirect_paths {'opts': (None, 0), 'width': 0}"]["error"]


def write_golden():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import rt_amd
    rows = walk(rt_amd.load())
    assert len(rows) == len(walk_table()), "a pass entry accepted " + rows[-1]["call"]
    with open(GOLDEN, "w") as f:
        f.write(_dump(rows))
    print("wrote", GOLDEN)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_post_errors_cpu.py --write")
    write_golden()
