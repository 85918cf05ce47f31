"""The operation sequences of tests/test_scene_state_gpu.py (no GPU): deterministic per seed, within the library's rules,
and covering every transition the state tests are there for. The state model's materials rule is DESIGN.md 6d's."""
import numpy as np

import scene_walk as sw
from scene_walk import WALK_SEEDS, WALK_STEPS

# what the walks must reach over the GPU test's seeds
REQUIRED = {
    *sw.MUTATIONS, *sw.OUTPUTS,
    "spheres:count", "spheres:same_count", "spheres:same_list",
    "spheres:above_8192", "spheres:cross64_up", "spheres:cross64_down", "spheres:cross65_up", "spheres:cross65_down",
    "lights:move", "lights:along_axis", "lights:count", "lights:colour", "lights:same", "lights:origin",
    "materials:k", "materials:ex", "materials:clear", "materials:kept", "materials:cleared_by_count",
    "materials:old_entry_clears_glass",
    "render:depth0", "render:depth1", "render:depth2", "render:depth3", "render:glass",
    "render:spp1", "render:spp2", "render:spp4", "render:cull0", "render:cull1", "render:band",
    "render:deferred_second_stream", "graph:set_camera", "query:primary", "query:random",
    "graph_after:lights", "graph_after:spheres", "query_after:lights", "query_after:spheres", "query_after:texture",
}


def test_generator_is_deterministic_per_seed():
    for seed in WALK_SEEDS:
        assert sw.generate(seed, WALK_STEPS) == sw.generate(seed, WALK_STEPS)
    assert sw.generate(WALK_SEEDS[0], WALK_STEPS) != sw.generate(WALK_SEEDS[1], WALK_STEPS)


def test_walks_cover_every_transition():
    seen = set()
    for seed in WALK_SEEDS:
        seen |= sw.transitions(sw.generate(seed, WALK_STEPS))
    assert not REQUIRED - seen, sorted(REQUIRED - seen)


def test_walks_respect_the_library_rules():
    for seed in WALK_SEEDS:
        state = sw.State()
        for i, op in enumerate(sw.generate(seed, WALK_STEPS)):
            where = "seed %d step %d: %s" % (seed, i, op)
            k = op["op"]
            if k == "render":
                w, h = op["size"]
                y0, y1 = op["band"]
                assert op["band"] == (0, 0) or 0 <= y0 < y1 <= h, where
                assert op["spp"] in (1, 2, 4) and 0 <= op["depth"] <= 3, where
                if op["depth"]:   # reflective frames: spheres only, one sample
                    assert state.reflect_ok() and op["spp"] == 1, where
            elif k == "lights":
                assert 1 <= len(op["lights"]) <= 4, where
            elif k == "materials" and op["mats"] is not None:
                assert state.n > 0, where
                m = sw.material_arrays(op["mats"][0], op["mats"][1], state.n)
                assert all(a.size == state.n for a in m), where           # one material per sphere
                k_, tau, ior = m
                assert not ((k_ > 0) & (tau > 0)).any(), where              # a mirror or glass, not both
                assert ((tau == 0) | ((ior >= 1) & (ior <= 4))).all(), where
                if op["mats"][0] == "k":
                    assert not tau.any(), where
            elif k == "spheres":
                assert op["spheres"][0] in sw.SPHERE_COUNTS, where
            state = sw.apply(state, op)


def test_light_moved_along_its_axis_keeps_the_axis_bits():
    """The "along_axis" moves keep the normalised axis the column tables are keyed on bit for bit (as
    rt_scene_prepare_lights forms it: binary32 length, then division) and change the position."""
    def axis(p):
        p = np.float32(p)
        ln = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2], dtype=np.float32)
        return (p / ln).astype(np.float32).view(np.uint32)
    n = 0
    for seed in WALK_SEEDS:
        lights = sw.DEFAULT_LIGHTS
        for op in sw.generate(seed, WALK_STEPS):
            if op["op"] != "lights":
                continue
            if op["how"] == "along_axis":
                moved = [(a, b) for a, b in zip(lights, op["lights"]) if a != b]
                assert len(moved) == 1
                a, b = moved[0]
                assert np.array_equal(axis(a[0:3]), axis(b[0:3])) and a[0:3] != b[0:3]
                n += 1
            lights = op["lights"]
    assert n > 0


def test_materials_kept_and_cleared_as_design_6d_says():
    s = sw.State(spheres=(64, 1, 0.0))
    s = sw.apply(s, {"op": "materials", "mats": ("ex", 3)})
    assert sw.apply(s, {"op": "spheres", "spheres": (64, 1, 0.5)}).mats == ("ex", 3)     # same count: kept
    assert sw.apply(s, {"op": "spheres", "spheres": (64, 2, 0.0)}).mats == ("ex", 3)
    gone = sw.apply(s, {"op": "spheres", "spheres": (65, 1, 0.0)})
    assert gone.mats is None                                                              # another count: cleared
    assert sw.apply(gone, {"op": "spheres", "spheres": (64, 1, 0.0)}).mats is None        # and they do not come back
    old = sw.apply(s, {"op": "materials", "mats": ("k", 3)})                             # the old entry: no glass
    k, tau, _ = sw.material_arrays(*old.mats, 64)
    assert not tau.any() and k.any()
    assert sw.apply(s, {"op": "materials", "mats": None}).mats is None
    # the ex arrays carry glass, and the k arrays of both kinds of one seed are the same mirrors
    k_ex, tau_ex, _ = sw.material_arrays("ex", 3, 64)
    assert tau_ex.any() and np.array_equal(k_ex, k)
