"""The operation sequences of tests/test_scene_state_gpu.py (no GPU): deterministic per seed, within the library's rules,
and covering every transition the state tests are there for. The state model's materials rule is DESIGN.md 6d's; the
rules of the plane and cube materials, the scope and the sampling mode are rt_engine.h's. The first vocabulary's
sequences are pinned by digest; the second vocabulary's walks must reach REQUIRED_2 and keep refusals rare. The third
vocabulary (roughness, gloss seed, glass model, the gather passes; tests/test_scene_state3_gpu.py) is pinned by digest
like the other two, its walks must reach sw.REQUIRED_3, and its model follows rt_engine.h's "Glossy reflections" and
"Fresnel glass"."""
import hashlib

import numpy as np

import scene_walk as sw
from scene_walk import WALK_SEEDS, WALK_SEEDS_2, WALK_STEPS

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


# ------------------------------------------------------------------------------------------------ the second vocabulary
# sha256 of repr(generate(seed, 60)) as the module gave it before it had a second vocabulary
OLD_WALKS = {
    1: "3d583f709ee6ab650e7cf81cfef6f64c694b067a1b942ce258fd4a2d5c6cad38",
    2: "f15aa82666891577da7f8378c6bbff54ea7e3900f4df5715876fdf65a872ac82",
    97: "e677782c7f7fc5b7020803a38da34d06f8b8fff74db3f0d78f2921161d609d3d",
    13: "6f0ffb8bd36167a58bc3653b26ffe5a7014142e3244137b089020a0bc7b9467e",
    22: "37f55e6d86995fc40dbc26ab3cda83134fe8f2f1cc4f879bb211d7048f4aaf0d",
    29: "d93a939dec5b823120daea69f5a3568156a049b60e43b1aaf225ce7d9d588303",
}

REQUIRED_2 = {
    *sw.MUTATIONS_2, *sw.OUTPUTS_2,
    "scope:to_scene", "scope:to_spheres", "samples:to_many", "samples:to_one", "view_lists:off", "view_lists:on",
    "planes:on", "planes:off", "planes:other_count", "planes:same_count_moved",
    "cubes:on", "cubes:off", "cubes:other_count", "cubes:same_count_moved",
    "plane_materials:set", "cube_materials:set", "cube_materials:clear",
    "kind_materials:kept", "kind_materials:cleared_by_count",
    "render:scene_scope_depth>0", "render:scene_scope_with_mesh", "render:many_two_groups",
    "render:many_accumulate_split", "render:many_sample_range", "render:aov", "render:aov_reflective",
    "refused:scope", "refused:samples",
    "pass:denoise", "pass:vdenoise", "pass:vdenoise_history", "pass:upsample_exact2", "pass:upsample_exact3",
    "pass:upsample_other_ratio",
    "pass:render_upscaled",
    "temporal:camera", "temporal:motion_spheres", "temporal:motion_cubes",
    "pass_deferred_then_mutation", "graph_after:view_lists", "render_upscaled_after:materials_cleared_by_count",
}
GROUPS = ("scope:", "samples:", "pass:", "temporal:")


def test_the_first_walks_are_what_they_were():
    assert set(OLD_WALKS) == set(WALK_SEEDS) and WALK_STEPS == 60
    for seed, digest in OLD_WALKS.items():
        assert hashlib.sha256(repr(sw.generate(seed, 60)).encode()).hexdigest() == digest, seed
        assert sw.generate(seed, 60, vocabulary=1) == sw.generate(seed, 60)


def test_second_generator_is_deterministic_per_seed():
    for seed in WALK_SEEDS_2:
        ops = sw.generate(seed, WALK_STEPS, vocabulary=2)
        assert ops == sw.generate(seed, WALK_STEPS, vocabulary=2) == sw.generate_2(seed, WALK_STEPS)
        assert len(ops) == WALK_STEPS and all(op["op"] in sw.MUTATIONS_2 + sw.OUTPUTS_2 for op in ops)
    assert sw.generate(WALK_SEEDS_2[0], WALK_STEPS, vocabulary=2) != sw.generate(WALK_SEEDS_2[1], WALK_STEPS, vocabulary=2)


def test_second_walks_cover_every_transition():
    walks = {label: 0 for label in REQUIRED_2}
    for seed in WALK_SEEDS_2:
        one = sw.transitions(sw.generate(seed, WALK_STEPS, vocabulary=2))
        for g in GROUPS:                              # every single walk: the scope, the samples, a pass, temporal
            assert any(label.startswith(g) for label in one), (seed, g)
        for label in one & REQUIRED_2:
            walks[label] += 1
    thin = sorted(label for label, n in walks.items() if n < 2)   # no transition rests on one walk alone
    assert not thin, thin


def test_refusals_are_the_headers_and_rare():
    """A refused step asks for what rt_engine.h names RT_ERR_UNSUPPORTED in the step's state, and nothing else is
    refused: at most a quarter of a walk's output steps."""
    for seed in WALK_SEEDS_2:
        state = sw.State()
        outputs = refused = 0
        for i, op in enumerate(sw.generate(seed, WALK_STEPS, vocabulary=2)):
            where = "seed %d step %d: %s" % (seed, i, op)
            if op["op"] in sw.OUTPUTS_2:
                outputs += 1
            if op["op"] == "refused":
                refused += 1
                assert 1 <= op["depth"] <= 3, where
                if op["why"] == "scope":
                    assert state.scope == "spheres" and (state.planes or state.cubes or state.mesh), where
                    assert op["request"] == {}, where
                else:
                    assert op["why"] == "samples" and state.samples == "one" and state.reflect_ok(), where
                    r = op["request"]
                    assert r.get("spp", 1) > 1 or r.get("sample_base", 0) != 0 or r.get("sample_total", 0) > 1 \
                        or r.get("accumulate"), where
                    n, total = r.get("spp", 1), r.get("sample_total", 0) or r.get("spp", 1)
                    assert 0 <= r.get("sample_base", 0) and r.get("sample_base", 0) + n <= total <= 16, where
            state = sw.apply(state, op)
        assert refused >= 1 and 4 * refused <= outputs, (seed, refused, outputs)


def test_second_walks_respect_the_library_rules():
    for seed in WALK_SEEDS_2:
        state = sw.State()
        for i, op in enumerate(sw.generate(seed, WALK_STEPS, vocabulary=2)):
            where = "seed %d step %d: %s" % (seed, i, op)
            k = op["op"]
            if k == "render":
                w, h = op["size"]
                y0, y1 = op["band"]
                assert (w, h) in sw.SIZES and (op["band"] == (0, 0) or 0 <= y0 < y1 <= h), where
                n, base, total = op["spp"], op["sample_base"], op["sample_total"]
                assert n in (1, 2, 4, 5) and 0 <= op["depth"] <= 3, where
                assert total == 0 or (0 <= base and base + n <= total <= 16), where
                if op["depth"]:
                    assert state.reflect_ok(), where
                    if n > 1 or total or op["split"]:
                        assert state.samples == "many", where
                else:
                    assert n in (1, 2, 4) and not total and not op["split"], where
                if op["split"]:
                    assert 1 <= op["split"] < n and not total, where
                if op["aov"]:                         # guides: one sample
                    assert n == 1 and total == 0 and not op["split"] and set(op["aov"]) <= set(sw.AOV), where
            elif k == "pass":
                assert op["what"] in ("denoise", "vdenoise", "upsample", "render_upscaled"), where
                if op["what"] == "render_upscaled" or op.get("depth"):
                    assert state.reflect_ok(), where
                if op["what"] in ("upsample", "render_upscaled"):
                    assert op["factor"] in (2, 3) and min(op["size"]) // op["factor"] >= 1, where
                    if op["factor"] == 2:             # "exact2" is what it says at every size of the pool
                        assert not (op["size"][0] % 2 or op["size"][1] % 2), where
            elif k == "temporal":
                m = op["mutation"]
                assert (m is None) == (op["form"] == "camera"), where
                a, b = op["cams"]                     # two views: the second frame reprojects the first's history
                assert a != b and sw.CAMERAS[a] != sw.CAMERAS[b], where
                if m is not None:                     # the counts stay: the history's displacements are defined
                    after = sw.apply(state, m)
                    assert (after.n, after.n_cubes) == (state.n, state.n_cubes) and after != state, where
                    assert m["how"] in ("same_count", "same_count_moved"), where
            elif k in ("planes", "cubes"):
                specs = sw.PLANE_SPECS if k == "planes" else sw.CUBE_SPECS
                assert op[k] is None or op[k] in specs, where
                old, new = sw.spec_of(getattr(state, k), specs), sw.spec_of(op[k], specs)
                assert {"on": old[0] == 0 < new[0], "off": new[0] == 0 < old[0],
                        "same_count_moved": old[0] == new[0] > 0 and old != new,
                        "other_count": 0 < old[0] != new[0] > 0}[op["how"]], where
            elif k in ("plane_materials", "cube_materials") and op["seed"] is not None:
                n = state.n_planes if k == "plane_materials" else state.n_cubes
                assert n > 0 and set(sw.kind_k(op["seed"], n).tolist()) <= set(sw.KIND_K), where
            elif k == "materials" and op["mats"] is not None:
                assert state.n > 0, where
            state = sw.apply(state, op)


def test_kind_tables_scope_and_samples_follow_the_header():
    """rt_engine.h: the plane / cube tables survive set_planes / set_cubes with the same count and are cleared by a
    different count; the scope and the sampling mode survive everything."""
    s = sw.State(planes=(2, 0), cubes=(5, 0), scope="scene", samples="many", view_lists=0)
    s = sw.apply(s, {"op": "plane_materials", "seed": 3})
    s = sw.apply(s, {"op": "cube_materials", "seed": 4})
    moved = sw.apply(s, {"op": "cubes", "cubes": (5, 1)})
    assert (moved.cube_mats, moved.plane_mats) == (4, 3)                                  # same count: kept
    fewer = sw.apply(moved, {"op": "cubes", "cubes": (4, 1)})
    assert fewer.cube_mats is None and fewer.plane_mats == 3                              # another count: that table only
    assert sw.apply(fewer, {"op": "cubes", "cubes": (5, 1)}).cube_mats is None            # and it does not come back
    assert sw.apply(s, {"op": "cubes", "cubes": None}).cube_mats is None
    assert sw.apply(s, {"op": "planes", "planes": (2, 1)}).plane_mats == 3
    assert sw.apply(s, {"op": "planes", "planes": (1, 0)}).plane_mats is None
    assert sw.apply(s, {"op": "planes", "planes": True}).plane_mats == 3                  # the first vocabulary's "on": 2 planes
    assert sw.apply(s, {"op": "plane_materials", "seed": None}).plane_mats is None
    assert sw.apply(s, {"op": "spheres", "spheres": (65, 1, 0.0)}).cube_mats == 4         # the spheres' count is no key
    ops = [{"op": "spheres", "spheres": (8, 2, 0.0)}, {"op": "planes", "planes": None}, {"op": "cubes", "cubes": (4, 0)},
           {"op": "mesh", "mesh": 2}, {"op": "materials", "mats": None}, {"op": "lights", "lights": sw.DEFAULT_LIGHTS[:1]},
           {"op": "cube_materials", "seed": None}, {"op": "tile_order", "tile_order": 0}]
    for op in ops:
        s = sw.apply(s, op)
        assert (s.scope, s.samples, s.view_lists) == ("scene", "many", 0), op
    # reflect_ok: the scene scope, or nothing but spheres
    assert s.reflect_ok() and not sw.apply(s, {"op": "scope", "scope": "spheres"}).reflect_ok()
    for field, value in (("planes", (1, 0)), ("cubes", (4, 1)), ("mesh", 1), ("mesh", 2)):
        assert not sw.State(**{field: value}).reflect_ok() and sw.State(scope="scene", **{field: value}).reflect_ok()
    assert sw.State().reflect_ok()
    # a temporal step carries its mutation into the state
    t = {"op": "temporal", "mutation": {"op": "spheres", "spheres": (256, 1, 0.25)}}
    assert sw.apply(sw.State(), t).spheres == (256, 1, 0.25)
    assert sw.apply(sw.State(), {"op": "temporal", "mutation": None}) == sw.State()


def test_the_variants_of_the_lists(rt):
    """The plane and cube lists of a spec: the first `count` primitives of the mixed scene, one of them translated in
    variant 1; the displacement tables are the difference of the two states' origins in binary32."""
    full_p, n_p, full_c, n_c = sw.planes_cubes(rt)
    assert (n_p, n_c) == (sw.PLANE_SPECS[0][0], sw.CUBE_SPECS[0][0])
    raw = lambda arr, i: bytes(arr[i])
    for count, variant in sw.CUBE_SPECS:
        arr, n = sw.cube_list(rt, (count, variant))
        assert n == count
        for i in range(count):
            assert (raw(arr, i) == raw(full_c, i)) == (not (variant and i == 1)), (count, variant, i)
    for count, variant in sw.PLANE_SPECS:
        arr, n = sw.plane_list(rt, (count, variant))
        assert n == count
        for i in range(count):
            assert (raw(arr, i) == raw(full_p, i)) == (not (variant and i == count - 1)), (count, variant, i)
    a, b = sw.State(spheres=(8, 1, 0.0), cubes=(5, 0)), sw.State(spheres=(8, 1, 0.25), cubes=(5, 1))
    sm, cm = sw.motion_tables(rt, a, b)
    # (fl(y + 0.25) - y is 0.25 up to the rounding of the sum)
    assert sm.shape == (8, 4) and not sm[:, [0, 2, 3]].any() and np.abs(sm[:, 1] - 0.25).max() < 1e-6
    assert cm.shape == (5, 4) and np.abs(cm[1, :3] - np.float32(sw.CUBE_MOVE)).max() < 1e-6 and not cm[[0, 2, 3, 4]].any()
    oa, ob = sw.origins(rt, a), sw.origins(rt, b)
    assert np.array_equal(sm[:, :3], ob[0] - oa[0]) and np.array_equal(cm[:, :3], ob[1] - oa[1])
    sm, cm = sw.motion_tables(rt, a, sw.State(spheres=(8, 1, 0.0), cubes=(5, 1)))
    assert sm.shape == (0, 4) and cm.shape == (5, 4)


# ------------------------------------------------------------------------------------------------ the third vocabulary
# sha256 of repr(generate(seed, 60, vocabulary=2)) as the module gave it before it had a third vocabulary
OLD_WALKS_2 = {
    17: "d4334273a920017e50326952f9ae5c0e91306ed31189d12818c2384175b63685",
    25: "cfd83cc728f8c839ef5bc3675cab48abbfc5a6ac67d51147f144b62044afeaea",
    149: "5e5f3501c3549d10c7b25185bd2b993d52d1cd7d59b10e16476cde57c6ad9f30",
    262: "d32dac465741cc577c062918528afaf09a9a1289ae4f834897299622ffef0ff5",
    1103: "b9a187c545009a3cff6a989a7b7fd7f4bfaaaf4a986a8b335f5f03aecc60f29c",
    1205: "3d127c39f3e101cba9a6bed29489eaa19e2cbc76c5b18fe7d542cede33ecba76",
}
# sha256 of repr(generate(seed, 60, vocabulary=3)): the walks tests/test_scene_state3_gpu.py was run with
WALKS_3 = {
    700: "edd8f71a064d5167313cbf0243fee0f38d3b2f1f7ec1a548cb17c8ea0d1ea9fd",
    1235: "0e8cd3157a17396348cd47aa6be42df35a35131928736890f83744a658563956",
    2191: "84a2712781267b4c6b104055a48342cdddfe7c9519afa746609b227585feb8fc",
    4727: "9453bba134da01d13a21ae40e3cc158640132fb74f284b1910e084877f7e28e5",
    6182: "faa7e6a30f8f2acf4357c406501a58fec4cfb13c93c3e2f3b6bf783eb390ee17",
    7125: "a540f888fe951eeea6e6cbd1ef71ef781bcd09ed4e7c6e265c95aa83d4d5026f",
}


def _digest(ops):
    return hashlib.sha256(repr(ops).encode()).hexdigest()


def test_the_second_walks_are_what_they_were():
    assert set(OLD_WALKS_2) == set(WALK_SEEDS_2) and WALK_STEPS == 60
    for seed, digest in OLD_WALKS_2.items():
        assert _digest(sw.generate(seed, 60, vocabulary=2)) == digest, seed
    # and the label sets of the first two vocabularies carry nothing of the third
    for seeds, v in ((WALK_SEEDS, 1), (WALK_SEEDS_2, 2)):
        for seed in seeds:
            new = {t for t in sw.transitions(sw.generate(seed, 60, vocabulary=v))
                   if t.split(":")[0] in ("roughness", "gather", "gather_after", "bvh_first_user", "gloss_seed", "glass_model")}
            assert not new, (v, seed, new)


def test_third_generator_is_deterministic_and_pinned():
    assert set(WALKS_3) == set(sw.WALK_SEEDS_3) and len(sw.WALK_SEEDS_3) == 6
    assert sw.MUTATIONS_3 == sw.MUTATIONS_2 + ("roughness", "gloss_seed", "glass_model")
    assert sw.OUTPUTS_3 == sw.OUTPUTS_2 + ("gather",)
    for seed, digest in WALKS_3.items():
        ops = sw.generate(seed, WALK_STEPS, vocabulary=3)
        assert ops == sw.generate(seed, WALK_STEPS, vocabulary=3) == sw.generate_3(seed, WALK_STEPS)
        assert len(ops) == WALK_STEPS and all(op["op"] in sw.MUTATIONS_3 + sw.OUTPUTS_3 for op in ops)
        assert _digest(ops) == digest, seed
    assert sw.generate(sw.WALK_SEEDS_3[0], WALK_STEPS, vocabulary=3) != sw.generate(sw.WALK_SEEDS_3[1], WALK_STEPS, vocabulary=3)


def test_third_walks_cover_every_transition():
    assert len(sw.REQUIRED_3) == 70 and set(sw.MUTATIONS_3 + sw.OUTPUTS_3) <= sw.REQUIRED_3
    walks = {label: 0 for label in sw.REQUIRED_3}
    for seed in sw.WALK_SEEDS_3:
        one = sw.transitions(sw.generate(seed, WALK_STEPS, vocabulary=3))
        assert "gather" in one and any(t.startswith("gather_after:") for t in one), seed     # every single walk
        for label in one & sw.REQUIRED_3:
            walks[label] += 1
    missing = sorted(label for label, n in walks.items() if n == 0)
    assert not missing, missing
    thin = sorted(label for label, n in walks.items() if n < 2)   # no transition rests on one walk alone
    assert not thin, thin


def test_third_walks_respect_the_library_rules():
    """Every walk replayed against apply: the second vocabulary's rules for what it shares, and the new steps within
    what rt_engine.h accepts -- a roughness table only for a kind with primitives, its values in [0, 1], a gather with
    rays in 1 .. RT_INDIRECT_MAX_RAYS and bounces in 1 .. RT_INDIRECT_MAX_BOUNCES, bounded above 1024 spheres;
    refusals are the header's and at most a quarter of a walk's output steps."""
    refused_all = 0
    for seed in sw.WALK_SEEDS_3:
        state = sw.State()
        outputs = refused = 0
        for i, op in enumerate(sw.generate(seed, WALK_STEPS, vocabulary=3)):
            where = "seed %d step %d: %s" % (seed, i, op)
            k = op["op"]
            outputs += k in sw.OUTPUTS_3
            if k == "roughness":
                n = state.count_of(op["kind"])
                assert op["kind"] in sw.ROUGH_KINDS and n > 0, where
                assert (op["how"], op["seed"] is None) in (("set", False), ("clear", True)), where
                if op["seed"] is not None:
                    rho = sw.roughness(op["seed"], n)
                    assert rho.dtype == np.float32 and rho.shape == (n,) and set(rho.tolist()) <= set(np.float32(sw.ROUGHNESS).tolist()), where
                    assert op["seed"] != getattr(state, "rough_" + op["kind"]), where
                else:
                    assert getattr(state, "rough_" + op["kind"]) is not None, where
            elif k == "gloss_seed":
                assert op["gloss_seed"] in sw.GLOSS_SEEDS and op["gloss_seed"] != state.gloss_seed, where
            elif k == "glass_model":
                assert op["glass_model"] in ("plain", "fresnel") and op["glass_model"] != state.glass_model, where
            elif k == "gather":
                assert op["entry"] in ("indirect", "paths") and 1 <= op["rays"] <= 16 and 1 <= op["bounces"] <= 4, where
                assert op["entry"] == "paths" or op["bounces"] == 1, where
                assert op["rays"] in sw.GATHER_RAYS and op["ray_base"] in (0, 3) and op["strength"] in (0.75, 1.0), where
                assert 0 <= op["seed"] < 1 << 32 and op["cull"] in (0, 1) and op["variant"] in (0, 1), where
                assert op["size"] in sw.SIZES and op["shrink"] in (1, 2) and op["aspect"] in sw.ASPECTS, where
                assert not (op["size"][0] % op["shrink"] or op["size"][1] % op["shrink"]), where
                assert op["colour"] in ("frame", None) and op["modulate"] in (True, False), where
                assert op["stream"] in (0, 1) and op["defer"] in (True, False), where
                if state.n > 1024:
                    assert op["rays"] <= 2 and op["bounces"] <= 2, where
            elif k == "refused":
                refused += 1
                assert 1 <= op["depth"] <= 3, where
                if op["why"] == "scope":
                    assert state.scope == "spheres" and (state.planes or state.cubes or state.mesh), where
                    assert op["request"] == {}, where
                else:
                    assert op["why"] == "samples" and state.samples == "one" and state.reflect_ok(), where
                    r = op["request"]
                    assert r.get("spp", 1) > 1 or r.get("sample_base", 0) != 0 or r.get("sample_total", 0) > 1 \
                        or r.get("accumulate"), where
            elif k == "render":
                assert (op["depth"] == 0 or state.reflect_ok()) and op["size"] in sw.SIZES, where
                if op["depth"] and (op["spp"] > 1 or op["sample_total"] or op["split"]):
                    assert state.samples == "many", where
                if op["aov"]:
                    assert op["spp"] == 1 and not op["sample_total"] and not op["split"], where
            elif k == "pass":
                if op["what"] == "render_upscaled" or op.get("depth"):
                    assert state.reflect_ok(), where
            elif k == "temporal" and op["mutation"] is not None:
                after = sw.apply(state, op["mutation"])
                assert (after.n, after.n_cubes) == (state.n, state.n_cubes) and after != state, where
            elif k in ("plane_materials", "cube_materials") and op["seed"] is not None:
                assert (state.n_planes if k == "plane_materials" else state.n_cubes) > 0, where
            elif k == "materials" and op["mats"] is not None:
                assert state.n > 0, where
            elif k == "spheres":
                assert op["spheres"][0] in sw.SPHERE_COUNTS, where
            state = sw.apply(state, op)
            # a table never outlives its list, nor has another length than it
            for kind in sw.ROUGH_KINDS:
                assert getattr(state, "rough_" + kind) is None or state.count_of(kind) > 0, where
        assert 4 * refused <= outputs, (seed, refused, outputs)
        refused_all += refused
    assert refused_all >= 1


def test_roughness_seed_and_model_follow_the_header():
    """rt_engine.h, "Glossy reflections": a table follows its kind's k table -- it survives the list set with the same
    count and is cleared by a different count; the material entries do not touch it. The gloss seed and the glass
    model ("Fresnel glass") survive everything."""
    s = sw.State(spheres=(64, 1, 0.0), planes=(2, 0), cubes=(5, 0), gloss_seed=5, glass_model="fresnel")
    assert s.rough() == ()
    for kind, seed in (("spheres", 3), ("planes", 4), ("cubes", 6)):
        s = sw.apply(s, {"op": "roughness", "kind": kind, "how": "set", "seed": seed})
    assert (s.rough_spheres, s.rough_planes, s.rough_cubes) == (3, 4, 6) and s.rough() == sw.ROUGH_KINDS
    tables = lambda st: (st.rough_spheres, st.rough_planes, st.rough_cubes)
    # the same count keeps the kind's table, another count clears that table only, and it does not come back
    for kind, same, other, at in (("spheres", (64, 2, 0.5), (65, 1, 0.0), 0), ("planes", (2, 1), (1, 0), 1),
                                  ("cubes", (5, 1), (4, 1), 2)):
        kept = sw.apply(s, {"op": kind, kind: same})
        assert tables(kept) == (3, 4, 6), kind
        gone = sw.apply(kept, {"op": kind, kind: other})
        assert tables(gone) == tuple(None if i == at else v for i, v in enumerate((3, 4, 6))), kind
        back = sw.apply(gone, {"op": kind, kind: same})
        assert tables(back) == tables(gone), kind
        if kind != "spheres":                                      # the list removed: another count
            assert tables(sw.apply(s, {"op": kind, kind: None}))[at] is None
    assert sw.apply(s, {"op": "planes", "planes": True}).rough_planes == 4      # the first vocabulary's "on": 2 planes
    # the k tables go with their lists as before, and with the roughness: one count change clears both
    m = sw.apply(sw.apply(s, {"op": "materials", "mats": ("ex", 3)}), {"op": "cube_materials", "seed": 4})
    gone = sw.apply(m, {"op": "spheres", "spheres": (63, 1, 0.0)})
    assert (gone.mats, gone.rough_spheres, gone.cube_mats, gone.rough_cubes) == (None, None, 4, 6)
    again = sw.apply(gone, {"op": "materials", "mats": ("ex", 3)})
    assert again.rough_spheres is None                              # the materials set again: the roughness stays cleared
    # the material entries do not touch a table; clearing one table leaves the others
    for op in ({"op": "materials", "mats": ("k", 9)}, {"op": "materials", "mats": ("ex", 9)}, {"op": "materials", "mats": None},
               {"op": "plane_materials", "seed": 2}, {"op": "plane_materials", "seed": None},
               {"op": "cube_materials", "seed": 2}, {"op": "cube_materials", "seed": None}):
        assert tables(sw.apply(m, op)) == (3, 4, 6), op
    assert tables(sw.apply(s, {"op": "roughness", "kind": "planes", "how": "clear", "seed": None})) == (3, None, 6)
    # the seed and the model survive every other op, outputs included
    ops = [{"op": "spheres", "spheres": (8, 2, 0.0)}, {"op": "planes", "planes": None}, {"op": "cubes", "cubes": (4, 0)},
           {"op": "mesh", "mesh": 2}, {"op": "materials", "mats": ("ex", 2)}, {"op": "materials", "mats": None},
           {"op": "lights", "lights": sw.DEFAULT_LIGHTS[:1]}, {"op": "texture", "texture": 1},
           {"op": "cube_materials", "seed": 3}, {"op": "plane_materials", "seed": None}, {"op": "tile_order", "tile_order": 0},
           {"op": "scope", "scope": "scene"}, {"op": "samples", "samples": "many"}, {"op": "view_lists", "view_lists": 0},
           {"op": "roughness", "kind": "cubes", "how": "set", "seed": 8},
           {"op": "roughness", "kind": "spheres", "how": "clear", "seed": None},
           {"op": "temporal", "mutation": {"op": "spheres", "spheres": (8, 2, 0.25)}}, {"op": "gather"}, {"op": "render"}]
    t = s
    for op in ops:
        t = sw.apply(t, op)
        assert (t.gloss_seed, t.glass_model) == (5, "fresnel"), op
    assert sw.apply(t, {"op": "gloss_seed", "gloss_seed": 0xffffffff}).gloss_seed == 0xffffffff
    u = sw.apply(t, {"op": "glass_model", "glass_model": "plain"})
    assert (u.glass_model, u.gloss_seed) == ("plain", 5)
    # the defaults leave a state of the first two vocabularies what it was
    assert sw.State() == sw.State(rough_spheres=None, rough_planes=None, rough_cubes=None, gloss_seed=0, glass_model="plain")
    # the helper: float32 out of ROUGHNESS, some primitives sharp and some rough
    rho = sw.roughness(3, 64)
    assert rho.dtype == np.float32 and (rho == 0).any() and (rho > 0).any() and rho.max() <= 1


def test_gather_scratch_is_the_headers():
    """rt_engine.h: variant 0 takes 256 bytes per pixel at four rays (576 with bounces > 1), 16 more per pixel with
    more than 4 rays; the yardstick variant none."""
    op = dict(size=(64, 36), shrink=1, rays=4, bounces=1, variant=0)
    bytes_of = lambda need: 16 * (need[0] + need[1] + need[2] + need[3])
    assert bytes_of(sw.gather_scratch(op)) == 256 * 64 * 36
    assert bytes_of(sw.gather_scratch(dict(op, bounces=3))) == 576 * 64 * 36
    assert bytes_of(sw.gather_scratch(dict(op, rays=9))) == (256 + 16) * 64 * 36
    assert bytes_of(sw.gather_scratch(dict(op, rays=2, shrink=2))) == 128 * 32 * 18
    assert sw.gather_scratch(dict(op, variant=1)) is None
