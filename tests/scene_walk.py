"""A long-lived scene as a sequence of operations: a state model of one rt_scene, a builder of a fresh scene for a
state, and a seeded generator of operation sequences that stay within what the library accepts.

tests/test_scene_state_gpu.py walks one scene through such a sequence and compares every output with a fresh scene
built from the walk's current state alone; tests/test_scene_walk_cpu.py checks the generator and the model.

The materials follow DESIGN.md section 6d: one per sphere; rt_scene_set_spheres with the same count keeps them, another
count clears them; the old entry (set_materials) sets every transparency to 0; NULL / 0 clears them."""
import random
from dataclasses import dataclass, replace

import numpy as np

# ------------------------------------------------------------------------------------------------ constants
# camera pool: (org x, y, z, yaw, pitch); more origins than the scene has eye-cone slots (3)
CAMERAS = (
    (4.0, 3.0, 10.0, 180.0, -20.0),      # the reference's default camera
    (1.0, 6.0, 9.0, 140.0, -35.0),
    (6.5, 2.0, 12.0, 200.0, -10.0),
    (3.0, 4.5, 7.5, 170.0, -25.0),
    (5.0, 1.0, 14.0, 185.0, -5.0),
    (2.0, 8.0, 11.0, 160.0, -40.0),
)
SIZES = ((64, 36), (96, 54), (72, 72), (40, 90))
ASPECTS = (None, 0.75, 1.25)            # None: rt_default_aspect()
SPHERE_COUNTS = (0, 8, 63, 64, 65, 256, 1024, 9000)   # 9000: no occluder lists, host-built eye cones
DEFAULT_LIGHTS = ((20.0, 20.0, 20.0, 20.0, 1.0, 0.0, 0.0),
                  (0.0, 20.0, -20.0, 20.0, 0.0, 0.0, 1.0),
                  (0.0, 20.0, 0.0, 20.0, 0.0, 1.0, 0.0))
GRAPH_FRAME = dict(w=64, h=48, spp=2)   # the frame of the walk's graph (captured at the start)
WALK_SEEDS = (1, 2, 97, 13, 22, 29)          # the random walks of tests/test_scene_state_gpu.py
WALK_STEPS = 60

MUTATIONS = ("spheres", "lights", "texture", "planes", "cubes", "mesh", "materials", "tile_order")
OUTPUTS = ("render", "query", "graph")


@dataclass(frozen=True)
class State:
    """What a fresh scene is built from. spheres: (count, seed, shift) -- rt_generate_spheres(count, seed) with `shift`
    added to every centre's y; lights: 7-tuples (pos, size, r, g, b); texture: 0 the stand-in, 1 a darker variant;
    mats: None, or (kind, seed) with kind "k" (old entry: mirrors only) or "ex" (mirrors and glass) -- the arrays are
    material_arrays(kind, seed, count)."""
    spheres: tuple = (256, 1, 0.0)
    lights: tuple = DEFAULT_LIGHTS
    texture: int = 0
    planes: bool = False
    cubes: bool = False
    mesh: bool = False
    mats: tuple = None
    tile_order: int = 1

    @property
    def n(self):
        return self.spheres[0]

    def reflect_ok(self):
        """Reflective frames take spheres only."""
        return not (self.planes or self.cubes or self.mesh)


def material_arrays(kind, seed, n):
    """(k, tau, ior) float32 per sphere: mirrors with k in {0.25, 0.5, 1} on about half the spheres; for "ex" glass
    (tau in {0.5, 0.9, 1}, ior in [1, 2.4]) on about a third of the others. A sphere is a mirror or glass, never both."""
    rng = np.random.default_rng(1000 + seed)
    k = np.where(rng.random(n) < 0.5, rng.choice(np.float32([0.25, 0.5, 1.0]), n), 0).astype(np.float32)
    tau = np.zeros(n, dtype=np.float32)
    ior = np.zeros(n, dtype=np.float32)
    if kind == "ex":
        glass = (k == 0) & (rng.random(n) < 0.35)
        tau[glass] = rng.choice(np.float32([0.5, 0.9, 1.0]), int(glass.sum()))
        ior[glass] = rng.choice(np.float32([1.0, 1.33, 1.5, 2.4]), int(glass.sum()))
    return k, tau, ior


def apply(state, op):
    """The state after a mutation `op` (outputs leave it as it is)."""
    kind = op["op"]
    if kind == "spheres":
        sp = op["spheres"]
        mats = state.mats if sp[0] == state.n else None          # another count clears the materials
        return replace(state, spheres=sp, mats=mats)
    if kind == "lights":
        return replace(state, lights=op["lights"])
    if kind == "texture":
        return replace(state, texture=op["texture"])
    if kind in ("planes", "cubes", "mesh", "tile_order"):
        return replace(state, **{kind: op[kind]})
    if kind == "materials":
        return replace(state, mats=op["mats"])                   # "k" is the old entry: it clears the glass
    return state


# ------------------------------------------------------------------------------------------------ generator
def _lights_op(rng, lights):
    """A light change of one of the kinds the caches key on differently."""
    how = rng.choice(("move", "along_axis", "count", "colour", "same", "origin"))
    L = [list(l) for l in lights]
    i = rng.randrange(len(L))
    if how == "move":
        L[i][0:3] = [round(rng.uniform(-25, 25), 2), round(rng.uniform(5, 30), 2), round(rng.uniform(-25, 25), 2)]
    elif how == "along_axis":
        if L[i][0:3] == [0.0, 0.0, 0.0]:
            L[i][0:3] = [10.0, 15.0, 5.0]
            how = "move"
        else:
            L[i][0:3] = [float(np.float32(v) * np.float32(2.0)) if abs(v) < 200 else v * 0.5 for v in L[i][0:3]]
    elif how == "count":
        if len(L) > 1 and (len(L) == 4 or rng.random() < 0.5):
            del L[i]
        else:
            L.append([round(rng.uniform(-20, 20), 2), round(rng.uniform(5, 25), 2), round(rng.uniform(-20, 20), 2),
                      rng.choice((5.0, 20.0)), round(rng.random(), 3), round(rng.random(), 3), round(rng.random(), 3)])
    elif how == "colour":
        L[i][3] = rng.choice((2.0, 10.0, 20.0, 35.0))
        L[i][4:7] = [round(rng.random(), 3) for _ in range(3)]
    elif how == "origin":
        L[i][0:3] = [0.0, 0.0, 0.0]
    return {"op": "lights", "how": how, "lights": tuple(tuple(float(v) for v in l) for l in L)}


def _spheres_op(rng, state):
    n, seed, shift = state.spheres
    how = rng.choice(("count", "count", "same_count", "same_list"))
    if how == "count" or n == 0:
        m = rng.choice([c for c in SPHERE_COUNTS if c != n])
        return {"op": "spheres", "how": "count", "spheres": (m, rng.randrange(1, 9), 0.0)}
    if how == "same_count":
        return {"op": "spheres", "how": "same_count", "spheres": (n, seed, round(shift + rng.choice((-0.5, 0.25, 1.0)), 2))}
    return {"op": "spheres", "how": "same_list", "spheres": (n, seed, shift)}


def _materials_op(rng, state):
    if state.n == 0 or rng.random() < 0.2:
        return {"op": "materials", "how": "clear", "mats": None}
    kind = rng.choice(("k", "ex", "ex"))
    return {"op": "materials", "how": kind, "mats": (kind, rng.randrange(1, 50))}


def _render_op(rng, state):
    w, h = rng.choice(SIZES)
    band = (0, 0)
    if rng.random() < 0.3:
        y0 = rng.randrange(0, h - 4)
        band = (y0, rng.randrange(y0 + 1, h + 1))
    depth = 0
    if state.reflect_ok() and rng.random() < 0.45:
        depth = rng.randrange(1, 4)
    spp = 1 if depth else rng.choice((1, 1, 2, 4))
    return {"op": "render", "cam": rng.randrange(len(CAMERAS)), "size": (w, h), "aspect": rng.choice(ASPECTS),
            "spp": spp, "cull": int(rng.random() < 0.75), "band": band, "depth": depth,
            "stream": rng.randrange(2), "defer": rng.random() < 0.3}


def _query_op(rng, state):
    w, h = rng.choice(SIZES)
    return {"op": "query", "rays": rng.choice(("primary", "random")), "cam": rng.randrange(len(CAMERAS)),
            "size": (w, h), "aspect": rng.choice(ASPECTS), "cull": int(rng.random() < 0.75),
            "modes": tuple(rng.sample(("nearest", "occluded", "shade"), 3)), "ray_seed": rng.randrange(1 << 30)}


def _graph_op(rng, state):
    return {"op": "graph", "cam": rng.randrange(len(CAMERAS)) if rng.random() < 0.4 else None}


def generate(seed, steps):
    """`steps` operations on one scene that starts as State(). Deterministic per seed."""
    rng = random.Random(seed)
    state = State()
    ops = []
    while len(ops) < steps:
        r = rng.random()
        if r < 0.5:
            kind = rng.choice(("spheres", "spheres", "spheres", "lights", "lights", "lights", "lights", "texture",
                               "planes", "cubes", "mesh", "materials", "materials", "materials", "tile_order"))
            if kind == "spheres":
                op = _spheres_op(rng, state)
            elif kind == "lights":
                op = _lights_op(rng, state.lights)
            elif kind == "texture":
                op = {"op": "texture", "texture": 1 - state.texture}
            elif kind in ("planes", "cubes", "mesh"):
                op = {"op": kind, kind: not getattr(state, kind)}
            elif kind == "materials":
                op = _materials_op(rng, state)
            else:
                op = {"op": "tile_order", "tile_order": 1 - state.tile_order}
            state = apply(state, op)
            ops.append(op)
            # an output right after the change, before any render: graph replays and queries read the scene as is
            if rng.random() < 0.5 and len(ops) < steps:
                ops.append(_graph_op(rng, state) if rng.random() < 0.5 else _query_op(rng, state))
        elif r < 0.82:
            ops.append(_render_op(rng, state))
        elif r < 0.9:
            ops.append(_query_op(rng, state))
        else:
            ops.append(_graph_op(rng, state))
    return ops


def transitions(ops):
    """Labels of what each step exercises (for the coverage test): the set over the whole walk."""
    seen = set()
    state = State()
    prev = None
    for op in ops:
        k = op["op"]
        seen.add(k)
        if k == "spheres":
            n0, m = state.n, op["spheres"][0]
            seen.add("spheres:" + op["how"])
            if m > 8192:
                seen.add("spheres:above_8192")   # no occluder lists, eye cones built on the host
            for t in (64, 65):
                if (n0 < t) != (m < t):
                    seen.add("spheres:cross%d_%s" % (t, "up" if m > n0 else "down"))
            if state.mats is not None:
                seen.add("materials:kept" if m == n0 else "materials:cleared_by_count")
        elif k == "lights":
            seen.add("lights:" + op["how"])
        elif k == "materials":
            seen.add("materials:" + op["how"])
            if op["how"] == "k" and state.mats is not None and state.mats[0] == "ex":
                seen.add("materials:old_entry_clears_glass")
        elif k == "render":
            seen.add("render:depth%d" % op["depth"])
            seen.add("render:spp%d" % op["spp"])
            seen.add("render:cull%d" % op["cull"])
            if op["band"] != (0, 0):
                seen.add("render:band")
            if op["stream"] == 1 and op["defer"]:
                seen.add("render:deferred_second_stream")
            if op["depth"] and state.mats is not None and state.mats[0] == "ex":
                seen.add("render:glass")
        elif k == "graph" and op["cam"] is not None:
            seen.add("graph:set_camera")
        elif k == "query":
            seen.add("query:" + op["rays"])
        if prev is not None and prev["op"] in MUTATIONS and k in ("graph", "query"):
            seen.add("%s_after:%s" % (k, prev["op"]))
        state = apply(state, op)
        prev = op
    return seen


# ------------------------------------------------------------------------------------------------ scene building
_cache = {}


def camera(rt, i):
    x, y, z, yaw, pitch = CAMERAS[i]
    return rt.Camera(rt.Vec3(x, y, z), rt.Vec3(0, 0, 1), 0.0, yaw, pitch)


def sphere_array(rt, spec):
    if ("sph", spec) not in _cache:
        n, seed, shift = spec
        arr = rt.generate_spheres(n, seed)
        if shift:
            for i in range(n):
                arr[i].orgin.y = float(np.float32(arr[i].orgin.y) + np.float32(shift))
        _cache[("sph", spec)] = arr
    return _cache[("sph", spec)]


def light_array(rt, lights):
    arr = (rt.Light * max(len(lights), 1))()
    for i, l in enumerate(lights):
        arr[i] = rt.Light(rt.Vec3(*l[0:3]), *l[3:7])
    return arr


def texture_planes(rt, variant):
    if ("tex", variant) not in _cache:
        planes = rt.synth_texture(0)
        if variant:
            planes = [np.ascontiguousarray(p[::-1] * np.float32(0.5), dtype=np.float32) for p in planes]
        _cache[("tex", variant)] = planes
    return _cache[("tex", variant)]


def sky(rt):
    if "sky" not in _cache:
        _cache["sky"] = (rt.sky_sphere(), rt.synth_texture(1))
    return _cache["sky"]


def planes_cubes(rt):
    if "mixed" not in _cache:
        from scenes import mixed_scene
        inp = mixed_scene(rt)
        _cache["mixed"] = (inp.planes, inp.n_planes, inp.cubes, inp.n_cubes)
    return _cache["mixed"]


def mesh(rt):
    if "mesh" not in _cache:
        from meshes import uv_sphere_obj
        _cache["mesh"] = rt.mesh_from_obj_text(uv_sphere_obj(cx=3.0, cy=1.0, cz=4.0, r=1.2, n_lat=6, n_lon=10))
    return _cache["mesh"]


def set_materials(scene, state_mats, n, old_entry=None):
    """Put `state_mats` on `scene` (None clears). The old entry is used for kind "k" unless `old_entry` says otherwise."""
    if state_mats is None:
        scene.set_materials(None)
        return
    kind, seed = state_mats
    k, tau, ior = material_arrays(kind, seed, n)
    if kind == "k" if old_entry is None else old_entry:
        scene.set_materials(k)
    else:
        scene.set_materials_ex(reflectivity=k, transparency=tau, ior=ior)


def apply_to_scene(rt, scene, op, state):
    """Carry a mutation out on a live scene whose state is `state` (before the op)."""
    k = op["op"]
    if k == "spheres":
        n = op["spheres"][0]
        scene.set_spheres(sphere_array(rt, op["spheres"]), n)
    elif k == "lights":
        scene.set_lights(light_array(rt, op["lights"]), len(op["lights"]))
    elif k == "texture":
        scene.set_texture(texture_planes(rt, op["texture"]))
    elif k == "planes":
        p, n_p, _, _ = planes_cubes(rt)
        scene.set_planes(p, n_p if op["planes"] else 0)
    elif k == "cubes":
        _, _, c, n_c = planes_cubes(rt)
        scene.set_cubes(c, n_c if op["cubes"] else 0)
    elif k == "mesh":
        scene.set_mesh(mesh(rt) if op["mesh"] else None)
    elif k == "materials":
        set_materials(scene, op["mats"], state.n)
    elif k == "tile_order":
        scene.set_tile_order(op["tile_order"])


def fresh_scene(rt, state):
    """A new scene holding `state`, its setters called in one canonical order."""
    s = rt.Scene()
    s.set_spheres(sphere_array(rt, state.spheres), state.n)
    p, n_p, c, n_c = planes_cubes(rt)
    if state.planes:
        s.set_planes(p, n_p)
    if state.cubes:
        s.set_cubes(c, n_c)
    if state.mesh:
        s.set_mesh(mesh(rt))
    s.set_texture(texture_planes(rt, state.texture))
    box, sky_planes = sky(rt)
    s.set_sky(box, sky_planes)
    s.set_lights(light_array(rt, state.lights), len(state.lights))
    if state.mats is not None:
        set_materials(s, state.mats, state.n)
    s.set_tile_order(state.tile_order)
    return s


def oracle_frame(oracle, rt, state, cam, w, h, aspect=None, y0=0, y1=None):
    """The CPU oracle's frame of `state` (no mesh, no materials)."""
    assert not state.mesh and state.mats is None
    p, n_p, c, n_c = planes_cubes(rt)
    box, sky_planes = sky(rt)
    return oracle.render(sphere_array(rt, state.spheres), state.n, texture_planes(rt, state.texture), sky_planes, box,
                         light_array(rt, state.lights), len(state.lights), cam, w, h,
                         rt.default_aspect() if aspect is None else aspect, y0=y0, y1=y1, nthreads=8,
                         cubes=c if state.cubes else None, n_cubes=n_c if state.cubes else 0,
                         planes=p if state.planes else None, n_planes=n_p if state.planes else 0)
