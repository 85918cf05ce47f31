"""A long-lived scene as a sequence of operations: a state model of one rt_scene, a builder of a fresh scene for a
state, and a seeded generator of operation sequences that stay within what the library accepts.

tests/test_scene_state_gpu.py walks one scene through such a sequence and compares every output with a fresh scene
built from the walk's current state alone; tests/test_scene_walk_cpu.py checks the generator and the model.

The materials follow DESIGN.md section 6d: one per sphere; rt_scene_set_spheres with the same count keeps them, another
count clears them; the old entry (set_materials) sets every transparency to 0; NULL / 0 clears them. The plane and cube
materials follow the same rule per list (rt_engine.h: they "survive rt_scene_set_planes / rt_scene_set_cubes with the same
count and are cleared by a different count"); the reflect scope, the sampling mode and the view-list mode are switches
that survive everything.

Two vocabularies: generate(seed, steps) is the first suite's (MUTATIONS, OUTPUTS; its sequences are pinned by digest in
tests/test_scene_walk_cpu.py), generate(seed, steps, vocabulary=2) adds the scope, the sampling mode, the view lists, the
plane and cube materials, plane and cube lists of several counts, G-buffer outputs, supersampled reflective frames,
refused requests, the post passes and temporal accumulation (MUTATIONS_2, OUTPUTS_2; seeds WALK_SEEDS_2).

generate(seed, steps, vocabulary=3) adds what came after that: the three roughness tables (rt_engine.h, "Glossy
reflections": a table follows its kind's k table -- it survives the list set with the same count and is cleared by
another count; the material entries do not touch it), the gloss seed and the glass model ("Fresnel glass"; both survive
everything), and the two gather passes as an output of their own, "gather": rt_scene_indirect / rt_scene_indirect_paths
over guides the scene renders itself, at full or half size, on either stream (MUTATIONS_3, OUTPUTS_3; seeds
WALK_SEEDS_3, which together reach every label of REQUIRED_3). The first two vocabularies' sequences stay what they
were; both are pinned by digest."""
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

# the second vocabulary
WALK_SEEDS_2 = (17, 25, 149, 262, 1103, 1205)    # chosen so that tests/test_scene_walk_cpu.py's conditions hold
MUTATIONS_2 = MUTATIONS + ("scope", "samples", "view_lists", "plane_materials", "cube_materials")
OUTPUTS_2 = OUTPUTS + ("refused", "pass", "temporal")
AOV = ("depth", "normal", "id", "albedo")
GUIDES = ("depth", "normal", "id")
# plane and cube lists (count, variant), derived from scenes.mixed_scene's (2 planes, 5 cubes): variant 0 is the first
# `count` primitives as they are, variant 1 the same with one primitive translated. None: no such primitives.
PLANE_SPECS = ((2, 0), (2, 1), (1, 0), (1, 1))
CUBE_SPECS = ((5, 0), (5, 1), (4, 0), (4, 1))
PLANE_MOVE = (0.0, -0.5, 0.0)            # added to the last plane's point
CUBE_MOVE = (0.25, 0.5, -0.25)           # added to cube 1's centre and bounds
KIND_K = (0.0, 0.25, 0.5, 1.0)

# the third vocabulary
WALK_SEEDS_3 = (700, 1235, 2191, 4727, 6182, 7125)   # every label of REQUIRED_3 is on two of these walks at the least
MUTATIONS_3 = MUTATIONS_2 + ("roughness", "gloss_seed", "glass_model")
OUTPUTS_3 = OUTPUTS_2 + ("gather",)
ROUGHNESS = (0.0, 0.0, 0.2, 0.6, 1.0)    # (two zeros: some primitives of a rough table stay sharp)
ROUGH_KINDS = ("spheres", "planes", "cubes")
GLOSS_SEEDS = (0, 1, 5, 0xffffffff)
GATHER_RAYS = (1, 2, 4, 5, 9)            # groups of 4: one group, a whole group, two groups, three groups
V3_OPS = ("roughness", "gloss_seed", "glass_model", "gather")
# what the third vocabulary's walks must reach over WALK_SEEDS_3 (the labels of _transitions_3)
REQUIRED_3 = frozenset(
    MUTATIONS_3 + OUTPUTS_3
    + tuple("roughness:%s:%s" % (k, how) for k in ("spheres", "planes", "cubes")
            for how in ("set", "clear", "kept", "cleared_by_count"))
    + ("gloss_seed", "glass_model:to_fresnel", "glass_model:to_plain",
       "render:glossy", "render:glossy_scene_scope", "render:glossy_many", "render:fresnel", "render:frosted",
       "pass:render_upscaled_glossy", "temporal:glossy",
       "gather:indirect", "gather:paths1", "gather:paths2", "gather:paths3", "gather:paths4",
       "gather:two_groups", "gather:three_groups", "gather:variant1", "gather:cull0", "gather:half_size",
       "gather:mesh", "gather:above_8192", "gather:grows", "gather:smaller", "gather:second_queue_appears",
       "gather_after:spheres:count", "gather_after:spheres:same_count", "gather_after:lights", "gather_after:texture",
       "gather_after:planes", "gather_after:cubes", "gather_after:mesh",
       "bvh_first_user:gather", "bvh_first_user:query", "bvh_first_user:render",
       "gather_deferred_then_mutation"))


@dataclass(frozen=True)
class State:
    """What a fresh scene is built from. spheres: (count, seed, shift) -- rt_generate_spheres(count, seed) with `shift`
    added to every centre's y; lights: 7-tuples (pos, size, r, g, b); texture: 0 the stand-in, 1 a darker variant;
    mats: None, or (kind, seed) with kind "k" (old entry: mirrors only) or "ex" (mirrors and glass) -- the arrays are
    material_arrays(kind, seed, count). planes / cubes: None (or False), or a spec (count, variant) out of PLANE_SPECS /
    CUBE_SPECS (True, the first vocabulary's "on": the first spec); mesh: 0 (or False) none, 1 (or True) the mesh, 2 the
    same mesh elsewhere; plane_mats / cube_mats: None, or the seed of kind_k(seed, count); rough_spheres / rough_planes / rough_cubes: None, or
    the seed of roughness(seed, count); gloss_seed: rt_scene_set_gloss_seed's; glass_model: "plain" / "fresnel"."""
    spheres: tuple = (256, 1, 0.0)
    lights: tuple = DEFAULT_LIGHTS
    texture: int = 0
    planes: tuple = None
    cubes: tuple = None
    mesh: int = 0
    mats: tuple = None
    tile_order: int = 1
    scope: str = "spheres"               # "spheres" / "scene"
    samples: str = "one"                 # "one" / "many"
    view_lists: int = 1
    plane_mats: int = None
    cube_mats: int = None
    rough_spheres: int = None
    rough_planes: int = None
    rough_cubes: int = None
    gloss_seed: int = 0
    glass_model: str = "plain"

    @property
    def n(self):
        return self.spheres[0]

    @property
    def n_planes(self):
        return spec_of(self.planes, PLANE_SPECS)[0]

    @property
    def n_cubes(self):
        return spec_of(self.cubes, CUBE_SPECS)[0]

    def count_of(self, kind):
        """The length of the list of `kind` (out of ROUGH_KINDS)."""
        return {"spheres": self.n, "planes": self.n_planes, "cubes": self.n_cubes}[kind]

    def rough(self):
        """The kinds that have a roughness table."""
        return tuple(k for k in ROUGH_KINDS if getattr(self, "rough_" + k) is not None)

    def reflect_ok(self):
        """Reflective frames take every primitive under the scene scope, spheres only under the other."""
        return self.scope == "scene" or not (self.planes or self.cubes or self.mesh)


def spec_of(value, specs):
    """(count, variant) of a State's planes / cubes field: the first vocabulary's booleans mean the whole list."""
    if not value:
        return (0, 0)
    return specs[0] if value is True else tuple(value)


def kind_k(seed, n):
    """k per plane or cube, float32, out of KIND_K."""
    return np.random.default_rng(2000 + seed).choice(np.float32(KIND_K), n).astype(np.float32)


def roughness(seed, n):
    """rho per primitive of one kind, float32, out of ROUGHNESS."""
    return np.random.default_rng(3000 + seed).choice(np.float32(ROUGHNESS), n).astype(np.float32)


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
        same = sp[0] == state.n                                  # another count clears the materials and the roughness
        return replace(state, spheres=sp, mats=state.mats if same else None,
                       rough_spheres=state.rough_spheres if same else None)
    if kind == "lights":
        return replace(state, lights=op["lights"])
    if kind == "texture":
        return replace(state, texture=op["texture"])
    if kind in ("planes", "cubes"):
        specs, mats = (PLANE_SPECS, "plane_mats") if kind == "planes" else (CUBE_SPECS, "cube_mats")
        same = spec_of(op[kind], specs)[0] == spec_of(getattr(state, kind), specs)[0]
        rough = "rough_" + kind
        return replace(state, **{kind: op[kind], mats: getattr(state, mats) if same else None,   # as the spheres' tables
                                 rough: getattr(state, rough) if same else None})
    if kind in ("mesh", "tile_order", "scope", "samples", "view_lists", "gloss_seed", "glass_model"):
        return replace(state, **{kind: op[kind]})
    if kind == "materials":
        return replace(state, mats=op["mats"])                   # "k" is the old entry: it clears the glass
    if kind == "plane_materials":
        return replace(state, plane_mats=op["seed"])
    if kind == "cube_materials":
        return replace(state, cube_mats=op["seed"])
    if kind == "roughness":
        return replace(state, **{"rough_" + op["kind"]: op["seed"]})
    if kind == "temporal" and op.get("mutation"):                # the change between the step's two frames
        return apply(state, op["mutation"])
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


def generate(seed, steps, vocabulary=1):
    """`steps` operations on one scene that starts as State(). Deterministic per seed. vocabulary 1: the first suite's
    operations, exactly as they were; 2: those of generate_2; 3: those of generate_3."""
    if vocabulary == 2:
        return generate_2(seed, steps)
    if vocabulary == 3:
        return generate_3(seed, steps)
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


# ------------------------------------------------------------------------------------------------ the second vocabulary
def _kind_list_op(rng, state, kind):
    """planes / cubes: on, off, the same count with one primitive moved, or another count."""
    specs = PLANE_SPECS if kind == "planes" else CUBE_SPECS
    cur = getattr(state, kind)
    if not cur:
        return {"op": kind, "how": "on", kind: rng.choice(specs)}
    count, variant = spec_of(cur, specs)
    how = rng.choice(("off", "same_count_moved", "same_count_moved", "other_count", "other_count"))
    if how == "off":
        return {"op": kind, "how": how, kind: None}
    if how == "same_count_moved":
        return {"op": kind, "how": how, kind: (count, 1 - variant)}
    return {"op": kind, "how": how, kind: rng.choice([s for s in specs if s[0] != count])}


def _kind_materials_op(rng, state, kind):
    n = state.n_planes if kind == "plane_materials" else state.n_cubes
    if n == 0 or rng.random() < 0.2:
        return {"op": kind, "how": "clear", "seed": None}
    return {"op": kind, "how": "set", "seed": rng.randrange(1, 50)}


def _stream_fields(rng):
    return {"stream": rng.randrange(2), "defer": rng.random() < 0.35}


def _render_op_2(rng, state):
    """The first vocabulary's frame plus guides, and under the "many" mode more than one sample of a reflective frame:
    spp 2, 4 or 5 (two groups), a sample range, or two accumulating calls (the first with resolve = -1). Guides go
    with one sample only (rt_engine.h refuses them otherwise)."""
    w, h = rng.choice(SIZES)
    band = (0, 0)
    if rng.random() < 0.3:
        y0 = rng.randrange(0, h - 4)
        band = (y0, rng.randrange(y0 + 1, h + 1))
    depth = rng.randrange(1, 4) if state.reflect_ok() and rng.random() < 0.55 else 0
    spp, base, total, split = 1, 0, 0, None
    if depth and state.samples == "many" and rng.random() < 0.75:
        spp = rng.choice((2, 4, 5))
        how = rng.choice(("plain", "range", "split"))
        if how == "range":
            total = spp + rng.randrange(1, 4)
            base = rng.randrange(0, total - spp + 1)
        elif how == "split":
            split = rng.randrange(1, spp)            # the first call's samples; the second takes the others
    elif not depth:
        spp = rng.choice((1, 1, 2, 4))
    aov = ()
    if spp == 1 and rng.random() < 0.5:
        aov = tuple(a for a in AOV if rng.random() < 0.6)
    op = {"op": "render", "cam": rng.randrange(len(CAMERAS)), "size": (w, h), "aspect": rng.choice(ASPECTS),
          "spp": spp, "cull": int(rng.random() < 0.75), "band": band, "depth": depth, "aov": aov,
          "sample_base": base, "sample_total": total, "split": split}
    op.update(_stream_fields(rng))
    return op


def _refused_op(rng, state):
    """A request rt_engine.h names RT_ERR_UNSUPPORTED for the state, or None if the state allows none: a reflective
    frame over a plane, a cube or a mesh under the spheres scope; under the "one" mode a reflective frame with spp 2, a
    sample range or accumulate."""
    w, h = rng.choice(SIZES)
    op = {"op": "refused", "cam": rng.randrange(len(CAMERAS)), "size": (w, h), "depth": rng.randrange(1, 4),
          "stream": rng.randrange(2)}
    if not state.reflect_ok():
        return dict(op, why="scope", request={})
    if state.samples == "one":
        return dict(op, why="samples", request=rng.choice(({"spp": 2}, {"sample_base": 1, "sample_total": 2},
                                                           {"accumulate": True}, {"spp": 4, "sample_total": 8})))
    return None


def _pass_op(rng, state):
    w, h = rng.choice(SIZES)
    what = rng.choice(("denoise", "vdenoise", "upsample", "upsample", "render_upscaled", "render_upscaled"))
    if what == "render_upscaled" and not state.reflect_ok():
        what = "upsample"
    op = {"op": "pass", "what": what, "cam": rng.randrange(len(CAMERAS)), "size": (w, h), "aspect": rng.choice(ASPECTS),
          "variant": rng.randrange(3 if what in ("denoise", "vdenoise") else 2)}
    if what == "denoise":
        op["shrink"] = rng.choice((1, 1, 2, 3))               # the pass at size // shrink
    elif what == "vdenoise":
        op["history"] = rng.random() < 0.6
        op["shrink"] = rng.choice((1, 2))
    else:
        op["factor"] = rng.choice((2, 3))                     # 2 divides every SIZES entry; 3 does not divide 64 x 36 and 40 x 90
        op["depth"] = rng.randrange(1, 3) if state.reflect_ok() else 0
    op.update(_stream_fields(rng))
    return op


def _temporal_op(rng, state):
    """Two frames from two cameras accumulated one onto the other; or, with a same-count move of the spheres or the
    cubes between the frames, temporal_motion with the history made before the move."""
    w, h = rng.choice(SIZES)
    a, b = rng.sample(range(len(CAMERAS)), 2)                # two views: the history is reprojected
    op = {"op": "temporal", "form": "camera", "cams": (a, b), "size": (w, h),
          "aspect": rng.choice(ASPECTS), "variant": rng.randrange(2), "mutation": None}
    forms = ["camera"]
    if 0 < state.n <= 1024:
        forms.append("motion_spheres")
    if state.cubes:
        forms.append("motion_cubes")
    form = rng.choice(forms)
    if form == "motion_spheres":
        n, seed, shift = state.spheres
        op["mutation"] = {"op": "spheres", "how": "same_count", "spheres": (n, seed, round(shift + rng.choice((-0.5, 0.25)), 2))}
    elif form == "motion_cubes":
        count, variant = spec_of(state.cubes, CUBE_SPECS)
        op["mutation"] = {"op": "cubes", "how": "same_count_moved", "cubes": (count, 1 - variant)}
    op["form"] = form
    op.update(_stream_fields(rng))
    return op


def generate_2(seed, steps):
    """`steps` operations of the second vocabulary on one scene that starts as State(). Deterministic per seed."""
    rng = random.Random(1000003 * 2 + seed)
    state = State()
    ops = []
    while len(ops) < steps:
        r = rng.random()
        if r < 0.46:
            kind = rng.choice(("spheres", "spheres", "spheres", "lights", "lights", "texture", "planes", "planes", "cubes",
                               "cubes", "mesh", "materials", "materials", "tile_order", "scope", "scope", "samples",
                               "samples", "view_lists", "view_lists", "plane_materials", "cube_materials", "cube_materials"))
            if kind == "spheres":
                op = _spheres_op(rng, state)
            elif kind == "lights":
                op = _lights_op(rng, state.lights)
            elif kind == "texture":
                op = {"op": "texture", "texture": 1 - state.texture}
            elif kind in ("planes", "cubes"):
                op = _kind_list_op(rng, state, kind)
            elif kind == "mesh":
                op = {"op": "mesh", "mesh": rng.choice([m for m in (0, 1, 2) if m != int(state.mesh)])}
            elif kind == "materials":
                op = _materials_op(rng, state)
            elif kind == "tile_order":
                op = {"op": "tile_order", "tile_order": 1 - state.tile_order}
            elif kind == "scope":
                op = {"op": "scope", "scope": "scene" if state.scope == "spheres" else "spheres"}
            elif kind == "samples":
                op = {"op": "samples", "samples": "many" if state.samples == "one" else "one"}
            elif kind == "view_lists":
                op = {"op": "view_lists", "view_lists": 1 - state.view_lists}
            else:
                op = _kind_materials_op(rng, state, kind)
            state = apply(state, op)
            ops.append(op)
            # an output right after the change, before any render: graph replays and queries read the scene as is
            if rng.random() < 0.45 and len(ops) < steps:
                ops.append(_graph_op(rng, state) if rng.random() < 0.5 else _query_op(rng, state))
        elif r < 0.70:
            ops.append(_render_op_2(rng, state))
        elif r < 0.75:
            ops.append(_query_op(rng, state))
        elif r < 0.81:
            ops.append(_graph_op(rng, state))
        elif r < 0.86:
            op = _refused_op(rng, state)
            if op is not None:
                ops.append(op)
        elif r < 0.95:
            ops.append(_pass_op(rng, state))
        else:
            op = _temporal_op(rng, state)
            state = apply(state, op)
            ops.append(op)
    return ops


# ------------------------------------------------------------------------------------------------ the third vocabulary
def _roughness_op(rng, state):
    """A table of a kind that has primitives set (a new seed) or cleared; None where the scene has no such kind."""
    kinds = [k for k in ROUGH_KINDS if state.count_of(k) > 0]
    if not kinds:
        return None
    kind = rng.choice(kinds)
    cur = getattr(state, "rough_" + kind)
    if cur is not None and rng.random() < 0.3:
        return {"op": "roughness", "kind": kind, "how": "clear", "seed": None}
    return {"op": "roughness", "kind": kind, "how": "set", "seed": rng.choice([s for s in range(1, 50) if s != cur])}


def _gather_op(rng, state):
    """One gather pass over guides the scene renders for it (reflect_depth 0, all four G-buffer outputs): entry
    "indirect", or "paths" with 1 .. 4 bounces (1 issues the other entry's launches). shrink 2: the guides and the pass
    at half the size, the result lifted onto a full-size frame by upsample(base=True, demodulate=True). Above 1024
    spheres at most 2 rays and 2 bounces."""
    w, h = rng.choice(SIZES)
    entry = rng.choice(("indirect", "paths", "paths"))
    bounces = rng.randrange(1, 5) if entry == "paths" else 1
    rays = rng.choice(GATHER_RAYS)
    if state.n > 1024:
        rays, bounces = rng.choice((1, 2)), min(bounces, 2)
    op = {"op": "gather", "entry": entry, "bounces": bounces, "rays": rays, "ray_base": rng.choice((0, 3)),
          "seed": rng.randrange(1 << 32), "strength": rng.choice((0.75, 1.0)), "cull": int(rng.random() < 0.75),
          "variant": int(rng.random() >= 0.75), "size": (w, h), "shrink": rng.choice((1, 1, 2)),
          "cam": rng.randrange(len(CAMERAS)), "aspect": rng.choice(ASPECTS), "colour": rng.choice(("frame", None)),
          "modulate": rng.random() < 0.7}
    op.update(_stream_fields(rng))
    return op


def gather_scratch(op):
    """What a gather asks of the scene's scratch, as rt_scene_indirect / _paths state it: (slots of the slab, float4 of
    the first queue, float4 of the second queue, pixels of the running sum); None for the yardstick variant, which
    takes none."""
    if op["variant"]:
        return None
    w, h = op["size"]
    npx = (w // op["shrink"]) * (h // op["shrink"])
    slots = min(op["rays"], 4) * npx
    paths = op["bounces"] > 1
    q = slots * (4 if paths else 3)
    return (slots, q, q if paths else 0, npx if op["rays"] > 4 else 0)


def generate_3(seed, steps):
    """`steps` operations of the third vocabulary on one scene that starts as State(). Deterministic per seed."""
    rng = random.Random(1000003 * 3 + seed)
    state = State()
    ops = []
    while len(ops) < steps:
        r = rng.random()
        if r < 0.47:
            kind = rng.choice(("spheres", "spheres", "spheres", "lights", "lights", "texture", "planes", "planes", "planes",
                               "cubes", "cubes", "cubes", "mesh", "mesh", "materials", "materials", "materials", "tile_order",
                               "scope", "scope", "scope", "samples", "samples", "view_lists", "plane_materials",
                               "plane_materials", "cube_materials", "cube_materials", "roughness", "roughness", "roughness",
                               "roughness", "roughness", "roughness", "gloss_seed", "glass_model", "glass_model"))
            if kind == "spheres":
                op = _spheres_op(rng, state)
            elif kind == "lights":
                op = _lights_op(rng, state.lights)
            elif kind == "texture":
                op = {"op": "texture", "texture": 1 - state.texture}
            elif kind in ("planes", "cubes"):
                op = _kind_list_op(rng, state, kind)
            elif kind == "mesh":
                op = {"op": "mesh", "mesh": rng.choice([m for m in (0, 1, 2) if m != int(state.mesh)])}
            elif kind == "materials":
                op = _materials_op(rng, state)
            elif kind == "tile_order":
                op = {"op": "tile_order", "tile_order": 1 - state.tile_order}
            elif kind == "scope":
                op = {"op": "scope", "scope": "scene" if state.scope == "spheres" else "spheres"}
            elif kind == "samples":
                op = {"op": "samples", "samples": "many" if state.samples == "one" else "one"}
            elif kind == "view_lists":
                op = {"op": "view_lists", "view_lists": 1 - state.view_lists}
            elif kind == "roughness":
                op = _roughness_op(rng, state)
                if op is None:
                    continue
            elif kind == "gloss_seed":
                op = {"op": "gloss_seed", "gloss_seed": rng.choice([g for g in GLOSS_SEEDS if g != state.gloss_seed])}
            elif kind == "glass_model":
                op = {"op": "glass_model", "glass_model": "fresnel" if state.glass_model == "plain" else "plain"}
            else:
                op = _kind_materials_op(rng, state, kind)
            state = apply(state, op)
            ops.append(op)
            # an output right after the change, before any render: gathers, graph replays and queries read the scene as is
            if rng.random() < 0.5 and len(ops) < steps:
                q = rng.random()
                ops.append(_gather_op(rng, state) if q < 0.6 else _graph_op(rng, state) if q < 0.8 else _query_op(rng, state))
        elif r < 0.67:
            ops.append(_render_op_2(rng, state))
        elif r < 0.70:
            ops.append(_query_op(rng, state))
        elif r < 0.73:
            ops.append(_graph_op(rng, state))
        elif r < 0.76:
            op = _refused_op(rng, state)
            if op is not None:
                ops.append(op)
        elif r < 0.83:
            ops.append(_pass_op(rng, state))
        elif r < 0.87:
            op = _temporal_op(rng, state)
            state = apply(state, op)
            ops.append(op)
        else:
            ops.append(_gather_op(rng, state))
    return ops


def _glossy(mats, rough, n, seeds_k):
    """Whether some primitive of a list of n is a mirror (k > 0) with roughness > 0."""
    if mats is None or rough is None or n == 0:
        return False
    return bool(((seeds_k(mats, n) > 0) & (roughness(rough, n) > 0)).any())


def _sphere_k(mats, n):
    return material_arrays(mats[0], mats[1], n)[0]


def _frame_kinds(state, depth):
    """What a frame of `depth` bounces in `state` exercises of the glossy and Fresnel paths: a set out of "glossy",
    "glossy_scene_scope", "fresnel", "frosted"."""
    out = set()
    if not depth:
        return out
    if _glossy(state.mats, state.rough_spheres, state.n, _sphere_k):
        out.add("glossy")
    if state.scope == "scene" and (_glossy(state.plane_mats, state.rough_planes, state.n_planes, kind_k) or
                                   _glossy(state.cube_mats, state.rough_cubes, state.n_cubes, kind_k)):
        out.add("glossy_scene_scope")
    if state.glass_model == "fresnel" and state.mats is not None and state.mats[0] == "ex" and state.n:
        tau = material_arrays(*state.mats, state.n)[1]
        if (tau > 0).any():
            out.add("fresnel")
            if state.rough_spheres is not None and ((tau > 0) & (roughness(state.rough_spheres, state.n) > 0)).any():
                out.add("frosted")
    return out


def _transitions_3(seen, state, op, prev, track):
    """The third vocabulary's labels of one step. `track` follows the walk: "since" the mutations since the last
    output, "bvh" whether the spheres changed since the shared BVH's last user, "scratch" the largest request per
    scratch buffer so far, "one_bounce" the largest one-bounce request of slots, "second" whether a second queue exists."""
    k = op["op"]
    if k == "roughness":
        seen.add("roughness:%s:%s" % (op["kind"], op["how"]))
    elif k == "gloss_seed":
        seen.add("gloss_seed")
    elif k == "glass_model":
        seen.add("glass_model:to_" + op["glass_model"])
    elif k in ROUGH_KINDS and getattr(state, "rough_" + k) is not None:
        kept = getattr(apply(state, op), "rough_" + k) is not None
        seen.add("roughness:%s:%s" % (k, "kept" if kept else "cleared_by_count"))
    elif k == "render":
        kinds = _frame_kinds(state, op["depth"])
        seen.update("render:" + f for f in kinds)
        if kinds & {"glossy", "glossy_scene_scope"} and op["spp"] > 1 and state.samples == "many":
            seen.add("render:glossy_many")
    elif k == "pass" and op["what"] == "render_upscaled" and state.rough():
        seen.add("pass:render_upscaled_glossy")
    elif k == "temporal" and state.rough():
        seen.add("temporal:glossy")
    elif k == "gather":
        seen.add("gather:indirect" if op["entry"] == "indirect" else "gather:paths%d" % op["bounces"])
        if op["rays"] > 4:
            seen.add("gather:two_groups")
        if op["rays"] > 8:
            seen.add("gather:three_groups")
        if op["variant"]:
            seen.add("gather:variant1")
        if not op["cull"]:
            seen.add("gather:cull0")
        if op["shrink"] == 2:
            seen.add("gather:half_size")
        if state.mesh:
            seen.add("gather:mesh")
        if state.n > 8192:
            seen.add("gather:above_8192")
        need = gather_scratch(op)
        if need is not None:
            have = track.get("scratch")
            if have is not None:
                if any(a > b for a, b in zip(need, have)):
                    seen.add("gather:grows")
                elif need[0] < have[0]:
                    seen.add("gather:smaller")
            if op["bounces"] > 1:
                if not track.get("second") and track.get("one_bounce", 0) >= need[0]:
                    seen.add("gather:second_queue_appears")     # only the second queue is new
                track["second"] = True
            else:
                track["one_bounce"] = max(track.get("one_bounce", 0), need[0])
            track["scratch"] = need if have is None else tuple(max(a, b) for a, b in zip(need, have))
        for m in track.get("since", ()):
            seen.add("gather_after:" + m)
    # the shared sphere BVH: who reads it first after a change of the spheres
    if k == "spheres" and op["how"] != "same_list" or k == "temporal" and op["form"] == "motion_spheres":
        track["bvh"] = True
    elif track.get("bvh") and state.n > 0:
        user = None
        if k == "gather" and op["cull"]:
            user = "gather"
        elif k == "query" and op["cull"]:
            user = "query"
        elif k == "render" and op["depth"] and op["cull"]:
            user = "render"
        elif k == "pass" and op.get("depth"):
            user = "pass"
        if user:
            seen.add("bvh_first_user:" + user)
            track["bvh"] = False
    # the mutations no output has read yet
    if k in MUTATIONS_3:
        since = track.setdefault("since", [])
        name = "spheres:" + op["how"] if k == "spheres" else k
        if name not in since:
            since.append(name)
    else:
        track["since"] = []
    if prev is not None and prev["op"] == "gather" and prev["defer"] and prev["stream"] == 1 and k in MUTATIONS_3:
        seen.add("gather_deferred_then_mutation")


def _transitions_2(seen, state, op, prev, cleared):
    """The second vocabulary's labels of one step; `cleared` is the set of material tables a count change has cleared
    and nothing has set again."""
    k = op["op"]
    if k in ("planes", "cubes") and "how" in op:
        seen.add("%s:%s" % (k, op["how"]))
        table = "plane_mats" if k == "planes" else "cube_mats"
        if getattr(state, table) is not None:
            kept = getattr(apply(state, op), table) is not None
            seen.add("kind_materials:kept" if kept else "kind_materials:cleared_by_count")
            if not kept:
                cleared.add(table)
    elif k == "spheres" and state.mats is not None and op["spheres"][0] != state.n:
        cleared.add("mats")
    elif k in ("materials", "plane_materials", "cube_materials"):
        cleared.discard({"materials": "mats", "plane_materials": "plane_mats", "cube_materials": "cube_mats"}[k])
        if k != "materials":
            seen.add("%s:%s" % (k, op["how"]))
    elif k == "scope":
        seen.add("scope:to_" + op["scope"])
    elif k == "samples":
        seen.add("samples:to_" + op["samples"])
    elif k == "view_lists":
        seen.add("view_lists:" + ("on" if op["view_lists"] else "off"))
    elif k == "render" and "aov" in op:
        if op["depth"] and state.scope == "scene":
            seen.add("render:scene_scope_depth>0")
            if state.mesh:
                seen.add("render:scene_scope_with_mesh")
        if op["depth"] and op["spp"] > 4:
            seen.add("render:many_two_groups")
        if op["split"]:
            seen.add("render:many_accumulate_split")
        if op["sample_total"]:
            seen.add("render:many_sample_range")
        if op["aov"]:
            seen.add("render:aov_reflective" if op["depth"] else "render:aov")
    elif k == "refused":
        seen.add("refused:" + op["why"])
    elif k == "pass":
        what = op["what"]
        if what == "denoise":
            seen.add("pass:denoise")
        elif what == "vdenoise":
            seen.add("pass:vdenoise_history" if op["history"] else "pass:vdenoise")
        elif what == "upsample":
            w, h = op["size"]
            exact = w % op["factor"] == 0 and h % op["factor"] == 0
            seen.add("pass:upsample_exact%d" % op["factor"] if exact else "pass:upsample_other_ratio")
        else:
            seen.add("pass:render_upscaled")
            if cleared:
                seen.add("render_upscaled_after:materials_cleared_by_count")
    elif k == "temporal":
        seen.add("temporal:" + op["form"])
    if prev is not None and prev["op"] in ("pass", "temporal") and prev["defer"] and prev["stream"] == 1 \
            and k in MUTATIONS_2:
        seen.add("pass_deferred_then_mutation")


def transitions(ops):
    """Labels of what each step exercises (for the coverage test): the set over the whole walk."""
    seen = set()
    state = State()
    prev = None
    cleared = set()
    third = any(op["op"] in V3_OPS for op in ops)        # the first two vocabularies' label sets stay what they are
    track = {}
    for op in ops:
        k = op["op"]
        seen.add(k)
        _transitions_2(seen, state, op, prev, cleared)
        if third:
            _transitions_3(seen, state, op, prev, track)
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
        if prev is not None and prev["op"] in MUTATIONS_2 and k in ("graph", "query"):
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


def plane_list(rt, value):
    """(array, count) of a State's planes field."""
    count, variant = spec_of(value, PLANE_SPECS)
    if ("planes", count, variant) not in _cache:
        import ctypes as C
        src = planes_cubes(rt)[0]
        arr = (rt.Plane * max(count, 1))()
        C.memmove(arr, src, C.sizeof(rt.Plane) * count)
        if variant:
            o = arr[count - 1].orgin
            o.x, o.y, o.z = (float(np.float32(v) + np.float32(d)) for v, d in zip((o.x, o.y, o.z), PLANE_MOVE))
        _cache[("planes", count, variant)] = arr
    return _cache[("planes", count, variant)], count


def cube_list(rt, value):
    """(array, count) of a State's cubes field."""
    count, variant = spec_of(value, CUBE_SPECS)
    if ("cubes", count, variant) not in _cache:
        import ctypes as C
        src = planes_cubes(rt)[2]
        arr = (rt.Cube * max(count, 1))()
        C.memmove(arr, src, C.sizeof(rt.Cube) * count)
        if variant:
            for o in (arr[1].orgin, arr[1].bounds[0], arr[1].bounds[1]):
                o.x, o.y, o.z = (float(np.float32(v) + np.float32(d)) for v, d in zip((o.x, o.y, o.z), CUBE_MOVE))
        _cache[("cubes", count, variant)] = arr
    return _cache[("cubes", count, variant)], count


MESH_AT = {1: (3.0, 1.0, 4.0), 2: (5.5, 1.5, 5.0)}


def mesh_text(variant):
    from meshes import uv_sphere_obj
    cx, cy, cz = MESH_AT[int(variant)]
    return uv_sphere_obj(cx=cx, cy=cy, cz=cz, r=1.2, n_lat=6, n_lon=10)


def mesh(rt, variant=1):
    if ("mesh", int(variant)) not in _cache:
        _cache[("mesh", int(variant))] = rt.mesh_from_obj_text(mesh_text(variant))
    return _cache[("mesh", int(variant))]


def origins(rt, state):
    """The sphere centres and each cube's bounds[0] of `state`, float32 [n, 3]: what displacements are formed from."""
    sp = sphere_array(rt, state.spheres)
    cu, n_c = cube_list(rt, state.cubes)
    a = np.array([[sp[i].orgin.x, sp[i].orgin.y, sp[i].orgin.z] for i in range(state.n)], dtype=np.float32).reshape(-1, 3)
    b = np.array([[cu[i].bounds[0].x, cu[i].bounds[0].y, cu[i].bounds[0].z] for i in range(n_c)], dtype=np.float32)
    return a, b.reshape(-1, 3)


def motion_tables(rt, before, after):
    """The displacement tables [n, 4] of the objects between two states of equal counts, binary32 (an empty table
    where nothing moved: nothing is to be inferred)."""
    out = []
    for a, b in zip(origins(rt, before), origins(rt, after)):
        assert a.shape == b.shape
        d = (b - a).astype(np.float32)
        m = np.zeros((a.shape[0] if d.any() else 0, 4), dtype=np.float32)
        if d.any():
            m[:, :3] = d
        out.append(m)
    return out


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


def set_roughness(scene, kind, seed, n):
    """Put roughness(seed, n) on the table of `kind` (out of ROUGH_KINDS) of `scene`; a seed of None clears it."""
    scene.set_roughness(kind[:-1], None if seed is None else roughness(seed, n))


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
        scene.set_planes(*plane_list(rt, op["planes"]))
    elif k == "cubes":
        scene.set_cubes(*cube_list(rt, op["cubes"]))
    elif k == "mesh":
        scene.set_mesh(mesh(rt, op["mesh"]) if op["mesh"] else None)
    elif k == "materials":
        set_materials(scene, op["mats"], state.n)
    elif k == "tile_order":
        scene.set_tile_order(op["tile_order"])
    elif k == "scope":
        scene.set_reflect_scope(op["scope"])
    elif k == "samples":
        scene.set_reflect_samples(op["samples"])
    elif k == "view_lists":
        scene.set_view_lists(op["view_lists"])
    elif k == "plane_materials":
        scene.set_plane_materials(None if op["seed"] is None else kind_k(op["seed"], state.n_planes))
    elif k == "cube_materials":
        scene.set_cube_materials(None if op["seed"] is None else kind_k(op["seed"], state.n_cubes))
    elif k == "roughness":
        set_roughness(scene, op["kind"], op["seed"], state.count_of(op["kind"]))
    elif k == "gloss_seed":
        scene.set_gloss_seed(op["gloss_seed"])
    elif k == "glass_model":
        scene.set_glass_model(op["glass_model"])


def fresh_scene(rt, state):
    """A new scene holding `state`, its setters called in one canonical order."""
    s = rt.Scene()
    s.set_spheres(sphere_array(rt, state.spheres), state.n)
    if state.planes:
        s.set_planes(*plane_list(rt, state.planes))
    if state.cubes:
        s.set_cubes(*cube_list(rt, state.cubes))
    if state.mesh:
        s.set_mesh(mesh(rt, state.mesh))
    s.set_texture(texture_planes(rt, state.texture))
    box, sky_planes = sky(rt)
    s.set_sky(box, sky_planes)
    s.set_lights(light_array(rt, state.lights), len(state.lights))
    if state.mats is not None:
        set_materials(s, state.mats, state.n)
    if state.plane_mats is not None:
        s.set_plane_materials(kind_k(state.plane_mats, state.n_planes))
    if state.cube_mats is not None:
        s.set_cube_materials(kind_k(state.cube_mats, state.n_cubes))
    for kind in state.rough():
        set_roughness(s, kind, getattr(state, "rough_" + kind), state.count_of(kind))
    if state.gloss_seed:
        s.set_gloss_seed(state.gloss_seed)
    if state.glass_model != "plain":
        s.set_glass_model(state.glass_model)
    if state.scope != "spheres":
        s.set_reflect_scope(state.scope)
    if state.samples != "one":
        s.set_reflect_samples(state.samples)
    if not state.view_lists:
        s.set_view_lists(0)
    s.set_tile_order(state.tile_order)
    return s


def oracle_frame(oracle, rt, state, cam, w, h, aspect=None, y0=0, y1=None):
    """The CPU oracle's frame of `state` (no mesh, no materials)."""
    assert not state.mesh and state.mats is None
    p, n_p = plane_list(rt, state.planes)
    c, n_c = cube_list(rt, state.cubes)
    box, sky_planes = sky(rt)
    return oracle.render(sphere_array(rt, state.spheres), state.n, texture_planes(rt, state.texture), sky_planes, box,
                         light_array(rt, state.lights), len(state.lights), cam, w, h,
                         rt.default_aspect() if aspect is None else aspect, y0=y0, y1=y1, nthreads=8,
                         cubes=c if n_c else None, n_cubes=n_c, planes=p if n_p else None, n_planes=n_p)
