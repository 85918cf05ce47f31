"""A long-lived scene against fresh ones, third part (the first two: tests/test_scene_state_gpu.py and
tests/test_scene_state2_gpu.py): the state that came after the second suite. The three roughness tables, the gloss seed
and the glass model through the switches that reflective frames go through, and the two gather passes
(rt_scene_indirect, rt_scene_indirect_paths) as readers of nearly everything a scene caches: the sphere BVH they share
with queries and reflective frames, the tables rt_scene_sync_aux hands over after a change of lights, texture, planes,
cubes or mesh, ray tables of their own keyed on width, height and aspect, and four scratch buffers with a second queue
that only bounces > 1 needs. Scripted transitions first, then seeded random walks of the third vocabulary of
tests/scene_walk.py on two streams with deferred comparison. Everything is compared bit for bit with fresh scenes built
from the current state alone; what the passes compute is checked against restatements in tests/test_indirect_gpu.py,
tests/test_indirect_paths_gpu.py, tests/test_gloss_gpu.py and tests/test_fresnel_gpu.py."""
import numpy as np
import pytest

import scene_walk as sw
import test_scene_state_gpu as B
import test_scene_state2_gpu as S2
from scene_walk import State
from test_scene_state2_gpu import _flat, _fresh, _render, _render_check, _same

pytestmark = pytest.mark.gpu

W, H = 48, 27


# ------------------------------------------------------------------------------------------------ the gather step
def _gather(entry="indirect", size=(W, H), **kw):
    """A "gather" op of tests/scene_walk.py with the scripted tests' defaults."""
    op = dict(op="gather", entry=entry, bounces=1, rays=2, ray_base=0, seed=11, strength=1.0, cull=1, variant=0, size=size,
              shrink=1, cam=0, aspect=None, colour="frame", modulate=True, stream=0, defer=False)
    op.update(kw)
    assert op["entry"] == "paths" or op["bounces"] == 1
    return op


def _call(rt, scene, op, frame, st):
    """The gather of `op` over the guides of `frame`, enqueued on `st`."""
    kw = dict(cam=sw.camera(rt, op["cam"]), aspect=op["aspect"], colour=op["colour"], rays=op["rays"],
              ray_base=op["ray_base"], seed=op["seed"], strength=op["strength"], modulate=op["modulate"],
              cull=bool(op["cull"]), variant=op["variant"], want_packed=True, stream=st)
    if op["entry"] == "indirect":
        return scene.indirect(frame, **kw)
    return scene.indirect_paths(frame, bounces=op["bounces"], **kw)


def _run_gather(rt, scene, op, st):
    """One "gather" step on `scene`, every call enqueued on `st` without a wait: the guide frame (reflect_depth 0, all
    four G-buffer outputs) at size // shrink, the pass over it, and with shrink 2 a full-size frame onto which upsample
    lifts the result."""
    import torch
    (w, h), s, cam, asp = op["size"], op["shrink"], sw.camera(rt, op["cam"]), op["aspect"]
    with torch.cuda.stream(st):
        guide = scene.render(w // s, h // s, cam=cam, aspect=asp, aov=sw.AOV, stream=st)
        res = {"guide": guide, "out": _call(rt, scene, op, guide, st)}
        if s > 1:
            res["hi"] = scene.render(w, h, cam=cam, aspect=asp, aov=sw.AOV, stream=st)
            res["up"] = scene.upsample(res["hi"], guide, colour=res["out"]["rgba"], base=True, demodulate=True, stream=st)
    return res


def _counts(scene):
    """The queue lengths of the scene's last gather (wait for it): rt_scene_indirect's, rt_scene_indirect_paths'."""
    return scene.indirect_counts(), scene.indirect_path_counts()


def _same_gather(got, want, where):
    """The guides first: a difference there is the frame's, not the pass's."""
    import torch
    torch.cuda.synchronize()                     # (the copies to the host run on the current stream, the work on either)
    g = _flat(got)
    guides = lambda d: {k: v for k, v in d.items() if k.startswith(("guide.", "hi."))}
    _same(guides(g), guides(want), where + ": the guide frames")
    _same(g, want, where)


def _walk_gather(rt, scene, state, op, streams, pending, where):
    import torch
    want, counts = _fresh(rt, state, lambda s: _run_gather(rt, s, op, torch.cuda.current_stream()), extra=_counts)
    st = streams[op["stream"]]
    st.wait_stream(torch.cuda.current_stream())
    got = _run_gather(rt, scene, op, st)
    if op["defer"]:                              # compared after the next step has run
        pending.append((where, got, want))
        return
    _same_gather(got, want, where)
    if not op["variant"]:
        assert _counts(scene) == counts, where + ": the gather's queue lengths"


# ------------------------------------------------------------------------------------------------ after a change
def test_gather_after_every_kind_of_change(rt, gpu):
    """64 spheres, the mixed scene's planes and cubes and the small mesh. Every kind of change the gather's host path
    reads through rt_scene_sync_aux or the shared BVH -- a light moved, a light removed, the texture, the planes moved
    and one fewer, a cube moved and one fewer, the mesh elsewhere and gone, the spheres moved, 65, 63, 9000 and 64
    again -- is followed at once by indirect(rays=2) and indirect_paths(bounces=3, rays=5), both variants, cull 1 and
    0 (the one that comes first rotates); every result equals a fresh scene's and differs from the one before the
    change."""
    import torch
    st = State(spheres=(64, 1, 0.0), planes=(2, 0), cubes=(5, 0), mesh=1)
    scene = sw.fresh_scene(rt, st)
    L = [list(l) for l in sw.DEFAULT_LIGHTS]
    moved = [list(l) for l in L]
    moved[0][0:3] = [25.0, 18.0, 12.0]
    as_lights = lambda ls: tuple(tuple(float(v) for v in l) for l in ls)
    changes = [{"op": "lights", "lights": as_lights(moved)}, {"op": "lights", "lights": as_lights(moved[:2])},
               {"op": "texture", "texture": 1}, {"op": "planes", "planes": (2, 1)}, {"op": "planes", "planes": (1, 1)},
               {"op": "cubes", "cubes": (5, 1)}, {"op": "cubes", "cubes": (4, 1)}, {"op": "mesh", "mesh": 2},
               {"op": "mesh", "mesh": 0}, {"op": "spheres", "spheres": (64, 1, 0.5)}, {"op": "spheres", "spheres": (65, 2, 0.0)},
               {"op": "spheres", "spheres": (63, 3, 0.0)}, {"op": "spheres", "spheres": (9000, 4, 0.0)},
               {"op": "spheres", "spheres": (64, 1, 0.0)}]

    def ops_of(state):
        big = state.n > 1024
        two = [_gather("indirect", rays=1 if big else 2), _gather("paths", bounces=2 if big else 3, rays=1 if big else 5)]
        return [dict(op, variant=v, cull=c) for v in (0, 1) for c in (1, 0) for op in two]

    def run(s, ops):
        return {str(i): _run_gather(rt, s, op, torch.cuda.current_stream()) for i, op in ops}

    try:
        before = None
        for n, change in enumerate([None] + changes):
            if change is not None:
                st = B._set(rt, scene, st, change)
            ops = list(enumerate(ops_of(st)))
            ops = ops[n % len(ops):] + ops[:n % len(ops)]          # another one is the first output after the change
            where = "after %s, first %s" % (change, ops[0][1])
            got = run(scene, ops)
            want = _fresh(rt, st, lambda s: run(s, ops))
            _same(got, want, where)
            for i, op in ops:                                      # both variants and both culls: one result
                for k in ("rgba", "packed"):
                    assert np.array_equal(want["%d.out.%s" % (i, k)], want["%d.out.%s" % (i & 1, k)]), (where, i, k)
            if before is not None:                                 # (to and from 9000 spheres the description changes too:
                key = "out" if before[1] == (st.n > 1024) else "guide"   # there the guide frame shows the change)
                for i, op in ops:
                    assert not np.array_equal(want["%d.%s.rgba" % (i, key)], before[0]["%d.%s.rgba" % (i, key)]), where + ": nothing changed"
            before = (want, st.n > 1024)
    finally:
        torch.cuda.synchronize()
        scene.close()


def test_what_the_gather_does_not_read(rt, gpu):
    """rt_engine.h: a gather ray meets mirrors and glass as diffuse surfaces and draws from the description's own seed.
    With one set of guides rendered up front, the sphere, plane and cube materials set and cleared, the three roughness
    tables, the gloss seed, the glass model, the reflect scope, the sampling mode, the view lists and the tile order
    leave the bits of both entries' outputs what they were."""
    import torch
    st = State(spheres=(64, 1, 0.0), planes=(2, 0), cubes=(5, 0))
    scene = sw.fresh_scene(rt, st)
    ops = [_gather("indirect", rays=2), _gather("paths", bounces=3, rays=5), _gather("paths", bounces=2, rays=2, variant=1)]
    steps = [{"op": "materials", "mats": ("k", 5)}, {"op": "materials", "mats": ("ex", 5)},
             {"op": "plane_materials", "seed": 7}, {"op": "cube_materials", "seed": 4},
             {"op": "roughness", "kind": "spheres", "seed": 3}, {"op": "roughness", "kind": "planes", "seed": 4},
             {"op": "roughness", "kind": "cubes", "seed": 6}, {"op": "gloss_seed", "gloss_seed": 5},
             {"op": "glass_model", "glass_model": "fresnel"}, {"op": "scope", "scope": "scene"},
             {"op": "samples", "samples": "many"}, {"op": "view_lists", "view_lists": 0}, {"op": "tile_order", "tile_order": 0},
             {"op": "materials", "mats": None}, {"op": "plane_materials", "seed": None}, {"op": "cube_materials", "seed": None},
             {"op": "roughness", "kind": "spheres", "seed": None}, {"op": "roughness", "kind": "planes", "seed": None},
             {"op": "roughness", "kind": "cubes", "seed": None}, {"op": "gloss_seed", "gloss_seed": 0},
             {"op": "glass_model", "glass_model": "plain"}, {"op": "scope", "scope": "spheres"},
             {"op": "samples", "samples": "one"}, {"op": "view_lists", "view_lists": 1}, {"op": "tile_order", "tile_order": 1}]
    try:
        guide = scene.render(W, H, cam=sw.camera(rt, 0), aov=sw.AOV)
        run = lambda: _flat({str(i): _call(rt, scene, op, guide, torch.cuda.current_stream()) for i, op in enumerate(ops)})
        first = run()
        torch.cuda.synchronize()
        lit = first["0.rgba"].view(np.float32)
        assert (lit[..., :3] > guide["rgba"].cpu().numpy()[..., :3]).any()         # the pass added light
        for step in steps:
            st = B._set(rt, scene, st, step)
            _same(run(), first, "after %s" % step)
            if step["op"] == "scope" and step["scope"] == "scene":                  # the tables are live: a frame shows them
                a = _render(rt, scene, W, H, depth=2)
                b = _render(rt, scene, W, H, depth=0)
                torch.cuda.synchronize()
                assert not torch.equal(a["rgba"], b["rgba"])
        assert st == State(spheres=(64, 1, 0.0), planes=(2, 0), cubes=(5, 0))
    finally:
        torch.cuda.synchronize()
        scene.close()


# ------------------------------------------------------------------------------------------------ the shared BVH
@pytest.mark.parametrize("first", ["gather", "query", "render"])
def test_the_shared_bvh_has_three_first_users(rt, gpu, first):
    """After a same-count move of the spheres the BVH that gathers, queries and reflective frames share is stale, and
    whoever comes first with cull != 0 refreshes it: in turn a gather, trace_rays("nearest") and a frame with mirrors at
    depth 2, the other two following on the other stream. All three outputs equal a fresh scene's, twice over (the
    second move finds a BVH that this order's first user built)."""
    import torch
    st = State(spheres=(64, 1, 0.0), mats=("k", 5))
    scene = sw.fresh_scene(rt, st)
    side = torch.cuda.Stream()
    rays = torch.from_numpy(B._random_rays(7, 1024)).cuda()
    op = _gather("paths", bounces=2, rays=5)
    users = {"gather": lambda s, stream: _run_gather(rt, s, op, stream),
             "query": lambda s, stream: s.trace_rays(rays, "nearest", cull=True, stream=stream),
             "render": lambda s, stream: _render(rt, s, W, H, depth=2, stream=stream)}
    order = [first] + [u for u in users if u != first]
    try:
        _render_check(rt, scene, st, W, H, "start", depth=2)                        # the BVH exists
        for shift in (0.5, -0.25):
            st = B._set(rt, scene, st, {"op": "spheres", "spheres": (64, 1, shift)})
            want = _fresh(rt, st, lambda s: {u: users[u](s, torch.cuda.current_stream()) for u in order})
            got = {}
            for i, u in enumerate(order):
                stream = side if i else torch.cuda.current_stream()
                if i == 1:
                    side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    got[u] = users[u](scene, stream)
            _same(got, want, "%s first, spheres at %s" % (first, shift))
            assert (want["query.kind"] == rt.RT_HIT_SPHERE).any()                   # some rays hit a sphere
    finally:
        torch.cuda.synchronize()
        scene.close()


# ------------------------------------------------------------------------------------------------ the scratch
def test_gather_scratch_through_sizes_bounces_and_streams(rt, gpu):
    """One scene, two streams, nothing waited for until the end. 40 x 90 one bounce; 96 x 54 four bounces with 9 rays
    (every buffer grows, the second queue and the running sum appear); 64 x 36 one bounce (all of them larger than
    needed); the same with another aspect (the pass's own ray tables) and a set_lights directly behind it; 96 x 54 two
    bounces by the yardstick variant; 72 x 72 three bounces. A denoise, a temporal and an upsample call run on the other
    stream in between. Every output equals a fresh scene's."""
    import torch
    st = State(spheres=(64, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    gathers = [_gather("indirect", size=(40, 90), rays=4), _gather("paths", size=(96, 54), bounces=4, rays=9, cam=1),
               _gather("indirect", size=(64, 36), rays=2, cam=2), _gather("paths", size=(64, 36), bounces=1, rays=2, cam=2, aspect=0.75),
               _gather("paths", size=(96, 54), bounces=2, rays=5, variant=1, cam=3), _gather("paths", size=(72, 72), bounces=3, rays=5, cam=4)]
    between = [S2._pass_op("denoise", (64, 36), cam=1), None,
               dict(op="temporal", form="camera", cams=(0, 3), size=(72, 72), aspect=None, variant=0, mutation=None), None,
               S2._pass_op("upsample", (96, 54), cam=2, factor=2, depth=0), None]
    L = [list(l) for l in sw.DEFAULT_LIGHTS]
    L[0][0:3] = [25.0, 18.0, 12.0]
    lights = {"op": "lights", "lights": tuple(tuple(l) for l in L)}
    st2 = sw.apply(st, lights)

    def other(s, op, stream):
        if op["op"] == "pass":
            return S2._run_pass(rt, s, op, stream)
        return S2._run_temporal(rt, op, s, s, stream)

    try:
        wants = []
        for i, (g, b) in enumerate(zip(gathers, between)):
            state = st if i < 4 else st2
            cur = torch.cuda.current_stream()
            wants.append((_fresh(rt, state, lambda s: _run_gather(rt, s, g, cur), extra=_counts),
                          None if b is None else _fresh(rt, state, lambda s: other(s, b, cur))))
        streams[1].wait_stream(streams[0])
        outs = []
        for i, (g, b) in enumerate(zip(gathers, between)):
            got = _run_gather(rt, scene, g, streams[i & 1])
            if i == 3:
                sw.apply_to_scene(rt, scene, lights, st)             # directly behind the un-waited call
            outs.append((got, None if b is None else other(scene, b, streams[1 - (i & 1)])))
        for i, ((got, got_b), ((want, _), want_b)) in enumerate(zip(outs, wants)):
            _same_gather(got, want, "gather %d: %s" % (i, gathers[i]))
            if want_b is not None:
                _same(got_b, want_b, "the pass beside gather %d: %s" % (i, between[i]))
        assert not np.array_equal(wants[2][0][0]["out.rgba"], wants[3][0][0]["out.rgba"])    # the aspect shows
        assert _counts(scene) == wants[5][0][1] and len(wants[5][0][1][1]) == 2          # the last call's queues: two groups
    finally:
        torch.cuda.synchronize()
        scene.close()


# ------------------------------------------------------------------------------------------------ rough and Fresnel frames
def test_rough_and_fresnel_frames_through_the_switches(rt, gpu):
    """Planes and cubes with materials and roughness, spheres with mirrors and glass, about half of them rough. Frames
    at depth 3 equal fresh scenes' through: the scope (spheres: refused, nothing written; scene); one sample, spp 5 and
    a split accumulate under "many", and back; the glass model; the gloss seed; a sphere count change that clears
    materials and roughness together, then the materials alone set again (the roughness stays cleared), then the
    roughness; render_upscaled and a temporal step in the rough Fresnel state."""
    import torch
    st = State(spheres=(64, 1, 0.0), planes=(2, 0), cubes=(5, 0), mats=("ex", 5), plane_mats=S2.ALL_MIRRORS["planes"],
               cube_mats=S2.ALL_MIRRORS["cubes"], rough_spheres=3, rough_planes=4, rough_cubes=6)
    rho = sw.roughness(3, 64)
    k, tau, _ = sw.material_arrays("ex", 5, 64)
    assert 0.3 < (rho > 0).mean() < 0.8 and ((rho > 0) & (k > 0)).any() and ((rho > 0) & (tau > 0)).any()
    assert (sw.roughness(4, 2) > 0).any() and (sw.roughness(6, 5) > 0).any()
    scene = sw.fresh_scene(rt, st)
    frames = {}

    def frame(name, **kw):
        frames[name] = _render_check(rt, scene, st, W, H, name, depth=3, **kw)["rgba"]
        return frames[name]

    def differ(a, b):
        assert not np.array_equal(frames[a], frames[b]), "%s and %s are the same frame" % (a, b)

    try:
        assert S2._refused(rt, scene, W, H, reflect_depth=3) == (2, True)            # the spheres scope: other primitives
        st = B._set(rt, scene, st, {"op": "scope", "scope": "scene"})
        frame("scene scope")
        st = B._set(rt, scene, st, {"op": "scope", "scope": "spheres"})
        assert S2._refused(rt, scene, W, H, reflect_depth=3) == (2, True)
        _render_check(rt, scene, st, W, H, "plain frame under the spheres scope")
        st = B._set(rt, scene, st, {"op": "scope", "scope": "scene"})
        assert np.array_equal(frame("scene scope again"), frames["scene scope"])
        # the rough tables show: the same state without them is another frame
        sharp = _fresh(rt, sw.replace(st, rough_spheres=None, rough_planes=None, rough_cubes=None),
                       lambda s: _render(rt, s, W, H, depth=3))
        assert not np.array_equal(sharp["rgba"], frames["scene scope"])
        st = B._set(rt, scene, st, {"op": "samples", "samples": "many"})
        frame("many, one sample")
        assert np.array_equal(frames["many, one sample"], frames["scene scope"])
        frame("many, spp 5", spp=5)
        frame("many, 3 + 2 accumulated", spp=5, split=3)
        st = B._set(rt, scene, st, {"op": "samples", "samples": "one"})
        assert S2._refused(rt, scene, W, H, reflect_depth=3, spp=5) == (2, True)
        frame("one again")
        st = B._set(rt, scene, st, {"op": "glass_model", "glass_model": "fresnel"})
        frame("fresnel")
        differ("fresnel", "one again")
        st = B._set(rt, scene, st, {"op": "glass_model", "glass_model": "plain"})
        assert np.array_equal(frame("plain again"), frames["one again"])
        st = B._set(rt, scene, st, {"op": "gloss_seed", "gloss_seed": 5})
        frame("gloss seed 5")
        differ("gloss seed 5", "plain again")
        st = B._set(rt, scene, st, {"op": "glass_model", "glass_model": "fresnel"})
        frame("fresnel, gloss seed 5", cam=1)
        # another count clears the spheres' materials and roughness together; the planes' and cubes' tables stay
        st = B._set(rt, scene, st, {"op": "spheres", "spheres": (65, 1, 0.0)})
        assert (st.mats, st.rough_spheres, st.rough_planes, st.rough_cubes) == (None, None, 4, 6)
        frame("65 spheres: no sphere tables")
        st = B._set(rt, scene, st, {"op": "materials", "mats": ("ex", 5)})
        frame("65 spheres: the materials again, sharp")
        differ("65 spheres: the materials again, sharp", "65 spheres: no sphere tables")
        st = B._set(rt, scene, st, {"op": "roughness", "kind": "spheres", "how": "set", "seed": 3})
        frame("65 spheres: rough again")
        differ("65 spheres: rough again", "65 spheres: the materials again, sharp")
        # the rough Fresnel state through render_upscaled and a temporal step over two cameras
        assert (st.glass_model, st.gloss_seed, st.rough()) == ("fresnel", 5, sw.ROUGH_KINDS)
        up = S2._pass_op("render_upscaled", (W, H + 1), factor=2, depth=3)
        cur = torch.cuda.current_stream()
        want = _fresh(rt, st, lambda s: S2._run_pass(rt, s, up, cur))
        _same(S2._run_pass(rt, scene, up, cur), want, "render_upscaled, rough and Fresnel")
        assert (want["out.source"] == 1).any()
        t = dict(op="temporal", form="camera", cams=(0, 3), size=(W, H), aspect=None, variant=0, mutation=None)
        _same(S2._run_temporal(rt, t, scene, scene, cur), S2._fresh_temporal(rt, t, st), "temporal, rough and Fresnel")
        frame("after the passes")
        assert np.array_equal(frames["after the passes"], frames["65 spheres: rough again"])
    finally:
        torch.cuda.synchronize()
        scene.close()


# ------------------------------------------------------------------------------------------------ random walks
@pytest.mark.parametrize("seed", sw.WALK_SEEDS_3)
def test_random_walk_3(rt, gpu, seed):
    """One scene through a seeded walk of the third vocabulary (sw.WALK_STEPS steps): every output equals a fresh
    scene's. Frames, passes, temporal steps and gathers may go to a second stream and be compared only after the next
    step (often a change) ran; the graph of the first walks is replayed after the new changes as well."""
    import torch
    ops = sw.generate(seed, sw.WALK_STEPS, vocabulary=3)
    st = State()
    scene = sw.fresh_scene(rt, st)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    gf = sw.GRAPH_FRAME
    g = B._Graph(rt, scene, gf["w"], gf["h"], spp=gf["spp"])
    pending = []
    try:
        for i, op in enumerate(ops):
            where = "seed %d step %d %s" % (seed, i, op)
            ready, pending = pending, []
            k = op["op"]
            if k in sw.MUTATIONS_3:
                sw.apply_to_scene(rt, scene, op, st)
            elif k == "render":
                S2._walk_render(rt, scene, st, op, streams, pending, where)
            elif k == "query":
                B._walk_query(rt, scene, st, op, where)
            elif k == "refused":
                S2._walk_refused(rt, scene, st, op, streams, where)
            elif k == "pass":
                S2._walk_pass(rt, scene, st, op, streams, pending, where)
            elif k == "temporal":
                S2._walk_temporal(rt, scene, st, op, streams, pending, where)
            elif k == "gather":
                _walk_gather(rt, scene, st, op, streams, pending, where)
            else:
                assert k == "graph", where
                if op["cam"] is not None:
                    g.set_camera(op["cam"])
                got = g.replay()
                want = g.want(st)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), where + ": graph replay"
            st = sw.apply(st, op)
            torch.cuda.synchronize()
            for w_, got, want in ready:
                _same(got, want, w_ + " (checked after step %d)" % i)
        for w_, got, want in pending:
            _same(got, want, w_)
    finally:
        torch.cuda.synchronize()
        g.destroy()
        scene.close()
