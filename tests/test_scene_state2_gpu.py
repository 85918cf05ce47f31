"""A long-lived scene against fresh ones, second part (the first: tests/test_scene_state_gpu.py): the state that came
after the first suite. The reflect scope with the plane and cube material tables, supersampled reflective frames on the
scene-owned scratch, the view-list slots and their switch (also under a recorded graph), G-buffer outputs, the post
passes (the two denoisers' shared scratch, temporal accumulation's raygen table, temporal_motion's host copies, guided
upsampling) and the wrapper's host mirrors that Scene.upsample_select() reads. Targeted transitions first, then seeded
random walks of the second vocabulary of tests/scene_walk.py on two streams, with deferred comparison for frames and
passes alike. Everything is compared bit for bit with fresh scenes built from the current state alone (rgba viewed as
uint32, packed words, guides, moments, variance, `source`, every rt_hit field, reflect queue lengths); each kind of
output has a checkpoint against a composer or a numpy restatement, so that the check is not circular."""
import ctypes as C
import types

import numpy as np
import pytest

import scene_walk as sw
import test_scene_state_gpu as B
from scene_walk import State

pytestmark = pytest.mark.gpu

POISON = 0x5a5a5a5a


# ------------------------------------------------------------------------------------------------ comparing
def _flat(out, prefix=""):
    """Every tensor of a result (nested dicts included) as {name: bits}: float32 viewed as uint32, the rest as is."""
    import torch
    res = {}
    for k, v in out.items():
        if isinstance(v, dict):
            res.update(_flat(v, prefix + k + "."))
        elif torch.is_tensor(v):
            a = v.detach().contiguous().cpu().numpy()
            res[prefix + k] = a.view(np.uint32) if a.dtype == np.float32 else a
    return res


def _same(got, want, where):
    """`got`: a result of the long-lived scene (tensors, waited for here); `want`: _flat() of the fresh scene's."""
    import torch
    torch.cuda.synchronize()
    g = got if not any(torch.is_tensor(v) or isinstance(v, dict) for v in got.values()) else _flat(got)
    assert set(g) == set(want), (where, sorted(g), sorted(want))
    for k in sorted(want):
        assert g[k].shape == want[k].shape, "%s: shape of %s" % (where, k)
        diff = g[k] != want[k]
        assert not diff.any(), "%s differs in %d elements: %s" % (k, int(diff.sum()), where)


def _fresh(rt, state, fn, extra=None):
    """_flat(fn(scene)) of a fresh scene built from `state`; with `extra` the pair of it and extra(scene), which is
    read after the scene's work is done (reflect queue lengths, the wrapper's tables)."""
    import torch
    s = sw.fresh_scene(rt, state)
    try:
        out = fn(s)
        torch.cuda.synchronize()
        return _flat(out) if extra is None else (_flat(out), extra(s))
    finally:
        s.close()


def _queue(scene):
    return scene.reflect_stats()["queue"]


def _fresh_frame(rt, state, w, h, **kw):
    """(the fresh scene's frame, its reflect queue lengths or None): what a frame of the long-lived scene must equal."""
    if kw.get("depth"):
        return _fresh(rt, state, lambda s: _render(rt, s, w, h, **kw), extra=_queue)
    return _fresh(rt, state, lambda s: _render(rt, s, w, h, **kw)), None


def _render(rt, scene, w, h, *, cam=0, aspect=None, spp=1, cull=1, band=(0, 0), depth=0, aov=(), sample_base=0,
            sample_total=0, split=None, stream=None):
    """Enqueue a frame (no wait). `split`: two calls into one pair of buffers, the first with `split` samples and
    resolve = -1, the second accumulating the others."""
    import torch
    c = sw.camera(rt, cam) if isinstance(cam, int) else cam
    st = torch.cuda.current_stream() if stream is None else stream
    common = dict(cam=c, aspect=aspect, cull=bool(cull), reflect_depth=depth)
    with torch.cuda.stream(st):
        if not split:
            return scene.render(w, h, y0=band[0], y1=band[1], spp=spp, sample_base=sample_base, sample_total=sample_total,
                                aov=aov, stream=st, **common)
        rows = (band[1] or h) - band[0]
        packed = torch.full((rows, w), POISON, dtype=torch.int32, device="cuda")
        rgba = torch.full((rows, w, 4), 3.0, dtype=torch.float32, device="cuda")
        for n, base, acc, resolve in ((split, 0, False, -1), (spp - split, split, True, 0)):
            fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), y0=band[0], y1=band[1], spp=n,
                                  sample_base=base, sample_total=spp, accumulate=acc, resolve=resolve, **common)
            scene.render_raw(fd, st.cuda_stream)
        return {"packed": packed, "rgba": rgba}


def _render_check(rt, scene, state, w, h, where, **kw):
    """A frame of the long-lived scene against the fresh scene's; with a reflective frame also the queue lengths."""
    want, queue = _fresh_frame(rt, state, w, h, **kw)
    _same(_render(rt, scene, w, h, **kw), want, where)
    if queue is not None:
        assert _queue(scene) == queue, where + ": reflect queues"
    return want


def _inputs(rt, state, cam=0, aspect=None):
    """`state` as the composers' and restatements' input (tests/scenes.py Inputs, plus planes and cubes)."""
    box, sky = sw.sky(rt)
    inp = types.SimpleNamespace(rt=rt, n=state.n, spheres=sw.sphere_array(rt, state.spheres),
                                tex=sw.texture_planes(rt, state.texture), sky=sky, sky_box=box,
                                lights=sw.light_array(rt, state.lights), n_lights=len(state.lights),
                                cam=sw.camera(rt, cam), aspect=rt.default_aspect() if aspect is None else aspect)
    inp.planes, inp.n_planes = sw.plane_list(rt, state.planes)
    inp.cubes, inp.n_cubes = sw.cube_list(rt, state.cubes)
    return inp


def _scene_mats(state):
    """The composers' material arguments of `state`."""
    k, tau, ior = sw.material_arrays(*state.mats, state.n) if state.mats else (None, None, None)
    return dict(k_sphere=k, tau=tau, ior=ior,
                k_plane=None if state.plane_mats is None else sw.kind_k(state.plane_mats, state.n_planes),
                k_cube=None if state.cube_mats is None else sw.kind_k(state.cube_mats, state.n_cubes))


def _refused(rt, scene, w, h, stream=None, **kw):
    """A request the header refuses with RT_ERR_UNSUPPORTED: the status, and nothing of the poisoned outputs written."""
    import torch
    st = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(st):
        packed = torch.full((h, w), POISON, dtype=torch.int32, device="cuda")
        rgba = torch.full((h, w, 4), POISON, dtype=torch.int32, device="cuda")
    cam = kw.pop("cam", 0)
    fd = scene.frame_desc(w, h, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), cam=sw.camera(rt, cam), **kw)
    rc = scene.lib.rt_scene_render(scene.handle, C.byref(fd), st.cuda_stream)
    torch.cuda.synchronize()
    return rc, bool((packed == POISON).all().item()) and bool((rgba == POISON).all().item())


# ------------------------------------------------------------------------------------------------ the passes
def _run_pass(rt, scene, op, st):
    """One "pass" step on `scene`, every call enqueued on `st` without a wait: the scene renders its own inputs."""
    import torch
    (w, h), cam, asp, what, v = op["size"], sw.camera(rt, op["cam"]), op["aspect"], op["what"], op["variant"]
    with torch.cuda.stream(st):
        if what in ("denoise", "vdenoise"):
            w, h = w // op["shrink"], h // op["shrink"]
            frame = scene.render(w, h, cam=cam, aspect=asp, aov=sw.AOV, stream=st)
            if what == "denoise":
                return {"out": scene.denoise(frame, variant=v, stream=st), "frame": frame}
            hist = None
            if op["history"]:         # the same view twice: every hit pixel's history is two frames long
                hist = scene.temporal(frame, None, cam=cam, aspect=asp, stream=st)
                hist = scene.temporal(scene.render(w, h, cam=cam, aspect=asp, aov=sw.AOV, stream=st), hist, cam=cam,
                                      aspect=asp, stream=st)
            return {"out": scene.denoise_variance(frame, hist, variant=v, stream=st), "frame": frame, "hist": hist or {}}
        f = op["factor"]
        if what == "upsample":
            hi = scene.render(w, h, cam=cam, aspect=asp, aov=sw.AOV, stream=st)
            lo = scene.render(w // f, h // f, cam=cam, aspect=asp, aov=sw.AOV, reflect_depth=op["depth"], stream=st)
            return {"out": scene.upsample(hi, lo, variant=v, stream=st), "hi": hi, "lo": lo}
        return {"out": scene.render_upscaled(w, h, f, reflect_depth=op["depth"], variant=v, want_parts=True, cam=cam,
                                             aspect=asp, stream=st)}


def _run_temporal(rt, op, before, after, st, between=None, tables=None):
    """One "temporal" step: a frame of camera a on scene `before` starts a history, a frame of camera b on scene `after`
    is accumulated onto it. With a mutation in the step `between()` carries it out in between and the calls are
    temporal_motion's: `tables` None lets the scene infer the displacements from the history's host copies."""
    import torch
    (w, h), asp, v = op["size"], op["aspect"], op["variant"]
    a, b = (sw.camera(rt, c) for c in op["cams"])
    with torch.cuda.stream(st):
        f1 = before.render(w, h, cam=a, aspect=asp, aov=sw.GUIDES, stream=st)
        if op["mutation"] is None:
            h1 = before.temporal(f1, None, cam=a, aspect=asp, variant=v, stream=st)
            f2 = after.render(w, h, cam=b, aspect=asp, aov=sw.GUIDES, stream=st)
            h2 = after.temporal(f2, h1, cam=b, aspect=asp, variant=v, stream=st)
            h3 = after.temporal(f2, h2, cam=b, aspect=asp, variant=v, stream=st)      # and again with the returned history
            return {"f1": f1, "h1": h1, "f2": f2, "h2": h2, "h3": h3}
        h1 = before.temporal_motion(f1, None, cam=a, aspect=asp, variant=v, stream=st)
        if between is not None:
            between()
        f2 = after.render(w, h, cam=b, aspect=asp, aov=sw.GUIDES, stream=st)
        kw = {} if tables is None else dict(sphere_motion=tables[0], cube_motion=tables[1])
        h2 = after.temporal_motion(f2, h1, cam=b, aspect=asp, variant=v, stream=st, **kw)
        return {"f1": f1, "h1": h1, "f2": f2, "h2": h2}


def _fresh_temporal(rt, op, state):
    """What _run_temporal gives on fresh scenes of the state before and after the step's mutation, the displacements
    given as the model forms them from the two states."""
    import torch
    after_state = sw.apply(state, op)
    s0 = sw.fresh_scene(rt, state)
    s1 = sw.fresh_scene(rt, after_state) if op["mutation"] else s0
    try:
        tables = sw.motion_tables(rt, state, after_state) if op["mutation"] else None
        out = _run_temporal(rt, op, s0, s1, torch.cuda.current_stream(), tables=tables)
        torch.cuda.synchronize()
        return _flat(out)
    finally:
        s0.close()
        if s1 is not s0:
            s1.close()


# ------------------------------------------------------------------------------------------------ host mirrors
# seeds of sw.kind_k whose every k is > 0 (asserted below): each plane and cube is a mirror
ALL_MIRRORS = {"planes": 7, "cubes": 4}


@pytest.mark.parametrize("kind", ["spheres", "planes", "cubes"])
def test_render_upscaled_after_a_count_change_cleared_the_materials(rt, gpu, kind):
    """Materials, then the list set to another count and back without setting them again: the library has cleared the
    table, so Scene.upsample_select() selects nothing of that kind and render_upscaled's every pixel of it is the
    full-resolution frame's -- as on a fresh scene of the same state. The whole result (rgba, packed, source, both
    frames with their guides) and the tables themselves are compared; the spheres' case also with the restatement."""
    import upsample_ref as U
    W, H = 160, 90
    if kind == "spheres":
        st = State(spheres=(256, 1, 0.0), mats=("ex", 5))
        there, back = {"op": "spheres", "spheres": (1024, 2, 0.0)}, {"op": "spheres", "spheres": (256, 1, 0.0)}
        key = "sphere"
    else:
        st = State(spheres=(256, 1, 0.0), planes=(2, 0), cubes=(5, 0), scope="scene", mats=("k", 5),
                   plane_mats=ALL_MIRRORS["planes"], cube_mats=ALL_MIRRORS["cubes"])
        assert sw.kind_k(st.plane_mats, 2).all() and sw.kind_k(st.cube_mats, 5).all()
        spec = (1, 0) if kind == "planes" else (4, 0)
        there, back = {"op": kind, kind: spec}, {"op": kind, kind: getattr(st, kind)}
        key = kind[:-1]
    scene = sw.fresh_scene(rt, st)
    run = lambda s: s.render_upscaled(W, H, 2, reflect_depth=2, want_parts=True, cam=sw.camera(rt, 0))
    tables = lambda s: s.upsample_select()
    try:
        want, select = _fresh(rt, st, run, extra=tables)
        assert tables(scene) == select and any(select[key])
        _same(run(scene), want, "%s: with materials" % kind)
        with_mats = want
        if kind == "spheres":         # the restatement, with the tables the materials give
            frame = lambda p: dict({k: want["%s.aov.%s" % (p, k)].view(np.float32 if k != "id" else np.int32)
                                    for k in sw.GUIDES}, rgba=want[p + ".rgba"].view(np.float32))
            ref = U.upsample(frame("hi"), frame("lo"), base=frame("hi")["rgba"], select=select, demodulate=False)
            assert np.array_equal(ref["rgba"].view(np.uint32), want["rgba"]) and np.array_equal(ref["packed"], want["packed"].view(np.uint32))
            assert np.array_equal(ref["source"], want["source"]) and (ref["source"] == 1).any()
        st = B._set(rt, scene, st, there)
        st = B._set(rt, scene, st, back)
        assert getattr(st, {"spheres": "mats", "planes": "plane_mats", "cubes": "cube_mats"}[kind]) is None
        want, select = _fresh(rt, st, run, extra=tables)
        assert not any(select[key])
        _same(run(scene), want, "%s: after the count change" % kind)
        assert tables(scene) == select, "%s: upsample_select() after the count change" % kind
        assert not np.array_equal(want["source"], with_mats["source"])       # the cleared table showed in the frame
        if kind == "spheres":         # no table: no pixel is selected, every pixel is the full-resolution frame's
            assert not want["source"].any() and np.array_equal(want["rgba"], want["hi.rgba"])
    finally:
        scene.close()


# ------------------------------------------------------------------------------------------------ the scope
def test_scene_scope_through_list_mesh_and_scope_changes(rt, oracle, gpu):
    """Under the scene scope: a reflective frame; the cubes moved at the same count (their materials kept); another
    count (cleared); the mesh replaced, removed and put back; the scope to spheres (the frame is refused, nothing is
    written) and back. A reflective frame with its guides and queue lengths and a NEAREST / OCCLUDED query after every
    step equal a fresh scene's; after the move the frame is also the composed reference's and its guides castRay's."""
    import torch
    import query_ref as Q
    from reflect_scene_ref import SceneComposer
    w, h = 64, 36
    st = State(spheres=(64, 1, 0.0), planes=(2, 0), cubes=(5, 0), mesh=1, scope="scene", mats=("ex", 5), plane_mats=3,
               cube_mats=4)
    scene = sw.fresh_scene(rt, st)
    rays = torch.from_numpy(B._random_rays(7, 1024)).cuda()

    def check(where, cam=0):
        want = _render_check(rt, scene, st, w, h, where, cam=cam, depth=2, aov=sw.GUIDES)
        B._query_check(rt, scene, st, rays, where, modes=("nearest", "occluded"))
        return want

    try:
        first = check("start")
        st = B._set(rt, scene, st, {"op": "cubes", "cubes": (5, 1)})
        moved = check("cubes moved, the same count")
        assert st.cube_mats == 4 and not np.array_equal(moved["rgba"], first["rgba"])
        # the checkpoint: the composed reference with the kept tables, and castRay's record of the primary rays
        inp = _inputs(rt, st)
        comp = SceneComposer(oracle, rt, inp, sw.mesh_text(1))
        rgba, packed, queue = comp.render(w, h, 2, **_scene_mats(st))
        assert np.array_equal(moved["rgba"], rgba.view(np.uint32)) and np.array_equal(moved["packed"].view(np.uint32), packed)
        assert scene.reflect_stats()["queue"] == list(queue) and queue[0] > 0
        O, D = comp.prim.primary(w, h, 0, h)
        rec = Q.CastRef(oracle, inp, sw.mesh_text(1)).nearest(O, D)
        assert np.array_equal(moved["aov.depth"].reshape(-1), rec["t"].view(np.uint32))
        assert np.array_equal(moved["aov.id"].reshape(-1, 2), np.stack([rec["kind"], rec["index"]], 1))
        assert {0, 1, 2, 3} <= set(rec["kind"].tolist())                     # every kind of primitive is in view
        st = B._set(rt, scene, st, {"op": "cubes", "cubes": (4, 1)})
        assert st.cube_mats is None
        check("cubes at another count: their materials cleared", cam=1)
        st = B._set(rt, scene, st, {"op": "cubes", "cubes": (5, 1)})
        again = check("the old count again: none come back")
        for mesh in (2, 0, 1):
            st = B._set(rt, scene, st, {"op": "mesh", "mesh": mesh})
            check("mesh %d" % mesh, cam=mesh)
        st = B._set(rt, scene, st, {"op": "scope", "scope": "spheres"})
        assert _refused(rt, scene, w, h, reflect_depth=2) == (2, True)
        _render_check(rt, scene, st, w, h, "plain frame after the refusal", aov=sw.AOV)
        B._query_check(rt, scene, st, rays, "queries under the spheres scope", modes=("nearest", "occluded"))
        st = B._set(rt, scene, st, {"op": "scope", "scope": "scene"})
        back = check("the scene scope again")
        assert np.array_equal(back["rgba"], again["rgba"]) and np.array_equal(back["packed"], again["packed"])
        assert not np.array_equal(back["rgba"], moved["rgba"])               # (the cubes' materials stayed cleared)
    finally:
        scene.close()


# ------------------------------------------------------------------------------------------------ the samples
def test_sample_scratch_through_sizes_groups_and_the_mode(rt, oracle, gpu):
    """Under "many": spp 4 -> 5 -> 1 -> 5, each at another size of SIZES (the scratch of a group grows and shrinks, the
    two-group sum comes and goes), "many" -> "one" -> "many" in between, one frame on the second stream left un-waited
    across a size change. Frames and queue lengths equal a fresh scene's; the first frame is also the composed
    reference's (tests/reflect_samples_ref.py)."""
    import torch
    from reflect_samples_ref import SampleRef
    from test_reflect_cpu import composer_for
    st = State(spheres=(256, 1, 0.0), mats=("k", 5), samples="many")
    scene = sw.fresh_scene(rt, st)
    side = torch.cuda.Stream()
    try:
        first = _render_check(rt, scene, st, 64, 36, "spp 4 at 64 x 36", depth=2, spp=4)
        ref = SampleRef(rt, composer_for(oracle, rt, _inputs(rt, st))).render(64, 36, 2, spp=4,
                                                                              k=sw.material_arrays("k", 5, 256)[0])
        assert np.array_equal(first["rgba"], ref["rgba"].view(np.uint32)) and np.array_equal(first["packed"].view(np.uint32), ref["packed"])
        assert scene.reflect_stats()["queue"] == ref["queue"] and ref["queue"][1] > 0
        st = B._set(rt, scene, st, {"op": "samples", "samples": "one"})
        assert _refused(rt, scene, 72, 72, reflect_depth=2, spp=2) == (2, True)
        _render_check(rt, scene, st, 72, 72, "one sample under the other mode", depth=2)
        st = B._set(rt, scene, st, {"op": "samples", "samples": "many"})
        # two groups at a larger size on the side stream, not waited for; one sample at another size right behind it
        kw5 = dict(depth=2, spp=5, cam=1)
        want5 = _fresh(rt, st, lambda s: _render(rt, s, 96, 54, **kw5))
        want1 = _fresh(rt, st, lambda s: _render(rt, s, 40, 90, depth=3, spp=1, sample_base=2, sample_total=4))
        side.wait_stream(torch.cuda.current_stream())
        got5 = _render(rt, scene, 96, 54, stream=side, **kw5)
        got1 = _render(rt, scene, 40, 90, depth=3, spp=1, sample_base=2, sample_total=4)
        _same(got1, want1, "one sample of four at 40 x 90 behind an un-waited frame")
        _same(got5, want5, "spp 5 at 96 x 54 on the side stream")
        _render_check(rt, scene, st, 72, 72, "spp 5 at 72 x 72", depth=2, spp=5, cull=0)
        _render_check(rt, scene, st, 72, 72, "3 + 2 accumulated at 72 x 72", depth=2, spp=5, split=3)
        st = B._set(rt, scene, st, {"op": "samples", "samples": "one"})
        st = B._set(rt, scene, st, {"op": "samples", "samples": "many"})
        again = _render_check(rt, scene, st, 64, 36, "spp 4 at 64 x 36 again", depth=2, spp=4)
        assert np.array_equal(again["rgba"], first["rgba"]) and np.array_equal(again["packed"], first["packed"])
    finally:
        torch.cuda.synchronize()
        scene.close()


# ------------------------------------------------------------------------------------------------ the view lists
def test_view_list_slots_the_switch_and_a_graph(rt, gpu):
    """Six views through the four slots on two streams, compared after all are enqueued; the switch off and on between
    frames of one view (view_lists_info()["read"] follows it); a graph captured with the lists on and replayed after the
    switch went off, after a sphere change and after larger frames re-allocated the slots' buffers."""
    import torch
    w, h = 64, 36
    st = State(spheres=(1024, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    g = B._Graph(rt, scene, sw.GRAPH_FRAME["w"], sw.GRAPH_FRAME["h"], spp=sw.GRAPH_FRAME["spp"])

    def replay(where):
        got, want = g.replay(), g.want(st)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "graph replay " + where

    try:
        replay("at the start")
        seq = [0, 1, 2, 3, 4, 5, 0, 2, 5, 1]
        wants = {cam: _fresh(rt, st, lambda s: _render(rt, s, w, h, cam=cam)) for cam in set(seq)}
        outs = []
        for i, cam in enumerate(seq):
            streams[i & 1].wait_stream(torch.cuda.current_stream())
            outs.append(_render(rt, scene, w, h, cam=cam, stream=streams[i & 1]))
        for cam, out in zip(seq, outs):
            _same(out, wants[cam], "camera %d through the slots" % cam)
        small = scene.view_lists_info()
        assert small["read"] == 1
        for mode in (0, 1, 0):
            st = B._set(rt, scene, st, {"op": "view_lists", "view_lists": mode})
            _same(_render(rt, scene, w, h, cam=1), wants[1], "camera 1 with the lists %s" % ("on" if mode else "off"))
            assert scene.view_lists_info()["read"] == mode
            _render_check(rt, scene, st, w, h, "camera 3, aov, lists %d" % mode, cam=3, aov=sw.AOV)
        replay("after the switch went off")
        st = B._set(rt, scene, st, {"op": "view_lists", "view_lists": 1})
        replay("after the switch went on again")
        st = B._set(rt, scene, st, {"op": "spheres", "spheres": (1024, 1, 0.5)})
        replay("after a sphere change")
        for cam in (0, 1, 2, 3, 4):           # every slot takes a larger view
            _render_check(rt, scene, st, 96, 54, "96 x 54 camera %d" % cam, cam=cam)
        large = scene.view_lists_info()
        assert large["read"] == 1 and large["blocks"] > small["blocks"]
        replay("after the slots' buffers were re-allocated")
        g.set_camera(2)
        replay("at another camera")
        _render_check(rt, scene, st, w, h, "the small view again", cam=0)
    finally:
        torch.cuda.synchronize()
        g.destroy()
        scene.close()


# ------------------------------------------------------------------------------------------------ the post passes
def _pass_op(what, size, cam=0, **kw):
    op = dict(op="pass", what=what, size=size, cam=cam, aspect=None, variant=0, shrink=1, history=True, factor=2, depth=0)
    op.update(kw)
    return op


def test_denoisers_share_their_scratch_across_sizes_and_streams(rt, gpu):
    """denoise at a small size, a larger one (the scratch grows) and the small one again, alternating with
    denoise_variance, which shares the scratch, on the other stream and never waited for in between; a sphere change
    directly behind an un-waited pass. Every pass (with the frames and histories the scene made for it) equals a fresh
    scene's; one denoise and one denoise_variance call are also the restatements' (every variant)."""
    import torch
    import test_denoise_gpu as D
    import test_vdenoise_gpu as V
    st = State(spheres=(1024, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    try:
        ops = [_pass_op("denoise", (64, 36)), _pass_op("vdenoise", (96, 54), cam=1, variant=1),
               _pass_op("denoise", (72, 72), cam=2, variant=2), _pass_op("vdenoise", (64, 36), cam=3, history=False),
               _pass_op("denoise", (64, 36), cam=4, variant=1), _pass_op("vdenoise", (40, 90), cam=5, variant=2)]
        wants = [_fresh(rt, st, lambda s, op=op: _run_pass(rt, s, op, torch.cuda.current_stream())) for op in ops]
        streams[1].wait_stream(streams[0])
        outs = [_run_pass(rt, scene, op, streams[i & 1]) for i, op in enumerate(ops)]
        # a sphere change right behind the last, un-waited pass; the frame after it is the new state's
        st2 = B._set(rt, scene, st, {"op": "spheres", "spheres": (1024, 1, 0.5)})
        for i, (op, out, want) in enumerate(zip(ops, outs, wants)):
            _same(out, want, "pass %d: %s at %s" % (i, op["what"], op["size"]))
        _render_check(rt, scene, st2, 64, 36, "frame after the change behind the passes")
        # the restatements, on the long-lived scene's own frames
        frame = scene.render(64, 36, cam=sw.camera(rt, 0), aov=sw.AOV)
        D._check(scene, frame)
        hist = scene.temporal(frame, scene.temporal(frame, None, cam=sw.camera(rt, 0)), cam=sw.camera(rt, 0))
        V._check(scene, frame, hist)
    finally:
        torch.cuda.synchronize()
        scene.close()


def test_temporal_at_another_size_keeps_the_frames_raygen(rt, gpu):
    """A temporal call on frames of another size (made by another scene) between two renders of one size: the call
    builds its own raygen table (keyed on width, height and aspect) and must not rebuild the frames'; the second render
    equals a fresh scene's. The temporal results equal a fresh scene's and the restatement's; then another aspect at the
    same size, and the first again."""
    import torch
    import test_temporal_gpu as T
    st = State(spheres=(1024, 1, 0.0))
    scene = sw.fresh_scene(rt, st)
    other = sw.fresh_scene(rt, st)
    fresh = sw.fresh_scene(rt, st)
    try:
        _render_check(rt, scene, st, 96, 54, "before", cam=0)
        for (w, h), asp in (((40, 90), None), ((40, 90), 0.75), ((40, 90), None), ((64, 36), 1.25)):
            cams = [sw.camera(rt, 0), sw.camera(rt, 3)]
            frames = [other.render(w, h, cam=c, aspect=asp, aov=sw.GUIDES) for c in cams]
            hist = want = None
            for c, f in zip(cams, frames):
                want = fresh.temporal(f, want, cam=c, aspect=asp)
                hist = scene.temporal(f, hist, cam=c, aspect=asp)
            _same(hist, _flat(want), "temporal at %d x %d, aspect %s" % (w, h, asp))
            _render_check(rt, scene, st, 96, 54, "render after temporal at %d x %d aspect %s" % (w, h, asp), cam=1, aspect=0.75)
            _render_check(rt, scene, st, 96, 54, "default aspect after temporal at %d x %d" % (w, h), cam=2)
        # the restatement (both variants), from the history the long-lived scene made
        f = other.render(64, 36, cam=sw.camera(rt, 2), aspect=1.25, aov=sw.GUIDES)
        T._step(rt, scene, f, hist, sw.camera(rt, 2), 1.25)
    finally:
        torch.cuda.synchronize()
        for s in (scene, other, fresh):
            s.close()


@pytest.mark.parametrize("form", ["motion_spheres", "motion_cubes"])
def test_temporal_motion_infers_what_the_model_computes(rt, gpu, form):
    """A history, then a same-count move of the spheres (or of one cube), then temporal_motion with that history: the
    long-lived scene forms the displacements from the host copies in its history; fresh scenes of the two states are
    given the tables the model computes. On the second stream, not waited for until the end; then the restatement."""
    import torch
    import test_tmotion_gpu as M
    st = State(spheres=(256, 1, 0.0), cubes=(5, 0), planes=(2, 0))
    mutation = ({"op": "spheres", "how": "same_count", "spheres": (256, 1, 0.25)} if form == "motion_spheres" else
                {"op": "cubes", "how": "same_count_moved", "cubes": (5, 1)})
    op = dict(op="temporal", form=form, cams=(0, 3), size=(96, 54), aspect=None, variant=0, mutation=mutation)
    scene = sw.fresh_scene(rt, st)
    side = torch.cuda.Stream()
    try:
        want = _fresh_temporal(rt, op, st)
        side.wait_stream(torch.cuda.current_stream())
        got = _run_temporal(rt, op, scene, scene, side, between=lambda: sw.apply_to_scene(rt, scene, mutation, st))
        after = sw.apply(st, op)
        _same(got, want, form)
        assert (want["h2.rgba"].view(np.float32)[..., 3] > 1).any()          # some history was taken over
        sm, cm = sw.motion_tables(rt, st, after)
        M._step(rt, scene, got["f2"], got["h1"], sw.camera(rt, 3), rt.default_aspect(), sm=sm if len(sm) else None,
                cm=cm if len(cm) else None)
        # another count: the history's host copies no longer fit and the wrapper says so
        B._set(rt, scene, after, {"op": "spheres", "spheres": (65, 1, 0.0)})
        with pytest.raises(rt.RtError):
            scene.temporal_motion(got["f2"], got["h2"], cam=sw.camera(rt, 3))
    finally:
        torch.cuda.synchronize()
        scene.close()


def test_upsample_behind_renders_and_in_front_of_a_change(rt, gpu):
    """upsample at the exact 2 x ratio and at a ratio that is not exact (both variants), render_upscaled with mirrors,
    all on the second stream behind the renders that make their inputs, none waited for; a sphere change right behind
    them. Each equals a fresh scene's; one pair is also the restatement's."""
    import torch
    import test_upsample_gpu as UG
    st = State(spheres=(256, 1, 0.0), mats=("k", 5))
    scene = sw.fresh_scene(rt, st)
    side = torch.cuda.Stream()
    try:
        ops = [_pass_op("upsample", (96, 54), factor=2, depth=2), _pass_op("upsample", (72, 72), factor=3, depth=1, cam=1),
               _pass_op("upsample", (40, 90), factor=3, variant=1, cam=2), _pass_op("upsample", (64, 36), variant=1, depth=2),
               _pass_op("render_upscaled", (96, 54), depth=2, cam=3), _pass_op("render_upscaled", (40, 90), factor=3, depth=1)]
        wants = [_fresh(rt, st, lambda s, op=op: _run_pass(rt, s, op, torch.cuda.current_stream())) for op in ops]
        side.wait_stream(torch.cuda.current_stream())
        outs = [_run_pass(rt, scene, op, side) for op in ops]
        st2 = B._set(rt, scene, st, {"op": "spheres", "spheres": (256, 1, -0.5)})
        for i, (op, out, want) in enumerate(zip(ops, outs, wants)):
            _same(out, want, "pass %d: %s at %s / %d" % (i, op["what"], op["size"], op["factor"]))
        assert st2.mats == st.mats
        _render_check(rt, scene, st2, 96, 54, "reflective frame after the change", depth=2)
        UG._check(scene, outs[1]["hi"], outs[1]["lo"])
    finally:
        torch.cuda.synchronize()
        scene.close()


# ------------------------------------------------------------------------------------------------ random walks
def _walk_render(rt, scene, state, op, streams, pending, where):
    import torch
    w, h = op["size"]
    kw = {k: op[k] for k in ("cam", "aspect", "spp", "cull", "band", "depth", "aov", "sample_base", "sample_total", "split")}
    want, queue = _fresh_frame(rt, state, w, h, **kw)
    st = streams[op["stream"]]
    st.wait_stream(torch.cuda.current_stream())
    got = _render(rt, scene, w, h, stream=st, **kw)
    if op["defer"]:                              # compared after the next step has run
        pending.append((where, got, want))
        return
    _same(got, want, where)
    if queue is not None:
        assert _queue(scene) == queue, where + ": reflect queues"


def _walk_refused(rt, scene, state, op, streams, where):
    w, h = op["size"]
    rc, untouched = _refused(rt, scene, w, h, stream=streams[op["stream"]], cam=op["cam"], reflect_depth=op["depth"],
                             **op["request"])
    assert rc == 2, where + ": status %d, not RT_ERR_UNSUPPORTED" % rc
    assert untouched, where + ": a refused frame wrote to its outputs"
    _same(_render(rt, scene, w, h, cam=op["cam"], stream=streams[op["stream"]]),
          _fresh_frame(rt, state, w, h, cam=op["cam"])[0], where + ": the frame after the refusal")


def _walk_pass(rt, scene, state, op, streams, pending, where):
    import torch
    want, select = _fresh(rt, state, lambda s: _run_pass(rt, s, op, torch.cuda.current_stream()),
                          extra=lambda s: s.upsample_select())
    if op["what"] == "render_upscaled":
        assert scene.upsample_select() == select, where + ": upsample_select()"
    st = streams[op["stream"]]
    st.wait_stream(torch.cuda.current_stream())
    got = _run_pass(rt, scene, op, st)
    if op["defer"]:
        pending.append((where, got, want))
    else:
        _same(got, want, where)


def _walk_temporal(rt, scene, state, op, streams, pending, where):
    import torch
    want = _fresh_temporal(rt, op, state)
    st = streams[op["stream"]]
    st.wait_stream(torch.cuda.current_stream())
    between = (lambda: sw.apply_to_scene(rt, scene, op["mutation"], state)) if op["mutation"] else None
    got = _run_temporal(rt, op, scene, scene, st, between=between)
    if op["defer"]:
        pending.append((where, got, want))
    else:
        _same(got, want, where)


@pytest.mark.parametrize("seed", sw.WALK_SEEDS_2)
def test_random_walk_2(rt, gpu, seed):
    """One scene through a seeded walk of the second vocabulary (sw.WALK_STEPS steps): every output equals a fresh
    scene's. Frames, passes and temporal steps may go to a second stream and be compared only after the next step
    (often a change) ran; the graph of the first walks is replayed after the new changes as well."""
    import torch
    ops = sw.generate(seed, sw.WALK_STEPS, vocabulary=2)
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
            if k in sw.MUTATIONS_2:
                sw.apply_to_scene(rt, scene, op, st)
            elif k == "render":
                _walk_render(rt, scene, st, op, streams, pending, where)
            elif k == "query":
                B._walk_query(rt, scene, st, op, where)
            elif k == "refused":
                _walk_refused(rt, scene, st, op, streams, where)
            elif k == "pass":
                _walk_pass(rt, scene, st, op, streams, pending, where)
            elif k == "temporal":
                _walk_temporal(rt, scene, st, op, streams, pending, where)
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
