"""Temporal accumulation over moving objects on the device (rt_scene_temporal_motion). Every comparison
is bit for bit, on rgba_out and the moments viewed as uint32 and on `pixels`: the product kernel (variant 0), the plain
yardstick (variant 1) and the numpy restatement (tests/tmotion_ref.py), on the device's own frames, guides and primary
rays, with spheres and cubes moved between the frames."""
import numpy as np
import pytest

import meshes
import tmotion_ref as M
from postpass import (GUIDES, SENTINEL, crop as _crop, cur as _cur, hist_np as _hist_np, move_cube,
                      move_spheres, path as _path, scene as _scene, tensor_bits as _bits, wide_path as _wide_path)
from scenes import Inputs, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
REF_KEYS = ("max_history", "depth_tolerance", "normal_cos_min", "want_moments", "clamp", "clamp_slack", "clamp_history")


def _same(a, b, what=""):
    for k in ("rgba", "moments", "packed"):
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            diff = _bits(a[k]) != _bits(b[k])
            assert not diff.any(), (what, k, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _step(rt, sc, frame, hist, cam, aspect, sm=None, cm=None, colour=None, **kw):
    """One call in both variants from the same history, against each other and against the restatement; returns variant
    0's history and the restatement's result. sm / cm: explicit displacement tables [n, 4] (None: a NULL pointer)."""
    import torch
    none = np.zeros((0, 4), dtype=f32)          # an explicit empty table: nothing is inferred
    outs = [sc.temporal_motion(frame, hist, cam=cam, aspect=aspect, colour=colour, variant=v,
                               sphere_motion=none if sm is None else sm, cube_motion=none if cm is None else cm, **kw)
            for v in (0, 1)]
    torch.cuda.synchronize()
    a, b = outs
    _same(a, b, "variant 0 / variant 1")
    h, w = frame["aov"]["depth"].shape
    rays = sc.primary_rays(w, h, cam=cam, aspect=aspect).cpu().numpy()
    terms = rt.view_terms(w, h, aspect, cam)
    same = hist is not None and bytes(hist["cam"]) == bytes(cam) and f32(hist["aspect"]) == f32(aspect)
    prev_terms = terms if hist is None else rt.view_terms(w, h, hist["aspect"], hist["cam"])
    tkw = {k: v for k, v in kw.items() if k in REF_KEYS and v is not None}
    want = M.temporal_motion(_cur(frame, colour), _hist_np(hist), rays[..., :3], rays[..., 3:], terms, prev_terms,
                             aspect if hist is None else hist["aspect"], same, sphere_motion=sm, cube_motion=cm,
                             details=True, **tkw)
    diff = (_bits(a["rgba"]) != want["rgba"].view(np.uint32)).any(axis=-1)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
    if a["moments"] is not None:
        assert np.array_equal(_bits(a["moments"]), want["moments"].view(np.uint32))
    if a["packed"] is not None:
        assert np.array_equal(_bits(a["packed"]), want["packed"])
    return a, want


def _visible(frame, kind, k, skip=(), x0=0):
    """The k objects of `kind` that cover most pixels of the frame's columns from x0 on (fewer if fewer are seen)."""
    ids = frame["aov"]["id"].cpu().numpy()[:, x0:]
    idx, cnt = np.unique(ids[..., 1][ids[..., 0] == kind], return_counts=True)
    order = [int(i) for i in idx[np.argsort(-cnt, kind="stable")] if int(i) not in skip]
    return order[:k]


MOVES = [(0.0, 0.2, 0.0), (-0.15, 0.1, 0.2), (0.1, 0.0, -0.1), (0.05, -0.1, 0.1)]


def _walk(rt, sc, inp, w, h, crop=None, cube=None, cams=None, movers=4, x0=0, **kw):
    """A camera translation with four spheres (and `cube`) displaced, the same camera again with other displacements,
    a yaw step; every step with the clamp on and off from the same history. Returns the restatement's results with
    the clamp on. cams: another path of that form; movers, x0: that many spheres per step, those that cover most of
    the columns from x0 on."""
    cams = _path(rt) if cams is None else cams
    hist, res, moved = None, [], []
    frame = None
    for k, cam in enumerate(cams):
        sm = cm = None
        if k in (1, 2) and frame is not None:
            # x0: what the coming camera sees there before the move, a sphere moved at the step before included (the
            # few spheres such columns show can leave them once displaced) -- `moved` may then name a sphere twice
            if x0:
                frame = sc.render(w, h, cam=cam, aspect=inp.aspect, aov=GUIDES)
            pick = _visible(frame, M.RT_HIT_SPHERE, movers, skip=() if x0 else moved, x0=x0)
            moved += pick
            sm = move_spheres(inp, {i: MOVES[(j + k) % 4] for j, i in enumerate(pick)})
            sc.set_spheres(inp.spheres, inp.n)
            if cube is not None:
                cm = move_cube(rt, inp, cube, (-0.1, 0.1, 0.15) if k == 1 else (0.05, 0.0, -0.1))
                sc.set_cubes(inp.cubes, inp.n_cubes)
        frame = sc.render(w, h, cam=cam, aspect=inp.aspect, aov=GUIDES)
        if crop is not None:
            frame = _crop(frame, *crop)
        _step(rt, sc, frame, hist, cam, inp.aspect, sm, cm, clamp=False, **kw)
        hist, want = _step(rt, sc, frame, hist, cam, inp.aspect, sm, cm, clamp=True, **kw)
        want["moved"], want["picked"] = list(moved), list(pick) if sm is not None else []
        res.append(want)
    return res


@pytest.mark.parametrize("name", ["spheres", "mixed", "mesh"])
def test_a_path_with_moving_objects(rt, gpu, name):
    mesh, cube = None, None
    if name == "spheres":
        inp, w, h = Inputs(rt, 256), 160, 90
    elif name == "mixed":
        inp, w, h, cube = mixed_scene(rt), 160, 96, 1
    else:
        inp, w, h, mesh = Inputs(rt, 64), 160, 90, meshes.uv_sphere_obj()
    sc = _scene(rt, inp, mesh)
    try:
        res = _walk(rt, sc, inp, w, h, cube=cube)
        assert not res[0]["has_history"].any()
        for k in (1, 2):
            r, ids = res[k], res[k]["id"]
            mover = (ids[..., 0] == M.RT_HIT_SPHERE) & np.isin(ids[..., 1], r["moved"][-4:])
            assert mover.sum() > 20 and not r["static"][mover].any()
            share = float(r["has_history"][mover].mean())
            # the moved camera loses what it loses for every pixel; the same camera again keeps a mover's history
            assert share > (0.0 if k == 1 else 0.5), (k, share)
        # the same camera again: what did not move keeps the single tap, but for what a mover uncovered
        hit = res[2]["id"][..., 0] >= 0
        assert res[2]["has_history"][hit & res[2]["static"]].mean() > 0.9
        if cube is not None:
            box = (res[2]["id"][..., 0] == M.RT_HIT_CUBE) & (res[2]["id"][..., 1] == cube)
            assert box.sum() > 20 and not res[2]["static"][box].any() and res[2]["has_history"][box].mean() > 0.3
        if name == "mesh":
            assert (res[3]["has_history"] & (res[3]["id"][..., 0] == 0)).any()      # triangles keep history too
    finally:
        sc.close()


@pytest.mark.parametrize("w,h", [(161, 91), (64, 1), (1, 64), (5, 5), (65, 9), (300, 17)])
def test_sizes_that_are_no_multiple_of_the_tiles(rt, gpu, w, h):
    """Frames rendered at the size itself, and buffers of that size cut out of 322 x 91 frames where spheres are (a cut
    is a buffer in its own right, as in test_temporal_gpu): the halo rows and columns of the staged tile at every
    border of the buffer."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        _walk(rt, sc, inp, w, h)
        inp = Inputs(rt, 256)
        sc.set_spheres(inp.spheres, inp.n)
        probe = sc.render(322, 91, cam=_path(rt)[0], aspect=inp.aspect, aov=GUIDES)
        ys, xs = np.nonzero(probe["aov"]["id"][..., 0].cpu().numpy() >= 0)
        cy, cx = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])
        y0, x0 = min(max(cy - h // 2, 0), 91 - h), min(max(cx - w // 2, 0), 322 - w)
        res = _walk(rt, sc, inp, 322, 91, crop=(slice(y0, y0 + h), slice(x0, x0 + w)))
        assert res[2]["has_history"].any()              # the repeated camera
    finally:
        sc.close()


@pytest.mark.parametrize("w,h,movers", [(576, 36, 1), (1088, 36, 2)])
def test_more_than_eight_tile_columns(rt, gpu, w, h, movers):
    """With MOTION tp_product keeps its grid, padded to a multiple of eight 64-pixel tile columns, and leaves in the tiles
    of the padding; at every width up to 512 the padded width is 8 columns. Here 9 and 17 columns (16 and 24 padded),
    along test_temporal_gpu's wide path, and the displaced spheres are picked among those seen in columns >= 512, so
    that movers -- the reprojection with a displacement, the exchange between lanes, the clamp's staged tile -- run in
    tiles of the second and third group under the moved and under the repeated camera. On CPU frames of the first two
    cameras (test_temporal_cpu.View) columns >= 512 of 576 x 36 show two spheres, of 333 and 1 850 pixels under the
    second camera, and the larger one fills them once displaced, which is why one sphere is displaced per step there
    and the same sphere may be displaced again; with the restatement, 2 304 and 11 131 mover pixels in the camera step."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        res = _walk(rt, sc, inp, w, h, cams=_wide_path(rt), movers=movers, x0=512)
        for k in (1, 2):
            r, ids = res[k], res[k]["id"]
            assert len(r["picked"]) == movers, (k, r["picked"])
            mover = (ids[..., 0] == M.RT_HIT_SPHERE) & np.isin(ids[..., 1], r["picked"])
            mover[:, :512] = False
            assert mover.sum() > 20 and not r["static"][mover].any(), (k, int(mover.sum()))
            print(w, "step", k, "mover pixels in columns >= 512:", int(mover.sum()), "with history:",
                  int(r["has_history"][mover].sum()))
        assert res[2]["has_history"][mover].any()              # the repeated camera: movers keep history
        assert res[1]["has_history"][:, 512:].mean() > 0.1     # and so does the moved camera there
    finally:
        sc.close()


class Case:
    """160 x 90 / 256 spheres: a frame, then four spheres and light 0 moved, and the frames of the standing and of a
    moved camera after that."""

    def __init__(self, rt):
        self.inp = inp = Inputs(rt, 256)
        self.sc = sc = _scene(rt, inp)
        self.cams = _path(rt)
        self.before = sc.render(160, 90, cam=self.cams[0], aspect=inp.aspect, aov=GUIDES)
        self.moved = _visible(self.before, M.RT_HIT_SPHERE, 4)
        self.tab = move_spheres(inp, dict(zip(self.moved, MOVES)))
        sc.set_spheres(inp.spheres, inp.n)
        inp.lights[0].pos.x += 2
        sc.set_lights(inp.lights, inp.n_lights)
        self.after = [sc.render(160, 90, cam=c, aspect=inp.aspect, aov=GUIDES) for c in self.cams[:2]]
        # a history of three frames of the scene before the move, through rt_scene_temporal
        h = None
        for _ in range(3):
            h = sc.temporal(self.before, h, cam=self.cams[0], aspect=inp.aspect)
        self.hist = h


@pytest.fixture(scope="module")
def case(rt, gpu):
    c = Case(rt)
    yield c
    c.sc.close()


@pytest.mark.parametrize("moving", [False, True])
def test_zero_displacements_and_no_clamp_are_rt_scene_temporal(rt, case, moving):
    """NULL pointers (rt_scene_temporal's kernels run) and tables of zeros (the new kernels run)."""
    import torch
    c = case
    cam, frame = c.cams[int(moving)], c.after[int(moving)]
    zeros = torch.zeros((c.inp.n, 4), dtype=torch.float32, device="cuda")
    for variant in (0, 1):
        want = c.sc.temporal(frame, c.hist, cam=cam, aspect=c.inp.aspect, variant=variant)
        null = c.sc.temporal_motion(frame, c.hist, cam=cam, aspect=c.inp.aspect, clamp=False, variant=variant)
        zero = c.sc.temporal_motion(frame, c.hist, cam=cam, aspect=c.inp.aspect, clamp=False, variant=variant,
                                    sphere_motion=zeros, cube_motion=zeros[:3])
        torch.cuda.synchronize()
        _same(null, want, "NULL tables")
        _same(zero, want, "tables of zeros")
    assert (want["rgba"][..., 3] > 1).any().item()


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("kw", [dict(clamp_slack=0.0), dict(clamp_slack=0.5), dict(clamp_history=1), dict(clamp_history=4),
                                dict(clamp_history=256), dict(max_history=1), dict(max_history=32),
                                dict(want_moments=False), dict(want_packed=False),
                                dict(want_moments=False, want_packed=False)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_options(rt, case, moving, kw):
    c = case
    i = int(moving)
    got, want = _step(rt, c.sc, c.after[i], c.hist, c.cams[i], c.inp.aspect, c.tab, clamp=True, **kw)
    assert want["clamped"].any() and want["has_history"].any() and not want["static"].all()
    ch = kw.get("clamp_history", 4)
    n = want["rgba"][..., 3]
    assert (n[want["clamped"]] <= min(ch + 1, kw.get("max_history", 32))).all()


def test_a_short_table_and_a_displacement_that_is_not_finite(rt, case):
    c = case
    for i in (0, 1):
        last = max(c.moved)
        _, want = _step(rt, c.sc, c.after[i], c.hist, c.cams[i], c.inp.aspect, c.tab[:last], clamp=True)
        ids = c.after[i]["aov"]["id"].cpu().numpy()
        assert want["static"][(ids[..., 0] == M.RT_HIT_SPHERE) & (ids[..., 1] == last)].all()
        for bad in (np.nan, np.inf):
            tab = c.tab.copy()
            tab[c.moved[0], 1] = bad
            got, want = _step(rt, c.sc, c.after[i], c.hist, c.cams[i], c.inp.aspect, tab, clamp=True)
            sel = (ids[..., 0] == M.RT_HIT_SPHERE) & (ids[..., 1] == c.moved[0])
            assert sel.any() and (got["rgba"].cpu().numpy()[sel, 3] == 1).all()
            assert np.array_equal(_bits(got["rgba"])[sel, :3], _bits(c.after[i]["rgba"])[sel, :3])


def test_jittered_samples(rt, case):
    """colour= takes the frames of samples k = 0 .. 2 of 4 of the moved scene, one after the other."""
    c = case
    hist = c.hist
    for k in range(3):
        sample = c.sc.render(160, 90, cam=c.cams[0], aspect=c.inp.aspect, sample_base=k, sample_total=4)["rgba"]
        hist, want = _step(rt, c.sc, c.after[0], hist, c.cams[0], c.inp.aspect, c.tab if k == 0 else None, colour=sample,
                           clamp=True)
    assert (hist["rgba"][..., 3] > 2).any().item()


def test_the_python_path_infers_the_displacements(rt, gpu):
    import torch
    inp = mixed_scene(rt)
    sc = _scene(rt, inp)
    try:
        cams = _path(rt)
        f0 = sc.render(160, 96, cam=cams[0], aspect=inp.aspect, aov=GUIDES)
        h0 = sc.temporal_motion(f0, None, cam=cams[0], aspect=inp.aspect)
        assert h0["spheres"].shape == (inp.n, 3) and h0["cubes"].shape == (inp.n_cubes, 3)
        assert h0["spheres"].dtype == np.float32 and h0["cubes"].dtype == np.float32
        assert tuple(h0["cubes"][1]) == (6.0, 1.0, 2.0)
        sm = move_spheres(inp, dict(zip(_visible(f0, M.RT_HIT_SPHERE, 4), MOVES)))
        cm = move_cube(rt, inp, 1, (-0.1, 0.1, 0.15))
        sc.set_spheres(inp.spheres, inp.n)
        sc.set_cubes(inp.cubes, inp.n_cubes)
        for cam in cams[:2]:
            f1 = sc.render(160, 96, cam=cam, aspect=inp.aspect, aov=GUIDES)
            inferred = sc.temporal_motion(f1, h0, cam=cam, aspect=inp.aspect)
            explicit = sc.temporal_motion(f1, h0, cam=cam, aspect=inp.aspect, sphere_motion=sm, cube_motion=cm[:, :3])
            tensors = sc.temporal_motion(f1, h0, cam=cam, aspect=inp.aspect, sphere_motion=torch.from_numpy(sm).cuda(),
                                         cube_motion=torch.from_numpy(cm).cuda())
            ignored = sc.temporal_motion(f1, h0, cam=cam, aspect=inp.aspect, sphere_motion=np.zeros((0, 3), dtype=f32),
                                         cube_motion=np.zeros((0, 3), dtype=f32))
            plain = sc.temporal_motion(f1, sc.temporal(f0, None, cam=cams[0], aspect=inp.aspect), cam=cam, aspect=inp.aspect)
            torch.cuda.synchronize()
            _same(inferred, explicit, "inferred / explicit")
            _same(inferred, tensors, "inferred / tensors")
            _same(ignored, plain, "explicit empty tables / a history without positions")
            assert (_bits(ignored["rgba"]) != _bits(inferred["rgba"])).any()
            now = np.array([[o.x, o.y, o.z] for o in (inp.spheres[i].orgin for i in range(inp.n))], dtype=f32)
            assert np.array_equal(inferred["spheres"], now) and (now != h0["spheres"]).any()
            assert np.array_equal((now - h0["spheres"]).astype(f32), sm[:, :3])
        # the new history goes on: nothing moved since
        again = sc.temporal_motion(f1, inferred, cam=cams[1], aspect=inp.aspect, clamp=False)
        same = sc.temporal(f1, inferred, cam=cams[1], aspect=inp.aspect)
        torch.cuda.synchronize()
        _same(again, same, "nothing moved")
        # another sphere or cube count: the caller must start over
        sc.set_spheres(inp.spheres, inp.n - 1)
        with pytest.raises(rt.RtError):
            sc.temporal_motion(f1, inferred, cam=cams[1], aspect=inp.aspect)
        sc.set_spheres(inp.spheres, inp.n)
        sc.set_cubes(inp.cubes, inp.n_cubes - 1)
        with pytest.raises(rt.RtError):
            sc.temporal_motion(f1, inferred, cam=cams[1], aspect=inp.aspect)
        sc.set_cubes(inp.cubes, inp.n_cubes)
        with pytest.raises(rt.RtError):
            sc.temporal_motion(f1, inferred, cam=cams[1], aspect=inp.aspect, sphere_motion=np.zeros((4, 2), dtype=f32))
        first = sc.temporal_motion(f1, None, cam=cams[1], aspect=inp.aspect)
        torch.cuda.synchronize()
        assert (first["rgba"][..., 3] == 1).all().item()
    finally:
        sc.close()


def _raw(c, out, mom=None, pk=None, stream=0, sm=None, cm=None, **kw):
    frame, hist = c.after[1], c.hist
    a = frame["aov"]
    h, w = frame["rgba"].shape[:2]
    args = dict(cam=c.cams[1], aspect=c.inp.aspect, prev_cam=hist["cam"], prev_aspect=hist["aspect"],
                rgba_in=frame["rgba"].data_ptr(), depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(),
                id=a["id"].data_ptr(), prev_rgba=hist["rgba"].data_ptr(), prev_depth=hist["depth"].data_ptr(),
                prev_normal=hist["normal"].data_ptr(), prev_id=hist["id"].data_ptr(),
                prev_moments=hist["moments"].data_ptr(), rgba_out=out.data_ptr() if out is not None else 0,
                moments_out=mom.data_ptr() if mom is not None else 0,
                pixels=pk.data_ptr() if pk is not None else 0,
                sphere_motion=sm.data_ptr() if sm is not None else 0, n_sphere_motion=sm.shape[0] if sm is not None else 0,
                cube_motion=cm.data_ptr() if cm is not None else 0, n_cube_motion=cm.shape[0] if cm is not None else 0)
    args.update(kw)
    return c.sc.temporal_motion_raw(c.sc.temporal_motion_desc(w, h, **args), stream)


@pytest.mark.parametrize("variant", [0, 1])
def test_inputs_and_unset_outputs_are_untouched(rt, case, variant):
    import torch
    c = case
    sm = torch.from_numpy(c.tab).cuda()
    cm = torch.full((4, 4), 0.25, dtype=torch.float32, device="cuda")
    want = c.sc.temporal_motion(c.after[1], c.hist, cam=c.cams[1], aspect=c.inp.aspect, sphere_motion=sm, variant=variant)
    torch.cuda.synchronize()
    ins = {f"cur_{k}": v for k, v in c.after[1]["aov"].items()}
    ins.update(cur_rgba=c.after[1]["rgba"], sm=sm, cm=cm,
               **{f"prev_{k}": c.hist[k] for k in ("rgba", "moments", "depth", "normal", "id")})
    before = {k: _bits(v).copy() for k, v in ins.items()}
    h, w = c.after[1]["rgba"].shape[:2]
    arena = torch.full((h * w * 4 + 512,), SENTINEL, dtype=torch.int32, device="cuda")     # guard words around the output
    out = arena[256:256 + h * w * 4].view(torch.float32).view(h, w, 4)
    other = torch.full((h, w, 2), SENTINEL, dtype=torch.int32, device="cuda")
    assert _raw(c, out, sm=sm, cm=cm, variant=variant) == 0
    torch.cuda.synchronize()
    assert (arena[:256] == SENTINEL).all() and (arena[256 + h * w * 4:] == SENTINEL).all() and (other == SENTINEL).all()
    assert np.array_equal(_bits(out), _bits(want["rgba"]))
    for k, v in ins.items():
        assert np.array_equal(_bits(v), before[k]), k


def test_refusals_write_nothing(rt, case):
    import torch
    c = case
    h, w = c.after[1]["rgba"].shape[:2]
    sm = torch.from_numpy(c.tab).cuda()
    out = torch.full((h, w, 4), SENTINEL, dtype=torch.int32, device="cuda")
    mom = torch.full((h, w, 2), SENTINEL, dtype=torch.int32, device="cuda")
    pk = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    for kw in (dict(max_history=0), dict(variant=2), dict(depth_tolerance=0.0), dict(prev_rgba=0), dict(prev_moments=0),
               dict(rgba_in=c.after[1]["rgba"].data_ptr() + 4),
               dict(n_sphere_motion=-1), dict(sphere_motion=0), dict(sphere_motion=sm.data_ptr() + 4),
               dict(cube_motion=0, n_cube_motion=2), dict(cube_motion=sm.data_ptr() + 8, n_cube_motion=2),
               dict(clamp_slack=float("nan")), dict(clamp_slack=17.0), dict(clamp_slack=-0.5), dict(clamp_history=0),
               dict(clamp_history=257), dict(rgba_out=sm.data_ptr()), dict(pixels=sm.data_ptr() + 16 * (c.inp.n - 1))):
        assert _raw(c, out, mom, pk, sm=sm, **kw) == 1, kw
        assert "rt_scene_temporal_motion" in c.sc.lib.rt_last_error().decode()
    before = _bits(c.hist["rgba"]).copy()
    tab_before = _bits(sm).copy()
    assert _raw(c, c.hist["rgba"], mom, pk, sm=sm) == 1
    assert "overlaps" in c.sc.lib.rt_last_error().decode()
    # a capturing stream is refused, with the reason
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = _raw(c, out, mom, pk, sm=sm, stream=s.cuda_stream)
        msg = c.sc.lib.rt_last_error().decode()
    assert rc == 2 and "captured" in msg
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (mom == SENTINEL).all() and (pk == SENTINEL).all()
    assert np.array_equal(_bits(c.hist["rgba"]), before) and np.array_equal(_bits(sm), tab_before)
    # and the scene still works
    assert _raw(c, out, mom, pk, sm=sm) == 0
    torch.cuda.synchronize()
    want = c.sc.temporal_motion(c.after[1], c.hist, cam=c.cams[1], aspect=c.inp.aspect, sphere_motion=sm)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.view(torch.float32)), _bits(want["rgba"]))
    assert np.array_equal(_bits(mom.view(torch.float32)), _bits(want["moments"])) and np.array_equal(_bits(pk), _bits(want["packed"]))


def test_two_streams_equal_one(rt, case):
    """Calls of both entries on two streams (each reads what the one before wrote: the scene orders them) give the bits
    of the same calls on one stream."""
    import torch
    c = case
    sc, aspect = c.sc, c.inp.aspect
    sm = torch.from_numpy(c.tab).cuda()
    zero = torch.zeros_like(sm)

    def chain(s1, s2):
        a1 = sc.temporal_motion(c.after[1], c.hist, cam=c.cams[1], aspect=aspect, sphere_motion=sm, stream=s1)
        a2 = sc.temporal(c.after[0], a1, cam=c.cams[0], aspect=aspect, stream=s2)
        a3 = sc.temporal_motion(c.after[1], a2, cam=c.cams[1], aspect=aspect, sphere_motion=zero, stream=s1)
        a4 = sc.temporal_motion(c.after[1], a3, cam=c.cams[1], aspect=aspect, sphere_motion=zero, variant=1, stream=s2)
        return a1, a2, a3, a4
    one = chain(None, None)
    torch.cuda.synchronize()
    two = chain(torch.cuda.Stream(), torch.cuda.Stream())
    torch.cuda.synchronize()
    for a, b in zip(one, two):
        _same(a, b, "two streams")


def test_launch_times_are_reported(rt, case):
    import torch
    c = case
    sm = torch.from_numpy(c.tab).cuda()
    c.sc.set_temporal_timing(True)
    try:
        for v in (0, 1):
            for kw in (dict(sphere_motion=sm), dict(clamp=False)):
                c.sc.temporal_motion(c.after[1], c.hist, cam=c.cams[1], aspect=c.inp.aspect, variant=v, **kw)
                t = c.sc.temporal_times()
                assert len(t) == 1 and t[0] > 0
    finally:
        c.sc.set_temporal_timing(False)
    c.sc.temporal_motion(c.after[1], c.hist, cam=c.cams[1], aspect=c.inp.aspect, sphere_motion=sm)
    assert c.sc.temporal_times() == []


def test_later_calls_are_what_they_were(rt, gpu):
    """A long-lived scene: calls of the new entry between renders change no render's bits, and where its history
    equals Scene.temporal's (nothing moved, clamp off) denoise_variance gives the same bits on both."""
    import torch
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        cams = _path(rt)
        aov = GUIDES + ("albedo",)
        before = [sc.render(160, 90, cam=c, aspect=inp.aspect, aov=aov) for c in cams[:2]]
        small = [sc.render(65, 9, cam=c, aspect=inp.aspect, aov=GUIDES) for c in cams[:2]]
        zeros = np.zeros((inp.n, 4), dtype=f32)
        hist = ht = hs = None
        for i in (0, 1):
            hist = sc.temporal_motion(before[i], hist, cam=cams[i], aspect=inp.aspect, clamp=False, sphere_motion=zeros)
            ht = sc.temporal(before[i], ht, cam=cams[i], aspect=inp.aspect)
            hs = sc.temporal_motion(small[i], hs, cam=cams[i], aspect=inp.aspect, variant=1, sphere_motion=zeros[:9] + f32(0.1))
        after = [sc.render(160, 90, cam=c, aspect=inp.aspect, aov=aov) for c in cams[:2]]
        torch.cuda.synchronize()
        for b, a in zip(before, after):
            for k in ("packed", "rgba"):
                assert np.array_equal(_bits(b[k]), _bits(a[k])), k
            for k in aov:
                assert np.array_equal(_bits(b["aov"][k]), _bits(a["aov"][k])), k
        _same(hist, ht, "the two histories")
        d1 = sc.denoise_variance(before[1], hist)
        d2 = sc.denoise_variance(before[1], ht)
        torch.cuda.synchronize()
        for k in ("rgba", "packed", "variance"):
            assert np.array_equal(_bits(d1[k]), _bits(d2[k])), k
        # a clamped history is accepted as it is
        clamped = sc.temporal_motion(before[1], hist, cam=cams[1], aspect=inp.aspect)
        d3 = sc.denoise_variance(before[1], clamped)
        torch.cuda.synchronize()
        assert torch.isfinite(d3["rgba"]).all().item()
    finally:
        sc.close()
