"""Temporal accumulation on the device (rt_scene_temporal). Every comparison is bit for bit, on rgba_out
and the moments viewed as uint32 and on `pixels`: the product kernel (variant 0), the plain yardstick (variant 1) and
the numpy restatement (tests/temporal_ref.py), on the device's own frames, guides and primary rays."""
import numpy as np
import pytest

import meshes
import temporal_ref as T
from postpass import (GUIDES, SENTINEL, WIDE_HISTORY_FLOOR, block_shares, cam as _cam, crop as _crop, cur as _cur,
                      hist_np as _hist_np, path as _path, scene as _scene, tensor_bits as _bits, wide_path as _wide_path)
from scenes import Inputs, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32


def _step(rt, sc, frame, hist, cam, aspect, colour=None, ref=True, **kw):
    """One call in both variants from the same history, against each other and against the restatement; returns variant
    0's history and the restatement's result."""
    import torch
    outs = [sc.temporal(frame, hist, cam=cam, aspect=aspect, colour=colour, variant=v, **kw) for v in (0, 1)]
    torch.cuda.synchronize()
    a, b = outs
    for k in ("rgba", "moments", "packed"):
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            diff = _bits(a[k]) != _bits(b[k])
            assert not diff.any(), (k, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    want = None
    if ref:
        h, w = frame["aov"]["depth"].shape
        rays = sc.primary_rays(w, h, cam=cam, aspect=aspect).cpu().numpy()
        terms = rt.view_terms(w, h, aspect, cam)
        same = hist is not None and bytes(hist["cam"]) == bytes(cam) and f32(hist["aspect"]) == f32(aspect)
        prev_terms = terms if hist is None else rt.view_terms(w, h, hist["aspect"], hist["cam"])
        tkw = {k: v for k, v in kw.items() if k in ("max_history", "depth_tolerance", "normal_cos_min", "want_moments")}
        want = T.temporal(_cur(frame, colour), _hist_np(hist), rays[..., :3], rays[..., 3:], terms, prev_terms,
                          aspect if hist is None else hist["aspect"], same, details=True, **tkw)
        diff = (_bits(a["rgba"]) != want["rgba"].view(np.uint32)).any(axis=-1)
        assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist())
        if a["moments"] is not None:
            assert np.array_equal(_bits(a["moments"]), want["moments"].view(np.uint32))
        if a["packed"] is not None:
            assert np.array_equal(_bits(a["packed"]), want["packed"])
    return a, want


def _chain(rt, sc, inp, w, h, cams, crop=None, **kw):
    """The frames of `cams` accumulated one after the other; returns the restatement's result of every step."""
    hist, res = None, []
    for cam in cams:
        frame = sc.render(w, h, cam=cam, aspect=inp.aspect, aov=GUIDES)
        if crop is not None:
            frame = _crop(frame, *crop)
        hist, want = _step(rt, sc, frame, hist, cam, inp.aspect, **kw)
        res.append(want)
    return res


@pytest.mark.parametrize("name", ["spheres", "mixed", "mesh"])
def test_a_camera_path(rt, gpu, name):
    mesh = None
    if name == "spheres":
        inp, w, h = Inputs(rt, 256), 160, 90
    elif name == "mixed":
        inp, w, h = mixed_scene(rt), 160, 96
    else:
        inp, w, h, mesh = Inputs(rt, 64), 160, 90, meshes.uv_sphere_obj()
    sc = _scene(rt, inp, mesh)
    try:
        res = _chain(rt, sc, inp, w, h, _path(rt))
        hit = res[3]["id"][..., 0] >= 0
        assert not res[0]["has_history"].any()
        shares = [(r["has_history"] & (r["id"][..., 0] >= 0)).sum() / (r["id"][..., 0] >= 0).sum() for r in res[1:]]
        assert 0.05 < shares[0] < 0.95 and shares[1] == 1.0 and 0.05 < shares[2] < 0.95, shares
        n = res[3]["rgba"][..., 3]
        assert n.max() > 3 and n.min() == 1 and (n[~hit] == 1).all()
        if name == "mesh":
            assert (res[3]["has_history"] & (res[3]["id"][..., 0] == 0)).any()      # triangles keep history too
        # the options: no moments, no packed words, both
        for kw in (dict(want_moments=False), dict(want_packed=False), dict(want_moments=False, want_packed=False)):
            opt = _chain(rt, sc, inp, w, h, _path(rt)[:2], **kw)
            assert np.array_equal(opt[1]["rgba"].view(np.uint32), res[1]["rgba"].view(np.uint32))
    finally:
        sc.close()


@pytest.mark.parametrize("w,h", [(161, 91), (64, 1), (1, 64), (5, 5), (65, 9), (300, 17)])
def test_sizes_that_are_no_multiple_of_the_tiles(rt, gpu, w, h):
    """Frames rendered at the size itself, and buffers of that size cut out of 322 x 91 frames where spheres are. A cut
    is a buffer in its own right: the pass forms the rays of a w x h view for it (the description carries no rays), so
    the restatement gets those -- a cut's depth and rays do not belong together, which the definition does not need."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        cams = _path(rt)
        res = _chain(rt, sc, inp, w, h, cams)
        if w > 1 and h > 1 and w * h > 25:
            assert any(r["has_history"].any() for r in res[1:])
        probe = sc.render(322, 91, cam=cams[0], aspect=inp.aspect, aov=GUIDES)
        ys, xs = np.nonzero(probe["aov"]["id"][..., 0].cpu().numpy() >= 0)
        cy, cx = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])
        y0, x0 = min(max(cy - h // 2, 0), 91 - h), min(max(cx - w // 2, 0), 322 - w)
        res = _chain(rt, sc, inp, 322, 91, cams, crop=(slice(y0, y0 + h), slice(x0, x0 + w)))
        assert res[2]["has_history"].any()              # the repeated camera
    finally:
        sc.close()


@pytest.mark.parametrize("w,h", [(576, 36), (1088, 36)])
def test_more_than_eight_tile_columns(rt, gpu, w, h):
    """tp_product pads its grid's width to a multiple of eight 64-pixel tile columns (nsegp) and finds its tile by
    b / nsegp and b - tyi * nsegp: at every width up to 512 nsegp is 8. 576 has 9 columns (nsegp = 16), 1088 has 17
    (nsegp = 24); frames rendered at the size itself, along the path with the yaw turned to 170, where the columns
    from 8 on show spheres that keep history over the camera step. Measured with the restatement on CPU frames
    (test_temporal_cpu): has_history share 0.84 in column 8 of 576; 0.17 in column 12 of 1088, the smallest of columns
    8 .. 16. The floor of 0.1 is asserted here on the restatement's has_history of the device's frames."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        res = _chain(rt, sc, inp, w, h, _wide_path(rt))
        shares = block_shares(res[1]["has_history"])
        print(w, "has_history share of tile columns 8 ..:", shares)
        assert len(shares) == -(-w // 64) - 8 and min(shares) >= WIDE_HISTORY_FLOOR, shares
        assert not res[0]["has_history"].any()
        hit = res[2]["id"][..., 0] >= 0
        assert res[2]["has_history"][hit].all()                         # the repeated camera
    finally:
        sc.close()


@pytest.fixture(scope="module")
def c2(rt, gpu):
    """160 x 90 / 256 spheres: the scene, its inputs and two frames a sideways step apart."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    cams = _path(rt)
    frames = [sc.render(160, 90, cam=c, aspect=inp.aspect, aov=GUIDES) for c in cams[:2]]
    yield sc, inp, cams, frames
    sc.close()


@pytest.mark.parametrize("max_history", [1, 2, 32])
def test_max_history(rt, c2, max_history):
    sc, inp, cams, frames = c2
    hist = None
    for k, i in enumerate((0, 0, 0, 1, 1, 1)):
        hist, want = _step(rt, sc, frames[i], hist, cams[i], inp.aspect, max_history=max_history)
        n = want["rgba"][..., 3]
        hit = want["id"][..., 0] >= 0
        assert n.max() <= max_history
        if k < 3:
            assert (n[hit] == min(k + 1, max_history)).all()
    if max_history == 1:            # the weight of the new frame is 1: H + (c - H) is c up to one rounding
        c = frames[1]["rgba"].cpu().numpy()[..., :3]
        top = max(float(c.max()), float(frames[0]["rgba"][..., :3].max()))
        assert np.abs(want["rgba"][..., :3] - c).max() <= 2.0 ** -22 * top


def test_reset_reads_no_history(rt, c2):
    import torch
    sc, inp, cams, frames = c2
    first, want = _step(rt, sc, frames[0], None, cams[0], inp.aspect)
    c = frames[0]["rgba"]
    assert np.array_equal(_bits(first["rgba"][..., :3]), _bits(c[..., :3])) and (first["rgba"][..., 3] == 1).all().item()
    assert np.array_equal(_bits(first["packed"]), _bits(frames[0]["packed"]))       # the frame's own words
    # prev_* pointers that must not be followed
    h, w = c.shape[:2]
    out = torch.empty_like(c)
    a = frames[0]["aov"]
    for v in (0, 1):
        d = sc.temporal_desc(w, h, cam=cams[0], aspect=inp.aspect, rgba_in=c.data_ptr(), depth=a["depth"].data_ptr(),
                             normal=a["normal"].data_ptr(), id=a["id"].data_ptr(), rgba_out=out.data_ptr(), reset=True,
                             variant=v)
        assert sc.temporal_raw(d, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(first["rgba"]))


def test_every_tap_outside_the_previous_buffer(rt, c2):
    """A previous view far to the side (in front of the point, outside the frame), one turned round (behind)."""
    sc, inp, cams, frames = c2
    first, _ = _step(rt, sc, frames[0], None, cams[0], inp.aspect)
    for prev_cam in (_cam(rt, 400, 3, 10, 180, -20), _cam(rt, 4, 3, 10, 0, 20)):
        moved = dict(first, cam=prev_cam)
        got, want = _step(rt, sc, frames[0], moved, cams[0], inp.aspect)
        assert not want["has_history"].any()
        assert (got["rgba"][..., 3] == 1).all().item()
        assert np.array_equal(_bits(got["rgba"][..., :3]), _bits(frames[0]["rgba"][..., :3]))


def test_jittered_samples_of_a_standing_camera(rt, c2):
    """colour= takes the frames of samples k = 0 .. 3 of 4; the history after four calls lies within 4 k ulp (k = 4) of
    the largest component of accumulate's four-sample frame divided by 4."""
    import torch
    sc, inp, cams, frames = c2
    w, h = 160, 90
    acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    pk = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for k in range(4):
        fd = sc.frame_desc(w, h, pixels=pk.data_ptr(), rgba=acc.data_ptr(), cam=cams[0], aspect=inp.aspect, spp=1,
                           sample_base=k, sample_total=4, accumulate=k > 0, resolve=0 if k == 3 else -1)
        sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    hist = None
    for k in range(4):
        sample = sc.render(w, h, cam=cams[0], aspect=inp.aspect, sample_base=k, sample_total=4)["rgba"]
        hist, _ = _step(rt, sc, frames[0], hist, cams[0], inp.aspect, colour=sample)
    torch.cuda.synchronize()
    mean = acc.cpu().numpy()[..., :3].astype(np.float64) / 4
    got = hist["rgba"].cpu().numpy()
    hit = frames[0]["aov"]["id"].cpu().numpy()[..., 0] >= 0
    assert (got[hit, 3] == 4).all()
    ulp = np.spacing(mean.max(axis=-1).astype(f32)).astype(np.float64)
    err = np.abs(got[..., :3].astype(np.float64) - mean).max(axis=-1)
    assert (err[hit] <= 16 * ulp[hit]).all(), float((err[hit] / ulp[hit]).max())
    assert (got[hit, :3] != sample.cpu().numpy()[hit, :3]).any()


def _raw(sc, inp, cams, frames, hist, out, moments=None, pixels=None, stream=0, **kw):
    a = frames[1]["aov"]
    h, w = frames[1]["rgba"].shape[:2]
    args = dict(cam=cams[1], aspect=inp.aspect, prev_cam=hist["cam"], prev_aspect=hist["aspect"],
                rgba_in=frames[1]["rgba"].data_ptr(), depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(),
                id=a["id"].data_ptr(), prev_rgba=hist["rgba"].data_ptr(), prev_depth=hist["depth"].data_ptr(),
                prev_normal=hist["normal"].data_ptr(), prev_id=hist["id"].data_ptr(),
                prev_moments=hist["moments"].data_ptr(), rgba_out=out.data_ptr() if out is not None else 0,
                moments_out=moments.data_ptr() if moments is not None else 0,
                pixels=pixels.data_ptr() if pixels is not None else 0)
    args.update(kw)
    return sc.temporal_raw(sc.temporal_desc(w, h, **args), stream)


@pytest.mark.parametrize("variant", [0, 1])
def test_inputs_and_unset_outputs_are_untouched(rt, c2, variant):
    import torch
    sc, inp, cams, frames = c2
    hist = sc.temporal(frames[0], None, cam=cams[0], aspect=inp.aspect)
    want = sc.temporal(frames[1], hist, cam=cams[1], aspect=inp.aspect, variant=variant)
    torch.cuda.synchronize()
    ins = {f"cur_{k}": v for k, v in frames[1]["aov"].items()}
    ins.update(cur_rgba=frames[1]["rgba"], **{f"prev_{k}": hist[k] for k in ("rgba", "moments", "depth", "normal", "id")})
    before = {k: _bits(v).copy() for k, v in ins.items()}
    h, w = frames[1]["rgba"].shape[:2]
    arena = torch.full((h * w * 4 + 512,), SENTINEL, dtype=torch.int32, device="cuda")     # guard words around the output
    out = arena[256:256 + h * w * 4].view(torch.float32).view(h, w, 4)
    other = torch.full((h, w, 2), SENTINEL, dtype=torch.int32, device="cuda")
    assert _raw(sc, inp, cams, frames, hist, out, variant=variant) == 0
    torch.cuda.synchronize()
    assert (arena[:256] == SENTINEL).all() and (arena[256 + h * w * 4:] == SENTINEL).all() and (other == SENTINEL).all()
    assert np.array_equal(_bits(out), _bits(want["rgba"]))
    for k, v in ins.items():
        assert np.array_equal(_bits(v), before[k]), k


def test_refusals_write_nothing(rt, c2):
    import torch
    sc, inp, cams, frames = c2
    hist = sc.temporal(frames[0], None, cam=cams[0], aspect=inp.aspect)
    h, w = frames[1]["rgba"].shape[:2]
    out = torch.full((h, w, 4), SENTINEL, dtype=torch.int32, device="cuda")
    mom = torch.full((h, w, 2), SENTINEL, dtype=torch.int32, device="cuda")
    pk = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    for kw in (dict(max_history=0), dict(max_history=257), dict(variant=2), dict(depth_tolerance=0.0),
               dict(depth_tolerance=float("nan")), dict(normal_cos_min=1.5), dict(prev_rgba=0), dict(prev_moments=0),
               dict(rgba_in=frames[1]["rgba"].data_ptr() + 4)):
        assert _raw(sc, inp, cams, frames, hist, out, mom, pk, **kw) == 1, kw
    # an output that overlaps an input: the history's colour written over itself, the tail of the current colour, the
    # packed words over the depth
    before = _bits(hist["rgba"]).copy()
    assert _raw(sc, inp, cams, frames, hist, hist["rgba"], mom, pk) == 1
    assert "overlaps" in sc.lib.rt_last_error().decode()
    assert _raw(sc, inp, cams, frames, hist, out, mom, pk, rgba_out=frames[1]["rgba"].data_ptr() + 16 * (h * w - 1)) == 1
    assert _raw(sc, inp, cams, frames, hist, out, mom, frames[1]["aov"]["depth"]) == 1
    # a capturing stream is refused, with the reason
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = _raw(sc, inp, cams, frames, hist, out, mom, pk, stream=s.cuda_stream)
        msg = sc.lib.rt_last_error().decode()
    assert rc == 2 and "captured" in msg
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (mom == SENTINEL).all() and (pk == SENTINEL).all()
    assert np.array_equal(_bits(hist["rgba"]), before)
    # and the scene still works
    assert _raw(sc, inp, cams, frames, hist, out, mom, pk) == 0
    torch.cuda.synchronize()
    want = sc.temporal(frames[1], hist, cam=cams[1], aspect=inp.aspect)
    assert np.array_equal(_bits(out.view(torch.float32)), _bits(want["rgba"]))
    assert np.array_equal(_bits(mom.view(torch.float32)), _bits(want["moments"])) and np.array_equal(_bits(pk), _bits(want["packed"]))


def test_two_streams_equal_one(rt, c2):
    """Two calls on different streams (the second reads what the first wrote: the scene orders them) give the bits of
    the same two calls on one stream."""
    import torch
    sc, inp, cams, frames = c2
    h0 = sc.temporal(frames[0], None, cam=cams[0], aspect=inp.aspect)
    a1 = sc.temporal(frames[1], h0, cam=cams[1], aspect=inp.aspect)
    a2 = sc.temporal(frames[0], a1, cam=cams[0], aspect=inp.aspect)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        b1 = sc.temporal(frames[1], h0, cam=cams[1], aspect=inp.aspect, stream=s1)
    with torch.cuda.stream(s2):
        b2 = sc.temporal(frames[0], b1, cam=cams[0], aspect=inp.aspect, stream=s2)
    torch.cuda.synchronize()
    for k in ("rgba", "moments", "packed"):
        assert np.array_equal(_bits(a1[k]), _bits(b1[k])) and np.array_equal(_bits(a2[k]), _bits(b2[k])), k


def test_the_next_render_is_what_it_was(rt, gpu):
    """A long-lived scene: temporal calls (of the frame's size and of another) between renders change no render's bits."""
    import torch
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        cams = _path(rt)
        before = [sc.render(160, 90, cam=c, aspect=inp.aspect, aov=GUIDES) for c in cams[:2]]
        small = [sc.render(65, 9, cam=c, aspect=inp.aspect, aov=GUIDES) for c in cams[:2]]
        hist = hs = None
        for i in (0, 1):
            hist = sc.temporal(before[i], hist, cam=cams[i], aspect=inp.aspect)
            hs = sc.temporal(small[i], hs, cam=cams[i], aspect=inp.aspect, variant=1)
        after = [sc.render(160, 90, cam=c, aspect=inp.aspect, aov=GUIDES) for c in cams[:2]]
        plain = sc.render(160, 90, cam=cams[1], aspect=inp.aspect)
        torch.cuda.synchronize()
        for b, a in zip(before, after):
            for k in ("packed", "rgba"):
                assert np.array_equal(_bits(b[k]), _bits(a[k])), k
            for k in GUIDES:
                assert np.array_equal(_bits(b["aov"][k]), _bits(a["aov"][k])), k
        assert np.array_equal(_bits(plain["rgba"]), _bits(before[1]["rgba"]))
        fresh = _scene(rt, inp)
        want = fresh.render(160, 90, cam=cams[1], aspect=inp.aspect)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(want["rgba"]), _bits(plain["rgba"]))
        fresh.close()
    finally:
        sc.close()


def test_launch_times_are_reported(rt, c2):
    sc, inp, cams, frames = c2
    hist = sc.temporal(frames[0], None, cam=cams[0], aspect=inp.aspect)
    sc.set_temporal_timing(True)
    try:
        for v in (0, 1):
            sc.temporal(frames[1], hist, cam=cams[1], aspect=inp.aspect, variant=v)
            t = sc.temporal_times()
            assert len(t) == 1 and t[0] > 0
    finally:
        sc.set_temporal_timing(False)
    sc.temporal(frames[1], hist, cam=cams[1], aspect=inp.aspect)
    assert sc.temporal_times() == []
