"""The variance-guided denoiser on the device (rt_scene_denoise_variance). Every comparison is bit for
bit, on rgba_out and variance_out viewed as uint32 and on `pixels`: the product kernels (variant 0), the plain
yardstick (variant 1), the product kernels with the other step-16 kernel (variant 2) and the numpy restatement
(tests/vdenoise_ref.py), on the device's own frames and guides and a history that Scene.temporal accumulated."""
import numpy as np
import pytest

import denoise_ref as R
import meshes
import vdenoise_ref as V
from postpass import (ALL, SENTINEL, WIDE_CAMS, WIDE_HIT_FLOOR, WIDE_SEGMENT, cam as _cam, crop, scene as _scene,
                      tensor_bits as _bits)
from scenes import Inputs, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
VARIANTS = (0, 1, 2)


def _path(rt):
    """tests/test_temporal_gpu.py's path -- a translation, the same camera again, a yaw step with a translation -- with
    the repeated camera held for three more frames: a pixel that keeps its history throughout arrives with n = 6, one
    that the yaw step disoccludes with n = 1."""
    return [_cam(rt, 4, 3, 10, 180, -20)] + [_cam(rt, 4.5, 3.1, 10.2, 180, -20)] * 4 + [_cam(rt, 4.7, 3.1, 10.1, 176, -21)]


def _accumulate(rt, sc, inp, w, h, cams=None, colour=None):
    """The last frame of the path (cams: of another one) and the history accumulated along it. colour(frame, k): what
    is accumulated for frame k instead of the frame's own colour; the last frame then carries it as its rgba."""
    hist = None
    for k, cam in enumerate(_path(rt) if cams is None else cams):
        frame = sc.render(w, h, cam=cam, aspect=inp.aspect, aov=ALL)
        if colour is not None:
            frame = dict(frame, rgba=colour(frame, k))
        hist = sc.temporal(frame, hist, cam=cam, aspect=inp.aspect)
    return frame, hist


def _crop(frame, hist, rows, cols):
    return crop(frame, rows, cols), {k: hist[k][rows, cols].contiguous() for k in ("rgba", "moments")}


def _np(frame, hist):
    a = frame["aov"]
    rgba = frame["rgba"] if hist is None else hist["rgba"]
    return (rgba.cpu().numpy(), a["depth"].cpu().numpy(), a["normal"].cpu().numpy(), a["albedo"].cpu().numpy(),
            a["id"].cpu().numpy(), None if hist is None else hist["moments"].cpu().numpy())


def _check(sc, frame, hist, variants=VARIANTS, ref=True, **kw):
    """Every variant against the first, and the first against the restatement; returns variant 0's (rgba, packed,
    variance) bits."""
    import torch
    outs = [sc.denoise_variance(frame, hist, variant=v, **kw) for v in variants]
    torch.cuda.synchronize()
    got = [(_bits(o["rgba"]), _bits(o["packed"]), _bits(o["variance"])) for o in outs]
    for v, g in zip(variants[1:], got[1:]):
        for k in range(3):
            diff = g[k] != got[0][k]
            assert not diff.any(), (kw, v, k, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    if ref:
        want, want_packed, want_var = V.denoise_variance(*_np(frame, hist), **kw)
        diff = (got[0][0] != want.view(np.uint32)).any(axis=-1)
        assert not diff.any(), (kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(got[0][1], want_packed), kw
        diff = got[0][2] != want_var.view(np.uint32)
        assert not diff.any(), (kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    return got[0]


@pytest.fixture(scope="module")
def c2(rt, gpu):
    """160 x 90 / 256 spheres: the device's own last frame of the path and its history."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    frame, hist = _accumulate(rt, sc, inp, 160, 90)
    yield sc, frame, hist
    sc.close()


def _classes(frame, hist, min_history=4):
    hit = frame["aov"]["id"][..., 0].cpu().numpy() >= 0
    n = hist["rgba"][..., 3].cpu().numpy()
    return hit, hit & (n >= min_history), hit & ~(n >= min_history)


def test_the_history_has_short_and_long_pixels(c2):
    sc, frame, hist = c2
    hit, long_, short = _classes(frame, hist)
    shares = long_.sum() / hit.sum(), short.sum() / hit.sum()
    print("long, short share of the hit pixels:", shares)
    assert shares[0] >= 0.05 and shares[1] >= 0.05, shares
    assert 0.5 < hit.mean() < 0.8
    m = hist["moments"].cpu().numpy()
    assert ((m[..., 1] - m[..., 0] * m[..., 0])[long_] > 0).any()       # and some temporal variance is not 0


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_variants_and_restatement_agree(c2, iterations):
    sc, frame, hist = c2
    seen = set()
    for h, min_history in ((hist, 1), (hist, 4), (hist, 256), (None, None)):
        for demodulate in (False, True):
            for normal_shift in (0, 5):
                got = _check(sc, frame, h, iterations=iterations, demodulate=demodulate, normal_shift=normal_shift,
                             **({} if min_history is None else dict(min_history=min_history)))
                seen.add(got[0].tobytes() + got[2].tobytes())
    assert len(seen) == 16           # every parameter changes the result


def test_defaults_options_and_other_parameters(rt, c2):
    sc, frame, hist = c2
    a = _check(sc, frame, hist)
    b = _check(sc, frame, hist, ref=False, **V.DEFAULTS)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for v in VARIANTS:
        for kw in (dict(want_packed=False), dict(want_variance=False), dict(want_packed=False, want_variance=False)):
            o = sc.denoise_variance(frame, hist, variant=v, **kw)
            assert (o["packed"] is None) == (not kw.get("want_packed", True))
            assert (o["variance"] is None) == (not kw.get("want_variance", True))
            assert np.array_equal(_bits(o["rgba"]), a[0])
            if o["packed"] is not None:
                assert np.array_equal(_bits(o["packed"]), a[1])
            if o["variance"] is not None:
                assert np.array_equal(_bits(o["variance"]), a[2])
    seen = {a[0].tobytes()}
    for kw in (dict(sigma_colour=1.0), dict(sigma_colour=0.0), dict(sigma_floor=0.25), dict(spatial_boost=0.0),
               dict(spatial_boost=1.5, sigma_depth=0.2), dict(sigma_colour=2.0 ** 20, iterations=6)):
        seen.add(_check(sc, frame, hist, **kw)[0].tobytes())
    assert len(seen) == 7
    # sky kept (the history's bits: n = 1 there), its variance 0, the rest filtered
    hit, _, _ = _classes(frame, hist)
    assert np.array_equal(a[0][~hit], _bits(hist["rgba"])[~hit]) and (a[2][~hit] == 0).all()
    assert (a[0][hit] != _bits(hist["rgba"])[hit]).any()
    v = a[2].view(np.float32)
    assert np.isfinite(v).all() and (v >= 0).all() and (v[hit] > 0).any()


@pytest.mark.parametrize("w,h", [(161, 91), (64, 1), (1, 64), (5, 5), (65, 9), (300, 17)])
def test_sizes_that_are_no_multiple_of_the_tiles(rt, gpu, w, h):
    """Cut out of a 322 x 91 frame and its history where spheres are (the denoiser filters a buffer as the buffer it
    is)."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        frame, hist = _accumulate(rt, sc, inp, 322, 91)
        ys, xs = np.nonzero(frame["aov"]["id"][..., 0].cpu().numpy() >= 0)
        cy, cx = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])          # a valid pixel amid the valid ones
        y0, x0 = min(max(cy - h // 2, 0), 91 - h), min(max(cx - w // 2, 0), 322 - w)
        part, phist = _crop(frame, hist, slice(y0, y0 + h), slice(x0, x0 + w))
        assert part["rgba"].shape == (h, w, 4) and (part["aov"]["id"][..., 0] >= 0).any()
        for n in (1, 2, 3, 4, 5, 6):
            _check(sc, part, phist, iterations=n)
        for n in (1, 4, 6):
            _check(sc, part, None, iterations=n)
        _check(sc, part, phist, iterations=5, demodulate=False, min_history=1)
    finally:
        sc.close()


def test_960x540(rt, gpu):
    inp = Inputs(rt, 1024)
    sc = _scene(rt, inp)
    try:
        frame, hist = _accumulate(rt, sc, inp, 960, 540)
        hit, long_, short = _classes(frame, hist)
        assert long_.sum() >= 0.05 * hit.sum() and short.sum() >= 0.05 * hit.sum()
        _check(sc, frame, hist, iterations=2)
        _check(sc, frame, hist, iterations=6, ref=False)
        _check(sc, frame, None, iterations=5, ref=False)
    finally:
        sc.close()


def _ambient(frame, k):
    """The frame's colour with an ambient term on every hit pixel: the albedo times a factor of the normal (0.05 ..
    0.35) that also changes from frame to frame, so that no hit pixel is black and a held camera has temporal variance."""
    import torch
    a = frame["aov"]
    shade = (0.2 + 0.15 * a["normal"][..., 1:2]) * (0.75 + 0.125 * ((5 * k) % 4))
    c = frame["rgba"].clone()
    c[..., :3] = torch.where(a["id"][..., :1] >= 0, c[..., :3] + shade * a["albedo"][..., :3], c[..., :3])
    return c


@pytest.mark.parametrize("colour", [None, _ambient], ids=["lights", "ambient"])
def test_more_than_eight_row_segments(rt, gpu, colour):
    """dn_iter_direct maps blockIdx.x to a 256-pixel row segment in groups of eight, seg = ((b >> 3) % nseg8) * 8 +
    (b & 7): nseg8 is 1 at every width up to 2048. 2100 x 36 has 9 segments (nseg8 = 2), rendered at the size itself
    along test_temporal_cpu's wide path (yaw 170) with the second camera held for four frames: on CPU frames the second
    camera hits 0.68 of the pixels and 0.59 of columns >= 2048, and there 0.22 of the pixels keep history over the
    camera step (0.38 of the valid ones). Those arrive with n = 5 and the others with n = 4, so min_history = 5 splits
    the valid pixels there into temporal and spatial initial variances (measured on the device's history: 0.380 and
    0.620 of the valid pixels there); each class is asserted to be 5 % of them at least. Iteration 5 puts
    its LAST = true instantiation at step 16 in one of variants 0 / 2; iteration 6 puts LAST = false at step 16 there and
    LAST = true at step 32 in both.
    No light reaches what columns >= 1920 show: every hit pixel there is black in the frame itself ("lights"), its
    irradiance and variance 0 whatever the weights. "ambient" accumulates the same frames with an ambient term, so that
    those columns carry colours and variances a wrong tap would change. On CPU frames the largest albedo channel of
    every hit pixel there is 0.353 at least and its normal's y lies in [-0.81, 0.02], so the ambient term is 0.02 at
    least in that channel (asserted below on the device's albedo as > 0); a filtered pixel is a mean of such values
    with weights >= 0 and a centre weight > 0, which is why every hit pixel of the result there must be non-black."""
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        w, h, min_history = 2100, 36, 5
        cams = [_cam(rt, *WIDE_CAMS[0])] + [_cam(rt, *WIDE_CAMS[1])] * 4
        frame, hist = _accumulate(rt, sc, inp, w, h, cams, colour)
        there = (slice(None), slice(WIDE_SEGMENT, None))
        hit, long_, short = (m[there] for m in _classes(frame, hist, min_history))
        shares = hit.mean(), long_.sum() / hit.sum(), short.sum() / hit.sum()
        print("columns >= 2048: hit share, long and short share of the hit pixels:", shares)
        assert shares[0] >= WIDE_HIT_FLOOR and shares[1] >= 0.05 and shares[2] >= 0.05, shares
        for n in (5, 6):
            with_history = _check(sc, frame, hist, iterations=n, min_history=min_history)
            without = _check(sc, frame, None, iterations=n)
            if colour is not None:
                assert (frame["aov"]["albedo"].cpu().numpy()[there][hit][:, :3].max(axis=-1) > 0).all()
                rgba, var = with_history[0][there].view(np.float32), with_history[2][there].view(np.float32)
                assert (rgba[hit][:, :3].max(axis=-1) > 0).all() and (var[long_] > 0).any() and (var[short] > 0).any()
                assert (with_history[0][there][hit] != _bits(hist["rgba"])[there][hit]).any()       # filtered there
                assert (with_history[0][there] != without[0][there]).any()
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_other_primitives(rt, gpu, name):
    mesh = None
    if name == "mixed":
        inp, w, h = mixed_scene(rt), 160, 96
    else:
        inp, w, h, mesh = Inputs(rt, 64), 160, 90, meshes.uv_sphere_obj()
    sc = _scene(rt, inp, mesh)
    try:
        frame, hist = _accumulate(rt, sc, inp, w, h)
        kinds = set(np.unique(frame["aov"]["id"][..., 0].cpu().numpy()).tolist())
        assert ({1, 2, 3} if name == "mixed" else {0, 1}) <= kinds
        hit, long_, short = _classes(frame, hist)
        assert long_.any() and short.any()
        for kw in (dict(), dict(iterations=2), dict(iterations=6, normal_shift=0, demodulate=False)):
            _check(sc, frame, hist, **kw)
        _check(sc, frame, None, iterations=3)
    finally:
        sc.close()


def test_nonfinite_guides_and_moments(rt, c2):
    sc, frame, hist = c2
    bad = {"rgba": frame["rgba"], "packed": frame["packed"], "aov": {k: v.clone() for k, v in frame["aov"].items()}}
    bhist = {"rgba": hist["rgba"].clone(), "moments": hist["moments"].clone()}
    ys, xs = np.nonzero((frame["aov"]["id"][..., 0] >= 0).cpu().numpy())
    pick = np.arange(0, len(ys), 29)
    for j, (y, x) in enumerate(zip(ys[pick], xs[pick])):
        k = j % 7
        if k == 0:
            bad["aov"]["depth"][y, x] = float("nan")
        elif k == 1:
            bad["aov"]["depth"][y, x] = float("-inf")
        elif k == 2:
            bad["aov"]["normal"][y, x, 1] = float("nan")
        elif k == 3:
            bad["aov"]["normal"][y, x, 0] = float("inf")
        elif k == 4:
            bhist["moments"][y, x, 1] = float("inf")
        elif k == 5:
            bhist["moments"][y, x, 0] = float("nan")
        else:
            bhist["rgba"][y, x, 3] = float("nan")
    for kw in (dict(), dict(iterations=1), dict(iterations=6, demodulate=False), dict(min_history=1)):
        got = _check(sc, bad, bhist, **kw)
        assert np.isfinite(got[0].view(np.float32)).all() and np.isfinite(got[2].view(np.float32)).all()
    _check(sc, bad, None)
    assert not np.array_equal(_check(sc, frame, hist, ref=False)[0], _check(sc, bad, bhist, ref=False)[0])


def _converged(frame, n=32):
    import torch
    rgba = frame["rgba"].clone()
    rgba[..., 3] = n
    Y = R.luma(rgba.cpu().numpy())
    mom = torch.from_numpy(np.stack([Y, (Y * Y).astype(f32)], axis=-1)).cuda()
    return {"rgba": rgba, "moments": mom}


@pytest.mark.parametrize("demodulate", [False, True])
def test_zero_variance_is_the_plain_filter_on_the_device(rt, c2, demodulate):
    sc, frame, _ = c2
    hist = _converged(frame)
    plain_frame = {"rgba": hist["rgba"], "packed": frame["packed"], "aov": frame["aov"]}
    for n in (1, 3, 5, 6):
        for v in VARIANTS:
            a = sc.denoise_variance(frame, hist, iterations=n, demodulate=demodulate, variant=v)
            b = sc.denoise(plain_frame, iterations=n, demodulate=demodulate, sigma_colour=2.0 ** -6)
            assert np.array_equal(_bits(a["rgba"]), _bits(b["rgba"])), (n, v)
            assert np.array_equal(_bits(a["packed"]), _bits(b["packed"])), (n, v)
            assert (a["variance"] == 0).all().item()


def _raw(sc, frame, hist, rgba_out, pixels, variance_out, stream=0, rgba_in=None, **kw):
    a = frame["aov"]
    h, w = frame["rgba"].shape[:2]
    src = (frame["rgba"] if hist is None else hist["rgba"]) if rgba_in is None else rgba_in
    d = sc.vdenoise_desc(w, h, rgba_in=src.data_ptr(), depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(),
                         albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(),
                         moments=hist["moments"].data_ptr() if hist is not None else 0,
                         rgba_out=rgba_out.data_ptr() if rgba_out is not None else 0,
                         pixels=pixels.data_ptr() if pixels is not None else 0,
                         variance_out=variance_out.data_ptr() if variance_out is not None else 0, **kw)
    return sc.denoise_variance_raw(d, stream)


@pytest.mark.parametrize("variant", VARIANTS)
def test_in_place_equals_out_of_place(rt, c2, variant):
    import torch
    sc, frame, hist = c2
    for n in (1, 2, 5):
        want = sc.denoise_variance(frame, hist, iterations=n, variant=variant)
        buf = hist["rgba"].clone()
        packed = torch.empty_like(frame["packed"])
        var = torch.empty_like(frame["aov"]["depth"])
        assert _raw(sc, frame, hist, buf, packed, var, rgba_in=buf, iterations=n, variant=variant) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(buf), _bits(want["rgba"])), n
        assert np.array_equal(_bits(packed), _bits(want["packed"])), n
        assert np.array_equal(_bits(var), _bits(want["variance"])), n


@pytest.mark.parametrize("variant", VARIANTS)
def test_inputs_and_guard_words_are_untouched(rt, c2, variant):
    import torch
    sc, frame, hist = c2
    before = {k: _bits(v).copy() for k, v in frame["aov"].items()}
    before.update(rgba=_bits(frame["rgba"]).copy(), hrgba=_bits(hist["rgba"]).copy(), moments=_bits(hist["moments"]).copy())
    h, w = frame["rgba"].shape[:2]
    arena = torch.full((h * w * 4 + 512,), SENTINEL, dtype=torch.int32, device="cuda")
    out = arena[256:256 + h * w * 4].view(torch.float32).view(h, w, 4)
    varena = torch.full((h * w + 512,), SENTINEL, dtype=torch.int32, device="cuda")
    var = varena[256:256 + h * w].view(torch.float32).view(h, w)
    other = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    assert _raw(sc, frame, hist, out, None, var, variant=variant) == 0
    torch.cuda.synchronize()
    assert (arena[:256] == SENTINEL).all() and (arena[256 + h * w * 4:] == SENTINEL).all()
    assert (varena[:256] == SENTINEL).all() and (varena[256 + h * w:] == SENTINEL).all()
    assert (other == SENTINEL).all()
    want = sc.denoise_variance(frame, hist, variant=variant)
    assert np.array_equal(_bits(out), _bits(want["rgba"])) and np.array_equal(_bits(var), _bits(want["variance"]))
    for k, v in frame["aov"].items():
        assert np.array_equal(_bits(v), before[k]), k
    assert np.array_equal(_bits(frame["rgba"]), before["rgba"])
    assert np.array_equal(_bits(hist["rgba"]), before["hrgba"]) and np.array_equal(_bits(hist["moments"]), before["moments"])


def test_refusals_write_nothing(rt, c2):
    import torch
    sc, frame, hist = c2
    h, w = frame["rgba"].shape[:2]
    out = torch.full((h, w, 4), SENTINEL, dtype=torch.int32, device="cuda")
    packed = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    var = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    fo, fv = out.view(torch.float32), var.view(torch.float32)
    nan, inf = float("nan"), float("inf")
    bad = [dict(iterations=0), dict(iterations=7), dict(normal_shift=-1), dict(normal_shift=9), dict(sigma_depth=0.0),
           dict(sigma_depth=nan), dict(sigma_colour=nan), dict(sigma_colour=-1.0), dict(sigma_colour=2.0 ** 21),
           dict(sigma_floor=0.0), dict(sigma_floor=inf), dict(min_history=0), dict(min_history=257),
           dict(spatial_boost=-1.0), dict(spatial_boost=nan), dict(variant=3), dict(variant=-1)]
    for kw in bad:
        assert _raw(sc, frame, hist, fo, packed, fv, **kw) == 1, kw
    a = frame["aov"]

    def desc():
        return sc.vdenoise_desc(w, h, rgba_in=hist["rgba"].data_ptr(), depth=a["depth"].data_ptr(),
                                normal=a["normal"].data_ptr(), albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(),
                                moments=hist["moments"].data_ptr(), rgba_out=fo.data_ptr(), pixels=packed.data_ptr(),
                                variance_out=fv.data_ptr())
    for field, off in (("rgba_in", 4), ("normal", 8), ("albedo", 4), ("id", 4), ("depth", 2), ("rgba_out", 8), ("pixels", 2),
                       ("moments", 4), ("variance_out", 2)):
        d = desc()
        setattr(d, field, getattr(d, field) + off)
        assert sc.denoise_variance_raw(d) == 1, field
    # overlaps: an output on an input, two outputs on each other, rgba_out inside rgba_in but not rgba_in itself
    for field, target in (("pixels", "depth"), ("variance_out", "depth"), ("rgba_out", "normal"), ("variance_out", "moments"),
                          ("pixels", "variance_out"), ("variance_out", "rgba_out"), ("pixels", "rgba_in")):
        d = desc()
        setattr(d, field, getattr(d, target))
        assert sc.denoise_variance_raw(d) == 1, (field, target)
        assert "overlap" in sc.lib.rt_last_error().decode()
    d = desc()
    d.rgba_out = d.rgba_in + 16
    assert sc.denoise_variance_raw(d) == 1
    for wh in ((0, h), (w, 0), (-1, h), (1 << 20, h)):
        d = desc()
        d.width, d.height = wh
        assert sc.denoise_variance_raw(d) == 1, wh
    # a capturing stream is refused, with the reason
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = _raw(sc, frame, hist, fo, packed, fv, stream=s.cuda_stream)
        msg = sc.lib.rt_last_error().decode()
    assert rc == 2 and "captured" in msg
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (packed == SENTINEL).all() and (var == SENTINEL).all()
    # and the scene still works
    assert _raw(sc, frame, hist, fo, packed, fv) == 0
    torch.cuda.synchronize()
    want = sc.denoise_variance(frame, hist)
    assert np.array_equal(_bits(fo), _bits(want["rgba"])) and np.array_equal(_bits(fv), _bits(want["variance"]))


def test_two_streams_and_both_denoisers_share_one_scratch(rt, gpu):
    """Calls of both denoisers on two streams, with no event of the caller's between them: the scene orders them."""
    import torch
    inp = Inputs(rt, 1024)
    sc = _scene(rt, inp)
    try:
        frame, hist = _accumulate(rt, sc, inp, 960, 540)
        want = sc.denoise_variance(frame, hist)
        want6 = sc.denoise_variance(frame, None, iterations=6)
        plain = sc.denoise(frame)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            a = sc.denoise_variance(frame, hist, stream=s1)
            p1 = sc.denoise(frame, stream=s1)
        with torch.cuda.stream(s2):
            b = sc.denoise_variance(frame, None, iterations=6, stream=s2)
            p2 = sc.denoise(frame, stream=s2)
            c = sc.denoise_variance(frame, hist, stream=s2)
        torch.cuda.synchronize()
        for got, ref in ((a, want), (b, want6), (c, want)):
            for k in ("rgba", "packed", "variance"):
                assert np.array_equal(_bits(got[k]), _bits(ref[k])), k
        assert np.array_equal(_bits(p1["rgba"]), _bits(plain["rgba"])) and np.array_equal(_bits(p2["rgba"]), _bits(plain["rgba"]))
    finally:
        sc.close()


def test_scratch_regrowth_equals_fresh_scenes(rt, gpu):
    """Small, large, small again on one scene, with a call of rt_scene_denoise in between: each equals a fresh scene's."""
    import torch
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        small, shist = _accumulate(rt, sc, inp, 160, 90)
        big, bhist = _accumulate(rt, sc, inp, 640, 360)
        order = [(small, shist, 0), (small, shist, 1), (big, bhist, 0), (big, bhist, 1), (small, shist, 0)]
        got = []
        for f, h, v in order:
            got.append(sc.denoise_variance(f, h, variant=v))
            sc.denoise(f)
        torch.cuda.synchronize()
        for (f, h, v), g in zip(order, got):
            fresh = inp.scene()
            want = fresh.denoise_variance(f, h, variant=v)
            torch.cuda.synchronize()
            for k in ("rgba", "packed", "variance"):
                assert np.array_equal(_bits(g[k]), _bits(want[k])), (v, k)
            fresh.close()
    finally:
        sc.close()


def test_the_other_entry_points_are_what_they_were(rt, gpu):
    import torch
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    try:
        cams = _path(rt)
        f0 = sc.render(160, 90, cam=cams[0], aspect=inp.aspect, aov=ALL)
        h0 = sc.temporal(f0, None, cam=cams[0], aspect=inp.aspect)
        f1 = sc.render(160, 90, cam=cams[1], aspect=inp.aspect, aov=ALL)
        h1 = sc.temporal(f1, h0, cam=cams[1], aspect=inp.aspect)
        d1 = sc.denoise(f1, sigma_colour=0.1)
        plain = sc.render(160, 90, cam=cams[1], aspect=inp.aspect)
        for v in VARIANTS:
            sc.denoise_variance(f1, h1, variant=v)
            sc.denoise_variance(f1, None, variant=v, iterations=6)
        f1b = sc.render(160, 90, cam=cams[1], aspect=inp.aspect, aov=ALL)
        plain_b = sc.render(160, 90, cam=cams[1], aspect=inp.aspect)
        h1b = sc.temporal(f1b, h0, cam=cams[1], aspect=inp.aspect)
        d1b = sc.denoise(f1b, sigma_colour=0.1)
        torch.cuda.synchronize()
        for k in ("rgba", "packed"):
            assert np.array_equal(_bits(f1[k]), _bits(f1b[k])) and np.array_equal(_bits(plain[k]), _bits(plain_b[k])), k
            assert np.array_equal(_bits(d1[k]), _bits(d1b[k])) and np.array_equal(_bits(h1[k]), _bits(h1b[k])), k
        assert np.array_equal(_bits(h1["moments"]), _bits(h1b["moments"]))
        for k in ALL:
            assert np.array_equal(_bits(f1["aov"][k]), _bits(f1b["aov"][k])), k
    finally:
        sc.close()


def test_launch_times_are_reported(rt, c2):
    sc, frame, hist = c2
    sc.set_vdenoise_timing(True)
    try:
        a = sc.denoise_variance(frame, hist, iterations=3)
        t0 = sc.vdenoise_times()
        b = sc.denoise_variance(frame, hist, iterations=3, variant=1)
        t1 = sc.vdenoise_times()
        assert len(t0) == 5 and len(t1) == 4 and all(t > 0 for t in t0 + t1)
        assert np.array_equal(_bits(a["rgba"]), _bits(b["rgba"]))
    finally:
        sc.set_vdenoise_timing(False)
    sc.denoise_variance(frame, hist)
    assert sc.vdenoise_times() == []
