"""The denoiser on the device (rt_scene_denoise). Every comparison is bit for bit, on rgba_out viewed as
uint32 and on `pixels`: the product kernels (variant 0), the plain yardstick (variant 1), the product kernels without
LDS staging (variant 2) and the numpy restatement (tests/denoise_ref.py), on the device's own frames and guides."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as R
import meshes
from postpass import ALL, SENTINEL, crop as _crop, scene as _scene, tensor_bits as _bits
from scenes import Inputs, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
VARIANTS = (0, 1, 2)


def _np(frame):
    """A frame's tensors as the restatement's arguments."""
    a = frame["aov"]
    return (frame["rgba"].cpu().numpy(), a["depth"].cpu().numpy(), a["normal"].cpu().numpy(), a["albedo"].cpu().numpy(),
            a["id"].cpu().numpy())


def _render(rt, inp, w, h, mesh=None, **kw):
    sc = _scene(rt, inp, mesh)
    return sc, sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=ALL, **kw)


def _check(sc, frame, variants=VARIANTS, ref=True, **kw):
    """Every variant against the first, and the first against the restatement; returns variant 0's (rgba, packed) bits."""
    import torch
    outs = [sc.denoise(frame, variant=v, **kw) for v in variants]
    torch.cuda.synchronize()
    got = [(_bits(o["rgba"]), _bits(o["packed"])) for o in outs]
    for v, g in zip(variants[1:], got[1:]):
        assert np.array_equal(g[0], got[0][0]), (kw, v, int((g[0] != got[0][0]).any(axis=-1).sum()))
        assert np.array_equal(g[1], got[0][1]), (kw, v)
    if ref:
        want, want_packed = R.denoise(*_np(frame), **kw)
        diff = (got[0][0] != want.view(np.uint32)).any(axis=-1)
        assert not diff.any(), (kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        assert np.array_equal(got[0][1], want_packed), kw
    return got[0]


@pytest.fixture(scope="module")
def c2(rt, gpu):
    """160 x 90 / 256 spheres: the device's own frame and guides."""
    sc, frame = _render(rt, Inputs(rt, 256), 160, 90)
    yield sc, frame
    sc.close()


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_variants_and_restatement_agree(c2, iterations):
    sc, frame = c2
    seen = set()
    for sigma_colour in (0.0, 0.1):
        for demodulate in (False, True):
            for normal_shift in (0, 5, 8):
                rgba, packed = _check(sc, frame, iterations=iterations, sigma_colour=sigma_colour,
                                      demodulate=demodulate, normal_shift=normal_shift)
                seen.add(rgba.tobytes())
    assert len(seen) == 12           # every parameter changes the result
    valid = _bits(frame["aov"]["id"])[..., 0].view(np.int32) >= 0
    assert 0.5 < valid.mean() < 0.8


def test_defaults_are_the_descriptions(rt, c2):
    sc, frame = c2
    a = _check(sc, frame)
    b = _check(sc, frame, ref=False, **R.DEFAULTS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    no_packed = sc.denoise(frame, want_packed=False)
    assert no_packed["packed"] is None and np.array_equal(_bits(no_packed["rgba"]), a[0])
    # it filtered: sky kept, the rest changed, and neighbours of one object are closer than before
    ids = frame["aov"]["id"].cpu().numpy()
    sky = ids[..., 0] < 0
    assert np.array_equal(a[0][sky], _bits(frame["rgba"])[sky]) and np.array_equal(a[1][sky], _bits(frame["packed"])[sky])
    assert (a[0][~sky] != _bits(frame["rgba"])[~sky]).any()


@pytest.mark.parametrize("w,h", [(161, 91), (64, 1), (1, 64), (5, 5), (65, 9), (300, 17)])
def test_sizes_that_are_no_multiple_of_the_tiles(rt, gpu, w, h):
    """Cut out of a 322 x 91 frame where spheres are (the denoiser filters a buffer as the buffer it is); 5 x 5: every
    step >= 4 has only its centre tap."""
    sc, frame = _render(rt, Inputs(rt, 256), 322, 91)
    try:
        ys, xs = np.nonzero(frame["aov"]["id"][..., 0].cpu().numpy() >= 0)
        cy, cx = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])          # a valid pixel amid the valid ones
        y0, x0 = min(max(cy - h // 2, 0), 91 - h), min(max(cx - w // 2, 0), 322 - w)
        part = _crop(frame, slice(y0, y0 + h), slice(x0, x0 + w))
        assert part["rgba"].shape == (h, w, 4)
        assert (part["aov"]["id"][..., 0] >= 0).any()
        for n in (1, 2, 3, 4, 6):
            _check(sc, part, iterations=n)
        _check(sc, part, iterations=5, sigma_colour=0.1, demodulate=False)
    finally:
        sc.close()


def test_960x540_against_the_restatement(rt, gpu):
    sc, frame = _render(rt, Inputs(rt, 1024), 960, 540)
    try:
        _check(sc, frame)
        _check(sc, frame, iterations=6, sigma_colour=0.1)
    finally:
        sc.close()


def test_c3_whole_frame_and_a_band(rt, gpu):
    """3840 x 2160 / 1024 spheres: the variants against each other on the whole frame; the restatement on a 64-row band
    of it, filtered as a band on both sides."""
    sc, frame = _render(rt, Inputs(rt, 1024), 3840, 2160)
    try:
        for kw in (dict(), dict(iterations=6, sigma_colour=0.1)):
            _check(sc, frame, ref=False, **kw)
        band = _crop(frame, slice(1056, 1120), slice(None))
        whole = _check(sc, frame, variants=(0,), ref=False)
        got = _check(sc, band)
        # rows of the band further than 2 (2^4 - 1) = 30 rows from its cuts are the whole frame's
        assert np.array_equal(got[0][30:34], whole[0][1086:1090])
        assert not np.array_equal(got[0][:30], whole[0][1056:1086])
    finally:
        sc.close()


@pytest.mark.parametrize("name", ["mixed", "mesh", "inside_sphere"])
def test_other_primitives_and_negative_depth(rt, gpu, name):
    mesh = None
    if name == "mixed":
        inp, w, h = mixed_scene(rt), 160, 96
    elif name == "mesh":
        inp, w, h, mesh = Inputs(rt, 64), 160, 90, meshes.uv_sphere_obj()
    else:
        inp, w, h = Inputs(rt, 256), 160, 90
        sp = (rt.Sphere * 256)()
        C.memmove(sp, inp.spheres, C.sizeof(sp))
        rt.load_library().rt_sphere_init(C.byref(sp[5]), 4.0, 3.0, 9.5, 2.0)   # around the ray origin
        inp.spheres = sp
    sc, frame = _render(rt, inp, w, h, mesh=mesh)
    try:
        ids = frame["aov"]["id"].cpu().numpy()
        kinds = set(np.unique(ids[..., 0]).tolist())
        if name == "mixed":
            assert {1, 2, 3} <= kinds
        elif name == "mesh":
            assert {0, 1} <= kinds                 # triangle ids compare by kind only
            tri = ids[..., 0] == 0
            assert len(np.unique(ids[tri][:, 1])) > 10
        else:
            assert (frame["aov"]["depth"] < 0).any().item()      # |z(p)|
        for kw in (dict(), dict(iterations=2), dict(iterations=6, sigma_colour=0.1, normal_shift=0)):
            got = _check(sc, frame, **kw)
        if name == "mesh":
            # the mesh's pixels were filtered across triangles
            assert (got[0][tri] != _bits(frame["rgba"])[tri]).any()
    finally:
        sc.close()


def test_nonfinite_guides(rt, c2):
    """NaN and inf written into a guide of some pixels: those taps are skipped, the pixel itself keeps a finite value."""
    import torch
    sc, frame = c2
    bad = {"rgba": frame["rgba"], "packed": frame["packed"], "aov": {k: v.clone() for k, v in frame["aov"].items()}}
    valid = (frame["aov"]["id"][..., 0] >= 0).cpu().numpy()
    ys, xs = np.nonzero(valid)
    pick = np.arange(0, len(ys), 29)
    for j, (y, x) in enumerate(zip(ys[pick], xs[pick])):
        if j % 4 == 0:
            bad["aov"]["depth"][y, x] = float("nan")
        elif j % 4 == 1:
            bad["aov"]["depth"][y, x] = float("-inf")
        elif j % 4 == 2:
            bad["aov"]["normal"][y, x, 1] = float("nan")
        else:
            bad["aov"]["normal"][y, x, 0] = float("inf")
    for kw in (dict(), dict(iterations=1), dict(iterations=6, sigma_colour=0.1)):
        got = _check(sc, bad, **kw)
        assert np.isfinite(got[0].view(np.float32)).all()
    clean = _check(sc, frame, ref=False)
    assert not np.array_equal(clean[0], _check(sc, bad, ref=False)[0])


def test_a_reflective_frame_without_demodulation(rt, gpu):
    n, w, h = 256, 160, 90
    inp = Inputs(rt, n)
    sc = inp.scene()
    try:
        sc.set_materials([0.6 if i % 3 == 1 else 0.0 for i in range(n)])
        frame = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=ALL, reflect_depth=2)
        flat = sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=ALL)
        assert not np.array_equal(_bits(frame["rgba"]), _bits(flat["rgba"]))
        _check(sc, frame, demodulate=False)
        _check(sc, frame, demodulate=False, iterations=6, sigma_colour=0.1)
        # without demodulation the albedo is not needed
        want, want_packed = R.denoise(*_np(frame), demodulate=False)
        del frame["aov"]["albedo"]
        a = sc.denoise(frame, demodulate=False)
        assert np.array_equal(_bits(a["rgba"]), want.view(np.uint32)) and np.array_equal(_bits(a["packed"]), want_packed)
        with pytest.raises(rt.RtError):
            sc.denoise(frame)
    finally:
        sc.close()


def _raw(sc, frame, rgba_out, pixels, stream=0, rgba_in=None, **kw):
    a = frame["aov"]
    h, w = frame["rgba"].shape[:2]
    d = sc.denoise_desc(w, h, rgba_in=(frame["rgba"] if rgba_in is None else rgba_in).data_ptr(), depth=a["depth"].data_ptr(),
                        normal=a["normal"].data_ptr(), albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(),
                        rgba_out=rgba_out.data_ptr() if rgba_out is not None else 0,
                        pixels=pixels.data_ptr() if pixels is not None else 0, **kw)
    return sc.denoise_raw(d, stream)


@pytest.mark.parametrize("variant", VARIANTS)
def test_in_place_equals_out_of_place(rt, c2, variant):
    import torch
    sc, frame = c2
    for n in (1, 2, 4):
        want = sc.denoise(frame, iterations=n, variant=variant)
        buf = frame["rgba"].clone()
        packed = torch.empty_like(frame["packed"])
        assert _raw(sc, frame, buf, packed, rgba_in=buf, iterations=n, variant=variant) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(buf), _bits(want["rgba"])), n
        assert np.array_equal(_bits(packed), _bits(want["packed"])), n


def test_scratch_regrowth_equals_fresh_scenes(rt, gpu):
    """Two calls in a row on one scene with different sizes (small, large, small again) equal fresh scenes."""
    import torch
    inp = Inputs(rt, 256)
    sc, small = _render(rt, inp, 160, 90)
    big = sc.render(960, 540, cam=inp.cam, aspect=inp.aspect, aov=ALL)
    try:
        got = [sc.denoise(f, variant=v) for f in (small, big, small) for v in (0, 1)]
        torch.cuda.synchronize()
        for (f, v), g in zip([(f, v) for f in (small, big, small) for v in (0, 1)], got):
            fresh = inp.scene()
            want = fresh.denoise(f, variant=v)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(g["rgba"]), _bits(want["rgba"])) and np.array_equal(_bits(g["packed"]), _bits(want["packed"]))
            fresh.close()
    finally:
        sc.close()


def test_a_side_stream_needs_no_host_sync(rt, gpu):
    """Render and denoise on one side stream, back to back; a second call on another stream is ordered behind the first
    by the scene (one scratch)."""
    import torch
    inp = Inputs(rt, 1024)
    sc = inp.scene()
    try:
        ref_frame = sc.render(960, 540, cam=inp.cam, aspect=inp.aspect, aov=ALL)
        want = sc.denoise(ref_frame)
        want6 = sc.denoise(ref_frame, iterations=6)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            frame = sc.render(960, 540, cam=inp.cam, aspect=inp.aspect, aov=ALL, stream=s1)
            a = sc.denoise(frame, stream=s1)
        with torch.cuda.stream(s2):
            # no event of the caller's between the streams: the scene orders this call behind the one on s1 (one
            # scratch), and that one is behind the render that wrote the frame
            b = sc.denoise(frame, iterations=6, stream=s2)
            c = sc.denoise(frame, stream=s2)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(a["rgba"]), _bits(want["rgba"])) and np.array_equal(_bits(a["packed"]), _bits(want["packed"]))
        assert np.array_equal(_bits(b["rgba"]), _bits(want6["rgba"]))
        assert np.array_equal(_bits(c["rgba"]), _bits(want["rgba"]))
    finally:
        sc.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_inputs_and_unset_outputs_are_untouched(rt, c2, variant):
    import torch
    sc, frame = c2
    before = {k: _bits(v).copy() for k, v in frame["aov"].items()}
    before["rgba"] = _bits(frame["rgba"]).copy()
    h, w = frame["rgba"].shape[:2]
    # one allocation around the output: guard words before and after it
    arena = torch.full((h * w * 4 + 512,), SENTINEL, dtype=torch.int32, device="cuda")
    out = arena[256:256 + h * w * 4].view(torch.float32).view(h, w, 4)
    other = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    assert _raw(sc, frame, out, None, variant=variant) == 0
    torch.cuda.synchronize()
    assert (arena[:256] == SENTINEL).all() and (arena[256 + h * w * 4:] == SENTINEL).all()
    assert (other == SENTINEL).all()
    want = sc.denoise(frame, variant=variant)
    assert np.array_equal(_bits(out), _bits(want["rgba"]))
    for k, v in frame["aov"].items():
        assert np.array_equal(_bits(v), before[k]), k
    assert np.array_equal(_bits(frame["rgba"]), before["rgba"])


def test_refusals_write_nothing(rt, c2):
    import torch
    sc, frame = c2
    h, w = frame["rgba"].shape[:2]
    out = torch.full((h, w, 4), SENTINEL, dtype=torch.int32, device="cuda")
    packed = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    fo = out.view(torch.float32)
    bad = [dict(iterations=0), dict(iterations=7), dict(normal_shift=-1), dict(normal_shift=9), dict(sigma_depth=0.0),
           dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf")), dict(sigma_colour=float("nan")),
           dict(variant=3), dict(variant=-1)]
    for kw in bad:
        assert _raw(sc, frame, fo, packed, **kw) == 1, kw
    a = frame["aov"]
    for field, off in (("rgba_in", 4), ("normal", 8), ("albedo", 4), ("id", 4), ("depth", 2), ("rgba_out", 8), ("pixels", 2)):
        d = sc.denoise_desc(w, h, rgba_in=frame["rgba"].data_ptr(), depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(),
                            albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(), rgba_out=fo.data_ptr(), pixels=packed.data_ptr())
        setattr(d, field, getattr(d, field) + off)
        assert sc.denoise_raw(d) == 1, field
        setattr(d, field, 0)
        assert sc.denoise_raw(d) == (0 if field == "pixels" else 1), field
        if field == "pixels":       # NULL pixels is a valid call: it wrote rgba_out, nothing else
            torch.cuda.synchronize()
            assert (packed == SENTINEL).all()
            out.fill_(SENTINEL)
    for wh in ((0, h), (w, 0), (-1, h), (1 << 20, h)):
        d = sc.denoise_desc(*wh, rgba_in=frame["rgba"].data_ptr(), depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(),
                            albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(), rgba_out=fo.data_ptr(), pixels=packed.data_ptr())
        assert sc.denoise_raw(d) == 1, wh
    # a capturing stream is refused, with the reason
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = _raw(sc, frame, fo, packed, stream=s.cuda_stream)
        msg = sc.lib.rt_last_error().decode()
    assert rc == 2 and "captured" in msg
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (packed == SENTINEL).all()
    # and the scene still works
    assert _raw(sc, frame, fo, packed) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fo), _bits(sc.denoise(frame)["rgba"]))


def test_the_plain_frame_is_what_it_was(rt, gpu):
    import torch
    inp = Inputs(rt, 256)
    sc = inp.scene()
    try:
        before = sc.render(160, 90, cam=inp.cam, aspect=inp.aspect)
        frame = sc.render(160, 90, cam=inp.cam, aspect=inp.aspect, aov=ALL)
        for v in VARIANTS:
            sc.denoise(frame, variant=v)
        after = sc.render(160, 90, cam=inp.cam, aspect=inp.aspect)
        after_aov = sc.render(160, 90, cam=inp.cam, aspect=inp.aspect, aov=ALL)
        torch.cuda.synchronize()
        for k in ("packed", "rgba"):
            assert np.array_equal(_bits(before[k]), _bits(after[k])), k
            assert np.array_equal(_bits(before[k]), _bits(frame[k])), k
            assert np.array_equal(_bits(before[k]), _bits(after_aov[k])), k
        for k in ALL:
            assert np.array_equal(_bits(frame["aov"][k]), _bits(after_aov["aov"][k])), k
    finally:
        sc.close()


def test_launch_times_are_reported(rt, c2):
    sc, frame = c2
    sc.set_denoise_timing(True)
    try:
        a = sc.denoise(frame, iterations=3)
        t0 = sc.denoise_times()
        b = sc.denoise(frame, iterations=3, variant=1)
        t1 = sc.denoise_times()
        assert len(t0) == 4 and len(t1) == 3 and all(t > 0 for t in t0 + t1)
        assert np.array_equal(_bits(a["rgba"]), _bits(b["rgba"]))
    finally:
        sc.set_denoise_timing(False)
    sc.denoise(frame)
    assert sc.denoise_times() == []
