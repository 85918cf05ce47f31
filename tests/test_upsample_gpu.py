"""Guided upsampling on the device (rt_scene_upsample). Every comparison is bit for bit, on rgba_out
viewed as uint32, on `pixels` and on `source`: the product kernel (variant 0, one thread per pixel), the lane-exchange
kernel that serves the exact 2 x ratio (variant 1; the product kernel at other ratios) and the numpy restatement (tests/upsample_ref.py), on the device's own frames and guides at both resolutions."""
import ctypes as C
import itertools

import numpy as np
import pytest

import denoise_ref as R
import meshes
import upsample_ref as U
from postpass import ALL, SENTINEL, mae, mirror_k, scene as _scene, tensor_bits as _bits
from scenes import Inputs, mixed_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [(2, 2, 1, 1), (64, 2, 32, 1), (2, 64, 1, 32), (128, 16, 64, 8), (130, 18, 65, 9), (256, 32, 64, 8),
         (96, 54, 32, 18), (96, 54, 64, 36), (161, 91, 81, 46), (64, 8, 64, 8), (960, 540, 480, 270)]


def _pair(sc, inp, W, H, w, h, **kw):
    return (sc.render(W, H, cam=inp.cam, aspect=inp.aspect, aov=ALL),
            sc.render(w, h, cam=inp.cam, aspect=inp.aspect, aov=ALL, **kw))


def _np(frame):
    a = frame["aov"]
    d = {k: v.cpu().numpy() for k, v in a.items()}
    d["rgba"] = frame["rgba"].cpu().numpy()
    return d


def _check(sc, hi, lo, ref=True, **kw):
    """One call in both variants, against each other and against the restatement; returns the restatement's result
    (or, without it, variant 0's arrays)."""
    import torch
    outs = [sc.upsample(hi, lo, variant=v, **kw) for v in (0, 1)]
    torch.cuda.synchronize()
    a, b = outs
    for k in ("rgba", "packed"):
        diff = _bits(a[k]) != _bits(b[k])
        assert not diff.any(), (k, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert torch.equal(a["source"], b["source"]), kw
    if not ref:
        return dict(rgba=a["rgba"].cpu().numpy(), packed=_bits(a["packed"]), source=a["source"].cpu().numpy())
    base = kw.get("base", True)
    base = hi["rgba"].cpu().numpy() if base is True else (None if base in (False, None) else base.cpu().numpy())
    rkw = {k: v for k, v in kw.items() if k in ("select", "normal_shift", "sigma_depth", "demodulate")}
    colour = kw.get("colour")
    lo_np = _np(lo)
    if colour is not None:
        lo_np["rgba"] = colour.cpu().numpy()
    want = U.upsample(_np(hi), lo_np, base=base, details=True, **rkw)
    diff = (_bits(a["rgba"]) != want["rgba"].view(np.uint32)).any(axis=-1)
    assert not diff.any(), (kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert np.array_equal(_bits(a["packed"]), want["packed"]), kw
    assert np.array_equal(a["source"].cpu().numpy(), want["source"]), kw
    return want


def _tables(n):
    """Every other sphere, and a table shorter than the scene."""
    return {"sphere": [1 if i % 2 == 0 else 0 for i in range(n // 2)]}


@pytest.fixture(scope="module")
def c2(rt, gpu):
    inp = Inputs(rt, 256)
    sc = _scene(rt, inp)
    yield sc, inp
    sc.close()


@pytest.mark.parametrize("W,H,w,h", SIZES)
def test_sizes(rt, c2, W, H, w, h):
    """The exact 2 x ratio (variant 1 is the quad kernel: one lane, part of a wave, more than one wave and workgroup,
    sizes that are no multiple of the tile), other ratios and equal sizes (both variants gather)."""
    sc, inp = c2
    hi, lo = _pair(sc, inp, W, H, w, h)
    r = _check(sc, hi, lo)
    hit = r["selected"]
    if W * H >= 64 * 8:
        assert hit.any() and (~hit).any() and (r["source"] == 1).any()
    _check(sc, hi, lo, base=False, demodulate=False, select=_tables(256))
    if (W, H) == (w, h):
        ok = r["source"] == 1
        assert ok.sum() > 0.9 * hit.sum()


@pytest.mark.parametrize("W,H,w,h", [(128, 16, 64, 8), (161, 91, 81, 46), (96, 54, 32, 18)])
def test_settings(rt, c2, W, H, w, h):
    sc, inp = c2
    hi, lo = _pair(sc, inp, W, H, w, h)
    seen = set()
    for demod, shift, base, tables in itertools.product((True, False), (0, 5, 8), (True, False), (False, True)):
        r = _check(sc, hi, lo, demodulate=demod, normal_shift=shift, base=base, select=_tables(256) if tables else None)
        seen.add(r["rgba"].tobytes())
    assert len(seen) == 24                                   # every setting changes the result


def test_an_all_sky_frame(rt, c2):
    """The guides say sky everywhere: base's bits, or the bilinear mean."""
    sc, inp = c2
    for (W, H, w, h) in ((128, 16, 64, 8), (96, 54, 32, 18)):
        hi, lo = _pair(sc, inp, W, H, w, h)
        hi["aov"]["id"][..., 0] = -1
        lo["aov"]["id"][..., 0] = -1
        r = _check(sc, hi, lo)
        assert (r["source"] == 0).all() and np.array_equal(r["rgba"].view(np.uint32), _bits(hi["rgba"]))
        r = _check(sc, hi, lo, base=False)
        assert (r["source"] == 0).all()
        assert np.array_equal(r["rgba"][..., :3].view(np.uint32), U.bilinear(_np(lo)["rgba"], W, H).view(np.uint32))


@pytest.mark.parametrize("name", ["mixed", "mesh", "inside_sphere"])
def test_other_primitives_and_negative_depth(rt, gpu, name):
    mesh = None
    if name == "mixed":
        inp, W, H = mixed_scene(rt), 160, 96
    elif name == "mesh":
        inp, W, H, mesh = Inputs(rt, 64), 160, 90, meshes.uv_sphere_obj()
    else:
        inp, W, H = Inputs(rt, 256), 160, 90
        sp = (rt.Sphere * 256)()
        C.memmove(sp, inp.spheres, C.sizeof(sp))
        rt.load_library().rt_sphere_init(C.byref(sp[5]), 4.0, 3.0, 9.5, 2.0)   # around the ray origin
        inp.spheres = sp
    sc = _scene(rt, inp, mesh)
    try:
        hi, lo = _pair(sc, inp, W, H, W // 2, H // 2)
        ids = hi["aov"]["id"].cpu().numpy()
        kinds = set(np.unique(ids[..., 0]).tolist())
        for kw in (dict(), dict(base=False), dict(demodulate=False, normal_shift=0)):
            r = _check(sc, hi, lo, **kw)
        if name == "mixed":
            assert {1, 2, 3} <= kinds
            sel = {"sphere": [1] * 100, "plane": [0, 1], "cube": [1, 0, 1]}
            r = _check(sc, hi, lo, select=sel)
            for kind in (1, 3):
                m = ids[..., 0] == kind
                assert r["selected"][m].any() and (~r["selected"][m]).any(), kind
            assert r["selected"][ids[..., 0] == 2].all()          # the view shows plane 1 only
        elif name == "mesh":
            assert {0, 1} <= kinds                 # a triangle's index is ignored: taps of other triangles count
            tri = ids[..., 0] == 0
            lo_ids = lo["aov"]["id"].cpu().numpy()
            assert len(np.unique(ids[tri][:, 1])) > 10
            r = _check(sc, hi, lo)
            assert (r["source"][tri] == 1).mean() > 0.9
            # with the index compared, most mesh pixels would find no tap of their own triangle
            x0, _ = U.positions(W, W // 2)
            y0, _ = U.positions(H, H // 2)
            same = np.zeros(ids.shape[:2], dtype=bool)
            for k in range(4):
                tx, ty = np.clip(x0 + (k & 1), 0, W // 2 - 1), np.clip(y0 + (k >> 1), 0, H // 2 - 1)
                same |= lo_ids[ty[:, None], tx[None, :], 1] == ids[..., 1]
            assert (~same & tri & (r["source"] == 1)).any()
            assert not _check(sc, hi, lo, select={"sphere": [1] * 64})["selected"][tri].any()   # triangles read as 0
        else:
            assert (hi["aov"]["depth"] < 0).any().item()      # |z(p)|
            assert (r["source"] == 1).any()
    finally:
        sc.close()


def test_nonfinite_guides(rt, c2):
    """NaN and inf written into guides of some pixels on either side: the hi pixel falls back on base, the lo pixel is
    no tap; every other pixel keeps its bits."""
    sc, inp = c2
    W, H, w, h = 160, 90, 80, 45
    hi, lo = _pair(sc, inp, W, H, w, h)
    clean = _check(sc, hi, lo)
    bad_hi = {"rgba": hi["rgba"], "aov": {k: v.clone() for k, v in hi["aov"].items()}}
    bad_lo = {"rgba": lo["rgba"], "aov": {k: v.clone() for k, v in lo["aov"].items()}}
    values = (float("nan"), float("inf"), float("-inf"))
    ys, xs = np.nonzero(clean["source"] == 1)
    pick = np.arange(0, len(ys), 53)
    touched = np.zeros((H, W), dtype=bool)
    for j, (y, x) in enumerate(zip(ys[pick], xs[pick])):
        if j % 2 == 0:
            bad_hi["aov"]["depth"][y, x] = values[j % 3]
        else:
            bad_hi["aov"]["normal"][y, x, j % 3] = values[j % 3]
        touched[y, x] = True
    r = _check(sc, bad_hi, lo)
    assert (r["source"][touched] == 2).all()
    assert np.array_equal(r["rgba"][~touched].view(np.uint32), clean["rgba"][~touched].view(np.uint32))
    lo_hit = np.nonzero(lo["aov"]["id"][..., 0].cpu().numpy() >= 0)
    near = np.zeros((H, W), dtype=bool)
    for j in range(0, len(lo_hit[0]), 41):
        y, x = int(lo_hit[0][j]), int(lo_hit[1][j])
        if j % 2 == 0:
            bad_lo["aov"]["depth"][y, x] = values[j % 3]
        else:
            bad_lo["aov"]["normal"][y, x, j % 3] = values[j % 3]
        near[max(2 * y - 1, 0):2 * y + 3, max(2 * x - 1, 0):2 * x + 3] = True
    r = _check(sc, hi, bad_lo)
    assert np.isfinite(r["rgba"]).all()
    assert np.array_equal(r["rgba"][~near].view(np.uint32), clean["rgba"][~near].view(np.uint32))
    assert not np.array_equal(r["rgba"].view(np.uint32), clean["rgba"].view(np.uint32))
    _check(sc, bad_hi, bad_lo, base=False, demodulate=False)


def test_a_reflective_frame_through_render_upscaled(rt, gpu):
    import torch
    n, W, H = 256, 160, 90
    inp = Inputs(rt, n)
    sc = inp.scene()
    try:
        sc.set_materials(list(mirror_k(n)))
        outs = [sc.render_upscaled(W, H, 2, reflect_depth=2, cam=inp.cam, aspect=inp.aspect, variant=v, want_parts=True)
                for v in (0, 1)]
        full = sc.render(W, H, cam=inp.cam, aspect=inp.aspect, reflect_depth=2)
        torch.cuda.synchronize()
        a, b = outs
        assert a["lo"]["rgba"].shape == (45, 80, 4)
        for k in ("rgba", "packed"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        assert torch.equal(a["source"], b["source"])
        hi, lo = _np(a["hi"]), _np(a["lo"])
        select = {"sphere": (mirror_k(n) > 0).astype(np.uint8)}
        assert sc.upsample_select()["sphere"] == select["sphere"].tolist()
        want = U.upsample(hi, lo, base=hi["rgba"], select=select, demodulate=False, details=True)
        assert np.array_equal(_bits(a["rgba"]), want["rgba"].view(np.uint32))
        assert np.array_equal(_bits(a["packed"]), want["packed"])
        assert np.array_equal(a["source"].cpu().numpy(), want["source"])
        sel = want["selected"]
        full_np = full["rgba"].cpu().numpy()
        assert 500 < sel.sum() < 0.25 * sel.size
        assert np.array_equal(_bits(a["rgba"])[~sel], full_np.view(np.uint32)[~sel])
        assert np.array_equal(_bits(a["packed"])[~sel], _bits(full["packed"])[~sel])
        # the relations of test_upsample_cpu.test_the_error_relations, on the device's frames
        got = a["rgba"].cpu().numpy()
        bil = U.bilinear(lo["rgba"], W, H)
        e_up, e_plain, e_bil = mae(got, full_np), mae(hi["rgba"], full_np), mae(bil, full_np)
        m_up, m_bil = mae(got, full_np, sel), mae(bil, full_np, sel)
        print("reflective 160x90 <- 80x45 on the device:", e_up, e_bil, e_plain, "mirror pixels", m_up, m_bil,
              "without a tap", int((want["source"] == 2).sum()), "of", int(sel.sum()))
        assert e_up < 0.75 * e_plain and e_up < 0.3 * e_bil
        assert m_up < m_bil
        assert (want["source"][sel] == 2).mean() <= 0.01
    finally:
        sc.close()


def test_c3_at_3840x2160(rt, gpu):
    """Both variants over the whole frame; the restatement on hi rows 1024 .. 1087: with the exact 2 x ratio the rows
    1022 .. 1089 over the lo rows 511 .. 544 are a problem of their own whose inner rows have the frame's taps."""
    import torch
    n, W, H = 1024, 3840, 2160
    inp = Inputs(rt, n)
    sc = inp.scene()
    try:
        sc.set_materials(list(mirror_k(n)))
        hi = sc.render(W, H, cam=inp.cam, aspect=inp.aspect, aov=ALL)
        lo = sc.render(W // 2, H // 2, cam=inp.cam, aspect=inp.aspect, aov=ALL, reflect_depth=1)
        select = sc.upsample_select()
        for kw in (dict(select=select, demodulate=False), dict()):
            a, b = (sc.upsample(hi, lo, variant=v, **kw) for v in (0, 1))
            torch.cuda.synchronize()
            assert torch.equal(a["rgba"].view(torch.int32), b["rgba"].view(torch.int32)), kw
            assert torch.equal(a["packed"], b["packed"]) and torch.equal(a["source"], b["source"]), kw
            cut = lambda f, r0, r1: {k: v[r0:r1].cpu().numpy() for k, v in dict(f["aov"], rgba=f["rgba"]).items()}
            hi_np, lo_np = cut(hi, 1022, 1090), cut(lo, 511, 545)
            rkw = {k: v for k, v in kw.items() if k != "select"}
            want = U.upsample(hi_np, lo_np, base=hi_np["rgba"], select=kw.get("select"), **rkw)
            rows = slice(1024, 1088)
            assert np.array_equal(_bits(a["rgba"][rows]), want["rgba"][2:66].view(np.uint32)), kw
            assert np.array_equal(_bits(a["packed"][rows]), want["packed"][2:66]), kw
            assert np.array_equal(a["source"][rows].cpu().numpy(), want["source"][2:66]), kw
            assert (want["source"][2:66] == 1).any() and (want["source"][2:66] == 0).any()
    finally:
        sc.close()


# ----------------------------------------------------------------------------- the host side
def _guarded(torch, shape, dtype, fill):
    """A tensor of `shape` inside a larger allocation whose 64 words on either side hold the sentinel."""
    n = int(np.prod(shape))
    item = torch.empty((), dtype=dtype).element_size()
    words = (n * item + 3) // 4 + 128
    raw = torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")
    view = raw[64:64 + (n * item + 3) // 4].view(torch.uint8)[:n * item].view(dtype).view(shape)
    if fill is not None:
        view.copy_(fill)
    return raw, view


def _guards_intact(raw, n_bytes):
    inner = (n_bytes + 3) // 4
    head, tail = raw[:64], raw[64 + inner:]
    return bool((head == SENTINEL).all().item()) and bool((tail == SENTINEL).all().item())


def test_outputs_are_fully_written_and_inputs_untouched(rt, c2):
    """Poisoned outputs between guard words, in both variants and both kernels: every output element is written, no
    guard word and no input changes; in place (rgba_out = base) gives the same bits; a refusal writes nothing."""
    import torch
    sc, inp = c2
    for (W, H, w, h) in ((130, 18, 65, 9), (96, 54, 32, 18)):
        hi, lo = _pair(sc, inp, W, H, w, h)
        sel = torch.tensor(_tables(256)["sphere"], dtype=torch.uint8, device="cuda")
        ins = {"rgba_lo": lo["rgba"], "depth_lo": lo["aov"]["depth"], "normal_lo": lo["aov"]["normal"],
               "albedo_lo": lo["aov"]["albedo"], "id_lo": lo["aov"]["id"], "depth": hi["aov"]["depth"],
               "normal": hi["aov"]["normal"], "albedo": hi["aov"]["albedo"], "id": hi["aov"]["id"], "base": hi["rgba"],
               "sphere_select": sel}
        before = {k: v.clone() for k, v in ins.items()}
        want = sc.upsample(hi, lo, select={"sphere": sel})
        for variant in (0, 1):
            raw_o, out = _guarded(torch, (H, W, 4), torch.float32, None)
            raw_p, pix = _guarded(torch, (H, W), torch.int32, None)
            raw_s, src = _guarded(torch, (H, W), torch.uint8, None)
            for t in (out, pix, src):
                t.view(torch.uint8).fill_(0x5a)
            d = sc.upsample_desc(W, H, w, h, **{k: v.data_ptr() for k, v in ins.items()}, n_sphere_select=sel.numel(),
                                 use_tables=True, rgba_out=out.data_ptr(), pixels=pix.data_ptr(), source=src.data_ptr(),
                                 variant=variant)
            assert sc.upsample_raw(d, torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), want["rgba"].view(torch.int32))
            assert torch.equal(pix, want["packed"]) and torch.equal(src, want["source"])
            assert (src <= 2).all().item()
            assert _guards_intact(raw_o, H * W * 16) and _guards_intact(raw_p, H * W * 4) and _guards_intact(raw_s, H * W)
            for k, v in ins.items():
                assert torch.equal(v, before[k]), k
            # in place: rgba_out is base itself
            raw_b, buf = _guarded(torch, (H, W, 4), torch.float32, hi["rgba"])
            d.base = d.rgba_out = buf.data_ptr()
            assert sc.upsample_raw(d, torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(buf.view(torch.int32), want["rgba"].view(torch.int32))
            assert _guards_intact(raw_b, H * W * 16)
            # refusals write nothing
            for t in (out, pix, src):
                t.view(torch.uint8).fill_(0x5a)
            d.base = hi["rgba"].data_ptr()
            for kw in (dict(rgba_out=lo["rgba"].data_ptr()), dict(normal_shift=9), dict(lo_width=W + 1),
                       dict(pixels=out.data_ptr()), dict(n_sphere_select=-1), dict(depth=0)):
                d2 = rt.UpsampleDesc.from_buffer_copy(d)
                d2.rgba_out = out.data_ptr()
                for k, v in kw.items():
                    setattr(d2, k, v)
                assert sc.upsample_raw(d2, 0) == 1, kw
            torch.cuda.synchronize()
            for t in (out, pix, src):
                assert (t.view(torch.uint8) == 0x5a).all().item()
            assert torch.equal(lo["rgba"], before["rgba_lo"])


def test_a_capturing_stream_is_refused(rt, c2):
    import torch
    sc, inp = c2
    hi, lo = _pair(sc, inp, 128, 16, 64, 8)
    out = torch.full((16, 128, 4), SENTINEL, dtype=torch.int32, device="cuda")
    d = sc.upsample_desc(128, 16, 64, 8, rgba_lo=lo["rgba"].data_ptr(), depth_lo=lo["aov"]["depth"].data_ptr(),
                         normal_lo=lo["aov"]["normal"].data_ptr(), id_lo=lo["aov"]["id"].data_ptr(),
                         depth=hi["aov"]["depth"].data_ptr(), normal=hi["aov"]["normal"].data_ptr(),
                         id=hi["aov"]["id"].data_ptr(), rgba_out=out.data_ptr(), demodulate=False)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    x = torch.zeros(4, device="cuda")
    with torch.cuda.graph(g, stream=s):
        x.add_(1)
        rc = sc.upsample_raw(d, s.cuda_stream)
        msg = sc.lib.rt_last_error().decode()
    assert rc == 2 and "captured" in msg
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # and the scene still works
    assert sc.upsample_raw(d, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    want = sc.upsample(hi, lo, base=False, demodulate=False)
    assert np.array_equal(_bits(out.view(torch.float32)), _bits(want["rgba"]))


def test_a_side_stream_and_the_plain_frame(rt, gpu):
    """Render and upsample on one side stream, back to back, without a host wait; timed calls report one launch; the
    plain frame of the scene is the same bits before and after."""
    import torch
    inp = Inputs(rt, 1024)
    sc = inp.scene()
    try:
        sc.set_materials(list(mirror_k(1024)))
        W, H = 960, 540
        before = sc.render(W, H, cam=inp.cam, aspect=inp.aspect)
        want = sc.render_upscaled(W, H, 2, reflect_depth=2, cam=inp.cam, aspect=inp.aspect)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        sc.set_upsample_timing(True)
        with torch.cuda.stream(s1):
            a = sc.render_upscaled(W, H, 2, reflect_depth=2, cam=inp.cam, aspect=inp.aspect, stream=s1, want_parts=True)
        with torch.cuda.stream(s2):
            s2.wait_stream(s1)            # the frames are the caller's to order; the two upsample calls are the scene's
            b = sc.upsample(a["hi"], a["lo"], base=True, select=sc.upsample_select(), demodulate=False, variant=1, stream=s2)
        ms = sc.upsample_times()
        sc.set_upsample_timing(False)
        torch.cuda.synchronize()
        assert len(ms) == 1 and 0 < ms[0] < 100
        for r in (a, b):
            assert np.array_equal(_bits(r["rgba"]), _bits(want["rgba"])) and torch.equal(r["packed"], want["packed"])
            assert torch.equal(r["source"], want["source"])
        after = sc.render(W, H, cam=inp.cam, aspect=inp.aspect)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(after["rgba"]), _bits(before["rgba"])) and torch.equal(after["packed"], before["packed"])
        # a call that is not timed leaves no times behind
        sc.upsample(a["hi"], a["lo"], base=True, demodulate=False)
        assert sc.upsample_times() == []
    finally:
        sc.close()
