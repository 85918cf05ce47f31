"""The display transform on the device (rt_scene_display). Every comparison is bit for bit, on rgba_out
viewed as uint32, on `pixels`, on the state and on the histogram: the product kernels (variant 0), the yardstick
(variant 1) and the numpy restatement (tests/display_ref.py), which takes its thresholds from the library."""
import ctypes as C
import itertools

import numpy as np
import pytest

import display_ref as D
from postpass import ALL, SENTINEL, bits, scene as _scene, tensor_bits as _bits
from scenes import Inputs

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [(1, 1), (3, 1), (70, 1), (1, 70), (64, 4), (50, 30)]
METERS, CURVES, TRANSFERS = ("auto", "lagged", "manual"), ("clip", "reinhard", "aces"), ("linear", "srgb")
SALT = np.array([0.0, -0.0, -0.75, 2.0 ** -140, 1e30, np.inf, -np.inf, np.nan], dtype=f32)


@pytest.fixture(scope="module")
def sc(rt, gpu):
    s = rt.Scene()
    yield s
    s.close()


@pytest.fixture(scope="module")
def T(rt):
    return D.table(rt)


class own_streams:
    """n HIP streams of the test's own, as raw handles, destroyed on the way out: a test that left streams behind
    would change which hardware queue the streams of later tests share with the null stream. torch never sees them (its
    allocator keeps what it has seen for good), so whatever runs on them is given buffers that are ready and is waited
    for here."""

    def __init__(self, rt, n):
        self.hip, self.n, self.raw = rt.load_library(), n, []          # the HIP runtime the library is linked against

    def __enter__(self):
        for _ in range(self.n):
            st = C.c_void_p()
            assert self.hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0   # hipStreamNonBlocking
            self.raw.append(st)
        return [st.value for st in self.raw]

    def sync(self):
        for st in self.raw:
            assert self.hip.hipStreamSynchronize(st) == 0

    def __exit__(self, *exc):
        self.sync()
        for st in self.raw:
            assert self.hip.hipStreamDestroy(st) == 0
        return False


def hand_frame(w, h, seed=0, salt=True):
    """Luminances log-normal over 2^-20 .. 2^20 with a tint per channel, salted with 0, -0, negatives, a subnormal,
    10^30, +-inf and NaN (in single channels and in whole pixels); alpha of every kind; ids with a fifth sky."""
    rng = np.random.default_rng(seed)
    l = np.exp2(np.clip(rng.normal(0, 7, (h, w, 1)), -20, 20))
    rgba = np.concatenate([l * rng.uniform(0.5, 1.5, (h, w, 3)), rng.uniform(-1, 2, (h, w, 1))], axis=-1).astype(f32)
    if salt:
        flat = rgba.reshape(-1, 4)
        n = flat.shape[0]
        for i, v in enumerate(SALT):
            flat[(3 * i + 1) % n, i % 4] = v                      # one channel
            if n >= 16:
                flat[(5 * i + 7) % n, :3] = v                     # the whole colour
    ids = np.stack([rng.integers(-1, 4, (h, w)), rng.integers(0, 9, (h, w))], axis=-1).astype(np.int32)
    return rgba, ids


def run(sc, T, rgba, ids=None, state=None, ref=True, variants=(0, 1), **kw):
    """One call per variant on copies of `state`, against each other and the restatement. Returns variant 0's dict
    (state included) and the restatement's."""
    import torch
    rgba_t = torch.from_numpy(np.ascontiguousarray(rgba)).cuda()
    frame = rgba_t if ids is None else {"rgba": rgba_t, "aov": {"id": torch.from_numpy(np.ascontiguousarray(ids)).cuda()}}
    manual = kw.get("meter", "auto") == "manual"
    outs = []
    for v in variants:
        st = None if state is None or manual else torch.from_numpy(np.array(state, dtype=f32)).cuda()
        outs.append(sc.display(frame, st, want_histogram=True, variant=v, **kw))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rgba_t), bits(rgba))                        # the input is not written
    a = outs[0]
    for b in outs[1:]:
        for k in ("rgba", "pixels", "state", "histogram"):
            assert (a[k] is None) == (b[k] is None), (k, kw)
            if a[k] is not None:
                diff = _bits(a[k]) != _bits(b[k])
                assert not diff.any(), (k, kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    want = None
    if ref:
        rkw = dict(kw)
        if "window" in rkw:
            rkw["meter_low"], rkw["meter_high"] = rkw.pop("window")
        if "limits" in rkw:
            rkw["min_exposure"], rkw["max_exposure"] = rkw.pop("limits")
        want = D.display(rgba, state, ids, T, **rkw)
        diff = (_bits(a["rgba"]) != bits(want["rgba"])).any(axis=-1)
        assert not diff.any(), (kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        diff = _bits(a["pixels"]) != want["pixels"]
        assert not diff.any(), (kw, int(diff.sum()), np.argwhere(diff)[:4].tolist())
        if manual:
            assert a["state"] is None and a["histogram"] is None
        else:
            assert np.array_equal(_bits(a["state"]), bits(want["state"])), (kw, a["state"].tolist(), want["state"].tolist())
            h = a["histogram"].cpu().numpy()
            assert np.array_equal(h, want["histogram"] if want["histogram"] is not None else np.zeros(D.BINS, dtype=np.int64))
    return a, want


# ----------------------------------------------------------------------------- identity
def test_identity_on_a_rendered_frame(rt, gpu, T):
    """MANUAL, exposure 1, CLIP, LINEAR: the frame's own rgba bits and its own packed words."""
    import torch
    inp = Inputs(rt, 256)
    s = _scene(rt, inp)
    frame = s.render(160, 90, cam=inp.cam, aspect=inp.aspect, aov=ALL)
    for v in (0, 1):
        out = s.display(frame, meter="manual", exposure=1.0, curve="clip", transfer="linear", variant=v)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out["rgba"]), _bits(frame["rgba"]))
        assert np.array_equal(_bits(out["pixels"]), _bits(frame["packed"]))
        assert out["state"] is None and out["histogram"] is None
    # and the metered frame: the sky is left out through the id guide
    ids = frame["aov"]["id"].cpu().numpy()
    a, want = run(s, T, frame["rgba"].cpu().numpy(), ids)
    assert (ids[..., 0] < 0).any() and 0 < want["state"][2] < 1
    assert int(a["histogram"].sum()) == int(((ids[..., 0] >= 0) & (D.bins(D.luma(frame["rgba"].cpu().numpy())) >= 0)).sum())
    s.close()


# ----------------------------------------------------------------------------- hand-made frames
@pytest.mark.parametrize("w,h", SIZES)
def test_hand_made_frames(sc, T, w, h):
    rgba, ids = hand_frame(w, h, seed=w * 100 + h)
    seen = set()
    for meter, curve, transfer in itertools.product(METERS, CURVES, TRANSFERS):
        for state in (None, [0.75, 0.5, 0.25, 1.0]):
            a, want = run(sc, T, rgba, ids, state, meter=meter, curve=curve, transfer=transfer, exposure=1.5, adapt=0.5)
            seen.add((bits(want["rgba"]).tobytes(), want["pixels"].tobytes()))
    if w * h >= 64:
        # auto and lagged: 3 curves x 2 transfers x 2 states each; manual's six are lagged's without a state (E = exposure)
        assert len(seen) == 24
    run(sc, T, rgba, ids, window=(0, 1024), limits=(0.5, 2.0), key=0.5, white=1.5, meter_sky=True, curve="reinhard")
    run(sc, T, rgba, None, [2.0, 0, 0, 1.0], window=(1000, 1001), adapt=2.0 ** -10, meter="lagged")


def test_codes_at_every_threshold_on_the_device(sc, T):
    """CLIP and SRGB on T[v] and its predecessor in each channel: the search and the count agree with v and v - 1."""
    below = np.nextafter(T, f32(-1))
    rgba = np.zeros((2, 256, 4), dtype=f32)
    rgba[0, :, 0], rgba[0, :, 1], rgba[0, :, 2] = T, below, T[::-1]
    rgba[1, :, 0], rgba[1, :, 1], rgba[1, :, 2] = below[::-1], T, below
    a, want = run(sc, T, rgba, meter="manual", curve="clip")
    v = np.arange(256)
    px = _bits(a["pixels"])
    assert np.array_equal(px[0] >> 16, v) and np.array_equal((px[0] >> 8) & 255, np.maximum(v - 1, 0))
    assert np.array_equal(px[0] & 255, v[::-1]) and np.array_equal((px[1] >> 8) & 255, v)


# ----------------------------------------------------------------------------- wave patterns for the histogram
def _pattern(name, n=64 * 12):
    """Luminances of n pixels in one row: 0 = not metered."""
    l = np.zeros(n, dtype=f32)
    lane, wave = np.arange(n) % 64, np.arange(n) // 64
    rng = np.random.default_rng(11)
    some = np.exp2(rng.uniform(-18, 18, n)).astype(f32)
    if name == "lane0":
        l[64 * 5] = 3.0
    elif name == "lane63":
        l[64 * 5 + 63] = 3.0
    elif name == "alternating":
        l[lane % 2 == 0] = some[lane % 2 == 0]
    elif name == "empty_wave_between":
        l[wave != 6] = some[wave != 6]
    elif name == "one_bin":
        l[:] = 1.0 + rng.uniform(0, 1 / 32, n).astype(f32)
    elif name == "lane_per_bin":
        k = (lane * 8 + wave % 8).astype(np.uint32)                  # the middle of bin k, by its bits
        l[:] = (((D.BIN0 + k) << 19) + (1 << 18)).astype(np.uint32).view(f32)
    return l


@pytest.mark.parametrize("name", ["lane0", "lane63", "alternating", "empty_wave_between", "one_bin", "lane_per_bin"])
def test_wave_patterns(sc, T, name):
    l = _pattern(name)
    rgba = np.stack([l, l, l, np.ones_like(l)], axis=-1)[None]
    for meter in ("auto", "lagged"):
        a, want = run(sc, T, rgba, meter=meter)
        h = a["histogram"].cpu().numpy()
        assert h.sum() == (l > 0).sum()
        if name == "one_bin":
            assert h[256] == l.size
        if name == "lane_per_bin":
            k = D.bins(D.luma(rgba))[0]
            assert all(len(set(k[i:i + 64])) == 64 for i in range(0, l.size, 64))


# ----------------------------------------------------------------------------- the id mask, N == 0
def test_the_id_mask(sc, T):
    rgba, ids = hand_frame(50, 30, seed=3)
    a, w0 = run(sc, T, rgba, ids)
    b, w1 = run(sc, T, rgba, ids, meter_sky=True)
    c, w2 = run(sc, T, rgba, None)
    assert w0["histogram"].sum() < w1["histogram"].sum() and np.array_equal(w1["histogram"], w2["histogram"])
    assert w0["state"][2] < w1["state"][2] == w2["state"][2]
    assert np.array_equal(_bits(b["rgba"]), _bits(c["rgba"]))


@pytest.mark.parametrize("kind", ["sky", "nan"])
@pytest.mark.parametrize("meter", ["auto", "lagged"])
def test_nothing_metered(sc, T, kind, meter):
    rgba, ids = hand_frame(50, 30, seed=4, salt=False)
    if kind == "sky":
        ids[..., 0] = -1
    else:
        rgba[..., 1] = np.nan
    for state, e in (([0.375, 2.0, 0.5, 1.0], 0.375), (None, 1.75), ([0.375, 2.0, 0.5, 0.0], 1.75)):
        a, want = run(sc, T, rgba, ids, state, meter=meter, exposure=1.75, curve="clip")
        assert a["state"].tolist() == [e, 0, 0, 1] and int(a["histogram"].sum()) == 0 and want["E"] == f32(e)


# ----------------------------------------------------------------------------- adaptation
@pytest.mark.parametrize("meter", ["auto", "lagged"])
def test_adaptation_over_six_calls(sc, T, meter):
    import torch
    dark, _ = hand_frame(50, 30, seed=5, salt=False)
    bright = (dark * f32(64)).astype(f32)
    dark = (dark * f32(1 / 64)).astype(f32)
    state_t = None
    state = np.zeros(4, dtype=f32)
    seen = []
    for k in range(6):
        rgba = dark if k % 2 == 0 else bright
        out = sc.display(torch.from_numpy(rgba).cuda(), state_t, meter=meter, adapt=0.25)
        want = D.display(rgba, state, None, T, meter=meter, adapt=0.25)
        man = sc.display(torch.from_numpy(rgba).cuda(), meter="manual", exposure=float(want["E"]))
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out["state"]), bits(want["state"])), k
        assert np.array_equal(_bits(out["rgba"]), bits(want["rgba"])) and np.array_equal(_bits(out["pixels"]), want["pixels"])
        assert np.array_equal(_bits(out["rgba"]), _bits(man["rgba"])) and np.array_equal(_bits(out["pixels"]), _bits(man["pixels"]))
        if meter == "lagged":                      # shown with the exposure the state held before the call
            assert want["E"] == (state[0] if k else f32(1))
        state_t, state = out["state"], want["state"]
        seen.append(float(state[0]))
    assert len(set(seen)) == 6 and seen[0] > seen[1] and seen[2] > seen[1]      # it follows the frames, a quarter of the way


# ----------------------------------------------------------------------------- outputs
def test_outputs_are_fully_overwritten_and_each_alone(sc, T):
    import torch
    w, h = 70, 9
    rgba, ids = hand_frame(w, h, seed=6)
    rgba_t, ids_t = torch.from_numpy(rgba).cuda(), torch.from_numpy(ids).cuda()
    full, _ = run(sc, T, rgba, ids, [0.5, 0, 0, 1.0], meter="lagged")

    def raw(variant, out, px, state, hist, meter=2, src=None):
        d = sc.display_desc(w, h, rgba_in=(rgba_t if src is None else src).data_ptr(), id=ids_t.data_ptr(),
                            rgba_out=out.data_ptr() if out is not None else 0, pixels=px.data_ptr() if px is not None else 0,
                            state=state.data_ptr(), histogram_out=hist.data_ptr() if hist is not None else 0, meter=meter,
                            variant=variant)
        assert sc.display_raw(d, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()

    for variant in (0, 1):
        new = lambda: (torch.full((h, w, 4), float("nan"), device="cuda"),
                       torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda"),
                       torch.tensor([0.5, 0, 0, 1.0], device="cuda"),
                       torch.full((D.BINS,), SENTINEL, dtype=torch.int32, device="cuda"))
        out, px, st, hist = new()
        raw(variant, out, px, st, hist)
        for got, want in ((out, full["rgba"]), (px, full["pixels"]), (st, full["state"]), (hist, full["histogram"])):
            assert np.array_equal(_bits(got), _bits(want)), variant
        # each output alone
        out, px, st, hist = new()
        raw(variant, out, None, st, None)
        assert np.array_equal(_bits(out), _bits(full["rgba"])) and (px == SENTINEL).all() and (hist == SENTINEL).all()
        out, px, st, hist = new()
        raw(variant, None, px, st, None)
        assert np.array_equal(_bits(px), _bits(full["pixels"])) and torch.isnan(out).all()
        assert np.array_equal(_bits(st), _bits(full["state"]))
        # a meter-only call writes nothing but state and histogram, under both metering modes
        for meter in (1, 2):
            out, px, st, hist = new()
            raw(variant, None, None, st, hist, meter=meter)
            assert np.array_equal(_bits(st), _bits(full["state"])) and np.array_equal(_bits(hist), _bits(full["histogram"]))
            assert torch.isnan(out).all() and (px == SENTINEL).all()
        # in place
        for meter in (1, 2):
            src = rgba_t.clone()
            _, px, st, hist = new()
            raw(variant, src, px, st, hist, meter=meter, src=src)
            ref, _ = run(sc, T, rgba, ids, [0.5, 0, 0, 1.0], meter=("auto", "lagged")[meter - 1], variants=(0,))
            assert np.array_equal(_bits(src), _bits(ref["rgba"])) and np.array_equal(_bits(px), _bits(ref["pixels"]))
            assert np.array_equal(_bits(st), _bits(ref["state"]))
    assert np.array_equal(_bits(rgba_t), bits(rgba))


def test_two_calls_back_to_back_each_get_their_histogram(sc, T):
    import torch
    a, _ = hand_frame(64, 40, seed=7)
    b, _ = hand_frame(50, 30, seed=8)
    b = (b * f32(8)).astype(f32)
    for variant in (0, 1):
        outs = [sc.display(torch.from_numpy(x).cuda(), want_histogram=True, variant=variant, meter=m)
                for x, m in ((a, "auto"), (b, "lagged"), (a, "lagged"), (b, "auto"))]
        torch.cuda.synchronize()
        for out, x in zip(outs, (a, b, a, b)):
            h = D.histogram(x)
            assert np.array_equal(out["histogram"].cpu().numpy(), h)
            assert int(out["histogram"].sum()) == int((D.bins(D.luma(x)) >= 0).sum())


# ----------------------------------------------------------------------------- a long-lived scene, two streams
def test_a_long_lived_scene_on_two_streams_equals_fresh_scenes(rt, gpu, T):
    import torch
    old = rt.Scene()
    old.set_display_timing(True)
    frames = [hand_frame(w, h, seed=20 + i) for i, (w, h) in enumerate([(50, 30), (1, 1), (300, 200), (64, 4), (70, 1)])]
    calls = list(itertools.product(range(len(frames)), (1, 2, 0), (0, 1)))        # AUTO, LAGGED, MANUAL
    tensors = [(torch.from_numpy(r).cuda(), torch.from_numpy(i).cuda()) for r, i in frames]
    got = []
    for f, meter, variant in calls:
        h, w = frames[f][0].shape[:2]
        got.append(dict(rgba=torch.full((h, w, 4), float("nan"), device="cuda"),
                        pixels=torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda"),
                        state=torch.tensor([0.5, 0, 0, 1.0], device="cuda"),
                        histogram=torch.zeros(D.BINS, dtype=torch.int32, device="cuda")))
    torch.cuda.synchronize()                                     # every buffer is ready before a stream of ours reads it
    streams = own_streams(rt, 2)
    with streams as raw:
        for n, ((f, meter, variant), o) in enumerate(zip(calls, got)):
            r, i = tensors[f]
            d = old.display_desc(r.shape[1], r.shape[0], rgba_in=r.data_ptr(), id=i.data_ptr(), rgba_out=o["rgba"].data_ptr(),
                                 pixels=o["pixels"].data_ptr(), state=o["state"].data_ptr(),
                                 histogram_out=o["histogram"].data_ptr(), meter=meter, variant=variant)
            assert old.display_raw(d, raw[n % 2]) == 0
        streams.sync()
        assert len(old.display_times()) == 1                     # the last call: MANUAL
    for (f, meter, variant), out in zip(calls, got):
        fresh = rt.Scene()
        r, i = tensors[f]
        state = None if meter == 0 else torch.tensor([0.5, 0, 0, 1.0], device="cuda")
        want = fresh.display({"rgba": r, "aov": {"id": i}}, state, meter=("manual", "auto", "lagged")[meter], variant=variant,
                             want_histogram=True)
        torch.cuda.synchronize()
        for k in ("rgba", "pixels", "state", "histogram"):
            if want[k] is not None:
                assert np.array_equal(_bits(out[k]), _bits(want[k])), (f, meter, variant, k)
        if meter == 0:                                           # MANUAL touches neither
            assert out["state"].tolist() == [0.5, 0, 0, 1.0] and not out["histogram"].any()
        fresh.close()
    for meter, n in (("auto", 3), ("lagged", 2)):
        old.display(tensors[0][0], meter=meter)
        assert len(old.display_times()) == n
    old.close()


# ----------------------------------------------------------------------------- refusals
def test_refusals_and_a_capturing_stream_write_nothing(rt, gpu, T):
    import torch
    lib = rt.load_library()
    s = rt.Scene()
    w, h = 50, 30
    rgba, ids = hand_frame(w, h, seed=9)
    rgba_t, ids_t = torch.from_numpy(rgba).cuda(), torch.from_numpy(ids).cuda()
    out = torch.full((h, w, 4), float("nan"), device="cuda")
    px = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.tensor([0.5, 7.0, 7.0, 1.0], device="cuda")
    hist = torch.full((D.BINS,), SENTINEL, dtype=torch.int32, device="cuda")

    def desc(**kw):
        base = dict(rgba_in=rgba_t.data_ptr(), id=ids_t.data_ptr(), rgba_out=out.data_ptr(), pixels=px.data_ptr(),
                    state=st.data_ptr(), histogram_out=hist.data_ptr())
        base.update(kw)
        return s.display_desc(base.pop("width", w), base.pop("height", h), **base)

    def untouched():
        torch.cuda.synchronize()
        return (torch.isnan(out).all() and (px == SENTINEL).all() and (hist == SENTINEL).all()
                and st.tolist() == [0.5, 7.0, 7.0, 1.0] and np.array_equal(_bits(rgba_t), bits(rgba)))
    for kw in (dict(width=0), dict(rgba_in=0), dict(state=0), dict(meter=3), dict(curve=-1), dict(transfer=2), dict(variant=2),
               dict(exposure=float("nan")), dict(key=0.0), dict(min_exposure=2.0, max_exposure=1.0), dict(meter_low=973),
               dict(adapt=0.0), dict(white=float("inf")), dict(rgba_out=rgba_t.data_ptr() + 16), dict(pixels=out.data_ptr()),
               dict(state=rgba_t.data_ptr()), dict(histogram_out=px.data_ptr()), dict(id=ids_t.data_ptr() + 4),
               dict(meter=0, rgba_out=0, pixels=0)):
        assert s.display_raw(desc(**kw)) == 1, kw
        assert untouched(), kw
    torch.cuda.synchronize()
    with own_streams(rt, 1) as (cap,):
        graph = C.c_void_p()
        assert lib.hipStreamBeginCapture(C.c_void_p(cap), 2) == 0                      # hipStreamCaptureModeRelaxed
        rcs = [s.display_raw(desc(meter=m, variant=v), cap) for m in (0, 1, 2) for v in (0, 1)]
        message = lib.rt_last_error().decode()
        assert lib.hipStreamEndCapture(C.c_void_p(cap), C.byref(graph)) == 0
        assert lib.hipGraphDestroy(graph) == 0
    assert rcs == [2] * 6 and "captured" in message
    assert untouched()
    assert s.display_raw(desc()) == 0                                     # and the scene still works
    torch.cuda.synchronize()
    want = D.display(rgba, [0.5, 7.0, 7.0, 1.0], ids, T)
    assert np.array_equal(_bits(out), bits(want["rgba"])) and np.array_equal(_bits(px), want["pixels"])
    assert np.array_equal(_bits(st), bits(want["state"])) and np.array_equal(hist.cpu().numpy(), want["histogram"])
    s.close()


# ----------------------------------------------------------------------------- more than one pass of the product's grid
def test_a_frame_beyond_one_pass_of_the_grid(sc, T):
    """1024 x 1030 is 4120 workgroups of 256 pixels: beyond the apply pass's 4096 and four times the metering passes'
    1024, so every strided loop goes round again (1024 x 520, the indirect suite's size, would pass the first only)."""
    rgba, ids = hand_frame(1024, 1030, seed=10)
    for meter in ("manual", "auto", "lagged"):
        a, _ = run(sc, T, rgba, ids, [0.25, 0, 0, 1.0], ref=False, meter=meter)
    want = D.display(rgba, [0.25, 0, 0, 1.0], ids, T, meter="lagged")
    assert np.array_equal(_bits(a["pixels"]), want["pixels"]) and np.array_equal(_bits(a["state"]), bits(want["state"]))
    assert np.array_equal(_bits(a["rgba"]), bits(want["rgba"]))
    assert np.array_equal(a["histogram"].cpu().numpy(), want["histogram"])


# ----------------------------------------------------------------------------- end to end
def test_the_half_resolution_pipeline_ends_in_display(rt, gpu, T):
    """The README's pipeline with an emissive sphere: pixels equals the restatement applied to the device's float input."""
    import torch
    inp = Inputs(rt, 64)
    s = _scene(rt, inp)
    tab = np.zeros((64, 3), dtype=f32)
    tab[::8] = (6.0, 5.0, 3.0)
    s.set_emission("sphere", tab)
    W, H = 160, 90
    kw = dict(cam=inp.cam, aspect=inp.aspect, aov=ALL)
    history, shown = None, None
    for frame_number in range(3):
        hi = s.render(W, H, **kw)
        lo = s.render(W // 2, H // 2, **kw)
        ind = s.indirect_paths(lo, bounces=2, rays=1, ray_base=frame_number, cam=inp.cam, aspect=inp.aspect)
        up = s.upsample(hi, lo, colour=ind["rgba"], base=True, demodulate=True)
        history = s.temporal(hi, history, colour=up["rgba"], cam=inp.cam, aspect=inp.aspect)
        out = s.denoise({"rgba": history["rgba"], "aov": hi["aov"]})["rgba"] + s.emission_term(hi)
        before = np.zeros(4, dtype=f32) if shown is None else shown["state"].cpu().numpy().copy()
        shown = s.display({"rgba": out, "aov": hi["aov"]}, shown["state"] if shown else None, meter="lagged", adapt=0.1)
        torch.cuda.synchronize()
        want = D.display(out.cpu().numpy(), before, hi["aov"]["id"].cpu().numpy(), T, meter="lagged", adapt=0.1)
        assert np.array_equal(_bits(shown["pixels"]), want["pixels"]), frame_number
        assert np.array_equal(_bits(shown["rgba"]), bits(want["rgba"])) and np.array_equal(_bits(shown["state"]), bits(want["state"]))
    assert (out[..., :3] > 1).any() and 0 < float(shown["state"][2]) <= 1
    s.close()
