"""The bloom pass on the device (rt_scene_bloom). Every comparison is bit for bit, on rgba_out and
glow_out viewed as uint32 and on `pixels`: the product kernels (variant 0), the yardstick (variant 1) and the numpy
restatement (tests/bloom_ref.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bloom_ref as B
from bloom_ref import hand_frame
import display_ref as D
from postpass import ALL, SENTINEL, bits, scene as _scene, tensor_bits as _bits
from scenes import Inputs

pytestmark = pytest.mark.gpu

f32 = np.float32
# odd sizes straddling a tile edge at every level (65 x 33), one pixel wide or high, more than one tile each way
SIZES = [(1, 1), (2, 1), (3, 1), (1, 3), (70, 1), (1, 70), (65, 33), (50, 30), (130, 70)]
STATE = [0.75, 0.5, 0.25, 1.0]
KEYS = ("rgba", "pixels", "glow")


@pytest.fixture(scope="module")
def sc(rt, gpu):
    s = rt.Scene()
    yield s
    s.close()


class own_streams:
    """n HIP streams of the test's own, as raw handles, destroyed on the way out: a test that left streams behind
    would change which hardware queue the streams of later tests share with the null stream. torch never sees them, so
    whatever runs on them is given buffers that are ready and is waited for here."""

    def __init__(self, rt, n):
        self.hip, self.n, self.raw = rt.load_library(), n, []

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


def same(a, b, what):
    for k in KEYS:
        assert (a[k] is None) == (b[k] is None), (k, what)
        if a[k] is not None:
            x = _bits(a[k]) if not isinstance(a[k], np.ndarray) else (bits(a[k]) if a[k].dtype == f32 else a[k])
            y = _bits(b[k]) if not isinstance(b[k], np.ndarray) else (bits(b[k]) if b[k].dtype == f32 else b[k])
            diff = x != y
            assert not diff.any(), (k, what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def run(sc, rgba, state=None, ref=True, variants=(0, 1), **kw):
    """One call per variant, against each other and the restatement. Returns variant 0's dict and the restatement's."""
    import torch
    rgba_t = torch.from_numpy(np.ascontiguousarray(rgba)).cuda()
    st = None if state is None else torch.from_numpy(np.array(state, dtype=f32)).cuda()
    outs = [sc.bloom(rgba_t, st, want_glow=True, variant=v, **kw) for v in variants]
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rgba_t), bits(rgba))                        # the input is not written,
    assert st is None or st.tolist() == list(state)                         # nor the state
    for b in outs[1:]:
        same(outs[0], b, kw)
    want = None
    if ref:
        want = B.bloom(rgba, state, **kw)
        same(outs[0], want, kw)
    return outs[0], want


# ----------------------------------------------------------------------------- hand-made frames
@pytest.mark.parametrize("w,h", SIZES)
def test_hand_made_frames(sc, w, h):
    rgba = hand_frame(w, h, seed=w * 100 + h)
    glows, colours = set(), set()
    for levels, spread, strength, state in itertools.product((1, 2, 5, 8), (0.0, 0.75), (0.0, 0.125), (None, STATE)):
        a, want = run(sc, rgba, state, levels=levels, spread=spread, strength=strength)
        glows.add(bits(want["glow"]).tobytes())
        if strength:
            colours.add((bits(want["rgba"]).tobytes(), want["pixels"].tobytes()))
    if w * h >= 1500:
        # with spread 0 every A_k is B_k, whatever the levels, as with one level: per state one glow, and one each for
        # 2, 5 and 8 levels at spread 0.75
        assert len(glows) == 8 and len(colours) == 8
    run(sc, rgba, [2.0, 0, 0, 1.0], levels=3, threshold=0.25, limit=3.0, spread=4.0, strength=2.0)
    run(sc, rgba, [2.0, 0, 0, 0.5], levels=4, threshold=0.0, limit=2.0 ** -3)


# ----------------------------------------------------------------------------- placement
def test_a_single_bright_pixel_wherever_a_tile_ends(sc):
    """130 x 70, three levels: the corners, the middle, both sides of the multiples of 32 and 64 columns and of 4, 8
    and 16 rows that a tile of the product kernels can end at in level 0, and of level 1's seen from level 0."""
    w, h = 130, 70
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2),
             (31, 3), (32, 4), (63, 7), (64, 8), (63, 15), (64, 16), (127, 31), (128, 32), (129, 63), (127, 64), (128, 7)]
    back = hand_frame(w, h, seed=1, salt=False) * f32(2.0 ** -12)
    seen = set()
    for x, y in spots:
        rgba = back.copy()
        rgba[y, x, :3] = (40, 30, 20)
        a, want = run(sc, rgba, levels=3)
        glow = want["glow"][..., 0]
        assert glow[y, x] > 0 and (glow == 0).any()                           # and what it does not reach keeps its bits
        assert np.array_equal(bits(want["rgba"])[glow == 0], bits(rgba)[glow == 0])
        seen.add(bits(want["glow"]).tobytes())
    assert len(seen) == len(spots)


@pytest.mark.parametrize("which", ["last_row", "last_column"])
def test_a_bright_last_row_or_column_alone(sc, which):
    for w, h in ((130, 70), (65, 33)):
        rgba = hand_frame(w, h, seed=2, salt=False) * f32(2.0 ** -12)
        if which == "last_row":
            rgba[-1, :, :3] = 9
        else:
            rgba[:, -1, :3] = 9
        a, want = run(sc, rgba, levels=3)
        glow = want["glow"][..., 0]
        assert (glow[-1, :] > 0).all() if which == "last_row" else (glow[:, -1] > 0).all()
        assert not glow[0, 0] and not (glow[0, :] if which == "last_row" else glow[:, 0]).any()


# ----------------------------------------------------------------------------- the identities on a rendered frame
def test_identities_on_a_rendered_frame(rt, gpu):
    import torch
    inp = Inputs(rt, 256)
    s = _scene(rt, inp)
    frame = s.render(160, 90, cam=inp.cam, aspect=inp.aspect, aov=ALL)
    rgba = frame["rgba"].cpu().numpy()
    top = float(np.nanmax(B.luma(rgba)))
    for v in (0, 1):
        out = s.bloom(frame, threshold=2 * top + 1, want_glow=True, variant=v)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out["rgba"]), _bits(frame["rgba"]))
        assert np.array_equal(_bits(out["pixels"]), _bits(frame["packed"]))
        assert not out["glow"].any()
    # emissive spheres through emission_term, the default threshold: they bloom, and what they do not reach is itself
    tab = np.zeros((256, 3), dtype=f32)
    tab[::8] = (6.0, 5.0, 3.0)
    s.set_emission("sphere", tab)
    lit = (frame["rgba"] + s.emission_term(frame)).cpu().numpy()
    a, want = run(s, lit)
    assert (want["glow"][..., :3] > 0).any()
    # five levels reach the whole of 160 x 90; one level reaches three pixels, and with the threshold at half the
    # brightest luminance only the emitters' neighbourhoods
    lit_top = float(np.nanmax(B.luma(lit)))
    for kw in (dict(levels=1), dict(levels=1, threshold=lit_top / 2), dict(levels=2, threshold=lit_top / 2)):
        a, want = run(s, lit, **kw)
        glow = want["glow"][..., :3]
        still = (glow == 0).all(axis=-1)
        assert (glow > 0).any() and (still.any() or "threshold" not in kw)
        assert np.array_equal(_bits(a["rgba"])[still], bits(lit)[still])
        assert np.array_equal(_bits(a["pixels"])[still], B.pack(lit)[still])
    s.close()


# ----------------------------------------------------------------------------- outputs
def test_outputs_are_fully_overwritten_each_alone_and_in_place(sc):
    import torch
    w, h = 70, 9
    rgba = hand_frame(w, h, seed=6)
    rgba_t = torch.from_numpy(rgba).cuda()
    full, _ = run(sc, rgba, STATE, levels=3)
    st = torch.tensor(STATE, device="cuda")

    def raw(variant, out, px, glow, src=None):
        d = sc.bloom_desc(w, h, rgba_in=(rgba_t if src is None else src).data_ptr(), state=st.data_ptr(),
                          rgba_out=out.data_ptr() if out is not None else 0, pixels=px.data_ptr() if px is not None else 0,
                          glow_out=glow.data_ptr() if glow is not None else 0, levels=3, variant=variant)
        assert sc.bloom_raw(d, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()

    for variant in (0, 1):
        new = lambda: (torch.full((h, w, 4), float("nan"), device="cuda"),
                       torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda"),
                       torch.full((h, w, 4), float("nan"), device="cuda"))
        out, px, glow = new()
        raw(variant, out, px, glow)
        same(dict(rgba=out, pixels=px, glow=glow), full, variant)
        assert not torch.isnan(glow).any() and not (px == SENTINEL).any()
        # each output alone
        out, px, glow = new()
        raw(variant, out, None, None)
        assert np.array_equal(_bits(out), _bits(full["rgba"])) and (px == SENTINEL).all() and torch.isnan(glow).all()
        out, px, glow = new()
        raw(variant, None, px, None)
        assert np.array_equal(_bits(px), _bits(full["pixels"])) and torch.isnan(out).all() and torch.isnan(glow).all()
        out, px, glow = new()
        raw(variant, None, None, glow)
        assert np.array_equal(_bits(glow), _bits(full["glow"])) and torch.isnan(out).all() and (px == SENTINEL).all()
        # in place
        src = rgba_t.clone()
        _, px, glow = new()
        raw(variant, src, px, glow, src=src)
        same(dict(rgba=src, pixels=px, glow=glow), full, (variant, "in place"))
    assert np.array_equal(_bits(rgba_t), bits(rgba)) and st.tolist() == STATE


# ----------------------------------------------------------------------------- a long-lived scene, two streams
def test_a_long_lived_scene_on_two_streams_equals_fresh_scenes(rt, gpu):
    """Twenty calls whose pyramid grows and shrinks, alternating between two streams of the test's own."""
    import torch
    old = rt.Scene()
    old.set_bloom_timing(True)
    shapes = [(50, 30), (1, 1), (300, 200), (64, 4), (70, 1), (130, 70), (3, 1), (301, 201), (65, 33), (2, 1)]
    frames = [hand_frame(w, h, seed=20 + i) for i, (w, h) in enumerate(shapes)]
    calls = [(f, (1, 5, 8, 2, 3)[(f + v) % 5], v) for f in range(len(frames)) for v in (0, 1)]
    tensors = [torch.from_numpy(r).cuda() for r in frames]
    got = []
    for f, levels, variant in calls:
        h, w = frames[f].shape[:2]
        got.append(dict(rgba=torch.full((h, w, 4), float("nan"), device="cuda"),
                        pixels=torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda"),
                        glow=torch.full((h, w, 4), float("nan"), device="cuda")))
    torch.cuda.synchronize()                                     # every buffer is ready before a stream of ours reads it
    streams = own_streams(rt, 2)
    with streams as raw:
        for n, ((f, levels, variant), o) in enumerate(zip(calls, got)):
            r = tensors[f]
            d = old.bloom_desc(r.shape[1], r.shape[0], rgba_in=r.data_ptr(), rgba_out=o["rgba"].data_ptr(),
                               pixels=o["pixels"].data_ptr(), glow_out=o["glow"].data_ptr(), levels=levels, variant=variant)
            assert old.bloom_raw(d, raw[n % 2]) == 0
        streams.sync()
        assert len(old.bloom_times()) == 2 * calls[-1][1]
    assert len(calls) == 20
    for (f, levels, variant), out in zip(calls, got):
        fresh = rt.Scene()
        want = fresh.bloom(tensors[f], levels=levels, variant=variant, want_glow=True)
        torch.cuda.synchronize()
        same(out, want, (f, levels, variant))
        fresh.close()
    for levels in (1, 4, 8):
        for variant in (0, 1):
            old.bloom(tensors[0], levels=levels, variant=variant)
            times = old.bloom_times()
            assert len(times) == 2 * levels and all(t >= 0 for t in times)
    old.set_bloom_timing(False)
    old.bloom(tensors[0])
    assert old.bloom_times() == []
    old.close()


# ----------------------------------------------------------------------------- more than one pass of the product's grids
@pytest.mark.parametrize("w,h", [(1030, 260)])
def test_a_frame_beyond_one_pass_of_the_grid(sc, w, h):
    rgba = hand_frame(w, h, seed=10)
    run(sc, rgba, STATE, levels=3)


# ----------------------------------------------------------------------------- refusals
def test_refusals_and_a_capturing_stream_write_nothing(rt, gpu):
    import torch
    lib = rt.load_library()
    s = rt.Scene()
    w, h = 50, 30
    rgba = hand_frame(w, h, seed=9)
    rgba_t = torch.from_numpy(rgba).cuda()
    out = torch.full((h, w, 4), float("nan"), device="cuda")
    px = torch.full((h, w), SENTINEL, dtype=torch.int32, device="cuda")
    glow = torch.full((h, w, 4), float("nan"), device="cuda")
    st = torch.tensor(STATE, device="cuda")

    def desc(**kw):
        base = dict(rgba_in=rgba_t.data_ptr(), state=st.data_ptr(), rgba_out=out.data_ptr(), pixels=px.data_ptr(),
                    glow_out=glow.data_ptr())
        base.update(kw)
        return s.bloom_desc(base.pop("width", w), base.pop("height", h), **base)

    def untouched():
        torch.cuda.synchronize()
        return (torch.isnan(out).all() and (px == SENTINEL).all() and torch.isnan(glow).all() and st.tolist() == STATE
                and np.array_equal(_bits(rgba_t), bits(rgba)))
    for kw in (dict(width=0), dict(height=32769), dict(rgba_in=0), dict(levels=0), dict(levels=9), dict(variant=2),
               dict(threshold=-1.0), dict(threshold=float("nan")), dict(limit=0.0), dict(limit=float("inf")),
               dict(spread=4.5), dict(spread=float("nan")), dict(strength=-1.0), dict(strength=float("inf")),
               dict(rgba_out=0, pixels=0, glow_out=0), dict(rgba_out=rgba_t.data_ptr() + 16), dict(pixels=out.data_ptr()),
               dict(glow_out=rgba_t.data_ptr()), dict(glow_out=st.data_ptr()), dict(state=st.data_ptr() + 4),
               dict(rgba_in=rgba_t.data_ptr() + 8), dict(pixels=px.data_ptr() + 2), dict(glow_out=out.data_ptr() + 32)):
        assert s.bloom_raw(desc(**kw)) == 1, kw
        assert lib.rt_last_error().decode().startswith("rt_scene_bloom: ")
        assert untouched(), kw
    torch.cuda.synchronize()
    with own_streams(rt, 1) as (cap,):
        graph = C.c_void_p()
        assert lib.hipStreamBeginCapture(C.c_void_p(cap), 2) == 0                      # hipStreamCaptureModeRelaxed
        rcs = [s.bloom_raw(desc(levels=n, variant=v), cap) for n in (1, 5) for v in (0, 1)]
        message = lib.rt_last_error().decode()
        assert lib.hipStreamEndCapture(C.c_void_p(cap), C.byref(graph)) == 0
        assert lib.hipGraphDestroy(graph) == 0
    assert rcs == [2] * 4 and "captured" in message
    assert untouched()
    assert s.bloom_raw(desc()) == 0                                       # and the scene still works
    torch.cuda.synchronize()
    same(dict(rgba=out, pixels=px, glow=glow), B.bloom(rgba, STATE), "after the refusals")
    s.close()


# ----------------------------------------------------------------------------- end to end
def test_the_half_resolution_pipeline_through_bloom_and_display(rt, gpu):
    """The README's pipeline with emissive spheres over three frames: bloom and display equal their restatements applied
    to the device's float input, the bloom on the scale of the exposure the display's state holds."""
    import torch
    T = D.table(rt)
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
        before = None if shown is None else shown["state"].cpu().numpy().copy()
        glow = s.bloom(out, shown["state"] if shown else None, want_glow=True)
        shown = s.display({"rgba": glow["rgba"], "aov": hi["aov"]}, shown["state"] if shown else None, meter="lagged", adapt=0.1)
        torch.cuda.synchronize()
        want = B.bloom(out.cpu().numpy(), before)
        same(glow, want, frame_number)
        assert (want["glow"] > 0).any() and want["t"] == (f32(1) if before is None else f32(1) / before[0])
        shows = D.display(want["rgba"], np.zeros(4, dtype=f32) if before is None else before, hi["aov"]["id"].cpu().numpy(), T,
                          meter="lagged", adapt=0.1)
        assert np.array_equal(_bits(shown["pixels"]), shows["pixels"]), frame_number
        assert np.array_equal(_bits(shown["rgba"]), bits(shows["rgba"])) and np.array_equal(_bits(shown["state"]), bits(shows["state"]))
    s.close()
