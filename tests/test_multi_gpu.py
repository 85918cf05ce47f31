"""The multi-device frame path (csrc/rt_multi.hip) at its edges, in one process on one device: several shares are the
same device several times with RT_MULTI_PEER_COPY, one share with RT_MULTI_RCCL runs the in-place one-rank gather.
Everything is bit-exact. The expected frame is the single-scene frame of the same description (which other suites pin
to the oracle); the smallest case of each family is held to the oracle directly as well. The exchange itself is
checked against tests/multi_ref.py, a plain numpy model written from the header (tests/test_multi_ref_cpu.py)."""
import ctypes as C
import time

import numpy as np
import pytest

import meshes
import multi_ref
from scenes import Inputs, mixed_scene

pytestmark = pytest.mark.gpu

RCCL, PEER = 1, 2
POISON = 0xDEADBEEF
SHARES = [(2, PEER), (3, PEER), (5, PEER), (8, PEER), (1, RCCL)]


def _poisoned(h, w):
    import torch
    return torch.full((h, w), POISON - (1 << 32), dtype=torch.int32, device="cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _rows_that_differ(got, want):
    return [int(y) for y in np.nonzero((got != want).any(axis=1))[0]]


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), "%s: rows %s differ" % (what, _rows_that_differ(got, want))


def _set_scene(lib, m, inp):
    fp = C.POINTER(C.c_float)
    ptr = lambda a: a.ctypes.data_as(fp)
    assert lib.rt_multi_set_spheres(m, inp.spheres, inp.n) == 0, lib.rt_last_error()
    h, w = inp.tex[0].shape
    assert lib.rt_multi_set_texture(m, ptr(inp.tex[0]), ptr(inp.tex[1]), ptr(inp.tex[2]), w, h) == 0
    h, w = inp.sky[0].shape
    assert lib.rt_multi_set_sky(m, C.byref(inp.sky_box), ptr(inp.sky[0]), ptr(inp.sky[1]), ptr(inp.sky[2]), w, h) == 0
    assert lib.rt_multi_set_lights(m, inp.lights, inp.n_lights) == 0


class Pool:
    """One rt_multi per (shares, transport), made when a test first asks for it and kept for the module; each holds the
    default scene of 256 spheres, and a test that changes it puts it back."""

    def __init__(self, rt):
        self.rt, self.lib = rt, rt.load_library()
        self.inp = Inputs(rt, 256)
        self.made, self.setup_s = {}, {}
        self.descs = rt.Scene()               # frame descriptions only: it renders nothing

    def get(self, shares, transport):
        key = (shares, transport)
        if key not in self.made:
            m = C.c_void_p()
            devs = (C.c_int * shares)(*([0] * shares))
            t0 = time.perf_counter()
            assert self.lib.rt_multi_create_ex(devs, shares, transport, C.byref(m)) == 0, self.lib.rt_last_error()
            self.setup_s[key] = time.perf_counter() - t0
            self.made[key] = m
            assert self.lib.rt_multi_device_count(m) == shares and self.lib.rt_multi_transport(m) == transport
            _set_scene(self.lib, m, self.inp)
        return self.made[key]

    def fd(self, w, h, **kw):
        return self.descs.frame_desc(w, h, **kw)

    def render(self, m, fd, out=None):
        return self.lib.rt_multi_render(m, C.byref(fd), out.data_ptr() if out is not None else None)

    def error(self):
        return self.lib.rt_last_error().decode(errors="replace")

    def sync(self, m):
        import torch
        assert self.lib.rt_multi_sync(m) == 0, self.error()
        torch.cuda.synchronize()

    def download(self, m, w, h):
        host = np.full((h, w), POISON, dtype=np.uint32)
        assert self.lib.rt_multi_download(m, host.ctypes.data) == 0, self.error()
        return host

    def close(self):
        for key, m in self.made.items():
            self.lib.rt_multi_destroy(m)
        self.made = {}
        self.descs.close()
        print("\nrt_multi set-up (shares, transport) -> s:",
              {k: round(v, 3) for k, v in sorted(self.setup_s.items())})


@pytest.fixture(scope="module")
def pool(rt, gpu):
    p = Pool(rt)
    try:
        yield p
    finally:
        p.close()


@pytest.fixture(scope="module")
def single(rt, gpu):
    """single(w, h, inp=None, **options): the single-scene packed frame, rendered once per description."""
    import torch
    scenes, frames = {}, {}
    default = Inputs(rt, 256)

    def frame(w, h, inp=None, key=None, cam_z=None, **kw):
        inp = default if inp is None else inp
        name = (key, w, h, cam_z, tuple(sorted(kw.items())))
        if name not in frames:
            if key not in scenes:
                scenes[key] = inp.scene()
            if cam_z is not None:
                kw = dict(kw, cam=_camera(inp.rt, cam_z))
            out = scenes[key].render(w, h, want_rgba=False, **kw)["packed"]
            torch.cuda.synchronize()
            frames[name] = _u32(out)
        return frames[name]

    yield frame
    for sc in scenes.values():
        sc.close()


def _camera(rt, z):
    cam = rt.default_camera()
    cam.Org.z = z
    return cam


_ORACLE = {}


def _oracle_frame(oracle, rt, w, h):
    """The oracle's packed frame of the default 256-sphere scene."""
    if (w, h) not in _ORACLE:
        _ORACLE[(w, h)] = Inputs(rt, 256).oracle_render(oracle, w, h)[1]
    return _ORACLE[(w, h)]


# ------------------------------------------------------------------------------------------------ a. the scatter kernel
SCATTER_CASES = [(4, 1, 1, 16), (4, 16, 3, 16), (8, 17, 2, 16), (12, 33, 5, 16), (36, 90, 8, 16), (164, 100, 3, 48),
                 (8, 17, 2, 32)]     # the last one: a slot taller than needed


@pytest.mark.parametrize("w,h,n,slot_rows", SCATTER_CASES)
def test_scatter_kernel_on_hand_made_bytes(rt, gpu, w, h, n, slot_rows):
    """rt_assemble_rows24 on slots filled by multi_ref.fill_slots from a frame of pairwise-distinct words with distinct
    bytes (a swapped channel, a neighbour's byte or another row cannot pass), 0xA5 in every slot byte nobody owns, the
    output poisoned and 16 rows taller than the frame."""
    import torch
    lib = rt.load_library()
    assert slot_rows >= multi_ref.slot_rows(h, n)
    frame = multi_ref.distinct_words(w, h, seed=1000 * w + h)
    recv_host = multi_ref.fill_slots(frame, n, slot_rows, 0xA5)
    want = multi_ref.assemble(recv_host, w, h, n, slot_rows)
    assert np.array_equal(want, frame)
    recv = torch.from_numpy(recv_host).cuda()
    out = _poisoned(h + 16, w)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.rt_assemble_rows24(recv.data_ptr(), out.data_ptr(), w, h, n, slot_rows, st) == 0, lib.rt_last_error()
    torch.cuda.synchronize()
    got = _u32(out)
    _same(got[:h], want, "assembled frame")
    assert (got[:h] >> 24 == 0).all()
    assert (got[h:] == POISON).all(), "rows past the frame were written"
    assert np.array_equal(_u32(recv.view(torch.int32)), recv_host.view(np.uint32).reshape(n, slot_rows, -1)), "the slots changed"


@pytest.mark.parametrize("what", ["width 6", "n 0", "slot_rows 0", "null recv", "null frame"])
def test_scatter_refusals_write_nothing(rt, gpu, what):
    import torch
    lib = rt.load_library()
    w, h, n, sr = 8, 17, 2, 16
    recv = torch.from_numpy(multi_ref.fill_slots(multi_ref.distinct_words(w, h, seed=3), n, sr, 0xA5)).cuda()
    out = _poisoned(h + 16, w)
    args = {"width 6": (recv.data_ptr(), out.data_ptr(), 6, h, n, sr), "n 0": (recv.data_ptr(), out.data_ptr(), w, h, 0, sr),
            "slot_rows 0": (recv.data_ptr(), out.data_ptr(), w, h, n, 0), "null recv": (None, out.data_ptr(), w, h, n, sr),
            "null frame": (recv.data_ptr(), None, w, h, n, sr)}[what]
    assert lib.rt_assemble_rows24(*args, torch.cuda.current_stream().cuda_stream) != 0
    torch.cuda.synchronize()
    assert (_u32(out) == POISON).all()


# ------------------------------------------------------------------------------------------------ b. small and ragged frames
SIZES = [(4, 1), (8, 15), (12, 16), (20, 17), (36, 33), (164, 100)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("shares,transport", SHARES)
def test_small_and_ragged_frames(rt, oracle, pool, single, shares, transport, w, h):
    """One quad wide, one row, fewer blocks than shares (8 shares at one block: seven own nothing), a short last block:
    into a poisoned caller buffer and into the internal one, every word is written and is the single-scene frame's."""
    m = pool.get(shares, transport)
    want = single(w, h)
    if (w, h) == SIZES[0]:
        _same(want, _oracle_frame(oracle, rt, w, h), "single scene against the oracle")
    fd = pool.fd(w, h)
    out = _poisoned(h, w)
    assert pool.render(m, fd, out) == 0, pool.error()
    pool.sync(m)
    _same(_u32(out), want, "caller buffer")
    assert pool.render(m, fd, None) == 0, pool.error()
    _same(pool.download(m, w, h), want, "internal buffer")


# ------------------------------------------------------------------------------------------------ c. bands
BAND_CASES = [(3, PEER, 164, 100), (1, RCCL, 36, 48)]


def _bands(h):
    return [(y, min(y + 16, h)) for y in range(0, h, 16)]


@pytest.mark.parametrize("shares,transport,w,h", BAND_CASES)
def test_single_block_bands_into_a_caller_buffer(rt, oracle, pool, single, shares, transport, w, h):
    m = pool.get(shares, transport)
    want = single(w, h)
    if h == 48:
        _same(want, _oracle_frame(oracle, rt, w, h), "single scene against the oracle")
    for (y0, y1) in _bands(h):                 # each band alone: exactly its rows change
        out = _poisoned(h, w)
        assert pool.render(m, pool.fd(w, h, y0=y0, y1=y1), out) == 0, pool.error()
        pool.sync(m)
        got = _u32(out)
        _same(got[y0:y1], want[y0:y1], "band [%d,%d)" % (y0, y1))
        assert (got[:y0] == POISON).all() and (got[y1:] == POISON).all(), "band [%d,%d) wrote outside its rows" % (y0, y1)
    out = _poisoned(h, w)                      # all of them back to back: three or more calls over two buffer sets
    for (y0, y1) in _bands(h):
        assert pool.render(m, pool.fd(w, h, y0=y0, y1=y1), out) == 0, pool.error()
    pool.sync(m)
    _same(_u32(out), want, "bands back to back")


@pytest.mark.parametrize("shares,transport,w,h", BAND_CASES)
def test_bands_into_the_internal_buffer_make_one_frame(rt, pool, single, shares, transport, w, h):
    """A frame rendered as bands with no caller buffer is ONE internal buffer: rt_multi_frame() is the same pointer after
    every band, rt_multi_download gives the whole frame. Both internal buffers hold another view's frame beforehand, so a
    band that landed in the other buffer shows as rows of that view."""
    m = pool.get(shares, transport)
    want = single(w, h)
    other = pool.fd(w, h, cam=_camera(rt, 12.5))
    for _ in range(2):
        assert pool.render(m, other, None) == 0, pool.error()
    assert not np.array_equal(pool.download(m, w, h), want)
    pointers = []
    for (y0, y1) in _bands(h):
        assert pool.render(m, pool.fd(w, h, y0=y0, y1=y1), None) == 0, pool.error()
        pointers.append(pool.lib.rt_multi_frame(m))
    got = pool.download(m, w, h)
    stale = single(w, h, cam_z=12.5)
    assert np.array_equal(got, want), "banded frame in the internal buffer: rows %s differ from the frame (%d of them are the earlier view's)" % (
        _rows_that_differ(got, want), sum(1 for y in _rows_that_differ(got, want) if np.array_equal(got[y], stale[y])))
    assert pointers[0] and len(set(pointers)) == 1, pointers
    assert pool.lib.rt_multi_frame(m) == pointers[0]
    # the next frame may take the other buffer; whichever it takes, it is whole
    assert pool.render(m, other, None) == 0, pool.error()
    _same(pool.download(m, w, h), stale, "the frame after the banded one")


@pytest.mark.parametrize("y0,y1", [(8, 32), (16, 24), (32, 32), (48, 32), (96, 112)])
def test_band_refusals_write_nothing(pool, single, y0, y1):
    """y0 and y1 that are no block boundaries, an empty or reversed band, a band past the frame."""
    w, h = 164, 100
    m = pool.get(3, PEER)
    out = _poisoned(h, w)
    assert pool.render(m, pool.fd(w, h, y0=y0, y1=y1), out) != 0
    assert "row band" in pool.error()
    pool.sync(m)
    assert (_u32(out) == POISON).all()
    assert pool.render(m, pool.fd(w, h), out) == 0, pool.error()
    pool.sync(m)
    _same(_u32(out), single(w, h), "the frame after the refusal")


# ------------------------------------------------------------------------------------------------ d. options
OPTIONS = [{"tile": 8}, {"tile": 16}, {"tile": 32}, {"tile": 64}, {"cull": False}, {"spp": 4}]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "-".join("%s%s" % kv for kv in o.items()))
@pytest.mark.parametrize("w,h", [(36, 33), (164, 100)])
@pytest.mark.parametrize("shares", [2, 3])
def test_options_the_header_promises(rt, oracle, pool, single, shares, w, h, opt):
    """opts.tile, opts.cull and opts.spp reach every share: the frame is the single scene's with the same option (for
    spp = 4 its one-launch four-sample frame; 24-bit rows of several samples are not refused, rt_render.cpp)."""
    m = pool.get(shares, PEER)
    want = single(w, h, **opt)
    if (w, h, shares) == (36, 33, 2):
        if "spp" in opt:
            _same(want, Inputs(rt, 256).oracle_render_spp(oracle, rt, w, h, 4)[1], "single scene against the oracle, 4 spp")
        else:
            _same(want, _oracle_frame(oracle, rt, w, h), "single scene against the oracle")
    out = _poisoned(h, w)
    assert pool.render(m, pool.fd(w, h, **opt), out) == 0, pool.error()
    pool.sync(m)
    _same(_u32(out), want, str(opt))


# ------------------------------------------------------------------------------------------------ e. other primitives
def test_planes_cubes_and_a_mesh_on_every_share(rt, oracle, pool, single):
    import oracle_py
    lib, w, h = pool.lib, 164, 100
    m = pool.get(3, PEER)
    inp = mixed_scene(rt)
    text = meshes.uv_sphere_obj()
    mesh = rt.mesh_from_obj_text(text)
    try:
        sc = inp.scene()
        sc.set_planes(inp.planes, inp.n_planes)
        sc.set_cubes(inp.cubes, inp.n_cubes)
        sc.set_mesh(mesh)
        want = _u32(sc.render(w, h, want_rgba=False)["packed"])
        sc.close()
        om = oracle_py.Mesh(text)
        _, ref, cnt = oracle_py.render(inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam, w, h,
                                       inp.aspect, nthreads=8, cubes=inp.cubes, n_cubes=inp.n_cubes, planes=inp.planes,
                                       n_planes=inp.n_planes, mesh=om.handle)
        _same(want, ref, "single scene against the oracle")
        assert lib.rt_multi_set_spheres(m, inp.spheres, inp.n) == 0, pool.error()
        assert lib.rt_multi_set_planes(m, inp.planes, inp.n_planes) == 0, pool.error()
        assert lib.rt_multi_set_cubes(m, inp.cubes, inp.n_cubes) == 0, pool.error()
        assert lib.rt_multi_set_mesh(m, mesh) == 0, pool.error()
        out = _poisoned(h, w)
        assert pool.render(m, pool.fd(w, h), out) == 0, pool.error()
        pool.sync(m)
        _same(_u32(out), want, "spheres, planes, cubes and a mesh")
        # and away again: the spheres alone
        assert lib.rt_multi_set_planes(m, None, 0) == 0, pool.error()
        assert lib.rt_multi_set_cubes(m, None, 0) == 0, pool.error()
        assert lib.rt_multi_set_mesh(m, None) == 0, pool.error()
        out = _poisoned(h, w)
        assert pool.render(m, pool.fd(w, h), out) == 0, pool.error()
        pool.sync(m)
        alone = single(w, h, inp=Inputs(rt, 200), key="200 spheres")
        _same(_u32(out), alone, "the primitives removed")
        assert not np.array_equal(alone, want)
    finally:
        lib.rt_multi_set_planes(m, None, 0)
        lib.rt_multi_set_cubes(m, None, 0)
        lib.rt_multi_set_mesh(m, None)
        lib.rt_multi_set_spheres(m, pool.inp.spheres, pool.inp.n)
        lib.rt_mesh_free(mesh)


# ------------------------------------------------------------------------------------------------ f. refusals
@pytest.mark.parametrize("what", ["reflect_depth", "aov_depth", "aov_normal", "aov_id", "aov_albedo", "width 162"])
def test_refused_frames_write_nothing(rt, oracle, pool, single, what):
    import torch
    w, h = (162, 33) if what == "width 162" else (36, 33)
    m = pool.get(2, PEER)
    guide = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")     # large enough for any G-buffer output
    kw = {"reflect_depth": {"reflect_depth": 1}, "width 162": {}}.get(what, {what: guide.data_ptr()})
    out = _poisoned(h, w)
    assert pool.render(m, pool.fd(w, h, **kw), out) != 0
    reason = {"reflect_depth": "reflect_depth", "width 162": "multiple of 4"}.get(what, what)
    assert reason in pool.error(), pool.error()
    pool.sync(m)
    assert (_u32(out) == POISON).all() and not guide.any()
    w, h = 36, 33
    out = _poisoned(h, w)
    assert pool.render(m, pool.fd(w, h), out) == 0, pool.error()
    pool.sync(m)
    _same(_u32(out), single(w, h), "the frame after the refusal")
    _same(single(w, h), _oracle_frame(oracle, rt, w, h), "single scene against the oracle")


@pytest.mark.parametrize("transport", [RCCL, PEER])
def test_a_width_of_162_on_one_share_takes_the_direct_path(pool, single, transport):
    w, h = 162, 33
    m = pool.get(1, transport)
    gathers = pool.lib.rt_multi_gathers(m)
    out = _poisoned(h, w)
    assert pool.render(m, pool.fd(w, h), out) == 0, pool.error()
    pool.sync(m)
    _same(_u32(out), single(w, h), "caller buffer")
    assert pool.render(m, pool.fd(w, h), None) == 0, pool.error()
    _same(pool.download(m, w, h), single(w, h), "internal buffer")
    assert pool.lib.rt_multi_gathers(m) == gathers        # no 24-bit rows, no exchange


def test_a_refused_resize_leaves_no_last_frame(pool, single):
    """A render that is refused after the buffers were re-made for its size (here: a tile width the frame kernel does
    not have) leaves nothing to download, to point at or to wait for. Return codes only."""
    m = pool.get(2, PEER)
    assert pool.render(m, pool.fd(36, 33), None) == 0, pool.error()
    pool.sync(m)
    assert pool.lib.rt_multi_frame(m)
    assert pool.render(m, pool.fd(20, 17, tile=7), None) != 0
    assert "tile" in pool.error()
    host = np.zeros((33, 36), dtype=np.uint32)
    assert pool.lib.rt_multi_frame(m) is None
    assert pool.lib.rt_multi_download(m, host.ctypes.data) != 0
    assert pool.lib.rt_multi_stream_wait(m, None) != 0
    assert pool.render(m, pool.fd(20, 17), None) == 0, pool.error()
    _same(pool.download(m, 20, 17), single(20, 17), "the frame after the refusal")


# ------------------------------------------------------------------------------------------------ g. changes in flight
def test_changes_with_frames_in_flight_on_three_shares(rt, oracle, pool, single):
    """A size change, new lights, 1024 spheres of another seed and a smaller size, each with two frames in flight (one
    into the internal buffer, one into a caller buffer) and no wait anywhere before the end: every caller buffer is the
    fresh single scene's frame of the state it was issued under."""
    lib = pool.lib
    m = pool.get(3, PEER)
    lights = rt.default_lights()
    lights[0] = rt.Light(rt.Vec3(-5, 25, 10), 20, 1, 1, 0)
    lights[2] = rt.Light(rt.Vec3(3, 20, 3), 20, 0, 1, 1)
    relit = Inputs(rt, 256)
    relit.lights = lights
    crowd = Inputs(rt, 1024, seed=2)
    crowd.lights = lights
    steps = [(None, None, "default", 164, 100),
             ("size", None, "default", 96, 48),
             ("lights", relit, "relit", 96, 48),
             ("spheres", crowd, "crowd", 96, 48),
             ("size", crowd, "crowd", 36, 33)]
    issued = []
    try:
        for k, (change, inp, key, w, h) in enumerate(steps):
            if change == "lights":
                assert lib.rt_multi_set_lights(m, inp.lights, 3) == 0, pool.error()
            elif change == "spheres":
                assert lib.rt_multi_set_spheres(m, inp.spheres, inp.n) == 0, pool.error()
            for j in range(2):
                z = 10.0 + 0.25 * (2 * k + j)
                out = _poisoned(h, w) if j else None
                assert pool.render(m, pool.fd(w, h, cam=_camera(rt, z)), out) == 0, pool.error()
                if j:
                    issued.append((out, inp, key, w, h, z))
        pool.sync(m)
        for (out, inp, key, w, h, z) in issued:
            _same(_u32(out), single(w, h, inp=inp, key=key, cam_z=z), "%s at %d x %d, z %.2f" % (key, w, h, z))
        out, inp, key, w, h, z = issued[-1]
        crowd.cam = _camera(rt, z)
        _same(_u32(out), crowd.oracle_render(oracle, w, h)[1], "the last state against the oracle")
    finally:
        lib.rt_multi_set_spheres(m, pool.inp.spheres, pool.inp.n)
        lib.rt_multi_set_lights(m, pool.inp.lights, 3)


# ------------------------------------------------------------------------------------------------ h. rt_multi_stream_wait
def test_stream_wait_orders_a_side_stream_behind_the_frame(rt, oracle, pool, single):
    """Before any render there is nothing to wait for. After one, a side stream that waited through rt_multi_stream_wait
    copies the frame to pinned host memory with no host wait in between, from the caller buffer and from
    rt_multi_frame(); once that stream alone is synchronised the copy is the frame."""
    import torch
    lib, w, h = pool.lib, 164, 100
    m = pool.get(4, PEER)                      # no other test uses four shares: nothing has been rendered on it
    side = torch.cuda.Stream()
    assert lib.rt_multi_frame(m) is None
    assert lib.rt_multi_stream_wait(m, side.cuda_stream) != 0
    assert "nothing has been rendered" in pool.error()
    want = single(w, h)
    _same(want, _oracle_frame(oracle, rt, w, h), "single scene against the oracle")
    out, staged = _poisoned(h, w), _poisoned(h, w)
    pinned = [torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32).pin_memory() for _ in range(2)]
    torch.cuda.synchronize()
    # from the caller buffer
    assert pool.render(m, pool.fd(w, h), out) == 0, pool.error()
    assert lib.rt_multi_stream_wait(m, side.cuda_stream) == 0, pool.error()
    with torch.cuda.stream(side):
        pinned[0].copy_(out, non_blocking=True)
    # from the internal buffer: a raw device pointer, so a copy kernel of the library (16 bytes a thread) brings it into
    # a tensor on the side stream, and the copy to the host follows it there
    assert pool.render(m, pool.fd(w, h), None) == 0, pool.error()
    assert lib.rt_multi_stream_wait(m, side.cuda_stream) == 0, pool.error()
    src = lib.rt_multi_frame(m)
    assert src and src != out.data_ptr()
    assert lib.rt_debug_copy16(src, staged.data_ptr(), w * h // 4, side.cuda_stream) == 0, pool.error()
    with torch.cuda.stream(side):
        pinned[1].copy_(staged, non_blocking=True)
    side.synchronize()
    _same(pinned[0].numpy().view(np.uint32), want, "copy of the caller buffer")
    _same(pinned[1].numpy().view(np.uint32), want, "copy of rt_multi_frame()")
    pool.sync(m)
