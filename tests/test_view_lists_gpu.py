"""Per-view candidate lists of the primary rays on the GPU: the device builder against the host
builder, that launches do read the lists where they should (and not where they must not), and culled == brute force
bit for bit across everything that decides which list a tile reads."""
import ctypes as C

import numpy as np
import pytest

from scenes import Inputs, Scn
from view_margins import assert_lists_equal

pytestmark = pytest.mark.gpu


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def _frame(scene, w, h, **kw):
    import torch
    out = scene.render(w, h, **kw)
    torch.cuda.synchronize()
    return _u32(out["packed"]), _u32(out["rgba"])


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), "packed differs: %s (%d pixels)" % (what, int((a[0] != b[0]).sum()))
    assert np.array_equal(a[1], b[1]), "rgba differs: %s" % (what,)


def _cam(rt, org=(4, 3, 10), yaw=180.0, pitch=-20.0):
    return rt.Camera(rt.Vec3(*[float(v) for v in org]), rt.Vec3(0, 0, 1), 0.0, float(yaw), float(pitch))


def _check(scene, w, h, what, read=True, off_too=False, **kw):
    """Culled (lists on) == brute force; the info entry says whether the culled launch read the lists."""
    got = _frame(scene, w, h, cull=True, **kw)
    info = scene.view_lists_info()
    assert info["read"] == (1 if read else 0), (what, info)
    _same(got, _frame(scene, w, h, cull=False, **kw), what)
    if off_too:
        scene.set_view_lists(0)
        off = _frame(scene, w, h, cull=True, **kw)
        assert scene.view_lists_info()["read"] == 0
        scene.set_view_lists(1)
        _same(got, off, what + " (lists off)")
    return info


@pytest.mark.parametrize("w,h,n", [(3840, 2160, 1024), (1920, 1080, 256), (164, 100, 300)])
def test_device_builder_equals_host_builder(rt, gpu, w, h, n):
    import torch
    inp = Inputs(rt, n)
    scene = inp.scene()
    y1 = min(h, 64)                                   # a band is enough: the lists are built for the whole view
    scene.render(w, h, y0=0, y1=y1, cull=True)
    torch.cuda.synchronize()
    dev = scene.view_lists_info(want_lists=True)
    assert dev["read"] == 1
    host = rt.view_lists_host(inp.spheres, n, scene.frame_desc(w, h))
    assert_lists_equal(dev, host, inp_table(inp))


_TABS = {}


def inp_table(inp):
    from test_reflect_cpu import sphere_table
    if id(inp) not in _TABS:
        _TABS[id(inp)] = sphere_table(inp.spheres, inp.n)
    return _TABS[id(inp)]


@pytest.mark.parametrize("w,h,n", [(3840, 2160, 1024), (1920, 1080, 256), (160, 90, 256)])
def test_launches_read_the_lists(rt, gpu, w, h, n):
    scene = Inputs(rt, n).scene()
    y0, y1 = (h // 2 // 8 * 8, h // 2 // 8 * 8 + 16)
    info = _check(scene, w, h, "band of the default view", y0=y0, y1=y1, off_too=True)
    assert info["blocks"] > 0 and info["overflowed"] == 0 and info["not_built"] == 0 and 0 < info["longest"] <= rt.RT_VIEW_CAP
    _frame(scene, w, h, cull=False, y0=y0, y1=y1)
    assert scene.view_lists_info()["read"] == 0          # brute force reads none
    _frame(scene, w, h, cull=True, force_slow=True, y0=y0, y1=y1)
    assert scene.view_lists_info()["read"] == 0          # nor does the slow path
    small = Inputs(rt, 32).scene()                       # no eye cones: no lists
    _check(small, w, h, "32 spheres", read=False, y0=y0, y1=y1)


def test_camera_sequence_and_cache(rt, gpu):
    w, h = 480, 270
    scene = Inputs(rt, 1024).scene()
    cams = [_cam(rt), _cam(rt, (4, 3, 10.5)), _cam(rt, (4, 3, 10.5), 171.0), _cam(rt, (4, 3, 10.5), 171.0, -31.0),
            _cam(rt, (4.5, 2, 9), 200.0, 5.0), _cam(rt)]
    first = None
    for i, c in enumerate(cams):
        _check(scene, w, h, "camera %d" % i, cam=c, off_too=(i in (0, 3)))
        if i == 0:
            first = _frame(scene, w, h, cam=c)
    _same(first, _frame(scene, w, h, cam=cams[0]), "the first view again")
    # more views than slots, then all of them again
    many = [_cam(rt, (4 + 0.3 * k, 3, 10), 180.0 + 2 * k) for k in range(6)]
    ref = [_frame(scene, w, h, cull=False, cam=c) for c in many]
    for rnd in range(2):
        for c, r in zip(many, ref):
            _same(_frame(scene, w, h, cam=c), r, "view cache round %d" % rnd)


def test_two_sizes_and_a_new_sphere_list(rt, gpu):
    inp = Inputs(rt, 1024)
    scene = inp.scene()
    for (w, h) in [(480, 270), (320, 180), (480, 270), (164, 100)]:
        _check(scene, w, h, "%dx%d" % (w, h))
    # another list of the same length, then a shorter one: the old view's lists must not be read
    for n, seed in [(1024, 7), (700, 3), (1024, 1)]:
        other = Inputs(rt, n, seed)
        scene.set_spheres(other.spheres, n)
        _check(scene, 480, 270, "spheres n=%d seed=%d" % (n, seed))
        fresh = other.scene()
        _same(_frame(scene, 480, 270), _frame(fresh, 480, 270), "against a fresh scene")


def test_tile_shapes_bands_and_interleaved_rows(rt, gpu):
    big = Inputs(rt, 256).scene()                       # 64 x 64 blocks: every tile shape nests
    for tile in (8, 16, 32, 64):
        _check(big, 1920, 1080, "tile %d" % tile, tile=tile, y0=640, y1=768)
    small = Inputs(rt, 256).scene()                     # 8 x 8 blocks: only the 8 x 8 tile nests
    _check(small, 160, 90, "tile 8 at 160x90", tile=8)
    for tile in (16, 32, 64):
        _check(small, 160, 90, "tile %d at 160x90" % tile, read=False, tile=tile)
    mid = Inputs(rt, 1024).scene()
    _check(mid, 480, 270, "band from a tile row", y0=96, y1=200)
    _check(mid, 480, 270, "band from the middle of a tile row", read=False, y0=100, y1=203)
    _check(mid, 480, 270, "band from row 100, 16x4 tiles", tile=16, y0=100, y1=203)
    _check(mid, 480, 270, "64x1 tiles in 16x16 blocks", read=False, tile=64)
    for idx in (0, 1, 2):
        _check(mid, 480, 270, "interleaved rows %d of 3" % idx, interleave=(3, idx, 16))
        _check(mid, 480, 270, "interleaved rows %d of 3 from row 64" % idx, interleave=(3, idx, 32), y0=64, y1=270)


def test_four_samples_in_one_launch_and_under_the_graph(rt, gpu):
    import torch
    w, h = 480, 270
    scene = Inputs(rt, 1024).scene()
    _check(scene, w, h, "4 spp", spp=4, off_too=True)
    _check(scene, w, h, "4 spp, tile 16", spp=4, tile=16)
    lib = rt.load_library()
    pk = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    rgba = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    cams = [_cam(rt), _cam(rt, (4, 3, 10.4), 176.0), _cam(rt, (3, 4, 9), 190.0, -28.0), _cam(rt)]
    fd = scene.frame_desc(w, h, pixels=pk.data_ptr(), rgba=rgba.data_ptr(), cam=cams[0])
    g = lib.rt_graph_capture(scene.handle, C.byref(fd), 4, None, stream.cuda_stream)
    assert g, lib.rt_last_error()
    try:
        for i, c in enumerate(cams):
            assert lib.rt_graph_set_camera(g, C.byref(c)) == 0, lib.rt_last_error()
            for rep in range(2):
                pk.zero_(); rgba.zero_()
                torch.cuda.synchronize()
                assert lib.rt_graph_launch(g, stream.cuda_stream) == 0, lib.rt_last_error()
                stream.synchronize()
                got = (_u32(pk), _u32(rgba))
                want = _frame(scene, w, h, cull=False, spp=4, cam=c)
                assert np.array_equal(got[0], want[0]), "graph, camera %d replay %d" % (i, rep)
                assert np.array_equal(got[1], want[1]), "graph, camera %d replay %d" % (i, rep)
    finally:
        lib.rt_graph_destroy(g)


def _filler(n, seed=5):
    rng = np.random.default_rng(seed)
    return [(float(rng.uniform(-8, 8)), float(rng.uniform(-3, 6)), float(rng.uniform(4, 30)), float(rng.uniform(0.1, 0.9))) for _ in range(n)]


def test_camera_inside_spheres_duplicates_and_overflow(rt, gpu):
    w, h = 320, 192
    cam = _cam(rt, (0, 0, 0), 0.0, 0.0)                  # rays start at (0, 0, -1/aspect) and look along +z
    eye = (0.0, 0.0, -1.0 / rt.default_aspect())
    # inside one sphere; between two concentric ones
    for name, extra in [("inside a sphere", [(eye[0], eye[1], eye[2] + 0.5, 3.0)]),
                        ("between concentric spheres", [(eye[0] + 0.2, eye[1], eye[2], 0.1), (eye[0] + 0.2, eye[1], eye[2], 40.0)]),
                        ("inside a far larger sphere than the scene", [(1.0, 1.0, 10.0, 60.0)])]:
        s = Scn(rt, _filler(90) + extra, cam=cam)
        _check(s.scene(), w, h, name, cam=cam, aspect=s.aspect, off_too=True)
    # duplicates: equal t, the first list position wins
    base = _filler(70, 9)
    s = Scn(rt, base + base[:40] + [base[3]] * 5, cam=cam)
    _check(s.scene(), w, h, "duplicate spheres", cam=cam, aspect=s.aspect, off_too=True)
    # 70 small spheres in a row behind the frame's centre: that block overflows its cap, the others do not
    row = [(0.0, 0.0, 5.0 + 0.4 * i, 0.05) for i in range(70)]
    s = Scn(rt, row + _filler(40, 11), cam=cam)
    sc = s.scene()
    info = _check(sc, w, h, "one block over the cap", cam=cam, aspect=s.aspect, off_too=True)
    assert 0 < info["overflowed"] < info["blocks"] and info["longest"] <= rt.RT_VIEW_CAP


def test_two_streams_two_frames_in_flight_with_a_moving_camera(rt, gpu):
    import torch
    w, h = 480, 270
    scene = Inputs(rt, 1024).scene()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    cams = [_cam(rt, (4, 3, 10 + 0.1 * k), 180.0 + 0.7 * k, -20.0 - 0.3 * k) for k in range(12)]
    outs = []
    for k, c in enumerate(cams):                          # no host wait anywhere: two frames in flight, a build per frame
        outs.append(scene.render(w, h, cam=c, stream=streams[k & 1]))
    torch.cuda.synchronize()
    assert scene.view_lists_info()["read"] == 1
    for k, c in enumerate(cams):
        want = _frame(scene, w, h, cull=False, cam=c)
        _same((_u32(outs[k]["packed"]), _u32(outs[k]["rgba"])), want, "frame %d in flight" % k)
