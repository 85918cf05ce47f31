"""Light verdicts on edge inputs: sphere counts on either side of the thresholds at which the
scene's tables appear and disappear (64: eye cones, light columns, occluder and view lists; 8192: no occluder lists,
cones built on the host), no lights and degenerate lights, cameras straight up and down and with a NaN origin, frames
smaller than a tile and ragged in both directions, layouts that leave the view lists, and other work on the same scene
between the recording launch and the reading ones. Each case is a resting view (verdict_runs.resting): four launches of
the same frame, each the oracle's bits, the launches going nothing, write, read, read."""
import ctypes as C

import numpy as np
import pytest

import verdict_runs as R
from scenes import Inputs, Scn

pytestmark = pytest.mark.gpu

W, H = 64, 48


def _brute(sc, width, height, **kw):
    """The brute-force frame of a scene of its own with verdicts off."""
    ref = sc.scene()
    ref.set_light_verdicts(0)
    return R.frame(ref, width, height, cull=False, **kw)


def _inputs(rt, n, lights=None, cam=None):
    inp = Inputs(rt, n)
    if lights is not None:
        inp.lights, inp.n_lights = Scn(rt, [], lights=lights).lights, len(lights)
    if cam is not None:
        inp.cam = cam
    return inp


# ---------------------------------------------------------------------------------------------- sphere counts
@pytest.mark.parametrize("n", [0, 1, 8, 63, 64, 65, 8192, 8193])
def test_sphere_counts(rt, gpu, oracle, n):
    inp = _inputs(rt, n)
    want = _brute(inp, W, H) if n > 8192 else R.oracle_frame(oracle, inp, W, H)   # (8193 spheres: the oracle takes too long)
    allowed = ([0, 0, 0, 0], [0, 1, 2, 2]) if n == 0 else None   # eligibility (rt_render.cpp) does not depend on n
    R.resting(inp.scene(), dict(width=W, height=H), want, what="%d spheres" % n, allowed_states=allowed)


# ---------------------------------------------------------------------------------------------- lights
ORDINARY = [((0, 20, -20), 20, 0, 0, 1), ((0, 20, 0), 20, 0, 1, 0)]


def _light_cases(rt):
    g = rt.generate_spheres(256, 1)
    big = max(range(256), key=lambda i: g[i].radius)
    inside = (g[big].orgin.x, g[big].orgin.y, g[big].orgin.z)
    return {
        "none": [],
        "at_the_origin": [((0, 0, 0), 20, 1, 0.5, 0.25)] + ORDINARY,     # a NaN axis: no culling for it
        "inside_a_sphere": [(inside, 20, 1, 0.5, 0.25)] + ORDINARY,
        "size_zero": [((20, 20, 20), 0, 1, 0, 0)] + ORDINARY,
        "two_identical": [((20, 20, 20), 20, 1, 0, 0)] * 2 + ORDINARY[:1],
    }


@pytest.mark.parametrize("case", ["none", "at_the_origin", "inside_a_sphere", "size_zero", "two_identical"])
def test_lights(rt, gpu, oracle, case):
    inp = _inputs(rt, 256, lights=_light_cases(rt)[case])
    want = R.oracle_frame(oracle, inp, W, H)
    R.resting(inp.scene(), dict(width=W, height=H), want, what="lights: " + case)


# ---------------------------------------------------------------------------------------------- cameras
@pytest.mark.parametrize("pitch", [90.0, -90.0])
def test_camera_straight_up_and_down(rt, gpu, oracle, pitch):
    inp = _inputs(rt, 256, cam=rt.Camera(rt.Vec3(4, 3, 10), rt.Vec3(0, 0, 1), 0.0, 180.0, pitch))
    want = R.oracle_frame(oracle, inp, W, H)
    R.resting(inp.scene(), dict(width=W, height=H, cam=inp.cam), want, what="pitch %g" % pitch)


def test_camera_origin_with_a_nan(rt, gpu):
    """The key is compared bit for bit, so a NaN in the origin still rests. Against the brute-force kernel; the two
    kernels may give NaNs of different bits, so a NaN matches a NaN (every other value bit for bit)."""
    inp = _inputs(rt, 256, cam=rt.Camera(rt.Vec3(float("nan"), 3, 10), rt.Vec3(0, 0, 1), 0.0, 180.0, -20.0))
    want = _brute(inp, W, H, cam=inp.cam)
    R.resting(inp.scene(), dict(width=W, height=H, cam=inp.cam), want, nan_equal=True, what="NaN origin")


# ---------------------------------------------------------------------------------------------- frame shapes
@pytest.fixture(scope="module")
def inp256(rt, gpu):
    return Inputs(rt, 256)


@pytest.fixture(scope="module")
def shape_wants(oracle, inp256):
    return {s: R.oracle_frame(oracle, inp256, *s) for s in ((1, 1), (7, 5), (65, 9), (130, 3))}


@pytest.mark.parametrize("tile", [8, 16, 32, 64])
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (65, 9), (130, 3)])
def test_frame_shapes(inp256, shape_wants, shape, tile):
    R.resting(inp256.scene(), dict(width=shape[0], height=shape[1], tile=tile), shape_wants[shape],
              what="%d x %d tile %d" % (shape[0], shape[1], tile))


# ---------------------------------------------------------------------------------------------- layouts off the view lists
def test_band_that_does_not_nest(oracle, inp256):
    sc = inp256.scene()
    R.resting(sc, dict(width=W, height=H, y0=4, y1=44, tile=8), R.oracle_frame(oracle, inp256, W, H, 4, 44), what="rows 4-44")
    assert sc.view_lists_info()["read"] == 0   # (tiles of 8 rows from row 4 straddle the view's blocks: a per-tile cull)


def test_view_lists_off(oracle, inp256):
    sc = inp256.scene()
    sc.set_view_lists(0)
    R.resting(sc, dict(width=W, height=H), R.oracle_frame(oracle, inp256, W, H), what="view lists off")
    assert sc.view_lists_info()["read"] == 0


def test_tile_order_with_a_band(oracle, inp256):
    sc = inp256.scene()
    sc.set_tile_order(1)
    # (the order is sorted again before launches 1, 2, 4 and 8 of an unchanged view)
    R.resting(sc, dict(width=W, height=H, y0=16, y1=40), R.oracle_frame(oracle, inp256, W, H, 16, 40), launches=9,
              what="tile order 1, rows 16-40")


# ---------------------------------------------------------------------------------------------- interleavings
def _graph_frame(rt, sc, cam):
    import torch
    lib = rt.load_library()
    pk = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    fd = sc.frame_desc(W, H, pixels=pk.data_ptr(), cam=cam)
    gr = lib.rt_graph_capture(sc.handle, C.byref(fd), 1, None, stream.cuda_stream)
    assert gr, lib.rt_last_error()
    try:
        assert lib.rt_graph_launch(gr, stream.cuda_stream) == 0, lib.rt_last_error()
        stream.synchronize()
    finally:
        lib.rt_graph_destroy(gr)


def test_other_work_between_the_launches(rt, gpu, oracle):
    """One long-lived scene; for each kind of other work a view V of its own: V, V (records), the other work, V (the
    first that may read), V, the other work, V. Every frame of V is the oracle's; which launches read is not fixed
    here."""
    import torch
    inp = Inputs(rt, 256)
    sc = inp.scene()
    sc.set_materials(np.full(256, 0.5, dtype=np.float32))
    other = rt.Camera(rt.Vec3(5, 4, 11), rt.Vec3(0, 0, 1), 0.0, 150.0, -10.0)
    work = {
        "frame graph": lambda: _graph_frame(rt, sc, other),
        "ray query": lambda: sc.trace_rays(sc.primary_rays(W, H, cam=other).reshape(-1, 6), "shade"),
        "reflective frame": lambda: sc.render(W, H, reflect_depth=2),
        "stats frame": lambda: sc.render(W, H, want_stats=True),
        "four samples": lambda: sc.render(W, H, spp=4),
        "another view": lambda: sc.render(W, H, cam=other),
    }
    seen = {}
    for i, (name, do) in enumerate(work.items()):
        cam = rt.Camera(rt.Vec3(4, 3, 10), rt.Vec3(0, 0, 1), 0.0, 180.0 - 4.0 * i, -20.0)
        inp.cam = cam
        want = R.oracle_frame(oracle, inp, W, H)
        states = []
        for step in ("V", "V", do, "V", "V", do, "V"):
            if step == "V":
                R.assert_same(R.frame(sc, W, H, cam=cam), want, "%s: plain frame %d" % (name, len(states)))
                states.append(sc.light_verdicts()["state"])
            else:
                step()
                torch.cuda.synchronize()
        seen[name] = states
    print(seen)
