"""Light verdicts at the application boundary: rt_launch_raytrace and update() render through the
library's own long-lived scene (rt_debug_shim_scene), which has verdicts switched on. The same frame rendered again and
again must stay the oracle's frame while the launches go from the plain kernel to the recording and the reading one --
also where update() cuts the frame into three row bands, each a layout of its own that comes round once per frame --
and a moving camera must keep paying nothing."""
import ctypes as C

import numpy as np
import pytest

import verdict_runs as R
from scenes import Inputs
from test_gpu_parity import _managed_sprite

pytestmark = pytest.mark.gpu


def test_raytrace_launch_at_rest(rt, gpu, oracle):
    """rt_launch_raytrace four times with identical arguments at 160 x 90: the oracle's words every time, the shim's scene
    going nothing, write, read, read; one sphere changed in place: nothing again, and the new frame."""
    import torch
    lib = rt.load_library()
    w, h, n = 160, 90, 256
    inp = Inputs(rt, n, seed=3)            # (a sphere list no other test hands the shim: its keys are new)
    obj = C.cast(lib.rt_managed_alloc(C.sizeof(rt.Object)), C.POINTER(rt.Object))
    C.memset(obj, 0, C.sizeof(rt.Object))
    obj.contents.sphere_count = n
    dsp = lib.rt_managed_alloc(32 * n)
    C.memmove(dsp, inp.spheres, 32 * n)
    obj.contents.d_spheres = C.cast(dsp, C.POINTER(rt.Sphere))
    obj.contents.texture = _managed_sprite(rt, inp.tex)
    sky = C.cast(lib.rt_managed_alloc(C.sizeof(rt.Skybox)), C.POINTER(rt.Skybox))
    box = C.cast(lib.rt_managed_alloc(32), C.POINTER(rt.Sphere))
    C.memmove(box, C.byref(inp.sky_box), 32)
    sky.contents.box = box
    sky.contents.skyboxTex = _managed_sprite(rt, inp.sky)
    pixels = torch.zeros((h, w), dtype=torch.int32, device="cuda")

    def launch():
        pixels.zero_()
        torch.cuda.synchronize()
        assert lib.rt_launch_raytrace(pixels.data_ptr(), w, h, inp.aspect, obj, inp.lights, 3, inp.cam, sky, None) == 0, \
            lib.rt_last_error()
        torch.cuda.synchronize()
        return pixels.cpu().numpy().view(np.uint32), R.shim_state(rt)

    want = R.oracle_frame(oracle, inp, w, h)[1]
    states = []
    for k in range(4):
        got, state = launch()
        assert np.array_equal(got, want), (k, state, int((got != want).sum()))
        states.append(state)
    assert states == [0, 1, 2, 2]
    lib.rt_sphere_init(C.byref(obj.contents.d_spheres[0]), 4.0, 3.0, 7.0, 0.9)
    C.memmove(inp.spheres, dsp, 32 * n)
    want2 = R.oracle_frame(oracle, inp, w, h)[1]
    got, state = launch()
    assert state == 0
    assert np.array_equal(got, want2) and not np.array_equal(want2, want)


def test_update_at_rest_in_three_bands(rt, gpu, oracle):
    """update() at 64 x 528: three row bands per frame (rows 0-176, 176-352, 352-528), each a key of its own that comes
    round once per frame. Five frames at rest: the oracle's frame every time; the bands record on the second frame and
    read from the third on (the state reported is that of the frame's last launch, the third band).

    Measured with a table written only when a launch's key equals that of the launch just before it, the policy before
    the history of recent keys: the bands A, B, C, A, B, C ... never meet that condition; the frames were right and the
    states [0, 0, 0, 0, 0], so a resting application never used its tables at 512 rows and more. With the history:
    [0, 1, 2, 2, 2]."""
    with R.App(rt, 256, 7, 64, 528) as app:
        want = R.oracle_frame(oracle, app.inp, 64, 528)[1]
        states = []
        for k in range(5):
            got, state = app.update()
            assert np.array_equal(got, want), (k, state, int((got != want).sum()))
            states.append(state)
        print("states of the last band over five frames at rest:", states)
        assert states == [0, 1, 2, 2, 2], states


def test_update_with_a_moving_camera_records_nothing(rt, gpu, oracle):
    """Org.z nudged before every one of six frames at 64 x 528: no launch writes or reads a table, every frame is the
    oracle's. (A moving camera pays nothing for the history of recent keys.)"""
    with R.App(rt, 256, 8, 64, 528) as app:
        for k in range(6):
            z = 10.0 + 0.03125 * (k + 1)
            app.cam.contents.Org.z = z
            app.inp.cam.Org.z = z
            got, state = app.update()
            want = R.oracle_frame(oracle, app.inp, 64, 528)[1]
            assert np.array_equal(got, want), (k, int((got != want).sum()))
            assert state == 0, (k, state)


def test_two_views_alternating(rt, gpu, oracle):
    """A, B, A, B ... on one fresh scene, the oracle's frames throughout. Both keys stay in the history of recent
    table-less keys, so each view records once it has been seen before and reads from then on. B's first launch puts its
    view lists into a buffer the scene did not have yet, which starts a new generation of buffers (the key's `epoch`): the
    A seen before it is not the A after it, so A is seen anew on its second launch. From then on nothing grows: B
    records on its second launch, A on its third, and every launch after that reads."""
    inp = Inputs(rt, 256)
    sc = inp.scene()
    cams = [inp.cam, rt.Camera(rt.Vec3(4.5, 3, 10), rt.Vec3(0, 0, 1), 0.0, 171.0, -20.0)]
    wants = []
    for cam in cams:
        inp.cam = cam
        wants.append(R.oracle_frame(oracle, inp, 64, 48))
    states = []
    for k in range(8):
        got = R.frame(sc, 64, 48, cam=cams[k % 2])
        states.append(sc.light_verdicts()["state"])
        R.assert_same(got, wants[k % 2], "launch %d, view %s" % (k, "AB"[k % 2]))
    assert states == [0, 0, 0, 1, 1, 2, 2, 2]
