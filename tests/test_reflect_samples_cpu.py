"""Supersampled reflective frames (rt_scene_set_reflect_samples), host side: the composed reference of
tests/reflect_samples_ref.py against the plain frame's 4 spp fixture, and the validation of the mode, which needs no
device."""
import ctypes as C
import os

import numpy as np
import pytest

from reflect_samples_ref import SampleRef, sample_offsets
from scenes import Inputs
from test_reflect_cpu import composer_for

GOLD = os.path.join(os.path.dirname(__file__), "golden")
RT_OK, RT_ERR_INVALID, RT_ERR_UNSUPPORTED = 0, 1, 2


def test_without_materials_the_reference_is_the_4spp_fixture(rt, oracle):
    """Every k = 0, four samples: the plain frame's accumulated sums (w = 4 included) and resolved words."""
    W, H, n = 96, 54, 256
    g = np.load(os.path.join(GOLD, "spp4_96x54_n256.npz"))
    ref = SampleRef(rt, composer_for(oracle, rt, Inputs(rt, n)))
    out = ref.render(W, H, 3, spp=4, k=np.zeros(n, dtype=np.float32))
    assert np.array_equal(out["rgba"].view(np.uint32), g["acc"].reshape(H, W, 4).view(np.uint32))
    assert np.array_equal(out["packed"], g["packed"].reshape(H, W))
    assert out["queue"] == [0, 0, 0] and [s["k"] for s in out["samples"]] == [0, 1, 2, 3]
    assert all(len(s["trace"]) == 1 for s in out["samples"])


def test_sample_offsets(rt):
    """What the reference's primary() is given: one sample is the pixel centre, four are four places inside the pixel."""
    assert sample_offsets(rt, 1) == [(0.5, 0.5)]
    four = sample_offsets(rt, 4)
    assert len(set(four)) == 4 and all(0.0 < x < 1.0 and 0.0 < y < 1.0 for x, y in four)


# ----------------------------------------------------------------------------- validation without a device
@pytest.fixture()
def host_scene(rt):
    lib = rt.load_library()
    s = lib.rt_scene_create()          # host only: no lists yet (every count 0)
    yield lib, s
    lib.rt_scene_destroy(s)


def test_the_new_symbol_resolves(rt):
    lib = rt.load_library()
    assert lib.rt_scene_set_reflect_samples is not None
    assert (rt.RT_REFLECT_SAMPLES_ONE, rt.RT_REFLECT_SAMPLES_MANY) == (0, 1)
    assert callable(rt.Scene.set_reflect_samples)


def _probe(rt, lib, s):
    """The status of a four-sample reflective frame of width 0. Under the default mode the samples are refused
    (RT_ERR_UNSUPPORTED) before anything else is looked at; under RT_REFLECT_SAMPLES_MANY the request passes that
    check and fails on its size (RT_ERR_INVALID). Neither touches a device."""
    fd = rt.FrameDesc()
    fd.struct_size = C.sizeof(rt.FrameDesc)
    fd.width, fd.height, fd.aspect = 0, 16, 1.0
    fd.opts.struct_size = C.sizeof(rt.LaunchOpts)
    fd.opts.spp = 4
    fd.opts.reflect_depth = 1
    return lib.rt_scene_render(s, C.byref(fd), None)


def test_mode_validation(rt, host_scene):
    lib, s = host_scene
    assert _probe(rt, lib, s) == RT_ERR_UNSUPPORTED                       # the default is ONE
    assert b"sample" in lib.rt_last_error()
    for bad in (-1, 2, 7):
        assert lib.rt_scene_set_reflect_samples(s, bad) == RT_ERR_INVALID
        assert b"rt_scene_set_reflect_samples" in lib.rt_last_error()
        assert _probe(rt, lib, s) == RT_ERR_UNSUPPORTED                   # still ONE
    assert lib.rt_scene_set_reflect_samples(s, rt.RT_REFLECT_SAMPLES_MANY) == RT_OK
    assert _probe(rt, lib, s) == RT_ERR_INVALID                           # the samples pass; the size does not
    assert lib.rt_scene_set_reflect_samples(s, 5) == RT_ERR_INVALID
    assert _probe(rt, lib, s) == RT_ERR_INVALID                           # still MANY after the error
    assert lib.rt_scene_set_reflect_samples(s, rt.RT_REFLECT_SAMPLES_ONE) == RT_OK
    assert _probe(rt, lib, s) == RT_ERR_UNSUPPORTED
    assert lib.rt_scene_set_reflect_samples(None, 0) == RT_ERR_INVALID


def test_python_names(rt):
    sc = rt.Scene()
    try:
        sc.set_reflect_samples("many")
        sc.set_reflect_samples("one")
        sc.set_reflect_samples(rt.RT_REFLECT_SAMPLES_MANY)
        with pytest.raises(rt.RtError):
            sc.set_reflect_samples("several")
        with pytest.raises(rt.RtError):
            sc.set_reflect_samples(3)
    finally:
        sc.close()
