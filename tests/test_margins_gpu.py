"""The margin scenes of tests/margins.py on the GPU: culled kernel at tiles 8 and 16 == brute-force kernel == oracle, bit
for bit in float4 and packed words. The scenes sit on the bounds the culling's exactness ledger rests on;
tests/test_margins_cpu.py checks that they do. Row 1 (starts outside the occluder lists' ball) also at 4 spp and
through a frame graph: the same kernel with other template arguments."""
import ctypes as C
import functools

import numpy as np
import pytest

import margins as M
from scenes import Scn, _bits

pytestmark = pytest.mark.gpu

CASES = [(name, seed) for name, (_, seeds) in M.BUILDERS.items() for seed in seeds]


@functools.lru_cache(maxsize=None)
def _margin(name, seed):
    import oracle_py
    import rt_amd
    return M.BUILDERS[name][0](rt_amd.load(), oracle_py, seed)


def _scn(rt, m):
    cam = rt.Camera(rt.Vec3(*[float(v) for v in m.cam[0]]), rt.Vec3(0, 0, 1), 0.0, float(m.cam[1]), float(m.cam[2]))
    return Scn(rt, m.spheres, lights=m.lights, cam=cam, aspect=m.aspect)


@pytest.mark.parametrize("name,seed", CASES)
def test_margin_scene_culled_equals_brute_force_and_oracle(rt, gpu, name, seed):
    m = _margin(name, seed)
    _scn(rt, m).check(m.w, m.h, tiles=(8, 16))


@pytest.mark.parametrize("seed", M.LIST_BALL_SEEDS[:6])
def test_list_ball_scenes_at_four_samples(rt, gpu, seed):
    m = _margin("list_ball", seed)
    _scn(rt, m).check(m.w, m.h, tiles=(8, 16), spp=4)


@pytest.mark.parametrize("seed", M.LIST_BALL_SEEDS[:6])
def test_list_ball_scenes_through_a_frame_graph(rt, gpu, oracle, seed):
    import torch
    m = _margin("list_ball", seed)
    sc = _scn(rt, m)
    lib = rt.load_library()
    scene = sc.scene()
    acc = torch.zeros((m.h, m.w, 4), dtype=torch.float32, device="cuda")
    pk = torch.zeros((m.h, m.w), dtype=torch.int32, device="cuda")
    host = torch.zeros((m.h, m.w), dtype=torch.int32).pin_memory()
    stream = torch.cuda.Stream()
    fd = scene.frame_desc(m.w, m.h, pixels=pk.data_ptr(), rgba=acc.data_ptr(), cam=sc.cam, aspect=m.aspect)
    gr = lib.rt_graph_capture(scene.handle, C.byref(fd), 1, host.data_ptr(), stream.cuda_stream)
    assert gr, lib.rt_last_error()
    try:
        assert lib.rt_graph_launch(gr, stream.cuda_stream) == 0, lib.rt_last_error()
        stream.synchronize()
    finally:
        lib.rt_graph_destroy(gr)
    rgba, packed, _ = oracle.render(sc.spheres, sc.n, sc.tex, sc.sky, sc.sky_box, sc.lights, sc.n_lights, sc.cam,
                                    m.w, m.h, m.aspect, nthreads=16)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(rgba))
    assert np.array_equal(host.numpy().view(np.uint32), packed)
