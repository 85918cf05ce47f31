"""The view-list margin scenes of tests/view_margins.py on the GPU: the culled kernel reading the view lists == the
culled kernel with the lists off == the brute-force kernel == the oracle, bit for bit in float4 and packed words, at
every tile shape that nests in the view's blocks; the launch did read the lists, the device builder's lists are the
host builder's, overflowed and unbuilt blocks counted alike. tests/test_view_margins_cpu.py checks that the scenes sit
on the bounds they name. The unbuilt blocks and a few corner scenes also through a frame graph, which builds its own
lists in a node."""
import ctypes as C
import functools

import numpy as np
import pytest

import view_margins as V
from scenes import Scn, _bits

pytestmark = pytest.mark.gpu

CASES = [(name, seed) for name, (_, seeds) in V.BUILDERS.items() for seed in seeds]


@functools.lru_cache(maxsize=None)
def _margin(name, seed):
    import oracle_py
    import rt_amd
    return V.BUILDERS[name][0](rt_amd.load(), oracle_py, seed)


def _scn(rt, m):
    return Scn(rt, m.spheres, lights=m.lights, cam=V.camera(rt, m.cam), aspect=m.aspect)


def _oracle(rt, oracle, sc, m):
    """float4 sums and packed words of the margin's band as the product defines them: float32 adds in sample order,
    divided by float(spp) and packed by the reference."""
    y0, y1 = m.band or (0, m.h)
    acc = packed = None
    for ox, oy in V.offsets(rt, m.spp):
        rgba, packed, _ = oracle.render(sc.spheres, sc.n, sc.tex, sc.sky, sc.sky_box, sc.lights, sc.n_lights, sc.cam,
                                        m.w, m.h, m.aspect, y0=y0, y1=y1, off=(ox, oy), nthreads=16)
        acc = rgba if acc is None else (acc + rgba).astype(np.float32)
    if m.spp > 1:
        mean = (acc[..., :3] / np.float32(m.spp)).astype(np.float32).reshape(-1, 3)
        olib = oracle.load()
        packed = np.array([olib.oracle_pack_color(float(r), float(g), float(b)) for r, g, b in mean],
                          dtype=np.uint32).reshape(acc.shape[:2])
    return _bits(acc), packed


def _frame(scene, sc, m, **kw):
    import torch
    y0, y1 = m.band or (0, 0)
    out = scene.render(m.w, m.h, y0=y0, y1=y1, spp=m.spp, cam=sc.cam, aspect=m.aspect, **kw)
    torch.cuda.synchronize()
    return _bits(out["rgba"].cpu().numpy()), out["packed"].cpu().numpy().view(np.uint32)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), "float4 differs: %s (%d pixels)" % (what, int((got[0] != want[0]).any(axis=2).sum()))
    assert np.array_equal(got[1], want[1]), "packed differs: %s (%d pixels)" % (what, int((got[1] != want[1]).sum()))


@pytest.mark.parametrize("name,seed", CASES)
def test_view_margin_scene_lists_on_off_brute_force_and_oracle(rt, gpu, oracle, name, seed):
    m = _margin(name, seed)
    sc = _scn(rt, m)
    scene = sc.scene()
    want = _oracle(rt, oracle, sc, m)
    host = V.host_view(rt, m)
    tab = V.table(m.spheres)
    for tile in m.tiles:
        what = "%s seed %d tile %d" % (name, seed, tile)
        on = _frame(scene, sc, m, cull=True, tile=tile)
        info = scene.view_lists_info(want_lists=True)
        assert info["read"] == 1, (what, info)
        assert info["overflowed"] == host["overflowed"] and info["not_built"] == host["not_built"], (what, info)
        V.assert_lists_equal(info, host, tab)
        scene.set_view_lists(0)
        off = _frame(scene, sc, m, cull=True, tile=tile)
        assert scene.view_lists_info()["read"] == 0
        scene.set_view_lists(1)
        brute = _frame(scene, sc, m, cull=False, tile=tile)
        _same(on, want, what + ", lists on against the oracle")
        _same(off, want, what + ", lists off against the oracle")
        _same(brute, want, what + ", brute force against the oracle")


GRAPH_CASES = [("view_not_built", s) for s in V.BUILDERS["view_not_built"][1]] + [("view_corner", s) for s in (0, 3, 13, 18, 29)] \
    + [("view_sample_edge", s) for s in (0, 3)]


@pytest.mark.parametrize("name,seed", GRAPH_CASES)
def test_view_margin_scene_through_a_frame_graph(rt, gpu, oracle, name, seed):
    import torch
    m = _margin(name, seed)
    assert m.band is None
    sc = _scn(rt, m)
    lib = rt.load_library()
    scene = sc.scene()
    acc = torch.zeros((m.h, m.w, 4), dtype=torch.float32, device="cuda")
    pk = torch.zeros((m.h, m.w), dtype=torch.int32, device="cuda")
    host = torch.zeros((m.h, m.w), dtype=torch.int32).pin_memory()
    stream = torch.cuda.Stream()
    fd = scene.frame_desc(m.w, m.h, pixels=pk.data_ptr(), rgba=acc.data_ptr(), cam=sc.cam, aspect=m.aspect, tile=8)
    gr = lib.rt_graph_capture(scene.handle, C.byref(fd), m.spp, host.data_ptr(), stream.cuda_stream)
    assert gr, lib.rt_last_error()
    try:
        assert lib.rt_graph_launch(gr, stream.cuda_stream) == 0, lib.rt_last_error()
        stream.synchronize()
    finally:
        lib.rt_graph_destroy(gr)
    want = _oracle(rt, oracle, sc, m)
    _same((_bits(acc.cpu().numpy()), host.numpy().view(np.uint32)), want, "%s seed %d through the graph" % (name, seed))
