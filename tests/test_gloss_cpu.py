"""Glossy reflections (rt_scene_set_roughness), host side: rf_gloss and the key through their host debug
entries against the numpy restatement of tests/gloss_ref.py bit for bit, the statistics of the ball from the restatement
alone, the refusals and clearing rules of the roughness tables, and the layouts."""
import ctypes as C
import math

import numpy as np
import pytest

import gloss_ref as G

f32 = np.float32
FALLBACK = (1.0 - math.pi / 6.0) ** 4      # four draws of the cube [-1, 1)^3 all miss the unit ball


def _vec3s(rt, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    arr = (rt.Vec3 * a.shape[0])()
    np.frombuffer(arr, dtype=np.float32).reshape(-1, 3)[:] = a
    return arr


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint))


def _dev_gloss(rt, R, N, rho, key, b):
    lib = rt.load_library()
    m = R.shape[0]
    out = (rt.Vec3 * m)()
    what = np.zeros(m, dtype=np.int32)
    rho = np.ascontiguousarray(rho, dtype=np.float32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.int32)
    assert lib.rt_debug_gloss(_vec3s(rt, R), _vec3s(rt, N), rho.ctypes.data_as(C.POINTER(C.c_float)), _up(key),
                              b.ctypes.data_as(C.POINTER(C.c_int)), m, out, what.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return np.frombuffer(out, dtype=np.float32).reshape(m, 3).copy(), what


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_mix_known_answers():
    assert [int(v) for v in G.mix(np.array([0, 1, 2, 0xffffffff], dtype=np.uint32))] == \
        [0, 0x688990c0, 0xd1132181, 0x6768824a]


def test_key_equals_the_restatement(rt):
    lib = rt.load_library()
    rng = np.random.default_rng(3)
    m = 20000
    a = [rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    a[0][:5000] = rng.integers(0, 4096, 5000)          # pixel-sized coordinates and small sample indices too
    a[1][:5000] = rng.integers(0, 4096, 5000)
    a[2][:5000] = rng.integers(0, 64, 5000)
    a[3][:2500] = 0
    out = np.zeros(m, dtype=np.uint32)
    assert lib.rt_debug_gloss_key(_up(a[0]), _up(a[1]), _up(a[2]), _up(a[3]), m, _up(out)) == 0
    assert np.array_equal(out, G.key(*a))
    # the key separates its four inputs
    assert len({int(G.key(1, 2, 3, 4)[0]), int(G.key(2, 1, 3, 4)[0]), int(G.key(1, 2, 4, 3)[0]), int(G.key(3, 2, 1, 4)[0])}) == 4


def test_gloss_equals_the_restatement(rt):
    rng = np.random.default_rng(17)
    m = 100000
    N = _unit(rng.standard_normal((m, 3)))
    R = _unit(rng.standard_normal((m, 3)))
    # grazing R: almost in the surface's plane, a hair to either side of it
    t = _unit(np.cross(N[:20000], rng.standard_normal((20000, 3))))
    R[:20000] = _unit(t + N[:20000] * rng.uniform(-1e-3, 1e-3, (20000, 1)))
    rho = rng.uniform(0, 1, m).astype(np.float32)
    rho[rng.integers(0, m, 10000)] = 0
    rho[rng.integers(0, m, 10000)] = 1
    rho[rng.integers(0, m, 2000)] = 0.05
    nan = rng.integers(0, m, 600)
    R[nan[:200], rng.integers(0, 3, 200)] = np.nan
    N[nan[200:400], rng.integers(0, 3, 200)] = np.nan
    R[nan[400:500]] = 0                                 # a zero mirror direction (G may be 0 where rho is 0 too)
    rho[nan[500:]] = np.nan
    key = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 9, m).astype(np.int32)
    got, what = _dev_gloss(rt, R, N, rho, key, b)
    ref, ref_what = G.gloss(R, N, rho, key, b)
    assert np.array_equal(what, ref_what)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # the inputs cover what they are meant to
    assert int((ref_what == 0).sum()) >= 5000 and int(((ref_what & G.HALVED) != 0).sum()) >= 2000
    assert int(((ref_what & G.REJECTED) != 0).sum()) >= 5000
    acc = (ref_what & (G.PERTURBED | G.REJECTED)) == G.PERTURBED
    assert int(acc.sum()) >= 50000 and (got[acc].view(np.uint32) != R[acc].view(np.uint32)).any(axis=1).mean() > 0.99
    # rho == 0, a rejected R' and a NaN leave R as it is, bit for bit
    same = (ref_what == 0) | ((ref_what & G.REJECTED) != 0)
    assert np.array_equal(got[same].view(np.uint32), R[same].view(np.uint32))
    assert ((ref_what[nan[:400]] & G.REJECTED) != 0).all() or (rho[nan[:400]] == 0).any()


def test_ball_statistics():
    """96 x 54 pixels x 16 samples x 4 hits, seed 0."""
    px, py, s = np.meshgrid(np.arange(96), np.arange(54), np.arange(16), indexing="ij")
    key = G.key(px.reshape(-1), py.reshape(-1), s.reshape(-1), 0)
    us, halved = [], []
    for b in range(4):
        u, h = G.ball(key, b)
        us.append(u)
        halved.append(h)
    u, h = np.concatenate(us), np.concatenate(halved)
    assert u.shape[0] == 331776
    for t in range(4):
        d = G.draw(key, 0, t)
        assert d.min() >= -1 and d.max() < 1
    len2 = (u.astype(np.float64) ** 2).sum(axis=1)
    assert len2.max() <= 1.0
    assert abs(h.mean() - FALLBACK) <= 0.005, h.mean()
    assert np.abs(u.astype(np.float64).mean(axis=0)).max() <= 0.01
    # draws of different hits, samples and seeds are different draws
    assert not np.array_equal(us[0], us[1])
    assert not np.array_equal(G.ball(G.key(px.reshape(-1), py.reshape(-1), s.reshape(-1), 1), 0)[0], us[0])


def test_layouts(rt):
    lib = rt.load_library()
    assert lib.rt_debug_reflect_entry_size() == 48
    assert C.sizeof(rt.Material) == 12 and C.sizeof(rt.MaterialEx) == 16
    assert rt.Material.roughness.offset == 8 and rt.MaterialEx.roughness.offset == 8 and rt.MaterialEx.ior.offset == 12


def _planes(rt, n):
    lib = rt.load_library()
    p = (rt.Plane * n)()
    for i in range(n):
        lib.rt_plane_init(C.byref(p[i]), 0.0, -4.0 - i, 0.0, 0.0, 1.0, 0.0)
    return p


def _cubes(rt, n):
    lib = rt.load_library()
    c = (rt.Cube * n)()
    for i in range(n):
        lib.rt_cube_init(C.byref(c[i]), 3.0 * i, 0.0, 0.0, 3.0 * i + 1.0, 1.0, 1.0)
    return c


def _set(rt, sc, kind, values):
    """The return code of rt_scene_set_roughness, called directly."""
    lib = rt.load_library()
    if values is None:
        return lib.rt_scene_set_roughness(sc.handle, kind, None, 0)
    v = np.ascontiguousarray(values, dtype=np.float32)
    return lib.rt_scene_set_roughness(sc.handle, kind, v.ctypes.data_as(C.POINTER(C.c_float)), v.shape[0])


KINDS = {"sphere": 1, "plane": 2, "cube": 3}          # RT_HIT_SPHERE, RT_HIT_PLANE, RT_HIT_CUBE
INVALID, UNSUPPORTED = 1, 2                            # RT_ERR_INVALID, RT_ERR_UNSUPPORTED


def set_list(rt, sc, kind, n):
    {"sphere": lambda: sc.set_spheres(rt.generate_spheres(n, 1), n), "plane": lambda: sc.set_planes(_planes(rt, n), n),
     "cube": lambda: sc.set_cubes(_cubes(rt, n), n)}[kind]()


def takes(rt, sc, kind, values):
    """Whether the kind's table takes `values` (anything else must be RT_ERR_INVALID)."""
    rc = _set(rt, sc, KINDS[kind], values)
    assert rc in (0, INVALID)
    return rc == 0


def check_table_rules(rt, sc, kind, n):
    """The refusals and clearing rules of one kind's table on a scene whose list of that kind has n entries (n = 0: a
    scene without a device, where no list can be set). Leaves the table cleared."""
    lib = rt.load_library()
    code = KINDS[kind]
    good = np.resize(np.array([0.0, 0.05, 0.3, 1.0], dtype=np.float32), max(n, 1))
    if n > 0:
        assert _set(rt, sc, code, good) == 0
        bads = [good[:-1], np.append(good, 0.5)]
        for v in (-0.01, 1.0001, np.nan, np.inf, -np.inf):
            b = good.copy()
            b[n // 2] = v
            bads.append(b)
    else:
        bads = [good, [0.0, 0.0]]                       # a list of 0 takes no values at all
    for bad in bads:
        assert _set(rt, sc, code, bad) == INVALID, bad
        assert b"rt_scene_set_roughness" in lib.rt_last_error()
    if n > 0:                                           # nothing changed on those errors: the same table is no change
        assert _set(rt, sc, code, good) == 0
    assert _set(rt, sc, 0, good) == INVALID             # RT_HIT_TRIANGLE
    assert _set(rt, sc, 7, None) == INVALID and _set(rt, sc, -1, None) == INVALID
    assert _set(rt, sc, code, None) == 0 and _set(rt, sc, code, None) == 0        # clearing always succeeds
    assert lib.rt_scene_set_roughness(sc.handle, code, good.ctypes.data_as(C.POINTER(C.c_float)), 0) == 0
    assert lib.rt_scene_set_roughness(None, code, None, 0) == INVALID
    assert lib.rt_scene_set_gloss_seed(None, 1) == INVALID
    for seed in (1, 0xffffffff, 0):
        assert lib.rt_scene_set_gloss_seed(sc.handle, seed) == 0
    # the wrapper: names, None, and errors as RtError
    if n > 0:
        sc.set_roughness(kind, good)
        sc.set_roughness(code, list(good))
    sc.set_roughness(kind, None)
    sc.set_roughness(kind, [])
    sc.set_gloss_seed(2 ** 32 + 5)
    sc.set_gloss_seed(0)
    with pytest.raises(rt.RtError):
        sc.set_roughness(kind, np.append(good, 0.5))
    with pytest.raises(rt.RtError):
        sc.set_roughness("triangle", good)
    if n > 0:                                           # the material entries keep refusing a roughness field
        m = (rt.Material * n)()
        m[n - 1].roughness = 0.1
        entry = {"sphere": "rt_scene_set_materials", "plane": "rt_scene_set_plane_materials",
                 "cube": "rt_scene_set_cube_materials"}[kind]
        assert getattr(lib, entry)(sc.handle, m, n) == UNSUPPORTED
        if kind == "sphere":
            mx = (rt.MaterialEx * n)()
            mx[0].roughness = 0.1
            assert lib.rt_scene_set_materials_ex(sc.handle, mx, n) == UNSUPPORTED


def check_count_rules(rt, sc, kind):
    """A table survives its list being set again with the same count and is cleared by a new count (needs a device)."""
    set_list(rt, sc, kind, 4)
    assert takes(rt, sc, kind, [0.1, 0.2, 0.3, 0.4]) and not takes(rt, sc, kind, [0.1, 0.2, 0.3])
    set_list(rt, sc, kind, 4)
    assert takes(rt, sc, kind, [0.1, 0.2, 0.3, 0.4])
    set_list(rt, sc, kind, 3)                           # (what the frames read after this is the GPU tests' matter)
    assert takes(rt, sc, kind, [0.1, 0.2, 0.3]) and not takes(rt, sc, kind, [0.1, 0.2, 0.3, 0.4])
    assert _set(rt, sc, KINDS[kind], None) == 0


@pytest.mark.parametrize("kind", ["sphere", "plane", "cube"])
def test_refusals_and_clearing(rt, kind):
    """The tables are host state until a reflective frame is launched, so the rules hold without a device; the lists
    themselves are device arrays, so where there is no device the scene's lists stay empty and the rules are checked
    against a count of 0 (tests/test_gloss_gpu.py runs the same checks against lists that exist)."""
    sc = rt.Scene()
    n = 5
    try:
        set_list(rt, sc, kind, n)
    except rt.RtError:
        n = 0
    check_table_rules(rt, sc, kind, n)
    if n:
        check_count_rules(rt, sc, kind)
    sc.close()
