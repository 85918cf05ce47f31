"""The indirect pass without a device (rt_scene_indirect): the gather direction against its numpy
restatement and its statistics, the separation of its hash streams, the descriptor's defaults and refusals, the
wrapper's errors and where the new methods sit."""
import ctypes as C

import numpy as np
import pytest

import gloss_ref
import indirect_ref as I

f32 = np.float32
M = 100000


def _vec3s(rt, a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(C.POINTER(rt.Vec3))


def _debug_dir(rt, n, k):
    lib = rt.load_library()
    n, np_ = _vec3s(rt, n)
    k = np.ascontiguousarray(k, dtype=np.uint32)
    G = np.zeros_like(n)
    tries = np.zeros(len(k), dtype=np.int32)
    assert lib.rt_debug_indirect_dir(np_, k.ctypes.data_as(C.POINTER(C.c_uint)), len(k), G.ctypes.data_as(C.POINTER(rt.Vec3)),
                                     tries.ctypes.data_as(C.POINTER(C.c_int))) == 0
    return G, tries


@pytest.fixture(scope="module")
def draws(rt):
    """M seeded (n, key): unit normals, among them the axes and normals with a zero component; keys of pixels, rays and a
    seed, among them 0 and 2^32 - 1. -> n, key, the device code's G and tries."""
    rng = np.random.default_rng(11)
    n = rng.standard_normal((M, 3)).astype(np.float32)
    n[:6] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    n[6:1000, 0] = 0
    n[1000:2000, 1] = 0
    n[2000:2500, 1:] = 0
    n = I._normalise(n)
    k = I.key(rng.integers(0, 4096, M), rng.integers(0, 4096, M), rng.integers(0, 1 << 24, M), np.full(M, 7)).astype(np.uint32)
    k[0], k[1], k[7], k[1001] = 0, 0xffffffff, 0, 0xffffffff
    G, tries = _debug_dir(rt, n, k)
    return n, k, G, tries


def test_direction_equals_the_restatement(rt, draws):
    n, k, G, tries = draws
    want_G, want_tries, u = I.direction(n, k)
    assert np.array_equal(G.view(np.uint32), want_G.view(np.uint32))
    assert np.array_equal(tries, want_tries)
    assert set(np.unique(tries)) >= {1, 2, 3}
    # the point of the sphere is one: |u| within 1.2e-7 of 1 wherever a pair qualified
    lu = np.sqrt((u.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(lu[tries > 0] - 1).max() < 2.4e-7
    assert not u[tries == 0].any()


def test_direction_statistics(draws):
    """Cosine-distributed about n: E[dot] = 2/3 (sd 0.236), E[dot^2] = 1/2 (sd 0.289); the bounds are about five standard
    errors at 10^5 draws. No pair qualifies with probability (1 - pi/4)^6 = 0.98e-4; the bound is ten times that."""
    n, k, G, tries = draws
    d = (G.astype(np.float64) * n.astype(np.float64)).sum(axis=1)
    assert abs(d.mean() - 2 / 3) < 0.004
    assert abs((d * d).mean() - 0.5) < 0.004
    assert (tries == 0).mean() < 1e-3
    assert (I.dot(G, n) > 0).all()
    lg = np.sqrt((G.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(lg - 1).max() <= 4 * 2.0 ** -24


def test_rays_of_a_pixel_are_distinct_and_apart_from_the_gloss_stream(rt):
    rng = np.random.default_rng(3)
    m = 10000
    x, y = rng.integers(0, 4096, m), rng.integers(0, 4096, m)
    base = rng.integers(0, (1 << 24) - 16, m)
    n = I._normalise(rng.standard_normal((m, 3)).astype(np.float32))
    Gs = []
    for j in range(16):
        k = I.key(x, y, base + j, np.full(m, 5)).astype(np.uint32)
        Gs.append(_debug_dir(rt, n, k)[0])
    Gs = np.stack(Gs, axis=1).view(np.uint32)          # [m, 16, 3]
    for a in range(16):
        for b in range(a + 1, 16):
            assert (Gs[:, a] != Gs[:, b]).any(axis=1).all(), (a, b)
    # the first draw of the gather stream against the first draw of the glossy stream of the same key
    # (gloss_ref.draw, which test_gloss_cpu.py holds against rt_debug_gloss): equal by chance only, 2^-24 per key
    k = I.key(x, y, base, np.full(m, 5))
    mine = I.draw(I.mix(k ^ I.SALT), 0, 0)
    gloss = gloss_ref.draw(k.astype(np.uint32), 0, 0)[:, 0]
    assert (mine.view(np.uint32) == np.ascontiguousarray(gloss, dtype=np.float32).view(np.uint32)).sum() <= 3
    # and the keys are the glossy key function's
    assert np.array_equal(k.astype(np.uint32), gloss_ref.key(x, y, base, 5))


# ----------------------------------------------------------------------------- the descriptor
def _desc(rt, lib, **kw):
    """A description that passes every check of its own fields (pointers are never followed before the checks end)."""
    d = rt.IndirectDesc()
    lib.rt_indirect_desc_init(C.byref(d))
    d.width, d.height, d.aspect, d.cam = 64, 32, 1.0, rt.default_camera()
    d.depth, d.normal, d.id, d.albedo = 0x10000, 0x20000, 0x30000, 0x40000
    d.rgba_in, d.rgba_out, d.pixels = 0x50000, 0x60000, 0x70000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_desc_init_gives_the_defaults(rt):
    lib = rt.load_library()
    d = rt.IndirectDesc()
    C.memset(C.byref(d), 0x5a, C.sizeof(d))
    lib.rt_indirect_desc_init(C.byref(d))
    assert d.struct_size == C.sizeof(rt.IndirectDesc)
    assert (d.rays, d.ray_base, d.seed, d.strength, d.cull, d.variant) == (1, 0, 0, 1.0, -1, 0)
    assert (d.width, d.height, d.aspect) == (0, 0, 0.0)
    for k in ("depth", "normal", "id", "albedo", "rgba_in", "rgba_out", "pixels"):
        assert not getattr(d, k)
    assert lib.rt_indirect_desc_init(None) is None


BAD = [("width", dict(width=0)), ("width", dict(width=32769)), ("height", dict(height=-1)), ("height", dict(height=32769)),
       ("depth", dict(depth=0)), ("normal", dict(normal=0)), ("id", dict(id=0)), ("rgba_out", dict(rgba_out=0)),
       ("aligned", dict(depth=0x10002)), ("aligned", dict(normal=0x20008)), ("aligned", dict(id=0x30004)),
       ("aligned", dict(albedo=0x40008)), ("aligned", dict(rgba_in=0x50004)), ("aligned", dict(rgba_out=0x60008)),
       ("aligned", dict(pixels=0x70001)),
       ("rays", dict(rays=0)), ("rays", dict(rays=17)), ("ray_base", dict(ray_base=-1)),
       ("ray_base", dict(ray_base=(1 << 24) - 3, rays=4)), ("cull", dict(cull=2)), ("cull", dict(cull=-2)),
       ("variant", dict(variant=2)), ("variant", dict(variant=-1)),
       ("strength", dict(strength=-0.5)), ("strength", dict(strength=float("nan"))), ("strength", dict(strength=float("inf"))),
       ("aspect", dict(aspect=0.0)), ("aspect", dict(aspect=float("nan"))),
       ("overlaps", dict(rgba_out=0x20000)), ("overlaps", dict(pixels=0x10000)), ("overlaps", dict(rgba_out=0x50010)),
       ("overlap", dict(pixels=0x60000)), ("overlaps", dict(rgba_out=0x40000))]


@pytest.mark.parametrize("name,kw", BAD, ids=[f"{n}-{i}" for i, (n, _) in enumerate(BAD)])
def test_refusals_name_their_field(rt, name, kw):
    lib = rt.load_library()
    s = rt.Scene()
    try:
        assert s.indirect_raw(_desc(rt, lib, **kw)) == 1
        assert name in lib.rt_last_error().decode(), lib.rt_last_error()
    finally:
        s.close()


def test_a_scene_without_sky_is_refused_after_the_fields(rt):
    lib = rt.load_library()
    s = rt.Scene()
    try:
        # every field in range, rgba_out == rgba_in allowed, the optional pointers NULL: only the scene is missing
        for kw in (dict(), dict(rgba_out=0x50000), dict(albedo=0, rgba_in=0, pixels=0), dict(ray_base=(1 << 24) - 4, rays=4)):
            assert s.indirect_raw(_desc(rt, lib, **kw)) == 1
            assert "sky" in lib.rt_last_error().decode()
        assert lib.rt_scene_indirect(None, C.byref(_desc(rt, lib)), None) == 1
        assert lib.rt_scene_indirect(s.handle, None, None) == 1
    finally:
        s.close()


def test_a_shorter_struct_reads_its_tail_as_zero(rt):
    lib = rt.load_library()
    s = rt.Scene()
    try:
        d = _desc(rt, lib, rays=4, strength=2.0)
        d.struct_size = rt.IndirectDesc.rays.offset          # the caller's layout ends before `rays`
        assert s.indirect_raw(d) == 1
        assert "rays" in lib.rt_last_error().decode()
        d.struct_size = 0                                     # 0 reads as this layout: rays = 4 passes, the scene does not
        assert s.indirect_raw(d) == 1
        assert "sky" in lib.rt_last_error().decode()
    finally:
        s.close()


def test_timing_entries_without_a_call(rt):
    lib = rt.load_library()
    s = rt.Scene()
    try:
        s.set_indirect_timing(True)
        assert s.indirect_times() == []
        assert s.indirect_counts() == []
        assert lib.rt_scene_set_indirect_timing(None, 1) == 1
        n = C.c_int(5)
        assert lib.rt_scene_indirect_times(s.handle, None, 4, C.byref(n)) == 1
    finally:
        s.close()


# ----------------------------------------------------------------------------- the wrapper
def test_wrapper_errors_and_where_the_methods_sit(rt):
    import torch
    s = rt.Scene()
    try:
        with pytest.raises(rt.RtError):
            s.indirect({"rgba": None, "aov": {"depth": None, "normal": None}})      # no id, no albedo
        with pytest.raises(rt.RtError):
            s.indirect({"aov": {}})
        if not torch.cuda.is_available():
            with pytest.raises(rt.RtError, match="no GPU"):
                s.indirect({"aov": dict.fromkeys(("depth", "normal", "id", "albedo"))})
        d = s.indirect_desc(640, 360)
        assert (d.width, d.height, d.rays, d.ray_base, d.seed, d.strength, d.cull, d.variant) == (640, 360, 1, 0, 0, 1.0, -1, 0)
        assert d.aspect == f32(rt.default_aspect()) and bytes(d.cam) == bytes(rt.default_camera())
        d = s.indirect_desc(8, 4, rays=3, ray_base=5, seed=9, strength=0.75, cull=0, variant=1, aspect=1.25)
        assert (d.rays, d.ray_base, d.seed, d.strength, d.cull, d.variant, d.aspect) == (3, 5, 9, 0.75, 0, 1, 1.25)
    finally:
        s.close()
    names = list(vars(rt.Scene))
    last = names.index("denoise_times")
    for n in ("indirect_desc", "indirect_raw", "indirect", "set_indirect_timing", "indirect_times"):
        assert names.index(n) > last, n


def test_every_new_header_function_is_exported(rt):
    lib = rt.load_library()
    for n in ("rt_indirect_desc_init", "rt_scene_indirect", "rt_scene_set_indirect_timing", "rt_scene_indirect_times",
              "rt_debug_indirect_dir", "rt_debug_indirect_counts"):
        assert hasattr(lib, n), n
    assert C.sizeof(rt.IndirectDesc) == 136 and rt.IndirectDesc.depth.offset == 56 and rt.IndirectDesc.rays.offset == 112
