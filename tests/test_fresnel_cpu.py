"""Fresnel glass (rt_scene_set_glass_model), host side: rf_fresnel and the choice through their host debug
entries against the numpy restatement of tests/fresnel_ref.py bit for bit, the reflectance against float64 physics, the
statistics of the draw from the restatement alone, the sense in which the estimator is unbiased (a frame's pixel is the
forced-reflect or the forced-transmit frame's pixel, never a reweighted one), the setting's rules and the layouts."""
import ctypes as C
import math

import numpy as np
import pytest

import fresnel_ref as FR
import gloss_ref as G
from scenes import Inputs
from test_reflect_cpu import nearest, normalise, sphere_table
from test_refract_cpu import _one_sphere, _rand_unit, _transmit_rays

f32 = np.float32
IORS = (1.0, 1.33, 1.5, 2.4, 4.0)
K_TABLE = (0.0, 0.25, 0.5, 1.0)
INVALID = 1                                            # RT_ERR_INVALID


def glass_mats(n):
    """tau = 0.8 on i % 4 == 2 with ior alternating 1.5 / 2.4 over the glass spheres; K_TABLE elsewhere."""
    tau = np.array([0.8 if i % 4 == 2 else 0.0 for i in range(n)], dtype=np.float32)
    ior = np.array([(1.5, 2.4)[(i // 4) % 2] if i % 4 == 2 else 0.0 for i in range(n)], dtype=np.float32)
    k = np.array([0.0 if i % 4 == 2 else K_TABLE[i % 4] for i in range(n)], dtype=np.float32)
    return k, tau, ior


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _same_floats(a, b):
    """Bit for bit, a NaN equal to any NaN (0 / 0 has no payload the restatement could promise)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _dev_fresnel(rt, c, ior):
    lib = rt.load_library()
    c = np.ascontiguousarray(c, dtype=np.float32)
    ior = np.ascontiguousarray(np.broadcast_to(np.asarray(ior, dtype=np.float32), c.shape))
    out = np.zeros(c.shape[0], dtype=np.float32)
    assert lib.rt_debug_fresnel(_fp(c), _fp(ior), c.shape[0], _fp(out)) == 0
    return out


def _dev_choice(rt, sph, O, D, ior, rho, key, b):
    lib = rt.load_library()
    m = O.shape[0]
    rays = (rt.Ray * m)()
    buf = np.frombuffer(rays, dtype=np.float32).reshape(m, 6)
    buf[:, :3], buf[:, 3:] = O, D
    out = (rt.Ray * m)()
    ior = np.ascontiguousarray(np.broadcast_to(np.asarray(ior, dtype=np.float32), (m,)))
    rho = np.ascontiguousarray(rho, dtype=np.float32)
    key = np.ascontiguousarray(key, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.int32)
    choice = np.zeros(m, dtype=np.int32)
    what = np.zeros(m, dtype=np.int32)
    F = np.zeros(m, dtype=np.float32)
    u = np.zeros(m, dtype=np.float32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    assert lib.rt_debug_glass_choice(C.byref(sph), _fp(ior), _fp(rho), key.ctypes.data_as(C.POINTER(C.c_uint)), ip(b), rays, m,
                                     out, ip(choice), _fp(F), _fp(u), ip(what)) == 0
    ob = np.frombuffer(out, dtype=np.float32).reshape(m, 6).copy()
    return ob[:, :3], ob[:, 3:], choice, F, u, what


# ----------------------------------------------------------------------------- the reflectance
def test_fresnel_equals_the_restatement(rt):
    rng = np.random.default_rng(31)
    m = 100000
    c = rng.uniform(0, 1, m).astype(np.float32)
    c[:3000] = rng.choice(np.array([0.0, 1.0, np.nextafter(f32(1), f32(2)), 1e-7, 1e-3], dtype=np.float32), 3000)
    c[3000:6000] = np.abs(rng.standard_normal(3000) * 1e-3).astype(np.float32)          # grazing
    ior = rng.choice(np.array(IORS, dtype=np.float32), m)
    ior[50000:] = rng.uniform(1, 4, m - 50000).astype(np.float32)
    c[-200:-100] = np.nan
    ior[-100:] = np.nan
    got = _dev_fresnel(rt, c, ior)
    want = FR.fresnel(c, ior)
    assert _same_floats(got, want)
    for v in (0.0, 1.0, float(np.nextafter(f32(1), f32(2)))):
        for n in IORS:
            assert ((c == f32(v)) & (ior == f32(n))).any(), (v, n)
    assert np.isnan(got[-200:]).all()
    # the figures the cosines of the glass test scenes give: the minimum of F is its value at normal incidence
    assert abs(float(_dev_fresnel(rt, [1.0], 1.5)[0]) - 0.04) < 1e-6
    assert abs(float(_dev_fresnel(rt, [1.0], 2.4)[0]) - (1.4 / 3.4) ** 2) < 1e-6


def test_fresnel_physics(rt):
    """In float64, from the binary32 results. F(c, 1) is 0 up to rounding for c >= 0.01: the radicand 1 - (1 - c*c) -- the
    one rf_refract forms -- keeps c*c only to the 2^-24 that 1 - c*c was rounded to, so that ct is c within 2^-25 / c^2
    relative, rs within half of that and F within its square: a bound of 1e-7 at c = 0.01 (5e-9 is what occurs) and of
    1e-3 at c = 1e-3 (5e-5 occurs), so that the 1e-6 asked of F(., 1) is asked where the cosine is at least 0.01."""
    c = np.linspace(0.0, 1.0, 4001).astype(np.float32)
    for n in (1.33, 1.5, 2.4, 3.7, 4.0):
        F = _dev_fresnel(rt, c, n).astype(np.float64)
        assert abs(F[-1] - ((n - 1) / (n + 1)) ** 2) < 1e-6, n                      # F(1, n)
        assert F[0] == 1.0, n                                                        # F(0, n)
        assert F.max() <= 1.0
        if n < 2 + math.sqrt(3):
            # it falls as the cosine grows. The exact unpolarised reflectance does so up to n = 2 + sqrt(3) = 3.73 only:
            # beyond, rp's fall towards Brewster's angle outweighs rs's rise at first (float64: at n = 4 it dips 0.0022
            # below F(1, 4) = 0.36, near c = 0.54), which the comparison with the float64 formula below covers
            assert (np.diff(F) <= 1e-6).all(), n
            assert F.min() >= F[-1] - 1e-6
        else:
            assert 0.0020 < F[-1] - F.min() < 0.0024 and abs(float(c[F.argmin()]) - 0.538) < 0.01
        # against the float64 formula
        cd = c.astype(np.float64)
        ct = np.sqrt(1 - (1 - cd * cd) / (n * n))
        want = 0.5 * (((cd - n * ct) / (cd + n * ct)) ** 2 + ((ct - n * cd) / (ct + n * cd)) ** 2)
        assert np.abs(F - want).max() < 2e-5, n
    c1 = np.linspace(0.01, 1.0, 4001).astype(np.float32)
    F1 = _dev_fresnel(rt, c1, 1.0).astype(np.float64)
    print("max F(c, 1) over c in [0.01, 1]:", F1.max())
    assert (F1 < 1e-6).all() and (F1 >= 0).all()


# ----------------------------------------------------------------------------- the choice
def _choice_case(rt, rng, R, m, ior, tiny=False):
    c = rng.uniform(-1, 1, 3) if not tiny else np.zeros(3)
    sph = _one_sphere(rt, c, R)
    tab = sphere_table((sph,), 1)
    if tiny:     # rule 3: P = new_org - 1e-5 N lies beyond a sphere of radius ~1e-6 (tests/test_refract_cpu.py)
        D = normalise(np.c_[rng.uniform(-R, R, (m, 2)), np.full(m, 1e-4)].astype(np.float32))
        O = np.tile(np.array([0.0, 0.0, -1e-4], dtype=np.float32), (m, 1))
    else:
        Reff = float(np.sqrt(np.float64(tab[0, 3])))
        O, D, _ = _transmit_rays(rng, tab[0, :3].astype(np.float64), Reff, m, sin_max=0.9999, dmax=min(300.0, 30.0 * Reff))
    rho = rng.choice(np.array([0.0, 0.05, 0.3, 1.0], dtype=np.float32), m)
    key = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 9, m).astype(np.int32)
    got = _dev_choice(rt, sph, O, D, ior, rho, key, b)
    idx, t = nearest(O, D, tab)
    hit = idx >= 0
    assert (got[2][~hit] == -1).all()
    Oh, Dh = O[hit], D[hit]
    with np.errstate(all="ignore"):
        new_org = (Oh + Dh * t[hit][:, None]).astype(np.float32)
    N = normalise((new_org - tab[0, :3]).astype(np.float32))
    start = (N * f32(0.00001) + new_org).astype(np.float32)
    (ro, rd, choice, F, u, what), plain = FR.glass_choice(Dh, N, start, new_org, np.repeat(tab, int(hit.sum()), 0), ior,
                                                          rho[hit], key[hit], b[hit])
    assert np.array_equal(got[2][hit], choice)
    assert np.array_equal(got[5][hit], what)
    assert _same_floats(got[3][hit], F) and _same_floats(got[4][hit], u)
    assert _same_floats(got[0][hit].reshape(-1), ro.reshape(-1)) and _same_floats(got[1][hit].reshape(-1), rd.reshape(-1))
    return choice, what, rho[hit], (ro, rd, plain, Dh, start)


def test_glass_choice_equals_the_restatement(rt):
    rng = np.random.default_rng(33)
    seen = {c: 0 for c in (FR.RULE1, FR.REFLECTED, FR.THROUGH, FR.RULE3)}
    pert = {FR.REFLECTED: 0, FR.THROUGH: 0}
    total = 0
    for R in (0.1, 1.0, 10.0):
        for ior in IORS[:4]:
            choice, what, rho, (ro, rd, plain, D, start) = _choice_case(rt, rng, R, 9000, ior)
            total += choice.shape[0]
            for c in seen:
                seen[c] += int((choice == c).sum())
            for c in pert:
                pert[c] += int(((choice == c) & ((what & (G.PERTURBED | G.REJECTED)) == G.PERTURBED)).sum())
            # a ray through a sphere without roughness is the plain glass step's, a reflected one starts at start_O
            smooth = (choice == FR.THROUGH) & (rho == 0)
            assert np.array_equal(rd[smooth].view(np.uint32), plain[1][smooth].view(np.uint32))
            assert np.array_equal(ro[choice == FR.THROUGH].view(np.uint32), plain[0][choice == FR.THROUGH].view(np.uint32))
            assert np.array_equal(ro[choice == FR.REFLECTED].view(np.uint32), start[choice == FR.REFLECTED].view(np.uint32))
            assert (what[rho == 0] == 0).all()
    for R in (1e-6, 2e-6, 4e-6):
        choice, what, _, _ = _choice_case(rt, rng, R, 4000, 1.5, tiny=True)
        total += choice.shape[0]
        seen[FR.RULE3] += int((choice == FR.RULE3).sum())
        assert (what[choice == FR.RULE3] == 0).all()                                # rule 3 leaves undeviated: no draw of rf_gloss
    assert total >= 100000
    assert seen[FR.REFLECTED] >= 5000 and seen[FR.THROUGH] >= 50000 and seen[FR.RULE3] >= 500, seen
    assert pert[FR.REFLECTED] >= 2000 and pert[FR.THROUGH] >= 20000, pert
    # rule 1: intersect()'s `t == 0` case -- the origin on the far surface, looking out; nothing is drawn
    sph = _one_sphere(rt, (0.0, 0.0, 0.0), 1.0)
    one = np.array([[0, 0, 1]], dtype=np.float32)
    ro, rd, choice, F, u, what = _dev_choice(rt, sph, one, one, 1.5, [1.0], [12345], [0])
    assert choice[0] == FR.RULE1 and F[0] == 0 and u[0] == 0 and what[0] == 0 and np.array_equal(rd, one)


def test_the_forced_branches_of_the_restatement():
    rng = np.random.default_rng(35)
    m = 2000
    tab = np.tile(np.array([[0, 0, 0, 1]], dtype=np.float32), (m, 1))
    new_org = normalise(_rand_unit(rng, m).astype(np.float32))
    N = new_org.copy()
    D = normalise((-N + 0.8 * _rand_unit(rng, m)).astype(np.float32))
    start = (N * f32(0.00001) + new_org).astype(np.float32)
    key = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    args = (D, N, start, new_org, tab, 1.5, np.zeros(m, dtype=np.float32), key, 0)
    free, _ = FR.glass_choice(*args)
    refl, _ = FR.glass_choice(*args, force="reflect")
    thru, plain = FR.glass_choice(*args, force="transmit")
    assert (refl[2] == FR.REFLECTED).all() and (thru[2] == FR.THROUGH).all()
    assert 20 <= int((free[2] == FR.REFLECTED).sum()) <= m - 20
    assert np.array_equal(thru[1].view(np.uint32), plain[1].view(np.uint32))
    r = free[2] == FR.REFLECTED
    assert np.array_equal(free[1][r].view(np.uint32), refl[1][r].view(np.uint32))
    assert np.array_equal(free[1][~r].view(np.uint32), thru[1][~r].view(np.uint32))
    for a in (refl, thru):                                   # F and u are recorded whatever the branch
        assert np.array_equal(a[3], free[3]) and np.array_equal(a[4], free[4])


# ----------------------------------------------------------------------------- the draw
def test_draw_statistics():
    """10^5 keys x b = 0 .. 8, from the restatement alone."""
    rng = np.random.default_rng(37)
    m = 100000
    key = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)
    key[:5184] = G.key(*(a.reshape(-1) for a in np.meshgrid(np.arange(96), np.arange(54), indexing="ij")), 0, 0)   # a frame's
    us = [FR.draw(key, b) for b in range(9)]
    u = np.concatenate(us)
    n = u.shape[0]
    assert u.min() >= 0 and u.max() < 1
    assert abs(float(u.astype(np.float64).mean()) - 0.5) <= 0.005
    for F in (0.04, 0.17, 0.5):
        share = float((u < f32(F)).mean())
        assert abs(share - F) <= 5 * math.sqrt(F * (1 - F) / n), (F, share)
    assert not np.array_equal(us[0], us[1])
    # the stream is apart from the gloss draws of the same (key, b): as 24-bit integers, equal no more often than chance
    # (9 * 10^5 draws x 12 components x 2^-24 = 0.64 expected)
    equal = 0
    for b in range(9):
        ui = (us[b].astype(np.float64) * 2.0 ** 24).astype(np.int64)
        for t in range(4):
            gi = ((G.draw(key, b, t).astype(np.float64) + 1.0) * 2.0 ** 23).astype(np.int64)
            equal += int((gi == ui[:, None]).sum())
    assert equal <= 6, equal


# ----------------------------------------------------------------------------- the composed reference
W0, H0, N0 = 48, 27, 128


def _composer(rt, oracle, n, rho=None, seed=0):
    return FR.fresnel_composer_for(oracle, rt, Inputs(rt, n)).set_gloss(sphere=rho, seed=seed)


def test_depth_one_is_one_forced_frame_per_pixel(rt, oracle):
    """The choice alone differs, never a weight: every pixel of the stochastic frame is the forced-reflect frame's where
    the trace says reflect and the forced-transmit frame's elsewhere."""
    k, tau, ior = glass_mats(N0)
    rho = np.where(tau > 0, 0.3, 0.0).astype(np.float32)                             # frosted: both branches perturbed
    comp = _composer(rt, oracle, N0, rho, seed=4)
    free = comp.set_glass_model().render(W0, H0, k, 1, tau=tau, ior=ior)
    trace = comp.fresnel_trace
    refl = comp.set_glass_model(force="reflect").render(W0, H0, k, 1, tau=tau, ior=ior)
    thru = comp.set_glass_model(force="transmit").render(W0, H0, k, 1, tau=tau, ior=ior)
    assert {t["b"] for t in trace} == {0}
    r = FR.reflected_pixels(trace, W0 * H0).reshape(H0, W0)
    assert FR.count(trace, FR.REFLECTED) >= 10 and FR.count(trace, FR.THROUGH) >= 50
    want = np.where(r[..., None], refl[0], thru[0])
    assert np.array_equal(free[0].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(free[1], np.where(r, refl[1], thru[1]))
    differ = (refl[0].view(np.uint32) != thru[0].view(np.uint32)).any(axis=2)
    assert int((differ & r).sum()) >= 10                                              # and the branches are different frames


def test_forced_transmission_and_the_plain_model_are_the_glass_composer(rt, oracle):
    k, tau, ior = glass_mats(N0)
    rho = np.where(tau > 0, 0.0, 0.3).astype(np.float32)                             # rough mirrors, clear glass
    want = G.gloss_composer_for(oracle, rt, Inputs(rt, N0), glass=True).set_gloss(sphere=rho, seed=4) \
        .render(W0, H0, k, 3, tau=tau, ior=ior)
    comp = _composer(rt, oracle, N0, rho, seed=4)
    got = comp.set_glass_model(force="transmit").render(W0, H0, k, 3, tau=tau, ior=ior)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    assert FR.count(comp.fresnel_trace, FR.THROUGH) >= 100 and FR.count(comp.fresnel_trace, FR.REFLECTED) == 0
    # the plain model: roughness on the glass itself changes nothing either
    comp.set_gloss(sphere=np.full(N0, 0.3, dtype=np.float32), seed=4)
    want = G.gloss_composer_for(oracle, rt, Inputs(rt, N0), glass=True).set_gloss(sphere=np.full(N0, 0.3), seed=4) \
        .render(W0, H0, k, 3, tau=tau, ior=ior)
    got = comp.set_glass_model(FR.PLAIN).render(W0, H0, k, 3, tau=tau, ior=ior)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])
    assert comp.fresnel_trace == []
    # and the Fresnel model is another frame
    free = comp.set_glass_model().render(W0, H0, k, 3, tau=tau, ior=ior)
    assert not np.array_equal(free[0].view(np.uint32), want[0].view(np.uint32))


# ----------------------------------------------------------------------------- the setting and the layouts
def check_model_rules(rt, sc):
    """The refusals of rt_scene_set_glass_model and of the wrapper (what a frame reads after them is the GPU tests')."""
    lib = rt.load_library()
    assert lib.rt_scene_set_glass_model(sc.handle, rt.RT_GLASS_FRESNEL) == 0
    for bad in (2, -1, 7, 1 << 20):
        assert lib.rt_scene_set_glass_model(sc.handle, bad) == INVALID, bad
        assert b"rt_scene_set_glass_model" in lib.rt_last_error()
    assert lib.rt_scene_set_glass_model(None, 0) == INVALID
    assert lib.rt_scene_set_glass_model(sc.handle, rt.RT_GLASS_PLAIN) == 0
    sc.set_glass_model("fresnel")
    sc.set_glass_model(rt.RT_GLASS_FRESNEL)
    with pytest.raises(rt.RtError):
        sc.set_glass_model("schlick")
    with pytest.raises(rt.RtError):
        sc.set_glass_model(2)
    sc.set_glass_model("plain")


def test_setting_rules_on_a_host_only_scene(rt):
    """The model is host state, read when a frame is launched: its rules hold without a device, between the scene's
    other setters (tests/test_fresnel_gpu.py checks on frames that it survives them)."""
    assert (rt.RT_GLASS_PLAIN, rt.RT_GLASS_FRESNEL) == (0, 1)
    sc = rt.Scene()
    check_model_rules(rt, sc)
    sc.set_glass_model("fresnel")
    try:
        sc.set_spheres(rt.generate_spheres(4, 1), 4)
        n = 4
    except rt.RtError:                                       # no device: the list stays empty
        n = 0
    lib = rt.load_library()
    assert lib.rt_scene_set_materials_ex(sc.handle, None, 0) == 0
    if n:
        sc.set_materials_ex([0.0] * n, [0.5] * n, [1.5] * n)
    check_model_rules(rt, sc)
    sc.close()


def test_layouts(rt):
    lib = rt.load_library()
    assert lib.rt_debug_reflect_entry_size() == 48
    assert C.sizeof(rt.Material) == 12 and C.sizeof(rt.MaterialEx) == 16
    assert rt.MaterialEx.transperancy.offset == 4 and rt.MaterialEx.roughness.offset == 8 and rt.MaterialEx.ior.offset == 12
