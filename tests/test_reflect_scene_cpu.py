"""Reflective frames over the whole scene (rt_scene_set_reflect_scope), host side: the composed reference
of tests/reflect_scene_ref.py against the oracle and against the spheres-only composers, and the validation of the
scope and of the plane / cube material tables, which needs no device."""
import ctypes as C

import numpy as np
import pytest

import meshes
from reflect_scene_ref import SceneComposer
from scenes import Inputs, mixed_scene


def _same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def test_without_materials_the_reference_is_the_oracle(rt, oracle):
    """Spheres, two planes, cubes and a small mesh, every k = 0: the oracle's frame bit for bit."""
    W, H = 48, 32
    inp = mixed_scene(rt)
    mesh = meshes.box_obj_no_normals(4.5, 2.0, 7.0, 1.0)      # in front of the camera
    om = oracle.Mesh(mesh)
    want_rgba, want_packed, _ = oracle.render(inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights,
                                              inp.cam, W, H, inp.aspect, nthreads=8, cubes=inp.cubes, n_cubes=inp.n_cubes,
                                              planes=inp.planes, n_planes=inp.n_planes, mesh=om.handle)
    comp = SceneComposer(oracle, rt, inp, mesh)
    rgba, packed, queue = comp.render(W, H, 3)
    kinds = set(comp.trace[0]["kind"].tolist())
    assert {0, 1, 2, 3} <= kinds, kinds            # every kind of primitive is seen
    assert queue == [0, 0, 0] and len(comp.trace) == 1
    assert np.array_equal(rgba.view(np.uint32), want_rgba.reshape(H, W, 4).view(np.uint32))
    assert np.array_equal(packed, want_packed.reshape(H, W))


def test_on_spheres_the_reference_is_the_mirror_and_the_glass_composer(rt, oracle):
    from test_reflect_cpu import composer_for
    from test_refract_cpu import glass_composer_for
    W, H, n, depth = 48, 32, 128, 3
    inp = Inputs(rt, n)
    k = np.array([(0.0, 0.25, 0.5, 1.0)[i % 4] for i in range(n)], dtype=np.float32)
    comp = SceneComposer(oracle, rt, inp)
    mirror = composer_for(oracle, rt, inp)
    want = mirror.render(W, H, k, depth)
    got = comp.render(W, H, depth, k_sphere=k)
    assert len(mirror.trace) > 2 and mirror.trace[2]["index"].size > 0      # rays reach the second bounce
    assert _same(got, want)
    assert got[2] == [b["index"].size for b in mirror.trace[1:]] + [0] * (depth + 1 - len(mirror.trace))
    # glass on every third sphere, mirrors on others
    tau = np.array([0.9 if i % 3 == 0 else 0.0 for i in range(n)], dtype=np.float32)
    ior = np.where(tau > 0, 1.5, 0.0).astype(np.float32)
    kg = np.where(tau > 0, 0.0, k).astype(np.float32)
    glass = glass_composer_for(oracle, rt, inp)
    want = glass.render(W, H, kg, depth, tau=tau, ior=ior)
    assert any((b["rule"] == 4).any() for b in glass.trace)                  # some ray passes through a sphere
    assert _same(comp.render(W, H, depth, k_sphere=kg, tau=tau, ior=ior), want)
    # and one walk serves several depths
    many = comp.render_depths(W, H, (1, 2, 3), k_sphere=kg, tau=tau, ior=ior)
    for d in (1, 2):
        assert _same(many[d], glass.render(W, H, kg, d, tau=tau, ior=ior)), d
    assert _same(many[3], want)


# ----------------------------------------------------------------------------- validation without a device
@pytest.fixture()
def host_scene(rt):
    lib = rt.load_library()
    s = lib.rt_scene_create()          # host only: no lists yet (every count 0)
    yield lib, s
    lib.rt_scene_destroy(s)


def test_the_new_symbols_resolve(rt):
    lib = rt.load_library()
    for name in ("rt_scene_set_reflect_scope", "rt_scene_set_plane_materials", "rt_scene_set_cube_materials"):
        assert getattr(lib, name) is not None
    assert (rt.RT_REFLECT_SPHERES, rt.RT_REFLECT_SCENE) == (0, 1)
    for name in ("set_reflect_scope", "set_plane_materials", "set_cube_materials"):
        assert callable(getattr(rt.Scene, name))


def test_scope_values(rt, host_scene):
    lib, s = host_scene
    for scope in (-1, 2, 7, 1 << 20):
        assert lib.rt_scene_set_reflect_scope(s, scope) == 1               # RT_ERR_INVALID
        assert b"rt_scene_set_reflect_scope" in lib.rt_last_error()
    assert lib.rt_scene_set_reflect_scope(s, 1) == 0
    assert lib.rt_scene_set_reflect_scope(s, 0) == 0
    assert lib.rt_scene_set_reflect_scope(None, 1) == 1


@pytest.mark.parametrize("entry", ["rt_scene_set_plane_materials", "rt_scene_set_cube_materials"])
def test_plane_and_cube_material_validation(rt, host_scene, entry):
    lib, s = host_scene
    fn = getattr(lib, entry)
    M = rt.Material
    two = (M * 2)(M(0.5, 0.0, 0.0), M(0.25, 0.0, 0.0))
    assert fn(s, two, 2) == 1                                                # 2 materials for a list of 0
    assert fn(s, two, 1) == 1
    assert fn(None, two, 2) == 1
    for bad in (float("nan"), -0.25, 1.5, float("inf")):
        m = (M * 2)(M(0.5, 0.0, 0.0), M(bad, 0.0, 0.0))
        assert fn(s, m, 2) == 1, bad                                         # RT_ERR_INVALID
    assert fn(s, (M * 1)(M(0.5, 0.1, 0.0)), 1) == 2                          # transperancy: RT_ERR_UNSUPPORTED
    assert fn(s, (M * 1)(M(0.5, 0.0, 0.3)), 1) == 2                          # roughness
    assert fn(s, (M * 2)(M(0.5, 0.0, 0.3), M(2.0, 0.0, 0.0)), 2) == 1        # a bad value is reported before that
    assert fn(s, None, 0) == 0                                               # clearing is always fine
    assert fn(s, two, 0) == 0
    assert fn(s, None, 5) == 0
    for scope in (1, 0):                                                     # under either scope
        assert lib.rt_scene_set_reflect_scope(s, scope) == 0
        assert fn(s, None, 0) == 0
        assert fn(s, two, 2) == 1
