"""Emissive surfaces (rt_scene_set_emission) without a device: the entry's refusals, each naming its
field, clearing, the wrapper's kinds and errors and where its two methods sit, Scene.emission_term on a hand-made id
tensor, and the wrapped restatement (tests/indirect_emit_ref.py) over the
three-plane scene of tests/indirect_paths_guides.py against paths composed by hand from query_ref.CastRef."""
import ctypes as C

import numpy as np
import pytest

import indirect_emit_ref as E
import indirect_guides as IG
import indirect_paths_guides as PG
import indirect_paths_ref as R
import indirect_ref as I
import margins
import postpass as P
import query_ref as Q

f32 = np.float32
FP = C.POINTER(C.c_float)


def _set(lib, s, kind, values):
    v = np.ascontiguousarray(values, dtype=np.float32)
    return lib.rt_scene_set_emission(s.handle if s is not None else None, kind, v.ctypes.data_as(FP), v.size // 3)


# ----------------------------------------------------------------------------- the C entry
# A scene without a device has no lists (setting one allocates): every count is 0 here. The values are checked before
# the count, so their refusals show all the same; tables that are taken, and what a new count does to them, are
# tests/test_indirect_emit_gpu.py's.
def test_refusals_name_their_field(rt):
    lib = rt.load_library()
    assert hasattr(lib, "rt_scene_set_emission")
    s = rt.Scene()
    try:
        ok = np.array([[0, 0, 0], [0.25, 0.5, 1.0], [3.0, 0, 0]], dtype=np.float32)
        # a null scene
        assert _set(lib, None, rt.RT_HIT_SPHERE, ok) == 1
        assert "rt_scene_set_emission: null scene" in lib.rt_last_error().decode()
        # kinds, with values or with NULL
        for kind in (rt.RT_HIT_TRIANGLE, rt.RT_HIT_NONE, 4, 99):
            assert _set(lib, s, kind, ok) == 1, kind
            msg = lib.rt_last_error().decode()
            assert msg.startswith("rt_scene_set_emission:") and f"kind {kind} " in msg, msg
            assert lib.rt_scene_set_emission(s.handle, kind, None, 0) == 1
        # counts: every list is empty
        for kind, n, what in ((rt.RT_HIT_SPHERE, 3, "sphere"), (rt.RT_HIT_PLANE, 1, "plane"), (rt.RT_HIT_CUBE, 2, "cube")):
            assert _set(lib, s, kind, np.zeros((n, 3), dtype=np.float32)) == 1
            msg = lib.rt_last_error().decode()
            assert f"{n} colours for 0 {what}s" in msg, msg
        assert lib.rt_scene_set_emission(s.handle, rt.RT_HIT_SPHERE, ok.ctypes.data_as(FP), -1) == 1
        assert "-1 colours" in lib.rt_last_error().decode()
        # values: the kind, the primitive, the channel and the value
        for kind, what in ((rt.RT_HIT_SPHERE, "sphere"), (rt.RT_HIT_PLANE, "plane"), (rt.RT_HIT_CUBE, "cube")):
            for bad, shown in ((-0.5, "-0.5"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf"),
                               (-1e-45, "-1.4")):
                for prim, ch in ((0, 0), (1, 2), (2, 1)):
                    e = ok.copy()
                    e[prim, ch] = bad
                    assert _set(lib, s, kind, e) == 1, (bad, prim, ch)
                    msg = lib.rt_last_error().decode()
                    assert f"{what} {prim}:" in msg and f"emission.{'rgb'[ch]} " in msg and shown in msg, msg
        # finite and >= 0, -0 included: only the count is wrong
        e = ok.copy()
        e[0, 0], e[2, 2] = -0.0, 3.0e38
        assert _set(lib, s, rt.RT_HIT_SPHERE, e) == 1 and "colours" in lib.rt_last_error().decode()
    finally:
        s.close()


def test_clearing_always_succeeds(rt):
    lib = rt.load_library()
    s = rt.Scene()
    try:
        v = np.ones(3, dtype=np.float32)
        for kind in (rt.RT_HIT_SPHERE, rt.RT_HIT_PLANE, rt.RT_HIT_CUBE):
            assert lib.rt_scene_set_emission(s.handle, kind, None, 0) == 0
            assert lib.rt_scene_set_emission(s.handle, kind, None, 7) == 0
            assert lib.rt_scene_set_emission(s.handle, kind, v.ctypes.data_as(FP), 0) == 0
        for kind in ("sphere", "plane", "cube", rt.RT_HIT_CUBE):
            s.set_emission(kind, None)
            s.set_emission(kind, [])
            s.set_emission(kind, np.zeros((0, 3)))
        assert s.emission == {}
    finally:
        s.close()


# ----------------------------------------------------------------------------- the wrapper
def test_wrapper_kinds_errors_and_where_the_methods_sit(rt):
    import inspect
    s = rt.Scene()
    try:
        with pytest.raises(rt.RtError, match="unknown emission kind 'triangle'"):
            s.set_emission("triangle", np.zeros((3, 3)))
        with pytest.raises(rt.RtError, match="kind 0 "):
            s.set_emission(rt.RT_HIT_TRIANGLE, np.zeros((3, 3)))
        with pytest.raises(rt.RtError, match=r"shape \[n, 3\]"):
            s.set_emission("sphere", np.zeros(9))
        for kind in ("sphere", "plane", "cube"):
            with pytest.raises(rt.RtError, match=f"{kind} 1: emission.g"):
                s.set_emission(kind, [[0, 0, 0], [0, -1, 0], [0, 0, 0]])
            with pytest.raises(rt.RtError, match=f"2 colours for 0 {kind}s"):
                s.set_emission(kind, np.zeros((2, 3)))
        assert s.emission == {}                                         # a refusal leaves the mirror alone
        with pytest.raises(rt.RtError, match="id"):
            s.emission_term({"aov": {}})
    finally:
        s.close()
    names = list(vars(rt.Scene))
    at = names.index("set_roughness")
    assert names[at + 1:at + 3] == ["set_emission", "emission_term"]    # next to set_roughness, ahead of the post passes
    assert names.index("emission_term") < names.index("denoise_desc") < names.index("indirect_times")
    for n in ("indirect", "indirect_paths"):                            # the passes keep their signatures
        assert "emission" not in str(inspect.signature(getattr(rt.Scene, n)))
    assert list(inspect.signature(rt.Scene.set_emission).parameters) == ["self", "kind", "values"]
    assert list(inspect.signature(rt.Scene.emission_term).parameters) == ["self", "frame"]
    assert C.sizeof(rt.IndirectDesc) == 136 and C.sizeof(rt.IndirectPathsOpts) == 8


def test_emission_term_on_a_hand_made_id_tensor(rt):
    """Plain indexing over the wrapper's host mirror, which this test fills itself: a scene without a device has no
    lists to set tables for (tests/test_indirect_emit_gpu.py goes through set_emission)."""
    import torch
    s = rt.Scene()
    try:
        rng = np.random.default_rng(3)
        sph, pl = rng.random((5, 3), dtype=np.float32), rng.random((2, 3), dtype=np.float32)
        s.emission = E.tables(sphere=sph, plane=pl)                     # the cubes have no table
        # kinds -1, 0, 1, 2, 3; the last entry of each table; a triangle index far beyond any table
        ids = np.array([[[-1, -1], [0, 0], [0, 12345], [1, 0], [1, 4]],
                        [[2, 0], [2, 1], [3, 0], [1, 2], [-1, 0]]], dtype=np.int32)
        frame = {"aov": {"id": torch.from_numpy(ids)}}
        want = E.term_lookup(E.tables(sphere=sph, plane=pl), ids)
        got = s.emission_term(frame)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 5, 4) and got.device.type == "cpu"
        assert np.array_equal(P.bits(got.numpy()), P.bits(want))
        assert np.array_equal(want[0, 4, :3], sph[4]) and np.array_equal(want[1, 1, :3], pl[1])
        assert not want[..., 3].any() and not want[0, :3].any() and not want[1, 2].any() and not want[1, 4].any()
        s.emission = E.tables(sphere=sph, plane=pl, cube=[[0.5, 0.25, 2.0]])
        assert s.emission_term(frame).numpy()[1, 2].tolist() == [0.5, 0.25, 2.0, 0.0]
        s.emission = {}
        assert not s.emission_term(frame).any()
    finally:
        s.close()


# ----------------------------------------------------------------------------- the wrapped restatement
TABLES = {"plane 0": [[0.25, 0.5, 1.0], [0, 0, 0], [0, 0, 0]],
          "all three": [[0.25, 0.5, 1.0], [0.125, 2.0, 0.0625], [1.5, 0.75, 0.375]]}


def _by_hand(ref, tex, tab, O, D, key, bounces):
    """c_j of one gather ray, steps (a) to (g) written out over CastRef, with + e at a hit."""
    O, D, key = O[None].astype(np.float32), D[None].astype(np.float32), np.array([key], dtype=np.uint64)
    L, T = None, None
    for b in range(bounces):
        rgba, _, rec = ref.shade(O, D)
        term = rgba[0, :3].astype(np.float32)
        kind, index = int(rec["kind"][0]), int(rec["index"][0])
        if kind == E.PLANE:
            term = (term + tab[index]).astype(np.float32)
        L = (f32(0) + term).astype(np.float32) if b == 0 else (L + (T * term).astype(np.float32)).astype(np.float32)
        if kind < 0 or b == bounces - 1:
            break
        a = R.texel(tex, rec["tx"][:1], rec["ty"][:1])[0]
        T = a if b == 0 else (T * a).astype(np.float32)
        ok, O, D, key = R.next_ray(O, D, rec["t"][:1], rec["normal"][:1], key)
        if not ok[0]:
            break
    return L


@pytest.mark.parametrize("which", list(TABLES))
def test_the_wrapped_restatement_equals_paths_composed_by_hand(rt, oracle, which):
    inp = PG.scene_inputs(rt)
    ref = Q.CastRef(oracle, inp)
    tab = np.array(TABLES[which], dtype=np.float32)
    w, h = 50, 30
    g = PG.masked(w, h, "mixed")
    O, Dir = margins.primary_rays(oracle, inp.cam, IG.view_aspect(rt, w, h), w, h)
    plain = R.castref_callables(ref)
    nearest, shade = E.emissive(*R.castref_callables(ref), E.tables(plane=tab))
    rays, kw = 2, dict(rays=2, ray_base=PG.RAY_BASE, seed=PG.SEED, strength=0.75, albedo=g.albedo, rgba_in=g.rgba_in)
    for bounces in (1, 2, 3):
        rgba, packed, det = R.indirect_paths(w, g.depth, g.normal, g.id, O, Dir, nearest, shade, inp.tex, bounces=bounces,
                                             details=True, **kw)
        bare, _, bdet = R.indirect_paths(w, g.depth, g.normal, g.id, O, Dir, plain[0], plain[1], inp.tex, bounces=bounces,
                                         details=True, **kw)
        assert det["counts"] == bdet["counts"] == PG.counts(g.kinds, rays, bounces)     # emission changes no path
        idx = det["idx"]
        kinds = g.kinds[idx]
        changed = (P.bits(rgba[idx, :3]) != P.bits(bare[idx, :3])).any(axis=1)
        assert changed[kinds == PG.STOP].all() and not changed[kinds == PG.MISS].any()   # A emits; the sky does not
        if which == "plane 0":
            assert not changed[kinds == PG.CONT].any()                  # C and A' are dark: a CONT path never meets A
        else:
            assert changed[kinds == PG.CONT].all()
        assert np.array_equal(P.bits(rgba[~det["live"]]), P.bits(g.rgba_in[~det["live"]]))
        for t in (PG.CONT, PG.STOP, PG.MISS):
            for k in np.nonzero(kinds == t)[0][[0, 1, 2, -1]]:
                p = idx[k]
                S = np.zeros(3, dtype=np.float32)
                for j in range(rays):
                    key = I.key(np.array([p % w]), np.array([p // w]), np.array([PG.RAY_BASE + j]), np.array([PG.SEED]))[0]
                    c = _by_hand(ref, inp.tex, tab, det["start"][p], det["G"][j][k], key, bounces)
                    assert np.array_equal(P.bits(c), P.bits(det["colours"][j][k])), (t, p, j, bounces)
                    S = (S + c).astype(np.float32)
                want = (g.rgba_in[p, :3] + ((f32(0.75) * (S / f32(rays)).astype(np.float32)).astype(np.float32)
                                            * g.albedo[p, :3]).astype(np.float32)).astype(np.float32)
                assert np.array_equal(P.bits(want), P.bits(rgba[p, :3])), (t, p, bounces)
                assert packed[p] == I.pack(want[None])[0]
