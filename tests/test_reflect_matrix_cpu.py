"""The cases of tests/reflect_matrix.py hold the conditions they are chosen for ("The matrix of
instantiations"), from the references' traces alone -- no device is needed. A cell's frame proves something about the
code the cell adds only where that code does work: rough hits at the primary pass and in a bounce and, in the scene, on
every kind of primitive; rays through glass; both choices of the Fresnel model in every sample; samples that disagree
about a pixel; primary hits of every kind with edges between them.

OBSERVED holds the counts the references gave when the cases were chosen. A condition's threshold is half the observed
count, and 3 at the least; the least observed count is 9."""
import ctypes as C

import pytest

import reflect_matrix as M

COLUMNS = (
    "perturbed at bounce 0", "perturbed at a later bounce", "halved or rejected",
    "perturbed on a sphere", "perturbed on a plane", "perturbed on a cube",
    "rule-4 passes",
    "reflect choices in the poorest sample", "transmit choices in the poorest sample", "perturbed exits",
    "queued in one sample and not in another", "reflected in one sample and through in another",
    "perturbed by different draws in two samples",
    "primary hits: triangle", "primary hits: sphere", "primary hits: plane", "primary hits: cube", "primary hits: sky",
    "pixels whose right neighbour is of another kind", "pixels whose samples meet different kinds")
_ = None
_K1 = (71, 313, 773, 123, 1792, 153, _)            # the staged scene's primary hits, one sample
_K5 = (67, 299, 767, 122, 1728, 142, 255)          # the poorest of samples 2 .. 6 of 8
OBSERVED = {
    #         bounce 0  later  h/r   sphere plane  cube  rule 4  refl  thru  exits  queue  r/t  draws
    "00000": (_,        _,     _,    _,     _,     _,    _,      _,    _,    _,     _,     _,   _) + (_,) * 7,
    "00010": (222,      17,    16,   _,     _,     _,    _,      _,    _,    _,     _,     _,   _) + (_,) * 7,
    "00100": (_,        _,     _,    _,     _,     _,    _,      _,    _,    _,     95,    _,   _) + (_,) * 7,
    "00110": (1104,     82,    128,  _,     _,     _,    _,      _,    _,    _,     95,    _,   183) + (_,) * 7,
    "01000": (_,        _,     _,    _,     _,     _,    _,      _,    _,    _,     _,     _,   _) + _K1,
    "01010": (975,      330,   319,  194,   901,   210,  _,      _,    _,    _,     _,     _,   _) + _K1,
    "01100": (_,        _,     _,    _,     _,     _,    _,      _,    _,    _,     198,   _,   _) + _K5,
    "01110": (4998,     1685,  1748, 958,   4672,  1053, _,      _,    _,    _,     198,   _,   925) + _K5,
    "10000": (_,        _,     _,    _,     _,     _,    51,     _,    _,    _,     _,     _,   _) + (_,) * 7,
    "10010": (178,      14,    14,   _,     _,     _,    47,     _,    _,    _,     _,     _,   _) + (_,) * 7,
    "10100": (_,        _,     _,    _,     _,     _,    45,     _,    _,    _,     95,    _,   _) + (_,) * 7,
    "10110": (891,      53,    108,  _,     _,     _,    47,     _,    _,    _,     95,    _,   152) + (_,) * 7,
    "11000": (_,        _,     _,    _,     _,     _,    124,    _,    _,    _,     _,     _,   _) + _K1,
    "11010": (975,      385,   327,  198,   952,   210,  118,    _,    _,    _,     _,     _,   _) + _K1,
    "11100": (_,        _,     _,    _,     _,     _,    124,    _,    _,    _,     197,   _,   _) + _K5,
    "11110": (4998,     1976,  1804, 987,   4934,  1053, 119,    _,    _,    _,     197,   _,   925) + _K5,
    "10011": (178,      13,    14,   _,     _,     _,    38,     9,    38,   35,    _,     _,   _) + (_,) * 7,
    "10111": (891,      56,    109,  _,     _,     _,    35,     9,    35,   178,   95,    41,  152) + (_,) * 7,
    "11011": (975,      392,   334,  204,   953,   210,  106,    11,   106,  105,   _,     _,   _) + _K1,
    "11111": (4998,     2011,  1833, 1019,  4937,  1053, 106,    9,    106,  556,   197,   43,  925) + _K5,
}


def observed(cell):
    return {c: v for c, v in zip(COLUMNS, OBSERVED[M.name(cell)]) if v is not None}


def threshold(seen):
    assert seen >= 6                     # half of it is 3 at the least
    return max(3, seen // 2)


def test_the_cells_are_the_instantiations():
    """FRESNEL comes with GLASS and GLOSS only (rf_primary_kernel): 16 cells without it and 4 with it, which run the
    10 instantiations of rt_reflect_bounce<GLASS, KINDS, GLOSS, FRESNEL>."""
    cells = set(M.CELLS)
    assert len(cells) == len(M.CELLS) == 20 and set(OBSERVED) == {M.name(c) for c in cells}
    assert all(set(c) <= {0, 1} and (not c.fresnel or (c.glass and c.gloss)) for c in cells)
    for flags in range(32):
        c = M.Cell(*(flags >> s & 1 for s in range(5)))
        assert (c in cells) == (not c.fresnel or bool(c.glass and c.gloss))
    assert len({M.bounce_kernel(c) for c in cells}) == 10
    for c in cells:
        assert len(OBSERVED[M.name(c)]) == len(COLUMNS)
        record = M.expected_dispatch(c)
        assert record["groups"] == (2 if c.samples else 1) and record["bvh"] == 1


@pytest.mark.parametrize("cell", M.CELLS, ids=M.name)
def test_the_case_holds_its_conditions(rt, oracle, cell):
    W, H, depth = M.shape(cell)
    ref = M.reference(rt, oracle, cell)
    assert len(ref["samples"]) == (M.SPP if cell.samples else 1)
    assert [s["k"] for s in ref["samples"]] == (list(range(M.BASE, M.BASE + M.SPP)) if cell.samples else [0])
    assert ref["rgba"].shape == (H, W, 4) and ref["packed"].shape == (H, W) and len(ref["queue"]) == depth
    assert (ref["rgba"][..., 3] == (M.SPP if cell.samples else 1)).all()
    assert all(q >= 6 for q in ref["queue"]), ref["queue"]                   # every bounce launch has rays to trace
    got = M.conditions(cell, ref)
    want = observed(cell)
    assert list(got) == [c for c in COLUMNS if c in want], (sorted(got), sorted(want))
    # what the cell's flags ask for is among the conditions
    assert ("perturbed at a later bounce" in got) == bool(cell.gloss)
    assert ("perturbed on a cube" in got) == bool(cell.gloss and cell.kinds)
    assert ("rule-4 passes" in got) == bool(cell.glass)
    assert ("perturbed exits" in got) == bool(cell.fresnel)
    assert ("queued in one sample and not in another" in got) == bool(cell.samples)
    assert ("perturbed by different draws in two samples" in got) == bool(cell.samples and cell.gloss)
    assert ("reflected in one sample and through in another" in got) == bool(cell.samples and cell.fresnel)
    assert ("primary hits: cube" in got) == bool(cell.kinds)
    assert ("pixels whose samples meet different kinds" in got) == bool(cell.kinds and cell.samples)
    short = {c: (got[c], threshold(seen)) for c, seen in want.items() if got[c] < threshold(seen)}
    assert not short, short


def test_roughness_by_index_meets_every_reflectivness():
    """Every pair of K_TABLE x RHO_TABLE occurs among the 48 spheres, and the staged scene's large mirror (sphere 0)
    and glass sphere (sphere 1) are rough."""
    rho = M.rho_by_index(M.N_SPHERES)
    k = M.materials(None, None, M.Cell(0, 0, 0, 0, 0))["k"]
    assert {(float(a), float(b)) for a, b in zip(k, rho)} == {(float(a), float(b)) for a in M.K_TABLE for b in
                                                               (C.c_float(v).value for v in M.RHO_TABLE)}
    assert rho[0] > 0 and rho[1] > 0 and M.SEED != 0


def test_the_record_before_any_reflective_frame(rt):
    """rt_debug_reflect_dispatch on a scene that has rendered nothing: the defined "none" (flags -1, no groups), and
    its argument checks."""
    lib = rt.load_library()
    sc = rt.Scene()
    try:
        assert M.dispatch(rt, sc) == M.NONE
        assert set(M.NONE.values()) == {-1, 0} and M.NONE["groups"] == 0
        out = (C.c_int * 8)(*([5] * 8))
        assert lib.rt_debug_reflect_dispatch(sc.handle, out, 6) == 1 and list(out) == [5] * 8
        assert b"rt_debug_reflect_dispatch" in lib.rt_last_error()
        assert lib.rt_debug_reflect_dispatch(sc.handle, None, 7) == 1
        assert lib.rt_debug_reflect_dispatch(None, out, 7) == 1
        assert lib.rt_debug_reflect_dispatch(sc.handle, out, 8) == 0 and list(out) == [-1] * 6 + [0, 5]
        sc.set_glass_model("fresnel")                                        # settings alone record nothing
        sc.set_reflect_samples("many")
        assert M.dispatch(rt, sc) == M.NONE
    finally:
        sc.close()
