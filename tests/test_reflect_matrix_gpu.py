"""Every instantiation of the reflective passes on the device against the composed reference (tests/reflect_matrix.py,
DESIGN.md 6n, "The matrix of instantiations"). Per cell (GLASS, KINDS, SAMPLES, GLOSS, FRESNEL): the frame's record of
what it launched (rt_debug_reflect_dispatch) is the cell -- checked before anything is compared, so that a case cannot silently run
another instantiation -- and then rgba with its .w, the packed words and queue[] equal the reference bit for bit, over
the sphere BVH and over the whole list. Cells with GLOSS or SAMPLES are rendered again in bands, SAMPLES cells sample by
sample, and a GLOSS or FRESNEL cell must differ from its neighbour without the feature. Every frame is rendered into
poisoned buffers. The last test asserts that the module saw all 20 primary and all 10 bounce instantiations."""
import ctypes as C

import numpy as np
import pytest

import reflect_matrix as M
from scenes import Scn

pytestmark = pytest.mark.gpu

SEEN = set()          # the cells whose own frame recorded exactly that cell, over the BVH and over the whole list
POISON_WORD, POISON_FLOAT = 0x5a5a5a5a, 3.0


def _frame(rt, sc, cell, *, y0=0, y1=None, **over):
    """(packed, rgba, queue, record) of the cell's call on `sc`, rows [y0, y1), into poisoned buffers."""
    import torch
    W, H, _ = M.shape(cell)
    y1 = H if y1 is None else y1
    packed = torch.full((y1 - y0, W), POISON_WORD, dtype=torch.int32, device="cuda")
    rgba = torch.full((y1 - y0, W, 4), POISON_FLOAT, dtype=torch.float32, device="cuda")
    _call(sc, cell, packed, rgba, y0=y0, y1=y1, **over)
    return packed.cpu().numpy().view(np.uint32), rgba.cpu().numpy(), sc.reflect_stats()["queue"], M.dispatch(rt, sc)


def _call(sc, cell, packed, rgba, **over):
    import torch
    W, H, _ = M.shape(cell)
    fd = sc.frame_desc(W, H, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), **{**M.call(cell), **over})
    sc.render_raw(fd, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _rows(frame, y0, y1):
    return frame[0][y0:y1], frame[1][y0:y1]


def _flags(record):
    return M.Cell(*(record[f] for f in M.Cell._fields))


@pytest.mark.parametrize("cell", M.CELLS, ids=M.name)
def test_cell(rt, oracle, gpu, cell):
    W, H, depth = M.shape(cell)
    sc = M.scene(rt, oracle, cell)
    assert M.dispatch(rt, sc) == M.NONE                                      # no reflective frame yet
    ref = M.reference(rt, oracle, cell)
    assert ref["queue"][0] > 0 and ref["queue"][depth - 1] > 0               # every bounce kernel launch has rays

    # ------------------------------------------------------------------------- dispatch first, then parity
    frames = {}
    for cull in (True, False):
        got = frames[cull] = _frame(rt, sc, cell, cull=cull)
        assert got[3] == M.expected_dispatch(cell, cull), (cull, got[3])
    SEEN.add(cell)
    for cull, got in frames.items():
        bad = int((got[1].view(np.uint32) != ref["rgba"].view(np.uint32)).any(axis=2).sum())
        assert bad == 0, (cull, "rgba", bad)                                 # (.w included: nothing poisoned is left)
        assert np.array_equal(got[0], ref["packed"]), (cull, "packed")
        assert got[2] == list(ref["queue"]), (cull, got[2], ref["queue"])
    full = frames[True]

    # ------------------------------------------------------------------------- bands
    if cell.gloss or cell.samples:
        # halves; where the half is a whole number of 8-row tiles (the scene's 24), also a split at a row that is not
        splits = [H // 2] + ([H // 2 - 4] if (H // 2) % 8 == 0 else [])
        for cut in splits:
            assert cut % 8 != 0 or cut == H // 2
            queue = [0] * len(full[2])
            for y0, y1 in ((0, cut), (cut, H)):
                band = _frame(rt, sc, cell, y0=y0, y1=y1)
                assert band[3] == M.expected_dispatch(cell), (y0, y1, band[3])
                assert _same(band, _rows(full, y0, y1)), (y0, y1)
                queue = [a + b for a, b in zip(queue, band[2])]
            assert queue == full[2], cut

    # ------------------------------------------------------------------------- sample algebra
    if cell.samples:
        import torch
        packed = torch.full((H, W), POISON_WORD, dtype=torch.int32, device="cuda")
        rgba = torch.full((H, W, 4), POISON_FLOAT, dtype=torch.float32, device="cuda")
        queue = [0] * len(full[2])
        for j in range(M.SPP):
            _call(sc, cell, packed, rgba, spp=1, sample_base=M.BASE + j, accumulate=j > 0,
                  resolve=0 if j == M.SPP - 1 else -1)
            assert M.dispatch(rt, sc) == dict(M.expected_dispatch(cell), groups=1), j
            queue = [a + b for a, b in zip(queue, sc.reflect_stats()["queue"])]
        one_by_one = (packed.cpu().numpy().view(np.uint32), rgba.cpu().numpy())
        assert _same(one_by_one, full) and queue == full[2]

    # ------------------------------------------------------------------------- the neighbours differ
    if cell.gloss:
        other = M.scene(rt, oracle, cell, gloss=False)
        smooth = _frame(rt, other, cell)
        # without its tables a cell runs GLOSS = 0, unless FRESNEL takes GLOSS along
        assert _flags(smooth[3]) == cell._replace(gloss=cell.fresnel), smooth[3]
        assert not _same(smooth, full) and smooth[2][0] == full[2][0]
    if cell.fresnel:
        other = M.scene(rt, oracle, cell, fresnel=False)
        plain = _frame(rt, other, cell)
        assert _flags(plain[3]) == cell._replace(fresnel=0), plain[3]
        assert not _same(plain, full) and plain[2][0] == full[2][0]


def _refused(sc, cell, code=2):
    """The cell's call is refused with `code` and writes nothing."""
    import torch
    W, H, _ = M.shape(cell)
    packed = torch.full((H, W), POISON_WORD, dtype=torch.int32, device="cuda")
    rgba = torch.full((H, W, 4), POISON_FLOAT, dtype=torch.float32, device="cuda")
    fd = sc.frame_desc(W, H, pixels=packed.data_ptr(), rgba=rgba.data_ptr(), **M.call(cell))
    rc = sc.lib.rt_scene_render(sc.handle, C.byref(fd), None)
    torch.cuda.synchronize()
    return rc == code and bool((packed == POISON_WORD).all()) and bool((rgba == POISON_FLOAT).all())


def test_the_dropping_rules_through_the_record(rt, oracle, gpu):
    mirrors, glass = M.Cell(0, 0, 0, 0, 0), M.Cell(1, 0, 0, 0, 0)
    rough = M.roughness(rt, oracle, M.Cell(0, 0, 0, 1, 0))["sphere"]
    flags = lambda sc, cell: _flags(_frame(rt, sc, cell)[3])

    # a frame without reflections records nothing
    sc = M.scene(rt, oracle, mirrors)
    sc.render(*M.shape(mirrors)[:2])
    assert M.dispatch(rt, sc) == M.NONE
    # an all-zero roughness table launches GLOSS = 0
    sc.set_roughness("sphere", np.zeros_like(rough))
    assert flags(sc, mirrors) == mirrors
    sc.set_roughness("sphere", rough)
    assert flags(sc, mirrors) == mirrors._replace(gloss=1)
    # the Fresnel model without glass launches FRESNEL = 0, and GLOSS as the tables say
    sc.set_glass_model("fresnel")
    assert flags(sc, mirrors) == mirrors._replace(gloss=1)
    sc.set_roughness("sphere", None)
    assert flags(sc, mirrors) == mirrors
    # one sample under `many`: a call that a one-sample frame serves takes the one-sample path ("same
    # launches, same bits"), SAMPLES = 0; one that needs the sample fields -- a sample of a range, accumulate, no
    # resolve -- launches SAMPLES = 1 with one group
    sc.set_reflect_samples("many")
    assert flags(sc, mirrors) == mirrors
    for kw in (dict(sample_base=M.BASE, sample_total=M.TOTAL), dict(sample_total=2), dict(resolve=-1), dict(accumulate=True)):
        record = _frame(rt, sc, mirrors, spp=1, **kw)[3]
        assert _flags(record) == mirrors._replace(samples=1) and record["groups"] == 1, kw
    # the Fresnel model with glass and no roughness launches GLOSS = 1
    sc = M.scene(rt, oracle, glass)
    assert flags(sc, glass) == glass
    sc.set_glass_model("fresnel")
    assert flags(sc, glass) == M.Cell(1, 0, 0, 1, 1)

    # plane roughness under the spheres-only scope: a plane table needs a plane, and a reflective frame of a scene with
    # a plane is refused under that scope -- nothing is launched, so the record keeps the last frame that was; under
    # the scene scope the same tables launch KINDS = 1 and GLOSS = 1, and on the way back the refusal returns
    scn = Scn(rt, [(4.0, 1.0, 2.0, 1.0), (6.0, 1.0, 1.0, 1.0)], planes=[(0, 0, 0, 0, 1, 0)])
    sp = scn.scene()
    sp.set_materials([0.5, 0.5])
    sp.set_plane_materials([0.5])
    sp.set_roughness("plane", [1.0])
    assert _refused(sp, mirrors) and M.dispatch(rt, sp) == M.NONE
    sp.set_reflect_scope("scene")
    assert flags(sp, mirrors) == M.Cell(0, 1, 0, 1, 0)
    sp.set_roughness("plane", [0.0])                                         # and all-zero tables under KINDS: GLOSS = 0
    assert flags(sp, mirrors) == M.Cell(0, 1, 0, 0, 0)
    sp.set_roughness("plane", [1.0])
    sp.set_reflect_scope("spheres")
    assert _refused(sp, mirrors) and _flags(M.dispatch(rt, sp)) == M.Cell(0, 1, 0, 0, 0)
    # the scene scope over spheres alone is the spheres-only frame
    sc = M.scene(rt, oracle, mirrors)
    sc.set_reflect_scope("scene")
    assert flags(sc, mirrors) == mirrors


def test_every_instantiation_was_dispatched():
    """20 of 20 primary kernels and 10 of 10 bounce kernels (which follow from the flags), each by a frame that was
    compared with its reference above (so this test needs the module's other tests to have run in its process)."""
    missing = sorted(M.name(c) for c in set(M.CELLS) - SEEN)
    assert not missing and len(SEEN) == 20, missing
    bounces = {M.bounce_kernel(c) for c in SEEN}
    assert len(bounces) == 10, sorted(bounces)
    print(f"\n{len(SEEN)} of 20 primary cells and {len(bounces)} of 10 bounce kernels dispatched")
