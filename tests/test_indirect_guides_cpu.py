"""The hand-made guides of tests/indirect_guides.py without a device: every mask shows the wave patterns it claims, and
the composed reference (query_ref.CastRef over the oracle, with the oracle's own primary rays of the view) agrees with
the intended outcome of every pixel -- indirect_ref.pixels marks exactly the D pixels dead, every gather ray of an H
pixel hits something and every gather ray of an M pixel hits nothing -- for every size, mask and ray range that
tests/test_indirect_guides_gpu.py uses. 100 % of the slots: a seed that yields a ray outside the rule is replaced in
indirect_guides.py, the rule stays."""
import numpy as np
import pytest

import indirect_guides as IG
import indirect_ref as I
import margins
import postpass as P
import query_ref as Q

H, M, D = IG.H, IG.M, IG.D


@pytest.fixture(scope="module")
def world(rt, oracle):
    inp = IG.scene_inputs(rt)
    rays = {}

    def primary(w, h):
        if (w, h) not in rays:
            rays[(w, h)] = margins.primary_rays(oracle, inp.cam, IG.view_aspect(rt, w, h), w, h)
        return rays[(w, h)]
    return inp, Q.CastRef(oracle, inp), primary


# ----------------------------------------------------------------------------- the masks
@pytest.mark.parametrize("w,h,name", IG.cases())
def test_a_mask_shows_the_patterns_it_claims(w, h, name):
    make, claims = IG.MASKS[(w, h)][name]
    types = make(w * h)
    assert types.shape == (w * h,) and set(np.unique(types)) <= {H, M, D}
    assert set(claims) == {1, IG.GROUP}
    for g, want in claims.items():
        found = IG.conditions(types, g)
        for c in sorted(want):
            assert c in found, (name, g, c)


def test_every_pattern_is_claimed_at_the_sizes_that_can_show_it():
    for size, want in (((50, 30), {1: IG.ALL - {"straddle"}, IG.GROUP: IG.ALL}),):
        for g, conds in want.items():
            claimed = set().union(*(c[g] for _, c in IG.MASKS[size].values()))
            assert claimed == conds, (size, g)
    both = lambda size, g: set().union(*(c[g] for _, c in IG.MASKS[size].values()))
    assert both((64, 4), IG.GROUP) == both((64, 4), 1) == {"lane 0 only", "lane 63 only", "alternating", "full H", "full M", "full D", "gap"}       # (whole waves only)
    for size in ((3, 1), (1, 1), (1, 70), (70, 1)):
        assert both(size, IG.GROUP) == {"tail", "straddle"}, size
    assert set(IG.MASKS) == set(IG.SIZES)


def test_the_patterns_are_told_apart():
    """conditions() itself: each pattern found where it was built and nowhere else."""
    w = IG._wave
    pad = np.full(64, H, dtype=np.int8)
    assert IG.conditions(w("lane 0 only"), 1) == {"lane 0 only"}
    assert IG.conditions(w("lane 63 only"), 1) == {"lane 63 only"}
    assert IG.conditions(w("alternating"), 1) == {"alternating"}
    assert IG.conditions(w("H"), 1) == {"full H"} and IG.conditions(w("M"), 1) == {"full M"}
    assert IG.conditions(w("D"), 1) == {"full D"}
    assert IG.conditions(np.concatenate([pad, w("dm"), pad]), 1) == {"full H", "gap"}
    assert IG.conditions(np.concatenate([pad, w("dm")]), 1) == {"full H"}              # no wave with a hit after it
    assert IG.conditions(np.concatenate([pad, w("M"), pad]), 1) == {"full H", "full M"}  # no dead pixel in it
    one = np.array([H], dtype=np.int8)
    assert IG.conditions(one, 1) == {"tail"} and IG.conditions(one, 2) == {"tail", "straddle"}
    assert IG.conditions(np.array([H, M], dtype=np.int8), 2) == {"straddle"}
    assert IG.conditions(np.array([M, H], dtype=np.int8), 1) == {"tail"}
    assert IG.conditions(np.array([H, M], dtype=np.int8), 1) == set()
    assert IG.conditions(np.array([M] * 63 + [H] * 2, dtype=np.int8), 1) == {"lane 63 only", "tail"}


@pytest.mark.parametrize("w,h,name", IG.cases())
def test_dead_reasons_live_normals_and_colours(w, h, name):
    g = IG.masked(w, h, name)
    dead = g.types == D
    assert np.array_equal(g.reason >= 0, dead) and np.array_equal(g.live_normal >= 0, ~dead)
    if dead.any():
        assert set(g.reason[dead].tolist()) == set(range(len(IG.DEAD_REASONS))), name
    if name == "patterns":
        for t in (H, M):
            assert set(g.live_normal[g.types == t].tolist()) == set(range(len(IG.LIVE_NORMALS))), t
    assert (g.id[g.types == H] == (IG.PLANE_KIND, 0)).all() and (g.id[g.types == M, 0] >= 0).all()
    for a in (g.albedo, g.rgba_in):
        assert len(np.unique(P.bits(a), axis=0)) == len(a)              # no two pixels share their bits
        assert (P.bits(a[:, :3]) != P.bits(a[:, 1:])).all()             # nor two neighbouring channels of a pixel
    # the guides are what the tables say, to the bit
    for p in np.nonzero(dead)[0]:
        how = IG.DEAD_REASONS[g.reason[p]][1]
        if "normal" in how:
            assert np.array_equal(P.bits(g.normal[p, :3]), P.bits(np.array(how["normal"], dtype=np.float32)))
    with np.errstate(all="ignore"):
        nn = I.dot(g.normal[:, :3], g.normal[:, :3])
    assert (nn[g.live_normal == 3] > 0).all() and (nn[g.live_normal == 3] < np.float32(1.1754944e-38)).all()   # subnormal
    assert np.isfinite(nn[g.live_normal == 2]).all() and (nn[g.reason == 9] == np.inf).all() and (nn[g.reason == 10] == 0).all()


# ----------------------------------------------------------------------------- the outcome of every pixel and ray
def _sets():
    """Every guide set of the GPU file: the masks, and the uniform sets of its stale-scratch test."""
    return [(w, h, name) for w, h, name in IG.cases()] + [(*IG.STALE_SIZE, "all H"), (*IG.STALE_SIZE, "all D")]


@pytest.mark.parametrize("w,h,name", _sets())
def test_the_reference_gives_every_pixel_its_intended_outcome(world, w, h, name):
    inp, ref, primary = world
    g = IG.uniform(w, h, {"all H": H, "all D": D}[name]) if name.startswith("all ") else IG.masked(w, h, name)
    O, Dir = primary(w, h)
    # the view of the constructions: one origin behind the camera (-1 / aspect along z), every direction forward
    assert (O == O[0]).all() and not O[0, :2].any() and -100 < O[0, 2] <= 0 and (Dir[:, 2] > 0).all()
    live, n, start, flip = I.pixels(g.depth, g.normal, g.id, O, Dir)
    assert np.array_equal(~live, g.types == D), np.nonzero(~live != (g.types == D))[0][:8]
    assert np.array_equal(flip[live], g.live_normal[live] == 4)         # only (0, 0, +1) is flipped
    assert (n[live, 2] < 0).all() and not n[live, :2].any()
    rays = max(IG.RAYS + IG.STALE_RAYS)                                  # every call's rays are among these
    idx, Gs = I.gather_rays(w, live, n, start, rays, IG.RAY_BASE, IG.SEED)
    want_hit = g.types[idx] == H
    for j, G in enumerate(Gs):
        assert (G[:, 2] < 0).all(), j
        kind = ref.nearest(start[idx], G)["kind"]
        assert np.array_equal(kind >= 0, want_hit), (j, idx[(kind >= 0) != want_hit][:8])
        assert (kind[want_hit] == IG.PLANE_KIND).all()                  # the sphere is out of every ray's reach
