"""The indirect pass on the device over hand-made guides (tests/indirect_guides.py), passed as raw pointers through
Scene.indirect_desc / indirect_raw: every dead reason of step 1 in both copies of the rule, guide normals that are not
unit length, chosen wave patterns in the cast pass's compaction, the scratch left by earlier calls, the optional
inputs, colours at the pack's edges and surface points beyond the finite range. Every comparison is on bits and every
count exact. Where an arithmetic result is NaN on both sides (colours at the pack's edges, far surface points) the two
NaNs count as equal: which payload and sign an operation gives a NaN is the processor's, not the contract's; a copied
NaN -- a dead pixel's rgba_in -- keeps its bits and is compared with them.

tests/test_indirect_guides_cpu.py has classified every pixel and gather ray of these inputs with the composed
reference beforehand; the device's primary rays are held against the oracle's here, so that classification is the
device's view too."""
from types import SimpleNamespace

import numpy as np
import pytest

import indirect_guides as IG
import indirect_ref as I
import margins
import postpass as P
import query_ref as Q

pytestmark = pytest.mark.gpu

f32 = np.float32
POISON = P.SENTINEL
STRENGTH = 0.75
H, M, D = IG.H, IG.M, IG.D
# bits a dead pixel's rgba_in carries through: quiet and signalling NaNs with payloads, infinities, values the pack clamps
DEAD_COLOURS = np.array([[0x7fc12345, 0x7f800000, 0xff800000, 0xffc00001],
                         [0x7f812345, 0x43960000, 0xc0a00000, 0x7fffffff]], dtype=np.uint32).view(np.float32)
EDGE_VALUES = (-5.0, 300.0, 1e30, float("inf"), float("-inf"), float("nan"))
FAR_DEPTHS = (1e6, -1e6, 1e30, 3e38)


class Memo:
    """A shade callable that keeps what it returned for a ray set: the calls of one guide set share their rays."""

    def __init__(self, fn):
        self.fn, self.seen = fn, {}

    def __call__(self, O, G):
        k = (O.tobytes(), G.tobytes())
        if k not in self.seen:
            self.seen[k] = self.fn(O, G)
        return self.seen[k]


@pytest.fixture(scope="module")
def world(rt, oracle, gpu):
    import torch
    inp = IG.scene_inputs(rt)
    sc = inp.scene()
    ref = Q.CastRef(oracle, inp)

    def device_shade(O, G):
        rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([O, G], axis=1), dtype=np.float32)).cuda()
        return sc.trace_rays(rays, "shade")["rgba"].cpu().numpy()

    views, sets = {}, {}

    def view(w, h):
        """The device's primary rays of the size, equal to the oracle's."""
        if (w, h) not in views:
            a = IG.view_aspect(rt, w, h)
            r = sc.primary_rays(w, h, cam=inp.cam, aspect=a).reshape(-1, 6).cpu().numpy()
            O, Dir = np.ascontiguousarray(r[:, :3]), np.ascontiguousarray(r[:, 3:])
            oO, oD = margins.primary_rays(oracle, inp.cam, a, w, h)
            assert np.array_equal(P.bits(O), P.bits(oO)) and np.array_equal(P.bits(Dir), P.bits(oD))
            views[(w, h)] = (O, Dir)
        return views[(w, h)]

    def guides(w, h, name):
        """The named mask's guides (or "all H" / "all D"), some dead pixels carrying DEAD_COLOURS."""
        if (w, h, name) not in sets:
            g = IG.uniform(w, h, {"all H": H, "all D": D}[name]) if name.startswith("all ") else IG.masked(w, h, name)
            dead = np.nonzero(g.types == D)[0]
            for k, p in enumerate(dead[:len(DEAD_COLOURS)]):
                g.rgba_in[p] = DEAD_COLOURS[k]
            sets[(w, h, name)] = g
        return sets[(w, h, name)]

    yield SimpleNamespace(rt=rt, inp=inp, sc=sc, view=view, guides=guides, composed=Memo(lambda O, G: ref.shade(O, G)[0]),
                          device=Memo(device_shade))
    sc.close()


# ----------------------------------------------------------------------------- helpers
def _upload(g):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(getattr(g, k))).cuda() for k in ("depth", "normal", "id", "albedo", "rgba_in")}


def _run(W, g, *, rays, variant=0, cull=1, albedo=True, rgba_in=True, pixels=True, in_place=False, sc=None):
    """One call over the guides `g` with poisoned outputs: the bits of rgba_out [m, 4] and of pixels [m] (None
    without)."""
    import torch
    sc = W.sc if sc is None else sc
    w, h = g.width, g.height
    dev = _upload(g)
    out = dev["rgba_in"].clone() if in_place else torch.full((h * w, 4), POISON, dtype=torch.int32, device="cuda")
    packed = torch.full((h * w,), POISON, dtype=torch.int32, device="cuda")
    src = out if in_place else dev["rgba_in"]
    d = sc.indirect_desc(w, h, cam=W.inp.cam, aspect=IG.view_aspect(W.rt, w, h), depth=dev["depth"].data_ptr(),
                         normal=dev["normal"].data_ptr(), id=dev["id"].data_ptr(),
                         albedo=dev["albedo"].data_ptr() if albedo else 0, rgba_in=src.data_ptr() if rgba_in else 0,
                         rgba_out=out.data_ptr(), pixels=packed.data_ptr() if pixels else 0, rays=rays,
                         ray_base=IG.RAY_BASE, seed=IG.SEED, strength=STRENGTH, cull=cull, variant=variant)
    assert sc.indirect_raw(d) == 0, W.rt.load_library().rt_last_error()
    torch.cuda.synchronize()
    if not pixels:
        assert (packed == POISON).all()                                 # a NULL `pixels` writes no packed word anywhere
    return P.tensor_bits(out).reshape(-1, 4), P.tensor_bits(packed).reshape(-1) if pixels else None


def _want(W, g, shade, *, rays, albedo=True, rgba_in=True):
    O, Dir = W.view(g.width, g.height)
    rgba, packed, det = I.indirect(g.width, g.depth, g.normal, g.id, O, Dir, shade, rays=rays, ray_base=IG.RAY_BASE,
                                   seed=IG.SEED, strength=STRENGTH, albedo=g.albedo if albedo else None,
                                   rgba_in=g.rgba_in if rgba_in else None, details=True)
    assert np.array_equal(~det["live"], g.types == D)
    return P.bits(rgba), packed


def _same(got, want, what, nan_class=False):
    """rgba bits and packed words; with nan_class a NaN on both sides counts as equal (the module's docstring)."""
    (rgba, packed), (wr, wp) = got, want
    assert not (rgba == POISON).any(), what
    ok = rgba == wr
    if nan_class:
        ok |= np.isnan(rgba.view(np.float32)) & np.isnan(wr.view(np.float32))
    bad = ~ok.all(axis=1)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8], rgba[bad][:2], wr[bad][:2])
    if packed is not None:
        assert not (packed == POISON).any(), what
        bad = packed != wp
        assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:8])


def _dead_pixels_carry_their_input(got, g, rgba_in, what):
    dead = g.types == D
    want = P.bits(g.rgba_in)[dead] if rgba_in else np.tile(P.bits(np.array([0, 0, 0, 1], dtype=f32)), (int(dead.sum()), 1))
    assert np.array_equal(got[0][dead], want), what
    if got[1] is not None:
        src = g.rgba_in[dead, :3] if rgba_in else np.zeros((int(dead.sum()), 3), dtype=f32)
        assert np.array_equal(got[1][dead], I.pack(src)), what


def _groups(rays):
    return [min(IG.GROUP, rays - j0) for j0 in range(0, rays, IG.GROUP)]


# ----------------------------------------------------------------------------- bits against the reference
@pytest.mark.parametrize("rays", IG.RAYS)
@pytest.mark.parametrize("w,h,name", IG.cases())
def test_bits_equal_the_reference(world, w, h, name, rays):
    """Both variants, with the BVH and with the whole lists, with and without rgba_in: rgba_out and pixels equal the
    restatement over the composed CastRef and over the device's own SHADE; no output element keeps the poison; dead
    pixels carry their input's bits, NaN payloads and infinities included; and the queue of every group holds
    (rays of the group) x (H pixels) entries."""
    W = world
    g = W.guides(w, h, name)
    n_hit = int((g.types == H).sum())
    for rgba_in in (True, False):
        want = _want(W, g, W.composed, rays=rays, rgba_in=rgba_in)
        again = _want(W, g, W.device, rays=rays, rgba_in=rgba_in)
        assert np.array_equal(want[0], again[0]) and np.array_equal(want[1], again[1]), "the two references"
        for variant in (0, 1):
            for cull in (1, 0):
                what = (name, rays, rgba_in, variant, cull)
                got = _run(W, g, rays=rays, variant=variant, cull=cull, rgba_in=rgba_in)
                _same(got, want, what)
                _dead_pixels_carry_their_input(got, g, rgba_in, what)
                if variant == 0:
                    assert W.sc.indirect_counts() == [k * n_hit for k in _groups(rays)], what


def test_queue_lengths_of_five_rays(world):
    """50 x 30 with rays = 5: a group of four and a group of one."""
    g = world.guides(50, 30, "patterns")
    n_hit = int((g.types == H).sum())
    assert n_hit > 0
    _run(world, g, rays=5)
    assert world.sc.indirect_counts() == [4 * n_hit, n_hit]
    _run(world, world.guides(50, 30, "all D"), rays=5)
    assert world.sc.indirect_counts() == [0, 0]
    _run(world, world.guides(50, 30, "all H"), rays=5)
    assert world.sc.indirect_counts() == [4 * 1500, 1500]


# ----------------------------------------------------------------------------- the scratch of earlier calls
def test_stale_scratch(world):
    """Neither the slab nor the queue is cleared between calls. An all-H call with rays = 8 fills every slot of the
    slab, the whole queue and the running sum; the masked set after it, with 8 and with 3 rays, equals a fresh scene's
    result and the reference. Then the other way round: all D first, all H after it (that reference over the device's
    SHADE: 12 000 hits are too many for the composed one in a quick test; the device's SHADE is held against the
    composed reference on the masks above)."""
    W = world
    w, h = IG.STALE_SIZE
    for first, then, shade in (("all H", "patterns", W.composed), ("all D", "all H", W.device)):
        sc = W.inp.scene()
        a, b = W.guides(w, h, first), W.guides(w, h, then)
        n_hit = int((b.types == H).sum())
        _run(W, a, rays=IG.STALE_RAYS[0], sc=sc)
        assert sc.indirect_counts() == [4 * int((a.types == H).sum())] * 2
        for rays in IG.STALE_RAYS:
            got = _run(W, b, rays=rays, sc=sc)
            assert sc.indirect_counts() == [k * n_hit for k in _groups(rays)]
            fresh = W.inp.scene()
            new = _run(W, b, rays=rays, sc=fresh)
            fresh.close()
            _same(got, new, (first, then, rays, "a fresh scene"))
            _same(got, _want(W, b, shade, rays=rays), (first, then, rays, "the reference"))
            _same(_run(W, b, rays=rays, sc=sc, variant=1), got, (first, then, rays, "the plain kernel"))
        sc.close()


# ----------------------------------------------------------------------------- optional inputs
@pytest.mark.parametrize("how", ["no albedo", "no rgba_in", "no pixels", "in place"])
def test_optional_inputs(world, how):
    W = world
    g = W.guides(50, 30, "patterns")
    kw = dict(albedo=how != "no albedo", rgba_in=how != "no rgba_in")
    want = _want(W, g, W.composed, rays=5, **kw)
    for variant in (0, 1):
        got = _run(W, g, rays=5, variant=variant, pixels=how != "no pixels", in_place=how == "in place", **kw)
        _same(got, want, (how, variant))
        _dead_pixels_carry_their_input(got, g, kw["rgba_in"], (how, variant))


# ----------------------------------------------------------------------------- the pack's edges
def test_colours_at_the_edges_of_the_pack(world):
    """Live pixels whose rgba_in or albedo holds -5, 300, 1e30, +inf, -inf or NaN in one channel: rgba_out and the
    packed word against the restatement, whose pack is rgbToInt(f2i(c * 254) ...) with the conversion's saturation."""
    import copy
    W = world
    g = copy.deepcopy(W.guides(50, 30, "patterns"))
    live = np.nonzero(g.types != D)[0]
    used = set()
    for k, p in enumerate(live):
        target, v, c = (k // 18) % 2, EDGE_VALUES[(k // 3) % 6], k % 3
        (g.rgba_in if target == 0 else g.albedo)[p, c] = v
        used.add((int(g.types[p]), target, (k // 3) % 6, c))
    assert len(used) == 2 * 2 * 6 * 3                                    # every value in every channel of both, on H and on M
    want = _want(W, g, W.composed, rays=4)
    col = want[0].view(np.float32)[live, :3]
    assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any() and (col < 0).any() and (col > 255).any()
    # the restatement's pack against the header's words, element by element in Python integers: v = c * 254 in
    # binary32; NaN -> 0, else truncated and saturated to an int, then rgbToInt's `> 255 -> 255` and `& 0xff`
    for p in live:
        word = 0
        for x in want[0].view(np.float32)[p, :3]:
            v = f32(x) * f32(254)
            i = 0 if np.isnan(v) else int(max(-2.0 ** 31, min(2.0 ** 31 - 1, np.trunc(np.float64(v)))))
            word = (word << 8) + (min(i, 255) & 0xff)
        assert word == int(want[1][p]), p
    for variant in (0, 1):
        _same(_run(W, g, rays=4, variant=variant), want, variant, nan_class=True)


# ----------------------------------------------------------------------------- far surface points
def test_far_surface_points(world):
    """H- and M-type pixels at depths 1e6, -1e6, 1e30 and 3e38 (there every product of P with itself leaves the finite
    range): the two variants agree to the bit, and both equal the restatement over the device's own SHADE, whose rays
    these are as any other. The composed reference is no yardstick where the intersection arithmetic overflows."""
    W = world
    w, h = 64, 4
    g = IG.guides(w, h, np.array([H, M] * (w * h // 2), dtype=np.int8))
    g.depth[:] = np.array([FAR_DEPTHS[(p // 2) % 4] for p in range(w * h)], dtype=f32)
    O, Dir = W.view(w, h)
    with np.errstate(all="ignore"):
        pz = (O[:, 2] + (Dir[:, 2] * g.depth).astype(f32)).astype(f32)
        assert np.isinf(pz * pz).any() and np.isfinite(pz * pz).any()   # D.z < 1 keeps P itself finite; its squares are not
    for rays in (1, 5):
        want = _want(W, g, W.device, rays=rays)
        a, b = _run(W, g, rays=rays, variant=0), _run(W, g, rays=rays, variant=1)
        _same(a, b, ("variants", rays))
        _same(a, want, ("variant 0", rays), nan_class=True)
        _same(b, want, ("variant 1", rays), nan_class=True)
