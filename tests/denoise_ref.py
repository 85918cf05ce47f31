"""The denoiser's semantics (rt_scene_denoise) restated in numpy binary32: vectorised over the pixels, a
Python loop over the 25 taps, every intermediate a float32 array (numpy rounds each float32 operation once, to
nearest even, as the device does with contraction off and correctly rounded division). Only + - * /, compares and
selections occur.

    denoise(rgba, depth, normal, albedo, ids, iterations=4, normal_shift=5, sigma_depth=0.05, sigma_colour=0.0,
            demodulate=True) -> (rgba_out float32 [H, W, 4], packed uint32 [H, W])

The inputs are arrays in the layouts of rt_frame_desc.aov_* ([H, W], [H, W, 4], [H, W, 4], [H, W, 2] (kind, index)).
`oracle_inputs` forms them on the CPU: the colour from the oracle, the guides from query_ref.CastRef.nearest over
the oracle's primary rays (what tests/test_aov_gpu.py proves the device's guides equal)."""
import numpy as np

f32 = np.float32
RT_HIT_TRIANGLE = 0
TINY = f32(2.0 ** -10)
H5 = (f32(1 / 16), f32(4 / 16), f32(6 / 16), f32(4 / 16), f32(1 / 16))
DEFAULTS = dict(iterations=4, normal_shift=5, sigma_depth=0.05, sigma_colour=0.0, demodulate=True)


def _max(a, b):
    """a > b ? a : b (a NaN `a` gives b)."""
    return np.where(a > b, a, b).astype(f32)


def luma(c):
    """Y = (0.2126 r + 0.7152 g) + 0.0722 b, every product and sum rounded."""
    return ((f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]).astype(f32) + f32(0.0722) * c[..., 2]).astype(f32)


def demodulated(rgba, albedo):
    """I0 = C / max(A, 2^-10) per channel."""
    with np.errstate(all="ignore"):
        return (rgba[..., :3].astype(f32) / _max(albedo[..., :3].astype(f32), TINY)).astype(f32)


def f2i(x):
    """(int)x as v_cvt_i32_f32: truncation, saturation, NaN -> 0."""
    x = np.asarray(x, dtype=f32).astype(np.float64)
    x = np.where(np.isnan(x), 0.0, np.clip(x, -2.0 ** 31, 2.0 ** 31 - 1))
    return np.trunc(x).astype(np.int64)


def pack(c):
    """rgbToInt(f2i(c * 254)) as oracle_pack_color: each channel clamped above at 255, then its low byte."""
    with np.errstate(all="ignore"):
        v = np.minimum(f2i((c[..., :3].astype(f32) * f32(254)).astype(f32)), 255) & 0xff
    return ((v[..., 0] << 16) + (v[..., 1] << 8) + v[..., 2]).astype(np.uint32)


def _shifted(a, oy, ox, fill):
    """b[y, x] = a[y + oy, x + ox] where that is inside the array, else `fill`."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, ye = max(0, -oy), min(h, h - oy)
    xs, xe = max(0, -ox), min(w, w - ox)
    if ys < ye and xs < xe:
        b[ys:ye, xs:xe] = a[ys + oy:ye + oy, xs + ox:xe + ox]
    return b


def _guides(depth, normal, ids, sigma_depth):
    """(kind, index, N, z, zden^2) of the guides: every triangle has index 0; zden = sigma_depth max(|z|, 2^-10)."""
    kind, index = ids[..., 0], np.where(ids[..., 0] == RT_HIT_TRIANGLE, 0, ids[..., 1])
    N = normal[..., :3].astype(f32)
    z = depth.astype(f32)
    with np.errstate(all="ignore"):
        zden = (f32(sigma_depth) * _max(np.abs(z), TINY)).astype(f32)
        zden2 = (zden * zden).astype(f32)
    return kind, index, N, z, zden2


def _geometry(N, z, zden2, kind, index, oy, ox, normal_shift):
    """(ok, e_n, e_z) of the tap at offset (oy, ox): ok = inside, valid and e_id; e_z = 1 / (1 + (dz / zden)^2) in the
    form zden^2 / (zden^2 + dz^2)."""
    h, w = z.shape
    ok = _shifted(np.ones((h, w), dtype=bool), oy, ox, False)
    kq = _shifted(kind, oy, ox, -1)
    iq = _shifted(index, oy, ox, -1)
    ok &= (kq >= 0) & (kq == kind) & (iq == index)
    Nq = _shifted(N, oy, ox, 0)
    zq = _shifted(z, oy, ox, 0)
    dot = ((N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]).astype(f32) + N[..., 2] * Nq[..., 2]).astype(f32)
    m = np.where(dot > 0, dot, f32(0)).astype(f32)
    for _ in range(normal_shift):
        m = (m * m).astype(f32)
    dz = (zq - z).astype(f32)
    ez = (zden2 / (zden2 + (dz * dz).astype(f32)).astype(f32)).astype(f32)
    return ok, m, ez


def iterate(I, depth, normal, ids, step, normal_shift, sigma_depth, sigma_colour):
    """One iteration: I [H, W, 3] float32 -> I' (pixels that are not valid keep I)."""
    h, w = depth.shape
    kind, index, N, z, zden2 = _guides(depth, normal, ids, sigma_depth)
    valid = kind >= 0
    sc = f32(sigma_colour)
    use_colour = bool(sc > 0)
    with np.errstate(all="ignore"):
        sc2 = f32(sc * sc)
        Yp = luma(I) if use_colour else None
        acc = np.zeros((h, w, 3), dtype=f32)
        wsum = np.zeros((h, w), dtype=f32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = dy * step, dx * step
                Iq = _shifted(I, oy, ox, 0)
                if dx == 0 and dy == 0:
                    wt = np.full((h, w), H5[2] * H5[2], dtype=f32)
                    ok = np.ones((h, w), dtype=bool)
                else:
                    ok, m, ez = _geometry(N, z, zden2, kind, index, oy, ox, normal_shift)
                    wt = ((H5[dx + 2] * H5[dy + 2]) * m).astype(f32)
                    wt = (wt * ez).astype(f32)
                    if use_colour:                                  # e_c in e_z's form
                        dl = (luma(Iq) - Yp).astype(f32)
                        wt = (wt * (sc2 / (sc2 + (dl * dl).astype(f32)).astype(f32)).astype(f32)).astype(f32)
                    ok &= (wt > 0) & (wt < np.inf)
                term = (wt[..., None] * Iq).astype(f32)
                acc = np.where(ok[..., None], (acc + term).astype(f32), acc)
                wsum = np.where(ok, (wsum + wt).astype(f32), wsum)
        out = (acc / wsum[..., None]).astype(f32)
    return np.where(valid[..., None], out, I).astype(f32)


def denoise(rgba, depth, normal, albedo, ids, iterations=4, normal_shift=5, sigma_depth=0.05, sigma_colour=0.0,
            demodulate=True, want_irradiance=False):
    rgba = np.ascontiguousarray(rgba, dtype=f32)
    valid = ids[..., 0] >= 0
    I = demodulated(rgba, albedo) if demodulate else rgba[..., :3].copy()
    I0 = I.copy()
    for i in range(iterations):
        I = iterate(I, depth, normal, ids, 1 << i, normal_shift, sigma_depth, sigma_colour)
    with np.errstate(all="ignore"):
        C = (I * albedo[..., :3].astype(f32)).astype(f32) if demodulate else I
    out = rgba.copy()
    out[valid, :3] = C[valid]
    out[valid, 3] = f32(1)
    packed = pack(out)
    if want_irradiance:
        return out, packed, I0, I
    return out, packed


def oracle_inputs(rt, oracle, inp, w, h, mesh_text=None):
    """(rgba, depth, normal, albedo, ids) of the scene `inp` (tests/scenes.py) at w x h, formed on the CPU."""
    import query_ref as Q
    from test_reflect_cpu import Composer
    om = oracle.Mesh(mesh_text) if mesh_text is not None else None
    rgba, _, _ = oracle.render(inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam, w, h,
                               inp.aspect, nthreads=8, cubes=getattr(inp, "cubes", None),
                               n_cubes=getattr(inp, "n_cubes", 0), planes=getattr(inp, "planes", None),
                               n_planes=getattr(inp, "n_planes", 0), mesh=om.handle if om else None)
    comp = Composer(oracle, None, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, inp.cam,
                    inp.aspect)
    O, D = comp.primary(w, h, 0, h)
    rec = Q.CastRef(oracle, inp, mesh_text).nearest(O, D)
    hit = rec["kind"] >= 0
    depth = rec["t"].reshape(h, w).astype(f32)
    normal = np.zeros((h, w, 4), dtype=f32)
    normal.reshape(-1, 4)[:, :3] = rec["normal"]
    ids = np.stack([rec["kind"], rec["index"]], axis=1).astype(np.int32).reshape(h, w, 2)
    # the texel the frame multiplies the light sum by: f2i(ty * th) * tw + f2i(tx * tw), clamped to the texture
    r, g, b = (np.ascontiguousarray(p, dtype=f32) for p in inp.tex)
    th, tw = r.shape
    ci = f2i((rec["ty"] * f32(th)).astype(f32)) * tw + f2i((rec["tx"] * f32(tw)).astype(f32))
    ci = np.clip(ci, 0, tw * th - 1)
    albedo = np.ones((h * w, 4), dtype=f32)
    albedo[:, 0], albedo[:, 1], albedo[:, 2] = r.reshape(-1)[ci], g.reshape(-1)[ci], b.reshape(-1)[ci]
    albedo[~hit, :3] = rgba.reshape(-1, 4)[~hit, :3]          # sky: the frame's colour
    return np.ascontiguousarray(rgba, dtype=f32), depth, normal, albedo.reshape(h, w, 4), ids
