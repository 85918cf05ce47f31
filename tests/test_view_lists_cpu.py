"""Per-view candidate lists of the primary rays, host side: the block's cone contains every primary ray
of the block, the host builder's lists are ordered, carry the right list positions and hold every pixel's closest
sphere, a block beyond the cap only raises its flag, and the default views at C2 and C3 stay below the cap."""
import ctypes as C

import numpy as np
import pytest

from scenes import Inputs, Scn
from test_reflect_cpu import nearest, sphere_table

f32 = np.float32


def _frame(rt, w, h, cam=None, aspect=None):
    fd = rt.FrameDesc()
    fd.struct_size = C.sizeof(rt.FrameDesc)
    fd.width, fd.height = w, h
    fd.aspect = rt.default_aspect() if aspect is None else aspect
    fd.cam = cam if cam is not None else rt.default_camera()
    fd.opts.struct_size = C.sizeof(rt.LaunchOpts)
    fd.opts.cull = 1
    return fd


def _cam(rt, org=(4, 3, 10), yaw=180.0, pitch=-20.0):
    return rt.Camera(rt.Vec3(*[float(v) for v in org]), rt.Vec3(0, 0, 1), 0.0, float(yaw), float(pitch))


def _rays(oracle, cam, aspect, w, h, pixels, offsets):
    """The oracle's primary rays (the directions the frame kernel reproduces bit for bit) of pixels x samples."""
    lib = oracle.load()
    ocam = C.cast(C.pointer(cam), C.POINTER(oracle.OCamera))
    r = oracle.ORay()
    O = np.empty((len(pixels) * len(offsets), 3), dtype=np.float32)
    D = np.empty_like(O)
    k = 0
    for (x, y) in pixels:
        for (ox, oy) in offsets:
            lib.oracle_primary_ray(int(x), int(y), w, h, aspect, ocam, ox, oy, C.byref(r))
            O[k] = (r.Org.x, r.Org.y, r.Org.z)
            D[k] = (r.Dir.x, r.Dir.y, r.Dir.z)
            k += 1
    return O, D


def _offsets(rt, spp):
    lib = rt.load_library()
    out = []
    for k in range(spp):
        ox, oy = C.c_double(), C.c_double()
        assert lib.rt_sample_offset(k, spp, C.byref(ox), C.byref(oy)) == 0
        out.append((ox.value, oy.value))
    return out


def _numpy_block_cone(cam, aspect, w, h, x0, y0, x1, y1):
    """Binary64 restatement of the block's cone: axis = normalised sum of the four corner directions at the pixel
    EDGES, sine of the half-angle = their largest deviation, padded x 1.01 + 1e-5 -> axis, slope."""
    a = float(f32(aspect))
    hw = float(f32(h) / f32(w))
    yaw, pitch = float(f32(cam.Camyaw * (3.1415 / 180))), float(f32(cam.Campitch * (3.1415 / 180)))
    cp, sp, cy, sy = np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    ez = float(f32(0) - (f32(-1) / f32(aspect)))
    dirs = []
    for xe in (x0, x1):
        for ye in (y0, y1):
            d = np.array([a * (2.0 * xe / w) - 1.0, (a * (2.0 * ye / h)) * hw - 1.0, ez])
            d /= np.linalg.norm(d)
            y = d[1] * cp - d[2] * sp
            z = d[1] * sp + d[2] * cp
            dirs.append(np.array([d[0] * cy + z * sy, y, -d[0] * sy + z * cy]))
    u = np.sum(dirs, axis=0)
    u /= np.linalg.norm(u)
    s = max(np.linalg.norm(np.cross(d, u)) for d in dirs)
    sn = s * 1.01 + 1.0e-5
    return u, sn / np.sqrt(1.0 - sn * sn), s


CAMS = [((4, 3, 10), 180.0, -20.0), ((4, 3, 10), 180.0, 89.0), ((4, 3, 10), 37.0, -89.0), ((-2, 8, 1), 301.5, 33.0)]


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160), (164, 100), (333, 77)])
@pytest.mark.parametrize("spp", [1, 4])
def test_block_cone_contains_every_ray_of_the_block(rt, oracle, w, h, spp):
    rng = np.random.default_rng(w * 7 + spp)
    offsets = _offsets(rt, spp)
    sph = rt.generate_spheres(64, 1)
    for org, yaw, pitch in CAMS:
        cam = _cam(rt, org, yaw, pitch)
        fd = _frame(rt, w, h, cam)
        v = rt.view_lists_host(sph, 64, fd, want_lists=False, want_beams=True)
        bw, bh, nbx, nby = v["block_w"], v["block_h"], v["blocks_x"], v["blocks_y"]
        assert nbx == -(-w // bw) and nby == -(-h // bh) and v["blocks"] == nbx * nby
        blocks = {0, nbx - 1, nbx * (nby - 1), nbx * nby - 1, (nby // 2) * nbx + nbx // 2} | set(rng.integers(0, nbx * nby, 3).tolist())
        for b in blocks:
            bx, by = b % nbx, b // nbx
            x0, y0, x1, y1 = bx * bw, by * bh, min((bx + 1) * bw, w), min((by + 1) * bh, h)
            u, k, s = _numpy_block_cone(cam, fd.aspect, w, h, x0, y0, x1, y1)
            # the product's cone is this one (its axis rounded to binary32, its rotation from the float cos / sin)
            beam = v["beams"][b].astype(np.float64)
            assert beam[3] > 0
            assert np.abs(beam[:3] - u).max() < 1e-6 and abs(beam[3] - k) <= 1e-5 * (1 + k)
            # border pixels (the extremes lie there) and a few inner ones, every sample
            px = [(x, y) for x in (x0, x1 - 1) for y in range(y0, y1, max(1, (y1 - y0) // 8))]
            px += [(x, y) for y in (y0, y1 - 1) for x in range(x0, x1, max(1, (x1 - x0) // 8))]
            px += [(x1 - 1, y1 - 1)] + [(int(rng.integers(x0, x1)), int(rng.integers(y0, y1))) for _ in range(4)]
            _, D = _rays(oracle, cam, fd.aspect, w, h, px, offsets)
            D = D.astype(np.float64)
            ub = beam[:3]
            sin_dev = np.linalg.norm(np.cross(D, ub), axis=1)
            assert (D @ ub > 0).all()
            assert sin_dev.max() <= s * 1.0001 + 2e-6, (b, sin_dev.max(), s)          # inside the corners' cone
            assert sin_dev.max() <= beam[3] / np.sqrt(1 + beam[3] ** 2), (b, sin_dev.max(), beam[3])   # and the padded one


def _lb(tab, org):
    v = tab[:, :3].astype(np.float64) - np.asarray(org, dtype=np.float64)
    dist, r = np.linalg.norm(v, axis=1), np.sqrt(tab[:, 3].astype(np.float64))
    return np.where(dist > r, dist - r, -(dist + r))


@pytest.mark.parametrize("seed,n,w,h,cam", [(1, 256, 164, 100, CAMS[0]), (2, 1024, 320, 180, ((3, 2, 6), 170.0, -10.0)),
                                                (3, 300, 96, 54, ((5, 6, 9), 185.0, -35.0))])
def test_host_lists_are_ordered_positioned_and_complete(rt, oracle, seed, n, w, h, cam):
    inp = Inputs(rt, n, seed)
    c = _cam(rt, *cam)
    fd = _frame(rt, w, h, c)
    v = rt.view_lists_host(inp.spheres, n, fd)
    tab = sphere_table(inp.spheres, n)
    bw, bh, nbx = v["block_w"], v["block_h"], v["blocks_x"]
    rng = np.random.default_rng(seed)
    assert v["overflowed"] + v["not_built"] < v["blocks"]
    checked = 0
    for b in rng.permutation(v["blocks"])[:24]:
        count, flags, ent, pos, lbs = v["lists"][b]
        if flags:
            assert count == 0
            continue
        assert len(set(pos.tolist())) == count and np.array_equal(ent, tab[pos])     # the right positions
        if count > 1:
            assert (np.diff(lbs) >= 0).all()                                            # front to back
            O, _ = _rays(oracle, c, fd.aspect, w, h, [(0, 0)], [(0.5, 0.5)])
            exact = _lb(tab[pos], O[0])
            assert (lbs[np.isfinite(lbs)] <= exact[np.isfinite(lbs)] + 1e-6).all()       # a LOWER bound of any t
        bx, by = int(b) % nbx, int(b) // nbx
        px = [(x, y) for y in range(by * bh, min((by + 1) * bh, h)) for x in range(bx * bw, min((bx + 1) * bw, w))]
        O, D = _rays(oracle, c, fd.aspect, w, h, px, [(0.5, 0.5)])
        idx, _ = nearest(O, D, tab)
        hit = idx[idx >= 0]
        assert np.isin(hit, pos).all(), (int(b), sorted(set(hit.tolist()) - set(pos.tolist())))
        checked += len(hit)
    assert checked > 0


def test_overflow_sets_the_flag_and_nothing_else(rt):
    # 70 small spheres in a row behind the frame's centre, a few elsewhere: the centre block overflows, others do not
    sph = [(0.0, 0.0, 5.0 + 0.4 * i, 0.05) for i in range(70)] + [(3.0 + i, -2.0, 12.0, 0.3) for i in range(6)]
    s = Scn(rt, sph, cam=_cam(rt, (0, 0, -1), 0.0, 0.0))
    fd = _frame(rt, 160, 96, s.cam)
    v = rt.view_lists_host(s.spheres, s.n, fd)
    over = [b for b, l in enumerate(v["lists"]) if l[1] & rt.RT_VIEW_OVERFLOW]
    assert 0 < len(over) < v["blocks"] and v["overflowed"] == len(over) and v["not_built"] == 0
    for b in over:
        count, flags, ent, pos, lbs = v["lists"][b]
        assert count == 0 and flags == rt.RT_VIEW_OVERFLOW
    assert any(l[0] > 0 and l[1] == 0 for l in v["lists"]) and v["longest"] <= rt.RT_VIEW_CAP


@pytest.mark.parametrize("w,h,n,may_overflow", [(1920, 1080, 256, False), (3840, 2160, 1024, False), (7680, 4320, 4096, True)])
def test_default_views_stay_below_the_cap(rt, w, h, n, may_overflow):
    """Cap condition: the default scene and camera at C2 and C3 overflow no block (C5 may, in a small share)."""
    inp = Inputs(rt, n)
    v = rt.view_lists_host(inp.spheres, n, _frame(rt, w, h), want_lists=False)
    print("view lists %dx%d n=%d: block %dx%d, %d blocks, overflowed %d, not built %d, longest %d, mean %.2f"
          % (w, h, n, v["block_w"], v["block_h"], v["blocks"], v["overflowed"], v["not_built"], v["longest"], v["mean"]))
    assert v["block_w"] == 64 and v["block_h"] == 64 and v["not_built"] == 0
    if not may_overflow:
        assert v["overflowed"] == 0
    assert v["longest"] <= rt.RT_VIEW_CAP and v["overflowed"] < v["blocks"]
