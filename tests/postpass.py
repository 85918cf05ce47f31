"""What the post-pass suites share (tests/test_{denoise,vdenoise,temporal,tmotion,upsample}_{cpu,gpu}.py): the constants,
the views and cameras they walk, frames formed on the CPU, and the small conversions between the device's tensors and
the restatements' arrays. A plain module like scenes.py and arena.py; fixtures stay with their suites, and so does every
helper that differs between two suites in anything a test can observe."""
import ctypes as C

import numpy as np

import denoise_ref as R
import temporal_ref as T

f32 = np.float32
GUIDES = ("depth", "normal", "id")
ALL = GUIDES + ("albedo",)
SENTINEL = 0x5a5a5a5a
TEMPORAL_FIELDS = ("struct_size", "width", "height", "aspect", "cam", "prev_aspect", "prev_cam", "rgba_in", "depth",
                   "normal", "id", "prev_rgba", "prev_depth", "prev_normal", "prev_id", "prev_moments", "rgba_out",
                   "moments_out", "pixels", "reset", "max_history", "depth_tolerance", "normal_cos_min", "variant")

# The wide path: the GPU tests' path with the yaw turned to 170, for buffers of more than eight tile
# columns (tp_product pads its grid to a multiple of eight 64-pixel columns, with MOTION too) and of more than eight
# 256-pixel row segments (dn_iter_direct). With yaw 180 columns 512 .. 575 of a 576 x 36 frame show no sphere at all.
WIDE_CAMS = ((4, 3, 10, 170, -20), (4.5, 3.1, 10.2, 170, -20), (4.5, 3.1, 10.2, 170, -20), (4.7, 3.1, 10.1, 166, -21))
WIDE_BLOCK = 64                 # a tile column of the two temporal product kernels
WIDE_FIRST = 8                  # the first tile column outside the first group of eight
WIDE_HISTORY_FLOOR = 0.1        # of every such column's pixels, in the moved-camera step
WIDE_SEGMENT = 2048             # the first column of dn_iter_direct's second group of eight row segments
WIDE_HIT_FLOOR = 0.3            # of the pixels from there on, for the second camera


def block_shares(mask, first=WIDE_FIRST):
    """The share of `mask` [H, W] in every 64-column block from block `first` on."""
    return [float(mask[:, x:x + WIDE_BLOCK].mean()) for x in range(first * WIDE_BLOCK, mask.shape[1], WIDE_BLOCK)]


# ----------------------------------------------------------------------------- bits
def bits(a):
    """An array's binary32 values as uint32."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensor_bits(t):
    """A 32-bit tensor's words as a uint32 array."""
    return t.contiguous().cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------- cameras and scenes
def cam(rt, x, y, z, yaw, pitch):
    return rt.Camera(rt.Vec3(x, y, z), rt.Vec3(0, 0, 1), 0.0, yaw, pitch)


def path(rt):
    """A translation, the same camera again, then a yaw step with a translation."""
    return [cam(rt, 4, 3, 10, 180, -20), cam(rt, 4.5, 3.1, 10.2, 180, -20), cam(rt, 4.5, 3.1, 10.2, 180, -20),
            cam(rt, 4.7, 3.1, 10.1, 176, -21)]


def wide_path(rt):
    """path with the yaw turned to 170 (WIDE_CAMS)."""
    return [cam(rt, *c) for c in WIDE_CAMS]


def scene(rt, inp, mesh=None):
    """The device scene of `inp` (tests/scenes.py) with its planes, cubes and a mesh."""
    sc = inp.scene()
    if getattr(inp, "n_planes", 0):
        sc.set_planes(inp.planes, inp.n_planes)
    if getattr(inp, "n_cubes", 0):
        sc.set_cubes(inp.cubes, inp.n_cubes)
    if mesh is not None:
        sc.set_mesh(rt.mesh_from_obj_text(mesh))
    return sc


def move_spheres(inp, moves):
    """Moves spheres of `inp` in binary32; returns the displacement table [n, 4] (now - before)."""
    tab = np.zeros((inp.n, 4), dtype=f32)
    for i, d in moves.items():
        o = inp.spheres[i].orgin
        before = np.array([o.x, o.y, o.z], dtype=f32)
        now = (before + np.array(d, dtype=f32)).astype(f32)
        o.x, o.y, o.z = (float(v) for v in now)
        tab[i, :3] = (now - before).astype(f32)
    return tab


def move_cube(rt, inp, i, d):
    lib = rt.load_library()
    tab = np.zeros((inp.n_cubes, 4), dtype=f32)
    b = inp.cubes[i].bounds
    lo = np.array([b[0].x, b[0].y, b[0].z], dtype=f32)
    hi = np.array([b[1].x, b[1].y, b[1].z], dtype=f32)
    d = np.array(d, dtype=f32)
    nlo, nhi = (lo + d).astype(f32), (hi + d).astype(f32)
    lib.rt_cube_init(C.byref(inp.cubes[i]), *[float(v) for v in nlo], *[float(v) for v in nhi])
    tab[i, :3] = (nlo - lo).astype(f32)
    return tab


def mirror_k(n):
    return np.array([0.5 if i % 4 == 0 else 0.0 for i in range(n)], dtype=np.float32)


# ----------------------------------------------------------------------------- frames
class View:
    """One camera's frame of a scene, formed on the CPU: the restatement's `cur`, the rays and the view terms."""

    def __init__(self, rt, oracle, inp, cam, w, h):
        from test_reflect_cpu import Composer
        inp.cam = cam
        rgba, depth, normal, _, ids = R.oracle_inputs(rt, oracle, inp, w, h)
        comp = Composer(oracle, None, inp.spheres, inp.n, inp.tex, inp.sky, inp.sky_box, inp.lights, inp.n_lights, cam,
                        inp.aspect)
        self.O, self.D = comp.primary(w, h, 0, h)
        self.cur = dict(rgba=rgba, depth=depth, normal=normal, id=ids)
        self.terms = rt.view_terms(w, h, inp.aspect, cam)
        self.aspect, self.cam, self.w, self.h = inp.aspect, cam, w, h

    def onto(self, hist, prev, same=False, **kw):
        """This view's frame blended into `hist`, which was accumulated in the view `prev`."""
        return T.temporal(self.cur, hist, self.O, self.D, self.terms, prev.terms, prev.aspect, same, details=True, **kw)


def crop(frame, rows, cols):
    """Rows and columns of a device frame as a frame of its own (contiguous tensors)."""
    cut = lambda t: t[rows, cols].contiguous()
    return {"rgba": cut(frame["rgba"]), "packed": cut(frame["packed"]), "aov": {k: cut(v) for k, v in frame["aov"].items()}}


def cur(frame, colour=None):
    """A device frame as the temporal restatements' `cur`."""
    a = frame["aov"]
    return dict(rgba=(frame["rgba"] if colour is None else colour).cpu().numpy(), depth=a["depth"].cpu().numpy(),
                normal=a["normal"].cpu().numpy(), id=a["id"].cpu().numpy())


def hist_np(h):
    """A device history as the temporal restatements' `prev`."""
    return None if h is None else dict(rgba=h["rgba"].cpu().numpy(), depth=h["depth"].cpu().numpy(),
                                       normal=h["normal"].cpu().numpy(), id=h["id"].cpu().numpy(),
                                       moments=None if h["moments"] is None else h["moments"].cpu().numpy())


def mae(a, b, mask=None):
    """The mean absolute error of the colour channels (over `mask`)."""
    d = np.abs(a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64))
    return float(d[mask].mean() if mask is not None else d.mean())
