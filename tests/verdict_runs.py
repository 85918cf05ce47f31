"""A resting view rendered through all three frame kernels: the first launch of a key runs the
plain kernel (MODE 0), the second records the tile's light verdicts (MODE 7), every later one reads them (MODE 6).
`resting` renders the same frame several times on one long-lived scene and holds every launch to the same expected
frame, which the callers take from the oracle (or, where the oracle is too slow, from the brute-force kernel of a
scene of its own with the switch off). Below it, what the suites of the table's sections share: the scenes, sizes and
layouts they render, the switched-off reference, and the application shell update() runs in."""
import ctypes as C

import numpy as np

from scenes import Inputs, _bits

GROUPS, LIGHTS = 4, 8         # RT_VERDICT_GROUPS, RT_VERDICT_LIGHTS: two bits per (group, light) at 16 * group + 2 * light
NOTHING, CLEAR = 1, 2         # RT_VERDICT_NOTHING, RT_VERDICT_CLEAR
SIZES = {1024: (160, 90), 256: (96, 54)}     # the scene of tests/golden/c3_160x90_n1024.npz, and a smaller one


def layouts(h):
    return {"tile8": dict(), "tile16": dict(tile=16), "tile32": dict(tile=32), "tile64": dict(tile=64),
            "band": dict(y0=16, y1=h - 18), "interleave": dict(interleave=(2, 1, 16))}


def rows_of(rt, h, kw):
    if kw.get("interleave"):
        cnt, idx, blk = kw["interleave"]
        return np.asarray(rt.interleaved_rows(h, idx, cnt, blk), dtype=np.int64)
    return np.arange(kw.get("y0", 0), kw.get("y1") or h)


def oracle_refs(rt, oracle):
    """Per scene of SIZES: its inputs and the oracle's whole frame (for a module-scoped fixture: computed once, never changed)."""
    out = {}
    for n, (w, h) in SIZES.items():
        inp = Inputs(rt, n)
        out[n] = (inp, oracle_frame(oracle, inp, w, h))
    return out


def tagged_of(tags):
    """tags uint8 [ty, tx, 4] -> (mask of used records, group, light)."""
    return (tags & 0x80) != 0, (tags >> 3) & 0xf, tags & 7


def copy_lights(rt, lights, n):
    arr = (rt.Light * n)()
    for i in range(n):
        arr[i] = rt.Light(rt.Vec3(lights[i].pos.x, lights[i].pos.y, lights[i].pos.z), lights[i].size, lights[i].r, lights[i].g, lights[i].b)
    return arr


def frame(scene, width, height, **kw):
    """(float4 bits, packed words) of one launch."""
    import torch
    out = scene.render(width, height, **kw)
    torch.cuda.synchronize()
    return _bits(out["rgba"].cpu().numpy()), out["packed"].cpu().numpy().view(np.uint32)


def oracle_frame(oracle, sc, width, height, y0=0, y1=None, nthreads=16):
    """The oracle's (float4 bits, packed words) of rows [y0, y1) for a scenes.Scn / scenes.Inputs-like `sc`."""
    rgba, packed, _ = oracle.render(sc.spheres, sc.n, sc.tex, sc.sky, sc.sky_box, sc.lights, sc.n_lights, sc.cam, width, height,
                                    sc.aspect, y0=y0, y1=y1 if y1 else None, nthreads=nthreads)
    return _bits(rgba), packed


def differing(got, want, nan_equal=False):
    """(pixels whose float4 differs, pixels whose packed word differs); nan_equal: a NaN matches any NaN."""
    d = got[0] != want[0]
    if nan_equal:
        d &= ~(np.isnan(got[0].view(np.float32)) & np.isnan(want[0].view(np.float32)))
    return int(d.any(axis=-1).sum()), int((got[1] != want[1]).sum())


def assert_same(got, want, what, nan_equal=False):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (what, got[0].shape, want[0].shape)
    assert differing(got, want, nan_equal) == (0, 0), (what, differing(got, want, nan_equal))


def grid(width, height, kw):
    """tiles_x, tiles_y of the launch: tiles are `tile` wide and 64 / tile high over the launch's own rows."""
    from rt_amd import load
    tile = kw.get("tile") or 8
    rows = (kw.get("y1") or height) - kw.get("y0", 0)
    if kw.get("interleave") is not None:
        cnt, idx, blk = kw["interleave"]
        rows = len(load().interleaved_rows(rows, idx, cnt, blk or 16))
    th = 64 // tile
    return (width + tile - 1) // tile, (rows + th - 1) // th


def codes(words):
    """uint64 [...] -> codes [..., GROUPS, LIGHTS]."""
    sh = np.array([[16 * g + 2 * li for li in range(LIGHTS)] for g in range(GROUPS)], dtype=np.uint64)
    return ((words[..., None, None] >> sh) & np.uint64(3)).astype(np.int64)


def resting(scene, render_kwargs, want, launches=4, nan_equal=False, what="", allowed_states=None):
    """Renders the frame `render_kwargs` (width, height and Scene.render's options) `launches` times on `scene`. Every
    launch gives `want` = (float4 bits, packed words); the launches go nothing, write, read, read ... (allowed_states:
    the sequences a caller accepts instead); the writing launch leaves no tile of its grid unwritten. -> the recorded
    words, uint64 [tiles_y, tiles_x] (None if no launch wrote)."""
    kw = dict(render_kwargs)
    width, height = kw.pop("width"), kw.pop("height")
    states, words = [], None
    for k in range(launches):
        got = frame(scene, width, height, **kw)
        info = scene.light_verdicts(want_words=(k == 1))
        assert_same(got, want, "%s launch %d (state %d)" % (what, k, info["state"]), nan_equal)
        states.append(info["state"])
        if k == 1 and info["state"] == 1:
            assert info["unwritten"] == 0, (what, info)
            assert (info["tiles_x"], info["tiles_y"]) == grid(width, height, kw), (what, info, grid(width, height, kw))
            words = info["words"]
    assert states in [list(s) for s in (allowed_states or [([0, 1] + [2] * launches)[:launches]])], (what, states)
    return words


def switched_off(inp, w, h, want=None, what="", read_back="light_verdicts", **kw):
    """A scene of `inp` of its own with the switch off: its frame (= `want` where one is given) leaves the read-back
    `read_back` at state 0 and equals its brute-force frame. -> (the frame, the read-back's info)."""
    ref = inp.scene()
    ref.set_light_verdicts(0)
    off = frame(ref, w, h, **kw)
    if want is not None:
        assert_same(off, want, what + "switch off")
    info = getattr(ref, read_back)()
    assert info["state"] == 0, (what, info)
    assert_same(frame(ref, w, h, cull=False, **kw), off if want is None else want, what + "brute force")
    return off, info


def shim_state(rt):
    """The light-verdict state of the last launch on the library's own long-lived scene (rt_debug_shim_scene)."""
    lib = rt.load_library()
    s = lib.rt_debug_shim_scene()
    assert s, "the shim has no scene yet"
    info = rt.LightVerdictsInfo()
    assert lib.rt_debug_light_verdicts(s, C.byref(info), None, 0) == 0, lib.rt_last_error()
    return info.state


class App:
    """onStart() with `n` spheres of `seed`, the offscreen window at w x h, the camera at its default; all put back."""

    def __init__(self, rt, n, seed, w, h):
        self.rt, self.lib, self.n, self.seed, self.w, self.h = rt, rt.load_library(), n, seed, w, h

    def __enter__(self):
        lib = self.lib
        assert lib.rt_config_set_sphere_count(self.n) == 0 and lib.rt_config_set_seed(self.seed) == 0
        assert lib.rt_config_set_gpus(0) == 0
        lib.rt_on_start()
        self.cam = lib.rt_config_camera()
        self.saved = self.rt.Camera.from_buffer_copy(self.cam.contents)
        d = self.rt.default_camera()
        for f in ("Org", "Dir", "Camyaw", "Campitch"):
            setattr(self.cam.contents, f, getattr(d, f))
        assert lib.rt_offscreen_resize(self.w, self.h) == 0
        self.inp = Inputs(self.rt, self.n, seed=self.seed)
        return self

    def __exit__(self, *exc):
        C.memmove(self.cam, C.byref(self.saved), C.sizeof(self.rt.Camera))
        self.lib.rt_config_set_sphere_count(256)
        self.lib.rt_config_set_seed(1)
        return False

    def update(self):
        self.lib.rt_update()
        return np.ctypeslib.as_array(self.lib.rt_offscreen_pixels(), shape=(self.h, self.w)).copy(), shim_state(self.rt)
