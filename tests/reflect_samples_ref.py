"""The composed reference of supersampled reflective frames (rt_scene_set_reflect_samples(RT_REFLECT_SAMPLES_MANY),
DESIGN.md 6h).

Nothing here traces a ray of its own. A sample is a frame of one of the composers the repository already trusts --
Composer (tests/test_reflect_cpu.py), GlassComposer (tests/test_refract_cpu.py), SceneComposer
(tests/reflect_scene_ref.py) -- whose primary() is replaced by one that asks oracle_primary_ray for sample k's offset
rt_sample_offset(k, total) instead of the pixel centre. The samples are then summed in float32 from zeros in ascending
k, the accumulate / total rule is applied and the result packed with oracle_pack_color. Beside the frame the reference
returns, per sample, the queue sizes and which pixels were live at every bounce, so that a test can assert the
conditions on its inputs from the reference alone."""
import ctypes as C

import numpy as np

f32 = np.float32


def sample_offsets(rt, total):
    """[(ox, oy)] of samples 0 .. total - 1 of a frame with `total` samples (rt_sample_offset)."""
    lib = rt.load_library()
    out = []
    for k in range(total):
        ox, oy = C.c_double(), C.c_double()
        assert lib.rt_sample_offset(k, total, C.byref(ox), C.byref(oy)) == 0
        out.append((ox.value, oy.value))
    return out


def primary_at(comp, ox, oy):
    """Composer.primary for the sample offset (ox, oy): the same loop, the offset instead of (0.5, 0.5)."""
    def primary(W, H, y0, y1):
        lib, oc = comp.lib, comp.oracle
        cam = C.cast(C.pointer(comp.cam), C.POINTER(oc.OCamera))
        r = oc.ORay()
        rows = y1 - y0
        O = np.empty((rows * W, 3), dtype=np.float32)
        D = np.empty((rows * W, 3), dtype=np.float32)
        i = 0
        for y in range(y0, y1):
            for x in range(W):
                lib.oracle_primary_ray(x, y, W, H, comp.aspect, cam, ox, oy, C.byref(r))
                O[i] = (r.Org.x, r.Org.y, r.Org.z)
                D[i] = (r.Dir.x, r.Dir.y, r.Dir.z)
                i += 1
        return O, D
    return primary


def _live_pixels(trace, m, cont):
    """Band-local pixels live at every bounce of a trace without `pix` (Composer's): those of the bounce before that
    hit something `cont` says continues. Checked against the trace's own sizes."""
    live = np.arange(m)
    out = []
    for b, tr in enumerate(trace):
        assert tr["index"].shape[0] == live.size
        out.append(live)
        idx = tr["index"]
        go = (idx >= 0) & cont[np.maximum(idx, 0)]
        live = live[go]
    return out


class SampleRef:
    """Frames of `comp` (a Composer, a GlassComposer or a SceneComposer) per sample, summed as the library defines it.

    render(...) -> dict:
      rgba [rows, W, 4] float32, packed [rows, W] uint32 (None for resolve = -1), queue (depth ints: rays entering
      bounce b + 1, summed over the call's samples), S [rows, W, 3] (the call's own sum) and samples: per sample k
      {"k", "rgba", "queue", "trace", "pix"} with pix[b] = the band-local pixels live at bounce b (pix[1]: the pixels
      whose primary hit was queued) and, for a SceneComposer, kind0 [rows * W] = the kind the primary ray met."""

    def __init__(self, rt, comp):
        self.rt, self.comp = rt, comp
        self.scene = hasattr(comp, "render_depths")
        self.prim = comp.prim if self.scene else comp      # whose primary() the frames call
        self.lib = self.prim.lib

    def _one(self, W, H, depth, y0, y1, mats):
        comp = self.comp
        rows = y1 - y0
        m = rows * W
        if self.scene:
            rgba, _, queue = comp.render(W, H, depth, y0=y0, y1=y1, **mats)
            trace = comp.trace
            pix = [tr["pix"] for tr in trace]
            kind0 = trace[0]["kind"].copy()
        else:
            k = np.asarray(mats["k"], dtype=np.float32)
            cont = k > 0
            if "tau" in mats:
                rgba, _ = comp.render(W, H, k, depth, y0=y0, y1=y1, tau=mats["tau"], ior=mats["ior"])
                cont = cont | (np.asarray(mats["tau"], dtype=np.float32) > 0)
            else:
                rgba, _ = comp.render(W, H, k, depth, y0=y0, y1=y1)
            trace = comp.trace
            pix = [tr["pix"] for tr in trace] if trace and "pix" in trace[0] else _live_pixels(trace, m, cont)
            queue = ([p.size for p in pix[1:]] + [0] * depth)[:depth]
            kind0 = None
        return {"rgba": rgba, "queue": list(queue), "trace": trace, "pix": pix, "kind0": kind0}

    def render(self, W, H, depth, *, spp=1, base=0, total=0, old=None, resolve=0, y0=0, y1=None, **mats):
        """`old`: the rgba the call accumulates onto (None: no accumulate). resolve = -1: no packed words."""
        y1 = H if y1 is None else y1
        n = spp if spp > 0 else 1
        total = total if total > 0 else n
        assert 0 <= base and base + n <= total
        offs = sample_offsets(self.rt, total)
        rows = y1 - y0
        S = np.zeros((rows, W, 3), dtype=np.float32)
        queue = [0] * depth
        samples = []
        saved = self.prim.primary
        try:
            for k in range(base, base + n):
                self.prim.primary = primary_at(self.prim, *offs[k])
                one = self._one(W, H, depth, y0, y1, mats)
                one["k"] = k
                S = (S + one["rgba"][..., :3]).astype(np.float32)
                queue = [a + b for a, b in zip(queue, one["queue"])]
                samples.append(one)
        finally:
            self.prim.primary = saved
        rgba = np.empty((rows, W, 4), dtype=np.float32)
        if old is None:
            rgba[..., :3] = S
            rgba[..., 3] = f32(n)
        else:
            old = np.asarray(old, dtype=np.float32).reshape(rows, W, 4)
            rgba[..., :3] = (old[..., :3] + S).astype(np.float32)
            rgba[..., 3] = (old[..., 3] + f32(n)).astype(np.float32)
        packed = None
        if resolve != -1:
            v = rgba[..., :3].reshape(-1, 3)
            mean = v if total == 1 else (v / f32(total)).astype(np.float32)
            packed = np.array([self.lib.oracle_pack_color(float(c[0]), float(c[1]), float(c[2])) for c in mean],
                              dtype=np.uint32).reshape(rows, W)
        return {"rgba": rgba, "packed": packed, "queue": queue, "S": S, "samples": samples}


def queued_disagree(samples, m):
    """Pixels (of m) whose samples disagree on whether the primary hit is queued."""
    q = np.zeros((len(samples), m), dtype=bool)
    for j, s in enumerate(samples):
        if len(s["pix"]) > 1:
            q[j, s["pix"][1]] = True
    return q.any(axis=0) & ~q.all(axis=0)


def end_bounce(sample, m):
    """Per pixel, the last bounce at which the sample's ray was live (0: it ended at the primary hit or the sky)."""
    end = np.zeros(m, dtype=np.int64)
    for b, p in enumerate(sample["pix"]):
        end[p] = b
    return end


def ends_differ(samples, m):
    """Pixels whose samples end at different bounces."""
    e = np.stack([end_bounce(s, m) for s in samples])
    return (e != e[0]).any(axis=0)


def kinds_differ(samples):
    """Pixels whose samples' primary hits are of different kinds (SceneComposer samples)."""
    k = np.stack([s["kind0"] for s in samples])
    return (k != k[0]).any(axis=0)
