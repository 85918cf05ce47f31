"""One long-lived scene through the post passes' shared host state (csrc/rt_post.cpp: one timer per timed entry, one
ordering event per owner of scratch): every entry's timings are those of its own last call, whatever ran in between;
switching one entry's timing off leaves the others alone; and two passes on two streams give the same bits before and
after the setters that wait for, or follow, every pass's event. 32 x 16 pixels: this is host plumbing, which no larger
shape reaches differently."""
import numpy as np
import pytest

from postpass import ALL, SENTINEL, tensor_bits as _bits

pytestmark = pytest.mark.gpu

W, H = 32, 16
TIMED = ("denoise", "vdenoise", "temporal", "upsample", "display", "bloom", "indirect")


def _times(sc):
    return {k: getattr(sc, f"{k}_times")() for k in TIMED}


def test_timers_and_ordering_events_of_one_scene(rt, gpu):
    import torch
    sc = rt.Scene.default(64)
    try:
        for k in TIMED:
            getattr(sc, f"set_{k}_timing")(True)
        frame = sc.render(W, H, aov=ALL)
        lo = sc.render(W // 2, H // 2, aov=ALL)
        hist = sc.temporal(frame)                               # (a timed call: the next temporal call replaces its events)
        assert (frame["aov"]["id"][..., 0] >= 0).any()          # there is something to filter and to gather from

        # ---- each entry once, the two denoisers apart: the intervals are those of the entry's own call
        sc.denoise(frame, iterations=3)                         # pack + 3 iterations
        plain = sc.denoise_times()
        sc.temporal(frame, hist)
        sc.denoise_variance(frame, hist, iterations=2, variant=1)   # variant 1 has no pack: v_0 + 2 iterations
        sc.upsample(frame, lo)
        sc.display(frame)                                       # "auto": metering, resolve, apply
        sc.bloom(frame, levels=2)                               # 2 * levels
        sc.indirect(frame, rays=5)                              # two groups of at most 4 rays: cast, shade, resolve each
        want = dict(denoise=4, vdenoise=3, temporal=1, upsample=1, display=3, bloom=4, indirect=6)
        got = _times(sc)
        assert {k: len(v) for k, v in got.items()} == want
        assert got["denoise"] == plain                          # the same events: the variance call recorded into its own
        sc.denoise_variance(frame, hist, iterations=1)          # pack, spatial estimate, 1 iteration
        sc.denoise(frame, iterations=2, variant=1)              # 2 iterations
        got = _times(sc)
        assert {k: len(v) for k, v in got.items()} == dict(want, denoise=2, vdenoise=3)
        assert all(t >= 0 for v in got.values() for t in v)

        # ---- one entry's timing off: its call reports nothing, the others keep what they had
        sc.set_upsample_timing(False)
        sc.upsample(frame, lo)
        after = _times(sc)
        assert after.pop("upsample") == [] and got.pop("upsample") != []
        assert after == got

        # ---- two passes on two streams, before and after the setters: the same bits into poisoned buffers
        a = frame["aov"]
        want_dn = sc.denoise(frame, iterations=2)
        want_bl = sc.bloom(frame, levels=3, want_glow=True)

        def poisoned():
            return dict(dn_rgba=torch.full((H, W, 4), float("nan"), device="cuda"),
                        dn_px=torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda"),
                        bl_rgba=torch.full((H, W, 4), float("nan"), device="cuda"),
                        bl_px=torch.full((H, W), SENTINEL, dtype=torch.int32, device="cuda"),
                        bl_glow=torch.full((H, W, 4), float("nan"), device="cuda"))
        runs = [poisoned(), poisoned()]
        torch.cuda.synchronize()                                # every buffer is ready before another stream uses it
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]

        def both(o):
            d = sc.denoise_desc(W, H, rgba_in=frame["rgba"].data_ptr(), depth=a["depth"].data_ptr(),
                                normal=a["normal"].data_ptr(), albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(),
                                rgba_out=o["dn_rgba"].data_ptr(), pixels=o["dn_px"].data_ptr(), iterations=2)
            assert sc.denoise_raw(d, streams[0].cuda_stream) == 0, sc.lib.rt_last_error()
            b = sc.bloom_desc(W, H, rgba_in=frame["rgba"].data_ptr(), rgba_out=o["bl_rgba"].data_ptr(),
                              pixels=o["bl_px"].data_ptr(), glow_out=o["bl_glow"].data_ptr(), levels=3)
            assert sc.bloom_raw(b, streams[1].cuda_stream) == 0, sc.lib.rt_last_error()
        both(runs[0])
        # no host wait in between: both passes' events are pending when the setters run. set_lights with the same lights
        # changes nothing; set_planes waits on the host for every pass's event (no planes before, none after)
        sc.set_lights(sc.lights, sc.n_lights)
        sc.set_planes(None, 0)
        both(runs[1])
        torch.cuda.synchronize()
        for k in runs[0]:
            assert np.array_equal(_bits(runs[0][k]), _bits(runs[1][k])), k
        for k, t in (("dn_rgba", want_dn["rgba"]), ("dn_px", want_dn["packed"]), ("bl_rgba", want_bl["rgba"]),
                     ("bl_px", want_bl["pixels"]), ("bl_glow", want_bl["glow"])):
            assert np.array_equal(_bits(runs[0][k]), _bits(t)), k   # every element written, with the wrapper's values
        assert len(sc.denoise_times()) == 3 and len(sc.bloom_times()) == 6
    finally:
        sc.close()
