"""Every output element is written, and nothing outside the output (tests/arena.py): each operation runs twice, into
guard | payload | guard arenas of two different patterns, at the smallest shapes that still have the edge -- partial
tiles right and below, bands, compact interleaved rows, 3-byte pixels, remainders of sample groups and of workgroups.
Asserted per call: the guards intact in both runs; the two payloads the same bytes; the payload equal to what the
package's wrapper returns for the same call (values the rest of the suite already ties to the references); a buffer the
call must not touch still all pattern."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as R
import meshes
import vdenoise_ref as V
from arena import PATTERNS, Run, as_bytes, assert_pair, run_twice, same_bytes
from scenes import Inputs, mixed_scene

pytestmark = pytest.mark.gpu

# bytes per pixel and required alignment of the per-pixel outputs (include/rt_engine.h)
LAYOUT = {"pixels": (4, 4), "rgba": (16, 16), "packed24": (3, 4), "depth": (4, 4), "normal": (16, 16), "id": (8, 8),
          "albedo": (16, 16), "moments": (8, 8), "host": (4, 4), "rays": (24, 4), "variance": (4, 4)}
AOV = ("depth", "normal", "id", "albedo")
GUIDES = ("depth", "normal", "id")


def _outs(npx, names, untouched=(), **extra):
    o = {k: dict(nbytes=npx * LAYOUT[k][0], align=LAYOUT[k][1], written=k not in untouched) for k in names}
    o.update(extra)
    return o


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _frame_call(sc, w, h, unset=(), **kw):
    """The frame into the arenas' pointers; `unset`: arenas that exist but are not handed to the call."""
    def call(p):
        g = lambda k: 0 if k in unset else p.get(k, 0)
        fd = sc.frame_desc(w, h, pixels=g("pixels"), rgba=g("rgba"), packed24=g("packed24"), stats=g("stats"),
                           aov_depth=g("depth"), aov_normal=g("normal"), aov_id=g("id"), aov_albedo=g("albedo"), **kw)
        sc.render_raw(fd, _stream())
    return call


def _against_wrapper(got, out, names, what=""):
    for k in names:
        want = out["packed"] if k == "pixels" else out[k] if k in ("rgba", "packed24") else out["aov"][k]
        same_bytes(got[k], want, f"{what} {k}")


def _full_scene(rt, inp, mesh=None):
    sc = inp.scene()
    if getattr(inp, "n_planes", 0):
        sc.set_planes(inp.planes, inp.n_planes)
    if getattr(inp, "n_cubes", 0):
        sc.set_cubes(inp.cubes, inp.n_cubes)
    if mesh is not None:
        sc.set_mesh(rt.mesh_from_obj_text(mesh))
    return sc


@pytest.fixture(scope="module")
def scene(rt, gpu):
    """256 spheres: eye cones and view lists need 64."""
    sc = rt.Scene.default(256)
    yield sc
    sc.close()


# ----------------------------------------------------------------------------- the frame kernel
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (67, 45), (130, 3), (9, 70)])
def test_frame_sizes_tiles_and_culling(rt, scene, w, h):
    outs = _outs(w * h, ("pixels", "rgba"))
    for tile in (0, 8, 16, 32, 64):
        for cull in (False, True):
            got = run_twice(_frame_call(scene, w, h, tile=tile, cull=cull), outs, f"tile {tile} cull {cull}")
            _against_wrapper(got, scene.render(w, h, tile=tile, cull=cull), outs, f"tile {tile} cull {cull}")


def test_frame_band(rt, scene):
    w, h, y0, y1 = 160, 96, 31, 47
    outs = _outs(w * (y1 - y0), ("pixels", "rgba"))
    for tile in (0, 16):
        got = run_twice(_frame_call(scene, w, h, y0=y0, y1=y1, tile=tile), outs)
        _against_wrapper(got, scene.render(w, h, y0=y0, y1=y1, tile=tile), outs, f"tile {tile}")


def test_frame_interleaved_compact_rows(rt, scene):
    w, h = 160, 74                                           # rank 1 of 3: blocks 1 and 4, the last one of 10 rows
    rows = len(rt.interleaved_rows(h, 1, 3, 16))
    assert rows == 26
    outs = _outs(w * rows, ("pixels", "rgba", "packed24"))
    got = run_twice(_frame_call(scene, w, h, interleave=(3, 1, 16)), outs)
    _against_wrapper(got, scene.render(w, h, interleave=(3, 1, 16), want_packed24=True), outs)


def test_frame_packed24_three_bytes_per_pixel(rt, scene):
    w, h = 164, 37                                           # a multiple of 4, not of a tile; the guard directly behind
    outs = _outs(w * h, ("pixels", "packed24"))
    for tile in (0, 16):
        got = run_twice(_frame_call(scene, w, h, tile=tile), outs)
        _against_wrapper(got, scene.render(w, h, tile=tile, want_packed24=True, want_rgba=False), outs, f"tile {tile}")


def test_frame_four_samples_in_one_launch(rt, scene):
    w, h = 67, 45
    outs = _outs(w * h, ("pixels", "rgba"))
    got = run_twice(_frame_call(scene, w, h, spp=4), outs)
    _against_wrapper(got, scene.render(w, h, spp=4), outs)


def test_frame_progressive_passes(rt, scene):
    """accumulate = 0 with resolve = -1 overwrites rgba and leaves `pixels` alone; accumulate = 1 adds to a known partial
    sum (the payload holds it, only the guards carry the pattern) and resolves."""
    w, h = 67, 45
    first = _outs(w * h, ("pixels", "rgba"), untouched=("pixels",))
    part = run_twice(_frame_call(scene, w, h, spp=1, sample_base=0, sample_total=2, resolve=-1), first)
    second = _outs(w * h, ("pixels", "rgba"))
    second["rgba"]["prefill"] = part["rgba"].tobytes()
    got = run_twice(_frame_call(scene, w, h, spp=1, sample_base=1, sample_total=2, accumulate=True), second)
    _against_wrapper(got, scene.render(w, h, spp=2), second)


def test_frame_one_output_at_a_time(rt, scene):
    w, h = 67, 45
    want = scene.render(w, h)
    for name in ("pixels", "rgba"):
        other = "rgba" if name == "pixels" else "pixels"
        outs = _outs(w * h, ("pixels", "rgba"), untouched=(other,))
        got = run_twice(_frame_call(scene, w, h, unset=(other,)), outs, name + " only")
        _against_wrapper(got, want, (name,), name + " only")


def test_frame_stats_words(rt, gpu):
    """The counters are added to: the payload starts from zeros, the guards carry the pattern."""
    w, h = 67, 45
    sc = rt.Scene.default(256)
    sc.set_view_lists(0)          # what a launch counts does not depend on what launches before it left behind
    try:
        outs = _outs(w * h, ("pixels",), stats=dict(nbytes=8 * rt.RT_STATS_COUNT, align=8, prefill=bytes(8 * rt.RT_STATS_COUNT)))
        got = run_twice(_frame_call(sc, w, h), outs)
        want = sc.render(w, h, want_stats=True)
        same_bytes(got["pixels"], want["packed"])
        counters = dict(zip(rt.STAT_NAMES, got["stats"].view(np.uint64).tolist()))
        assert counters == want["stats"]
        assert counters["hit_pixels"] > 0 and counters["primary_tests"] > 0
    finally:
        sc.close()


@pytest.mark.parametrize("tile", [0, 8])
def test_frame_gbuffer_outputs(rt, scene, tile):
    w, h = 67, 45
    names = ("pixels", "rgba") + AOV
    got = run_twice(_frame_call(scene, w, h, tile=tile), _outs(w * h, names))
    want = scene.render(w, h, tile=tile, aov=AOV)
    _against_wrapper(got, want, names)
    # a subset: the unset ones are not touched
    outs = _outs(w * h, names, untouched=("normal", "albedo"))
    got = run_twice(_frame_call(scene, w, h, tile=tile, unset=("normal", "albedo")), outs)
    _against_wrapper(got, want, ("pixels", "rgba", "depth", "id"))


@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_frame_other_primitives(rt, gpu, name):
    w, h = 67, 45
    sc = _full_scene(rt, mixed_scene(rt)) if name == "mixed" else _full_scene(rt, Inputs(rt, 64), meshes.uv_sphere_obj())
    try:
        names = ("pixels", "rgba") + AOV
        for cull in (True, False):
            got = run_twice(_frame_call(sc, w, h, cull=cull), _outs(w * h, names))
            _against_wrapper(got, sc.render(w, h, cull=cull, aov=AOV), names, f"cull {cull}")
        outs = _outs(w * h, ("pixels", "rgba"))
        got = run_twice(_frame_call(sc, w, h, tile=16, spp=4), outs)
        _against_wrapper(got, sc.render(w, h, tile=16, spp=4), outs, "tile 16, 4 samples")
    finally:
        sc.close()


# ----------------------------------------------------------------------------- the tile order
def _camera(rt, k):
    cam = rt.default_camera()
    cam.Org.z += 0.07 * k
    cam.Camyaw += 0.6 * k
    return cam


@pytest.mark.parametrize("moving", [False, True], ids=["resting", "moving"])
def test_launches_that_read_a_sorted_tile_order(rt, gpu, moving):
    """136 x 136 at tile 8: 17 x 17 tiles in 2 x 2 blocks, all partial but one. A scene sorts its tiles before the
    second and the third launch of a resting view, and before the second, fifth, ... of a moving one; every launch
    renders into fresh arenas (a scene per pattern, so that both see the same sequence of launches)."""
    w = h = 136
    scenes = [rt.Scene.default(256) for _ in PATTERNS]
    plain = rt.Scene.default(256)
    plain.set_tile_order(0)
    try:
        outs = _outs(w * h, ("pixels", "rgba"))
        for k in range(6 if moving else 3):
            cam = _camera(rt, k if moving else 0)
            got = []
            for sc, pattern in zip(scenes, PATTERNS):
                run = Run(outs, pattern)
                _frame_call(sc, w, h, tile=8, cam=cam)(run.ptrs)
                got.append(run.collect())
            assert_pair(outs, got[0], got[1], f"launch {k}")
            _against_wrapper(got[0], plain.render(w, h, tile=8, cam=cam), outs, f"launch {k}")
    finally:
        for sc in scenes + [plain]:
            sc.close()


# ----------------------------------------------------------------------------- the frame graph
@pytest.mark.parametrize("passes", [4, -4])
def test_frame_graph_replays(rt, scene, passes):
    import torch
    lib = rt.load_library()
    w, h = 67, 45
    outs = _outs(w * h, ("pixels", "rgba"), host=dict(nbytes=4 * w * h, align=4, pinned=True))
    moved = _camera(rt, 3)
    want = [scene.render(w, h, spp=4), scene.render(w, h, spp=4, cam=moved)]
    stream = torch.cuda.Stream()
    got = []
    for pattern in PATTERNS:
        run = Run(outs, pattern)
        fd = scene.frame_desc(w, h, pixels=run.ptrs["pixels"], rgba=run.ptrs["rgba"])
        gr = lib.rt_graph_capture(scene.handle, C.byref(fd), passes, run.ptrs["host"], stream.cuda_stream)
        assert gr, lib.rt_last_error()
        try:
            frames = []
            for _ in range(2):
                assert lib.rt_graph_launch(gr, stream.cuda_stream) == 0, lib.rt_last_error()
            stream.synchronize()
            frames.append(run.collect())
            assert lib.rt_graph_set_camera(gr, C.byref(moved)) == 0, lib.rt_last_error()
            assert lib.rt_graph_launch(gr, stream.cuda_stream) == 0, lib.rt_last_error()
            stream.synchronize()
            frames.append(run.collect())
        finally:
            lib.rt_graph_destroy(gr)
        got.append(frames)
    for k in range(2):
        assert_pair(outs, got[0][k], got[1][k], f"frame {k}")
        _against_wrapper(got[0][k], want[k], ("pixels", "rgba"), f"frame {k}")
        same_bytes(got[0][k]["host"], want[k]["packed"], f"frame {k} host")
    assert not np.array_equal(got[0][0]["pixels"], got[0][1]["pixels"])


# ----------------------------------------------------------------------------- reflective frames
def _k_by_index(n, table=(0.0, 0.25, 0.5, 1.0)):
    return np.array([table[i % 4] for i in range(n)], dtype=np.float32)


@pytest.mark.parametrize("case", ["depth1", "depth3", "spp5", "scene_scope"])
def test_reflective_frames(rt, gpu, case):
    w, h = 50, 30                                            # 1 500 pixels: a multiple of neither 64 nor 256
    if case == "scene_scope":
        inp = mixed_scene(rt)
        sc = _full_scene(rt, inp)
        sc.set_reflect_scope("scene")
        sc.set_plane_materials([0.5, 0.0])
        sc.set_cube_materials([0.0, 0.5, 1.0, 0.0, 0.25])
        kw = dict(reflect_depth=2)
    else:
        inp = Inputs(rt, 48)
        sc = inp.scene()
        kw = dict(reflect_depth={"depth1": 1, "depth3": 3, "spp5": 2}[case])
        if case == "spp5":                                   # a full group of four samples and a remainder of one
            sc.set_reflect_samples("many")
            kw["spp"] = 5
    sc.set_materials(_k_by_index(inp.n))
    try:
        outs = _outs(w * h, ("pixels", "rgba"))
        got = run_twice(_frame_call(sc, w, h, **kw), outs)
        assert sc.reflect_stats()["queue"][0] > 0            # rays were reflected
        _against_wrapper(got, sc.render(w, h, **kw), outs)
    finally:
        sc.close()


# ----------------------------------------------------------------------------- ray queries
@pytest.fixture(scope="module")
def rays(scene):
    """The frame's own primary rays, 40 x 8: sky above, spheres below."""
    import torch
    r = scene.primary_rays(40, 8).reshape(-1, 6).contiguous()
    torch.cuda.synchronize()
    return r


def _query_call(sc, mode, r, unset=()):
    def call(p):
        g = lambda k: 0 if k in unset else p.get(k, 0)
        q = sc.query(mode, r.shape[0], rays=r.data_ptr(), hits=g("hits"), occluded=g("occluded"), rgba=g("rgba"),
                     packed=g("packed"))
        assert sc.trace_rays_raw(q, _stream()) == 0, sc.lib.rt_last_error()
    return call


def _query_outs(n, names, untouched=()):
    size = {"hits": (64, 4), "occluded": (4, 4), "rgba": (16, 16), "packed": (4, 4)}
    return {k: dict(nbytes=n * size[k][0], align=size[k][1], written=k not in untouched) for k in names}


def _hit_records(out, n):
    """The wrapper's nearest hits as whole 64-byte records: the kernel stores a zero-initialised record, so the three
    padding words are 0."""
    rec = np.zeros((n, 16), dtype=np.uint32)
    word = lambda t: t.contiguous().cpu().numpy().view(np.uint32).reshape(n, -1)
    rec[:, 0:1], rec[:, 1:2], rec[:, 2:3] = word(out["t"]), word(out["kind"]), word(out["index"])
    rec[:, 3:5], rec[:, 5:7], rec[:, 7:10], rec[:, 10:13] = word(out["uv"]), word(out["txy"]), word(out["normal"]), word(out["new_org"])
    return rec


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_ray_queries(rt, scene, rays, n):
    """On either side of the workgroup size of the query kernels (256)."""
    r = rays[320 - n:].contiguous()                          # the last rays: the rows with spheres
    everything = ("hits", "occluded", "rgba", "packed")
    nearest = scene.trace_rays(r, "nearest")
    got = run_twice(_query_call(scene, "nearest", r, unset=("occluded", "rgba", "packed")),
                    _query_outs(n, everything, untouched=("occluded", "rgba", "packed")), "nearest")
    want_hits = _hit_records(nearest, n)
    assert n == 1 or (want_hits[:, 1].view(np.int32) >= 0).any()
    same_bytes(got["hits"], want_hits, "nearest")
    got = run_twice(_query_call(scene, "occluded", r, unset=("hits", "rgba", "packed")),
                    _query_outs(n, everything, untouched=("hits", "rgba", "packed")), "occluded")
    same_bytes(got["occluded"], scene.trace_rays(r, "occluded")["occluded"], "occluded")
    shade = scene.trace_rays(r, "shade")
    for unset in (("hits", "packed"), ("hits", "rgba"), ()):
        names = tuple(k for k in ("hits", "rgba", "packed") if k not in unset)
        got = run_twice(_query_call(scene, "shade", r, unset=unset + ("occluded",)),
                        _query_outs(n, everything, untouched=unset + ("occluded",)), f"shade {names}")
        for k in names:
            same_bytes(got[k], want_hits if k == "hits" else shade[k], f"shade {names} {k}")


def test_primary_rays_of_a_band(rt, scene):
    w, h, y0, y1 = 160, 96, 31, 47
    def call(p):
        fd = scene.frame_desc(w, h, y0=y0, y1=y1)
        assert scene.lib.rt_scene_primary_rays(scene.handle, C.byref(fd), p["rays"], _stream()) == 0
    got = run_twice(call, _outs(w * (y1 - y0), ("rays",)))
    same_bytes(got["rays"], scene.primary_rays(w, h, y0=y0, y1=y1))


# ----------------------------------------------------------------------------- denoise and temporal
SIZES = [(64, 1), (1, 64), (5, 5), (65, 9), (161, 91)]
# Beyond the first group of eight: 17 tile columns of 64 for the two temporal product kernels, whose grid
# is padded to a multiple of eight columns; 9 row segments of 256 for dn_iter_direct, which walks them in groups of eight.
WIDE_TEMPORAL, WIDE_DENOISE = (1088, 5), (2100, 3)


@pytest.mark.parametrize("w,h", SIZES)
def test_denoise(rt, scene, w, h):
    import torch
    frame = scene.render(w, h, aov=AOV)
    torch.cuda.synchronize()
    a = frame["aov"]
    inputs = dict(rgba_in=frame["rgba"].data_ptr(), depth=a["depth"].data_ptr(), normal=a["normal"].data_ptr(),
                  albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr())
    before = as_bytes(frame["rgba"]).copy()
    host = [t.cpu().numpy() for t in (frame["rgba"], a["depth"], a["normal"], a["albedo"], a["id"])]
    # The passes go through scratch of the scene's (irradiance, packed guides), which no arena can stand for: an element
    # the pack pass leaves out keeps what the call before put there, in both runs alike, and after one call of this
    # frame that is the right value. So every call below follows a call on a decoy -- the same size, every input
    # different -- and is compared with the restatement, not only with another run of the library.
    kind = a["id"][..., :1]
    decoy = {"rgba": frame["rgba"] * 0.5 + 0.25,
             "aov": {"depth": a["depth"] * 1.5, "normal": a["normal"].roll(1, dims=-1).contiguous(),
                     "albedo": a["albedo"] * 0.5 + 0.125,
                     "id": torch.cat((kind, torch.where(kind >= 0, a["id"][..., 1:] + 1, a["id"][..., 1:])), dim=-1).contiguous()}}

    def dirty_the_scratch():
        scene.denoise(decoy, iterations=1, variant=0)

    for iterations in (1, 6):
        ref_rgba, ref_packed = R.denoise(*host, iterations=iterations)
        for variant in (0, 1, 2):
            def call(p, unset=()):
                dirty_the_scratch()
                d = scene.denoise_desc(w, h, rgba_out=p["rgba"], pixels=0 if "pixels" in unset else p["pixels"],
                                       iterations=iterations, variant=variant, **inputs)
                assert scene.denoise_raw(d, _stream()) == 0, scene.lib.rt_last_error()
            what = f"iterations {iterations} variant {variant}"
            got = run_twice(call, _outs(w * h, ("rgba", "pixels")), what)
            want = scene.denoise(frame, iterations=iterations, variant=variant)
            same_bytes(got["rgba"], want["rgba"], what)
            same_bytes(got["pixels"], want["packed"], what)
            same_bytes(got["rgba"], ref_rgba, what + " against the restatement")
            same_bytes(got["pixels"], ref_packed, what + " against the restatement")
            got = run_twice(lambda p: call(p, ("pixels",)), _outs(w * h, ("rgba", "pixels"), untouched=("pixels",)), what)
            same_bytes(got["rgba"], want["rgba"], what + " without pixels")
            # in place: rgba_out is rgba_in
            outs = _outs(w * h, ("rgba",))
            outs["rgba"]["prefill"] = before.tobytes()
            def in_place(p):
                dirty_the_scratch()
                d = scene.denoise_desc(w, h, rgba_out=p["rgba"], iterations=iterations, variant=variant,
                                       **dict(inputs, rgba_in=p["rgba"]))
                assert scene.denoise_raw(d, _stream()) == 0, scene.lib.rt_last_error()
            got = run_twice(in_place, outs, what + " in place")
            same_bytes(got["rgba"], want["rgba"], what + " in place")      # rgba_out may be rgba_in itself: the same bits
    assert np.array_equal(as_bytes(frame["rgba"]), before)


def _accumulated(rt, scene, w, h, ks):
    """The frame of the last of the cameras `ks` with every G-buffer output, and Scene.temporal's history over them."""
    hist = None
    for k in ks:
        frame = scene.render(w, h, cam=_camera(rt, k), aov=AOV)
        hist = scene.temporal(frame, hist, cam=_camera(rt, k))
    return frame, hist


@pytest.mark.parametrize("w,h", SIZES + [WIDE_DENOISE])
def test_denoise_variance(rt, scene, w, h):
    """rt_scene_denoise_variance into arenas for rgba_out, pixels and variance_out, with a history of two cameras and
    without. The passes go through six scratch arrays of the scene's (two of irradiance, the packed guides and keys,
    two of variance) and leave parts of them unwritten by design: the pack pass stores no guide and no key for a sky
    pixel, the spatial pass leaves per workgroup. As in test_denoise no arena can stand for them, so every call follows
    a decoy call of the same size -- two iterations of the product kernels, which write all six -- on the frame and
    history of a camera 2.4 degrees and 0.28 units away: its valid pixels differ from the real call's in both
    directions (on CPU frames 70 and 65 of 585 pixels at 65 x 9, 1 271 and 1 727 of 6 300 at 2100 x 3), so that stale
    guides, keys and variances are plausible values exactly where the real call has sky; and the result is compared
    with the restatement, not only with another run of the library."""
    import torch
    frame, hist = _accumulated(rt, scene, w, h, (0, 1))
    decoy = _accumulated(rt, scene, w, h, (4, 5))
    torch.cuda.synchronize()
    a = frame["aov"]
    valid, decoy_valid = ((f["aov"]["id"][..., 0] >= 0).cpu().numpy() for f in (frame, decoy[0]))
    if w * h >= 65 * 9:
        assert (valid & ~decoy_valid).any() and (~valid & decoy_valid).any() and valid.any() and not valid.all()
    ins = [frame["rgba"], hist["rgba"], hist["moments"], a["depth"], a["normal"], a["albedo"], a["id"]]
    before = [as_bytes(t).copy() for t in ins]
    guides = [a[k].cpu().numpy() for k in ("depth", "normal", "albedo", "id")]
    names = ("rgba", "pixels", "variance")

    def dirty_the_scratch():
        scene.denoise_variance(*decoy, iterations=2, variant=0)

    for iterations in (1, 5, 6):
        for history in (hist, None):
            src = frame["rgba"] if history is None else history["rgba"]
            moments = None if history is None else history["moments"]
            ref = dict(zip(names, V.denoise_variance(src.cpu().numpy(), *guides, None if moments is None else moments.cpu().numpy(),
                                                     iterations=iterations)))
            for variant in (0, 1, 2):
                def call(p, unset=(), in_place=False):
                    dirty_the_scratch()
                    g = lambda k: 0 if k in unset else p[k]
                    d = scene.vdenoise_desc(w, h, rgba_in=p["rgba"] if in_place else src.data_ptr(), depth=a["depth"].data_ptr(),
                                            normal=a["normal"].data_ptr(), albedo=a["albedo"].data_ptr(), id=a["id"].data_ptr(),
                                            moments=0 if moments is None else moments.data_ptr(), rgba_out=p["rgba"],
                                            pixels=g("pixels"), variance_out=g("variance"), iterations=iterations, variant=variant)
                    assert scene.denoise_variance_raw(d, _stream()) == 0, scene.lib.rt_last_error()
                what = f"iterations {iterations} variant {variant} history {history is not None}"
                got = run_twice(call, _outs(w * h, names), what)
                out = scene.denoise_variance(frame, history, iterations=iterations, variant=variant)
                want = dict(rgba=out["rgba"], pixels=out["packed"], variance=out["variance"])
                for k in names:
                    same_bytes(got[k], want[k], f"{what} {k}")
                    same_bytes(got[k], ref[k], f"{what} {k} against the restatement")
                for unset in ("pixels", "variance"):
                    got = run_twice(lambda p: call(p, (unset,)), _outs(w * h, names, untouched=(unset,)), f"{what} without {unset}")
                    for k in names:
                        if k != unset:
                            same_bytes(got[k], want[k], f"{what} without {unset}: {k}")
                # in place: rgba_out is rgba_in
                outs = _outs(w * h, names)
                outs["rgba"]["prefill"] = as_bytes(src).tobytes()
                got = run_twice(lambda p: call(p, in_place=True), outs, what + " in place")
                for k in names:
                    same_bytes(got[k], want[k], f"{what} in place {k}")
    for t, b in zip(ins, before):
        assert np.array_equal(as_bytes(t), b)


@pytest.mark.parametrize("w,h", SIZES + [WIDE_TEMPORAL])
def test_temporal_motion(rt, scene, w, h):
    """rt_scene_temporal_motion into arenas for rgba_out, moments_out and pixels, with every second sphere that the
    frames show displaced: under the moved view every hit pixel is reprojected; under the identical view the movers go
    through tp_product<MOTION>'s reprojection and exchange while the static lanes of the same waves take the single tap."""
    import torch
    cams = [_camera(rt, 0), _camera(rt, 1)]
    frames = [scene.render(w, h, cam=c, aov=GUIDES) for c in cams]
    hist = scene.temporal(frames[0], None, cam=cams[0])
    torch.cuda.synchronize()
    ids = np.stack([f["aov"]["id"].cpu().numpy() for f in frames])
    shown = np.unique(ids[..., 1][ids[..., 0] == 1])             # RT_HIT_SPHERE
    assert shown.size > 0
    table = np.zeros((256, 4), dtype=np.float32)
    moves = np.array([(0.0, 0.05, 0.0), (-0.04, 0.02, 0.05), (0.03, 0.0, -0.03)], dtype=np.float32)
    table[shown[::2], :3] = moves[np.arange(shown[::2].size) % 3]
    mover = (ids[..., 0] == 1) & np.isin(ids[..., 1], shown[::2])
    if w * h >= 65 * 9:
        assert mover[0].any() and mover[1].any() and ((ids[..., 0] >= 0) & ~mover)[0].any()
    if w > 512:             # movers and static hits in tiles beyond the first group of eight, in both frames
        assert mover[:, :, 512:].any(axis=(1, 2)).all() and ((ids[..., 0] >= 0) & ~mover)[:, :, 512:].any(axis=(1, 2)).all()
    sm = torch.from_numpy(table).cuda()
    names = ("rgba", "moments", "pixels")
    for variant in (0, 1):
        for clamp in (True, False):
            for i, view in ((1, "moved"), (0, "identical")):
                def call(p, unset=()):
                    f = frames[i]["aov"]
                    g = lambda k: 0 if k in unset else p[k]
                    d = scene.temporal_motion_desc(
                        w, h, cam=cams[i], rgba_in=frames[i]["rgba"].data_ptr(), depth=f["depth"].data_ptr(),
                        normal=f["normal"].data_ptr(), id=f["id"].data_ptr(), prev_cam=hist["cam"], prev_aspect=hist["aspect"],
                        prev_rgba=hist["rgba"].data_ptr(), prev_depth=hist["depth"].data_ptr(),
                        prev_normal=hist["normal"].data_ptr(), prev_id=hist["id"].data_ptr(),
                        prev_moments=hist["moments"].data_ptr(), rgba_out=p["rgba"], moments_out=g("moments"),
                        pixels=g("pixels"), variant=variant, clamp=clamp, sphere_motion=sm.data_ptr(), n_sphere_motion=256)
                    assert scene.temporal_motion_raw(d, _stream()) == 0, scene.lib.rt_last_error()
                what = f"variant {variant} clamp {clamp} {view} view"
                want = scene.temporal_motion(frames[i], hist, cam=cams[i], sphere_motion=sm, clamp=clamp, variant=variant)
                got = run_twice(call, _outs(w * h, names), what)
                for k, t in (("rgba", want["rgba"]), ("moments", want["moments"]), ("pixels", want["packed"])):
                    same_bytes(got[k], t, f"{what} {k}")
                # the MOMENTS = false instantiation
                got = run_twice(lambda p: call(p, ("moments", "pixels")), _outs(w * h, names, untouched=("moments", "pixels")),
                                what + " rgba only")
                same_bytes(got["rgba"], want["rgba"], what + " rgba only")


@pytest.mark.parametrize("w,h", SIZES + [WIDE_TEMPORAL])
def test_temporal(rt, scene, w, h):
    import torch
    cams = [_camera(rt, 0), _camera(rt, 1)]
    frames = [scene.render(w, h, cam=c, aov=GUIDES) for c in cams]
    torch.cuda.synchronize()
    names = ("rgba", "moments", "pixels")
    for variant in (0, 1):
        def call(p, frame, cam, hist, unset=()):
            a = frame["aov"]
            prev = {}
            if hist is not None:
                prev = dict(prev_cam=hist["cam"], prev_aspect=hist["aspect"], prev_rgba=hist["rgba"].data_ptr(),
                            prev_depth=hist["depth"].data_ptr(), prev_normal=hist["normal"].data_ptr(),
                            prev_id=hist["id"].data_ptr(), prev_moments=hist["moments"].data_ptr())
            g = lambda k: 0 if k in unset else p[k]
            d = scene.temporal_desc(w, h, cam=cam, rgba_in=frame["rgba"].data_ptr(), depth=a["depth"].data_ptr(),
                                    normal=a["normal"].data_ptr(), id=a["id"].data_ptr(), rgba_out=p["rgba"],
                                    moments_out=g("moments"), pixels=g("pixels"), reset=hist is None, variant=variant, **prev)
            assert scene.temporal_raw(d, _stream()) == 0, scene.lib.rt_last_error()
        # reset: no history is read
        hist = scene.temporal(frames[0], None, cam=cams[0], variant=variant)
        got = run_twice(lambda p: call(p, frames[0], cams[0], None), _outs(w * h, names), f"variant {variant} reset")
        for k, t in (("rgba", hist["rgba"]), ("moments", hist["moments"]), ("pixels", hist["packed"])):
            same_bytes(got[k], t, f"variant {variant} reset {k}")
        # a moved camera: the history is reprojected
        want = scene.temporal(frames[1], hist, cam=cams[1], variant=variant)
        got = run_twice(lambda p: call(p, frames[1], cams[1], hist), _outs(w * h, names), f"variant {variant} moved")
        for k, t in (("rgba", want["rgba"]), ("moments", want["moments"]), ("pixels", want["packed"])):
            same_bytes(got[k], t, f"variant {variant} moved {k}")
        got = run_twice(lambda p: call(p, frames[1], cams[1], hist, ("moments", "pixels")),
                        _outs(w * h, names, untouched=("moments", "pixels")), f"variant {variant} rgba only")
        same_bytes(got["rgba"], want["rgba"], f"variant {variant} rgba only")


# ----------------------------------------------------------------------------- the root side of the row exchange
@pytest.mark.parametrize("world", [2, 5])
def test_assemble_rows24(rt, scene, world):
    import torch
    from ray_tracer_engine_amd import distributed as rd
    w, h = 164, 100
    root = rd.InterleavedGather(h, w, world, "cuda", 16, rgb24=True)
    root.recv.fill_(0x3c3c3c3c)                              # rows of a slot that no rank owns
    for r in range(world):
        out = scene.render(w, h, interleave=(world, r, 16), want_packed24=True, want_rgba=False)
        root.views[r][: out["packed24"].shape[0]].copy_(out["packed24"])
    torch.cuda.synchronize()
    def call(p):
        assert rt.load_library().rt_assemble_rows24(root.recv.data_ptr(), p["frame"], w, h, world, root.max_rows, _stream()) == 0
    got = run_twice(call, dict(frame=dict(nbytes=4 * w * h, align=4)))
    same_bytes(got["frame"], scene.render(w, h, want_rgba=False)["packed"])
