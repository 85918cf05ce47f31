"""G-buffer outputs (rt_frame_desc.aov_*), host side: the ctypes mirror of rt_frame_desc against the
header's layout, and the refusals, which happen before the scene touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_FRAME = ("struct_size", "width", "height", "aspect", "cam", "pixels", "opts", "aov_depth", "aov_normal", "aov_id",
          "aov_albedo")
AOV_FIELDS = ("aov_depth", "aov_normal", "aov_id", "aov_albedo")


def _c_layout(tmp_path, struct, fields):
    """sizeof and offsetof as a C compiler lays the header's struct out."""
    src = tmp_path / "layout.c"
    body = "".join(f'    printf("%zu\\n", offsetof({struct}, {f}));\n' for f in fields)
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "rt_engine.h"\nint main(void) {{\n'
                   f'    printf("%zu\\n", sizeof({struct}));\n{body}    return 0;\n}}\n')
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_frame_desc_layout_matches_the_header(rt, tmp_path):
    want = _c_layout(tmp_path, "rt_frame_desc", _FRAME)
    assert C.sizeof(rt.FrameDesc) == want[0]
    assert [getattr(rt.FrameDesc, f).offset for f in _FRAME] == want[1:]
    # appended after opts: nothing before them moved, rt_launch_opts keeps its layout, an old struct_size ends before them
    opts = _c_layout(tmp_path, "rt_launch_opts", ("reflect_depth",))
    assert C.sizeof(rt.LaunchOpts) == opts[0] == 112 and rt.LaunchOpts.reflect_depth.offset == opts[1]
    assert want[1 + _FRAME.index("aov_depth")] == want[1 + _FRAME.index("opts")] + opts[0]
    assert rt.AOV_NAMES == ("depth", "normal", "id", "albedo")


def _frame(rt, aov=None, **opts):
    fd = rt.FrameDesc()
    fd.struct_size = C.sizeof(rt.FrameDesc)
    fd.width, fd.height = 64, 32
    fd.aspect = rt.default_aspect()
    fd.cam = rt.default_camera()
    fd.opts.struct_size = C.sizeof(rt.LaunchOpts)
    fd.opts.cull = -1
    for k, v in opts.items():
        setattr(fd.opts, k, v)
    for k, v in (aov or {}).items():
        setattr(fd, k, v)
    return fd


def test_refusals_without_a_device(rt):
    """Every refusal returns before the scene is used: a host-only scene (no sky, no texture, nothing uploaded) gets
    the G-buffer statuses, and the host buffers standing in for the outputs keep their sentinel."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(1 << 16, 0x5a5a5a5a, dtype=np.uint32)
        base = sentinel.ctypes.data
        p = (base + 255) & ~255              # 256-byte aligned, as a device allocation would be
        assert p % 16 == 0
        for field in AOV_FIELDS:
            # unsupported with any one of them set
            for extra in ({"spp": 2}, {"sample_total": 2}, {"tile": 16}, {"tile": 64}, {"stats": p + 4096},
                          {"profile": 1}, {"force_slow_path": 1}):
                fd = _frame(rt, {field: p}, **extra)
                assert lib.rt_scene_render(s, C.byref(fd), None) == 2, (field, extra)
                assert field in lib.rt_last_error().decode()
            # misaligned: normal and albedo need 16 bytes, id 8, depth 4
            for off in {"aov_depth": (1, 2), "aov_normal": (4, 8), "aov_id": (4,), "aov_albedo": (8, 12)}[field]:
                fd = _frame(rt, {field: p + off})
                assert lib.rt_scene_render(s, C.byref(fd), None) == 1, (field, off)
            # a graph does not record them: NULL and the field's name
            fd = _frame(rt, {field: p})
            assert not lib.rt_graph_capture(s, C.byref(fd), 1, None, None)
            assert field in lib.rt_last_error().decode()
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_old_struct_size_ignores_the_fields(rt):
    """A caller whose struct_size ends before aov_depth: the fields read as NULL. With a refused combination set
    (spp 2) the new size is refused as UNSUPPORTED; the old size is not, and reaches the frame checks (a width of 0:
    INVALID) without a device."""
    lib = rt.load_library()
    s = lib.rt_scene_create()
    try:
        sentinel = np.full(4096, 0x5a5a5a5a, dtype=np.uint32)
        p = (sentinel.ctypes.data + 255) & ~255
        fd = _frame(rt, {"aov_depth": p, "aov_id": p}, spp=2)
        fd.width = 0
        assert lib.rt_scene_render(s, C.byref(fd), None) == 2
        fd.struct_size = rt.FrameDesc.aov_depth.offset
        assert lib.rt_scene_render(s, C.byref(fd), None) == 1
        assert "bad frame" in lib.rt_last_error().decode()
        # struct_size 0 reads as the layout before reflect_depth: the same
        fd.struct_size = 0
        assert lib.rt_scene_render(s, C.byref(fd), None) == 1
        assert (sentinel == 0x5a5a5a5a).all()
    finally:
        lib.rt_scene_destroy(s)


def test_render_rejects_unknown_names(rt):
    sc = rt.Scene()
    try:
        with pytest.raises(rt.RtError, match="unknown G-buffer output 'uv'"):
            sc.render(16, 16, aov=("depth", "uv"))
    finally:
        sc.close()
