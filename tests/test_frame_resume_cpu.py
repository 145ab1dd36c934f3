"""CPU checks of resumable frames (pt_frame_*, binding.Frame, include/PathTrace/frame_render.h): the symbols, the pt_frame_info layout,
argument checks that need no device, the failure without a device, and the C++ header and test program compile."""
import ctypes as C
import os
import re
import subprocess

import pytest

from cpupathtrace_amd import binding, build, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    build.build()
    lib = binding.load()
    lib.pt_frame_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p]
    return lib


def _args(width=8, height=8):
    cam = binding._camera({"origin": (0, 0, -3), "look_at": (0, 0, 0), "up": (0, 1, 0), "focal_length": 1.0, "height": 1.0, "aspect_ratio": 1.0})
    return cam, binding.Options(width, height, 1, 1, 1e-3), binding.job_tiles(width, height)


def test_symbols_are_exported():
    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(binding.FRAME_EXPORTS) <= names


def test_info_layout_matches_header():
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    body = re.search(r"typedef struct pt_frame_info \{(.*?)\} pt_frame_info;", header, re.S).group(1)
    fields = re.findall(r"^\s*(u?int\d+_t)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in binding.FrameInfo._fields_]
    sizes = {"uint64_t": 8, "int32_t": 4}
    assert [sizes[t] for t, _ in fields] == [C.sizeof(t) for _, t in binding.FrameInfo._fields_]
    assert C.sizeof(binding.FrameInfo) == 80 and binding.FrameInfo.status.offset == 76


def test_create_rejects_bad_arguments():
    lib = _lib()
    cam, opt, tiles = _args()
    out = C.c_void_p()
    tp = C.c_void_p(tiles.ctypes.data)

    def create(scenes, n, t=tp, n_t=len(tiles), o=opt, frame=C.byref(out)):
        return lib.pt_frame_create(scenes, n, C.byref(cam), C.byref(o), t, n_t, 1, frame)

    dummy = C.create_string_buffer(64)  # (never dereferenced: every check below fails before a scene is used)
    one = (C.c_void_p * 1)(C.addressof(dummy))
    assert create(None, 1) == 1  # no scenes
    assert create((C.c_void_p * 1)(None), 1) == 1  # a null scene
    assert create(one, 0) == 1  # no replica
    assert create(one, 1, frame=None) == 1  # nowhere to put the frame
    assert create(one, 1, t=None) == 1  # null tiles
    bad = tiles.copy()
    bad[0]["w"] = 0
    assert create(one, 1, t=C.c_void_p(bad.ctypes.data)) == 1  # an empty tile
    bad = tiles.copy()
    bad[-1]["x"] = 7
    assert create(one, 1, t=C.c_void_p(bad.ctypes.data)) == 1  # a tile outside the image
    assert create(one, 1, o=binding.Options(0, 8, 1, 1, 1e-3)) == 1  # no image
    assert out.value is None
    assert b"tile" in lib.pt_last_error() or b"image" in lib.pt_last_error()


def test_null_frame_is_invalid():
    lib = _lib()
    assert lib.pt_frame_render(None, None, None, None, None, None) == 1
    assert lib.pt_frame_get_info(None, C.byref(binding.FrameInfo())) == 1
    assert lib.pt_frame_destroy(None) == 1


@pytest.mark.skipif(binding.device_count() > 0, reason="a HIP device is present")
def test_create_without_a_device_fails_with_a_message():
    lib = _lib()
    cam, opt, tiles = _args()
    dummy = C.create_string_buffer(64)  # (never dereferenced: without a device the call fails first)
    one = (C.c_void_p * 1)(C.addressof(dummy))
    out = C.c_void_p()
    rc = lib.pt_frame_create(one, 1, C.byref(cam), C.byref(opt), C.c_void_p(tiles.ctypes.data), len(tiles), 1, C.byref(out))
    assert rc == 2  # PT_ERR_NO_DEVICE
    assert out.value is None
    assert b"device" in lib.pt_last_error()


def test_cpp_header_compiles_standalone(tmp_path):
    src = tmp_path / "only_header.cpp"
    src.write_text("#include <PathTrace/frame_render.h>\nint main() { pt_frame_info i{}; return static_cast<int>(i.streams_parked); }\n")
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_cpp_program_compiles(tmp_path):
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_render_test.cpp")], str(tmp_path / "frame_render_test"), extra_flags=["-O1"])
