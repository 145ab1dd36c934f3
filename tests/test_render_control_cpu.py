"""CPU checks of the controlled render (pt_render_tiles_ctl / pt_render_cancel, include/PathTrace/render_control.h): the symbols, the
error code, argument checks that need no device, and the C++ header and test program compile."""
import ctypes as C
import os
import re
import subprocess

from cpupathtrace_amd import binding, build, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    build.build()
    return binding.load()


def test_symbols_are_exported():
    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert {"pt_render_tiles_ctl", "pt_render_cancel"} <= names


def test_cancelled_code_is_six():
    header = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert re.search(r"#define\s+PT_ERR_CANCELLED\s+6\b", header)
    assert binding.PT_ERR_CANCELLED == 6 and binding.ERRORS[6] == "PT_ERR_CANCELLED"


def test_control_layout_matches_header():
    # the ctypes mirror of pt_render_control: 5 eight-byte fields, a pointer, an int32 (padded to 56 bytes)
    assert C.sizeof(binding.RenderControl) == 56
    assert binding.RenderControl.cancel_requested.offset == 48


def test_cancel_of_null_is_invalid():
    assert _lib().pt_render_cancel(None) == 1  # PT_ERR_INVALID


def test_cancel_sets_the_flag():
    ctl = binding.RenderControl()
    ctl.cancel()
    assert ctl.cancel_requested == 1


def test_ctl_rejects_bad_arguments():
    lib = _lib()
    cam, opt, ctl = binding._camera({"origin": (0, 0, -3), "look_at": (0, 0, 0), "up": (0, 1, 0), "focal_length": 1.0, "height": 1.0,
                                     "aspect_ratio": 1.0}), binding.Options(8, 8, 1, 1, 1e-3), binding.RenderControl()
    tiles = binding.job_tiles(8, 8)
    image = (C.c_float * (8 * 8 * 4))()

    def call(scenes, n, control, tiles_ptr=C.c_void_p(tiles.ctypes.data), img=image):
        return lib.pt_render_tiles_ctl(scenes, C.c_int(n), C.byref(cam), C.byref(opt), tiles_ptr, C.c_size_t(len(tiles)), C.c_uint64(1), img, None, None, None,
                                       control)

    assert call(None, 1, C.byref(ctl)) in (1, 2)  # no scenes
    null_scene = (C.c_void_p * 1)(None)
    assert call(null_scene, 1, C.byref(ctl)) in (1, 2)  # a null scene
    assert call(null_scene, 0, C.byref(ctl)) in (1, 2)  # no replica
    assert call(null_scene, 1, None) == 1  # no control


def test_cpp_header_compiles_standalone(tmp_path):
    src = tmp_path / "only_header.cpp"
    src.write_text("#include <PathTrace/render_control.h>\nint main() { RenderControl c; c.cancel(); return c.cancelled() ? 1 : 0; }\n")
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_cpp_program_compiles(tmp_path):
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "render_control_test.cpp")], str(tmp_path / "render_control_test"), extra_flags=["-O1"])
