"""CPU checks of progressive frames (pt_frame_set_progressive, pt_frame_get_progress; binding.Frame.set_progressive / progress;
FrameRender::setProgressive / progress and the same on ViewBatchRender): the symbols and their declarations, the refusals that need no
device, the layouts of the structs on both sides, the C++ headers and the test program.  Nothing that existed changed its layout or left
the export list."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

from cpupathtrace_amd import binding, build, build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1

DECLARATIONS = {
    "pt_frame_set_progressive": "int pt_frame_set_progressive(pt_frame *frame, int32_t quantum, int32_t max_passes_per_call);",
    "pt_frame_get_progress": "int pt_frame_get_progress(const pt_frame *frame, pt_frame_progress *out);",
}
# every entry point the library had before this mode existed
EARLIER_EXPORTS = """pt_device_count pt_last_error pt_scene_create pt_scene_destroy pt_scene_info pt_scene_emissive pt_scene_bvh_dump pt_intersect_batch
pt_render_streams pt_render_item pt_render_tiles pt_render_tiles_progress pt_render_tiles_multi pt_render_tiles_device pt_render_tiles_ctl pt_render_cancel
pt_job_tiles pt_pixel_seed pt_rng_seed_to_state pt_post_process pt_post_process_device pt_frame_preview pt_frame_create pt_frame_render pt_frame_get_info
pt_frame_destroy pt_render_views pt_render_views_device pt_denoise_params_default pt_render_features pt_render_features_device pt_denoise pt_denoise_device
pt_frame_create_views pt_render_features_views pt_render_features_views_device pt_denoise_views pt_denoise_views_device pt_temporal_params_default
pt_temporal_create pt_temporal_denoise pt_temporal_denoise_device pt_temporal_reset pt_temporal_destroy""".split()


@pytest.fixture(scope="module")
def lib():
    build.build()
    return binding.load()


def test_symbols_are_exported_and_declared(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(binding.PROGRESSIVE_EXPORTS) == set(DECLARATIONS)
    assert set(binding.PROGRESSIVE_EXPORTS) <= names
    assert set(binding.PROGRESSIVE_EXPORTS) <= set(binding.EXPORTS)
    header = " ".join(open(os.path.join(ROOT, "include", "pt_hip.h")).read().split())
    for name, decl in DECLARATIONS.items():
        assert decl in header, name
    assert set(EARLIER_EXPORTS) <= names, set(EARLIER_EXPORTS) - names
    assert set(EARLIER_EXPORTS) | set(DECLARATIONS) == set(binding.EXPORTS)


def test_refusals_need_no_device(lib):
    dummy = C.create_string_buffer(1024)  # (never dereferenced: every check below fails before the frame is used)
    frame = C.c_void_p(C.addressof(dummy))
    out = binding.FrameProgress()
    assert lib.pt_frame_set_progressive(None, C.c_int32(4), C.c_int32(0)) == PT_ERR_INVALID
    assert lib.pt_frame_set_progressive(None, C.c_int32(0), C.c_int32(0)) == PT_ERR_INVALID
    assert lib.pt_frame_set_progressive(frame, C.c_int32(-1), C.c_int32(0)) == PT_ERR_INVALID
    assert b"quantum" in lib.pt_last_error()
    assert lib.pt_frame_set_progressive(frame, C.c_int32(-2 ** 31), C.c_int32(3)) == PT_ERR_INVALID
    assert lib.pt_frame_get_progress(None, C.byref(out)) == PT_ERR_INVALID
    assert lib.pt_frame_get_progress(frame, None) == PT_ERR_INVALID
    assert dummy.raw == bytes(1024)


def test_struct_layouts_agree_with_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pt_frame_info), sizeof(pt_frame_progress), offsetof(pt_frame_progress, target), '
                   'offsetof(pt_frame_progress, min_samples), offsetof(pt_frame_progress, streams_at_target), offsetof(pt_frame_progress, samples_lost)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    P = binding.FrameProgress
    assert got == [80, C.sizeof(P), P.target.offset, P.min_samples.offset, P.streams_at_target.offset, P.samples_lost.offset], got
    assert C.sizeof(binding.FrameInfo) == 80, "pt_frame_info keeps its layout"
    assert [k for k, _ in P._fields_] == ["quantum", "max_passes_per_call", "passes_completed", "target", "pass_in_progress", "min_samples", "max_samples",
                                           "streams_at_target", "samples_lost"]


def test_binding_methods():
    for cls in (binding.Frame, binding.ViewsFrame):
        assert list(inspect.signature(cls.set_progressive).parameters) == ["self", "quantum", "max_passes_per_call"]
        assert inspect.signature(cls.set_progressive).parameters["max_passes_per_call"].default == 0
        assert list(inspect.signature(cls.progress).parameters) == ["self"]
    frame = binding.Frame.__new__(binding.Frame)
    frame._h = None
    with pytest.raises(ValueError):
        frame.set_progressive(4)
    with pytest.raises(ValueError):
        frame.progress()
    frame._h = C.c_void_p(1)
    with pytest.raises(ValueError):
        frame.set_progressive(-1)  # (refused before the library sees the handle)
    frame._h = None


def test_cpp_headers_declare_the_methods(tmp_path):
    src = tmp_path / "only_headers.cpp"
    src.write_text("#include <PathTrace/frame_render.h>\n#include <PathTrace/view_batch_render.h>\n"
                   "void (FrameRender::*a)(int, int) = &FrameRender::setProgressive;\n"
                   "pt_frame_progress (FrameRender::*b)() const = &FrameRender::progress;\n"
                   "void (ViewBatchRender::*c)(int, int) = &ViewBatchRender::setProgressive;\n"
                   "pt_frame_progress (ViewBatchRender::*d)() const = &ViewBatchRender::progress;\n"
                   "int main() { return a == nullptr || b == nullptr || c == nullptr || d == nullptr; }\n")
    subprocess.run(["g++", "-std=c++20", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def test_cpp_program_compiles_and_links(tmp_path):
    exe = str(tmp_path / "frame_progressive_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "frame_progressive_test.cpp")], exe, extra_flags=["-O1"])
    assert os.path.exists(exe)
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", build_host.build()], capture_output=True, text=True, check=True).stdout
    for name in ("FrameRender::setProgressive(int, int)", "FrameRender::progress() const", "ViewBatchRender::setProgressive(int, int)",
                 "ViewBatchRender::progress() const"):
        assert name in out, name
