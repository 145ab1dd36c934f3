"""The reference-compatible C++ API (include/PathTrace + cpupathtrace_amd/libPathTrace.so).

CPU: the library builds; the reference's OWN unchanged test and demo sources compile and link against it (only in the build
container, where /root/reference exists); the tests that need no GPU pass.  GPU: the API test program and, if it was built,
the reference's test binary run in full."""
import os
import subprocess

import pytest

from cpupathtrace_amd import build_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "cpp", "shim")
REF = "/root/reference"
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
GPU_TESTS = "RenderTest,SceneTest,PostProcessingTest"  # tests of the reference's suite that render, query a Scene or post-process a frame (all on the GPU)


def _lib_env(**extra):
    """The environment for a program linked against libPathTrace.so: the loader is pointed at this tree's libraries, whichever
    directory or link the program itself lies in (its runpath is relative to its own location, which a link or a copy moves)."""
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    return dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path), **extra)


def _run(exe, skip=None):
    env = _lib_env()
    if skip:
        env["PT_TEST_SKIP"] = skip
    return subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def api_test_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "api_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "api_test.cpp")], out, extra_includes=[SHIM], extra_flags=["-O1"])
    return out


def build_reference_programs():
    """Compile the reference's unchanged test/ and demo/ sources against this repository's include/ (outputs: oracle/_ref/)."""
    os.makedirs(REF_OUT, exist_ok=True)
    tests = [os.path.join(REF, "test", f) for f in ("main.cpp", "render_test.cpp", "post_processing_test.cpp", "test_utils.cpp", "scene/boundig_box_test.cpp",
                                                      "scene/scene_test.cpp", "scene/mesh_test.cpp", "image/image_io_test.cpp")]
    build_host.compile_program(tests, os.path.join(REF_OUT, "ref_tests"), extra_includes=[SHIM, os.path.join(REF, "test")], extra_flags=["-O1"])
    build_host.compile_program([os.path.join(REF, "demo", "main.cpp")], os.path.join(REF_OUT, "ref_demo"), extra_flags=["-O1"])
    # the reference's benchmark program, unchanged, against tests/cpp/shim/benchmark/benchmark.h (Google Benchmark is not installed)
    build_host.compile_program([os.path.join(REF, "benchmark", "main.cpp")], os.path.join(REF_OUT, "ref_benchmark"), extra_includes=[SHIM], extra_flags=["-O2"])


def test_host_library_builds_and_links():
    lib = build_host.build()
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", lib], capture_output=True, text=True, check=True).stdout
    for symbol in ("processJob(", "processItem(", "Scene::getIntersection(", "Scene::sampleLights(", "Camera::shootRay(", "makeBox(", "makePlane(",
                   "io::loadMesh(", "postProcess(", "io::writeRGBImage(", "AABB::getIntersection("):
        assert symbol in out, symbol


def test_api_program_compiles_and_cpu_cases_pass(api_test_exe):
    r = _run(api_test_exe, skip="Render,Scene,WorkItem")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "[       OK ] Box.SlabTestKnownAnswers" in r.stdout


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "test", "render_test.cpp")), reason="reference sources not present")
def test_reference_sources_compile_unchanged():
    build_reference_programs()
    r = _run(os.path.join(REF_OUT, "ref_tests"), skip=GPU_TESTS)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("AABBTest.IntersectionTest", "MeshTest.SimpleMeshTest", "ImageIOTest.EncodeDecodeTest"):
        assert "[       OK ] " + name in r.stdout, r.stdout


@pytest.mark.gpu
def test_api_program_on_gpu(api_test_exe):
    r = _run(api_test_exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[       OK ]") == 12, r.stdout


@pytest.mark.gpu
def test_reference_benchmark_on_gpu(tmp_path):
    """benchmark/main.cpp of the reference, compiled unchanged (benchmark/main.cpp:15-32,59-110): renderSceneBox as it is, renderSceneDragonBox
    with the procedural stand-in mesh written where the program looks for assets/xyzrgb_dragon.obj -- the whole C++ path
    io::loadMesh -> moveObjects -> Scene::Scene -> processJob, 128 x 128 x 256 spp per iteration.  (Here a 179,400-triangle mesh; DESIGN.md has
    the 7.2 M-triangle run.)"""
    import re
    import sys
    exe = os.path.join(REF_OUT, "ref_benchmark")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_benchmark was not built (it is compiled from /root/reference in the build container)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import write_standin_obj
    assert write_standin_obj.write(str(tmp_path / "assets" / "xyzrgb_dragon.obj"), 300) == 179400
    r = subprocess.run([exe, "--benchmark_min_time=0.3"], cwd=str(tmp_path), env=_lib_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rates = dict(re.findall(r"^(renderScene\w+)/real_time.*items_per_second_per_iteration=([0-9.e+]+)", r.stdout, re.M))
    assert set(rates) == {"renderSceneBox", "renderSceneDragonBox"}, r.stdout
    print(r.stdout)
    assert float(rates["renderSceneBox"]) > 1e7 and float(rates["renderSceneDragonBox"]) > 1e7  # samples per second (the reference: ~1.3e6 on 8 cores)


@pytest.mark.gpu
def test_reference_test_binary_on_gpu():
    exe = os.path.join(REF_OUT, "ref_tests")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_tests was not built (it is compiled from /root/reference in the build container)")
    r = _run(exe)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "11 tests, 0 failed" in r.stdout, r.stdout


def _decode_png(path):
    """A minimal PNG reader (8-bit RGB or RGBA, no interlace): width, height, channels, rows of bytes."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, width, height, channels = 8, b"", 0, 0, 0
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if kind == b"IHDR":
            width, height, depth, colour, _, _, interlace = struct.unpack(">IIBBBBB", body)
            assert depth == 8 and interlace == 0 and colour in (2, 6)
            channels = 3 if colour == 2 else 4
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    raw = zlib.decompress(idat)
    stride = width * channels
    rows, prev = [], bytearray(stride)
    for y in range(height):
        f, line = raw[y * (stride + 1)], bytearray(raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        for i in range(stride):
            a = line[i - channels] if i >= channels else 0
            b, c = prev[i], (prev[i - channels] if i >= channels else 0)
            if f == 1:
                line[i] = (line[i] + a) & 255
            elif f == 2:
                line[i] = (line[i] + b) & 255
            elif f == 3:
                line[i] = (line[i] + (a + b) // 2) & 255
            elif f == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                line[i] = (line[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
        rows.append(bytes(line))
        prev = line
    return width, height, channels, rows


@pytest.mark.gpu
def test_reference_demo_on_gpu(tmp_path):
    """demo/main.cpp of the reference, compiled UNCHANGED against this repository's headers (demo/main.cpp:47-241: BASELINE.json configs[0]'s
    definition), run as a user would: the Cornell scene with the glass mesh (the stand-in written where the program looks for
    assets/xyzrgb_dragon.obj, demo/main.cpp:149), a mirror sphere and a box, 256 x 256, 16..64 spp, thin-lens camera; processJob with its
    progress callback, postProcess, io::writeRGBImage.  The PNG must be a 256 x 256 frame whose centre was hit (alpha > 0 -> a colour) and
    the progress lines must run up to 100 %."""
    import sys
    exe = os.path.join(REF_OUT, "ref_demo")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ref_demo was not built (it is compiled from /root/reference in the build container)")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import write_standin_obj
    assert write_standin_obj.write(str(tmp_path / "assets" / "xyzrgb_dragon.obj"), 300) == 179400
    out_png = str(tmp_path / "out" / "demo.png")
    r = subprocess.run([exe, out_png], cwd=str(tmp_path), env=_lib_env(PATHTRACE_SEED="1234"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "100.00% (64 / 64 tiles)" in r.stdout, r.stdout[-500:]
    width, height, channels, rows = _decode_png(out_png)
    assert (width, height) == (256, 256) and channels in (3, 4)
    centre = rows[128][128 * channels:128 * channels + 3]
    assert max(centre) > 0, "the centre of the frame shows the scene"
    lit = sum(1 for row in rows for i in range(0, len(row), channels) if max(row[i:i + 3]) > 0)
    assert lit > 0.5 * 256 * 256, "most of the frame is inside the box"
    # the same program again with the same seed: the frame is reproducible bit for bit
    out2 = str(tmp_path / "out" / "demo2.png")
    r2 = subprocess.run([exe, out2], cwd=str(tmp_path), env=_lib_env(PATHTRACE_SEED="1234"), capture_output=True, text=True, timeout=900)
    assert r2.returncode == 0 and open(out2, "rb").read() == open(out_png, "rb").read()
