"""View batches on the GPU (pt_render_views*, Scene.process_views*, PathTrace/view_batch.h): V cameras of one scene in one launch, each view
bit for bit what process_job gives for its camera and seed -- on every instantiation of the path kernel, at ragged sizes, at 64 views, into
device memory, over replicas, with progress; bad arguments fail before anything is launched."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cpupathtrace_amd import binding, build_host, scenes
from tests.util import assert_bits_equal, env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [11, 2024, 77, 9001, 123456789012]


def _views(cam, n):
    """n cameras around `cam`: pinhole, thin lens with a circular aperture and hexagonal aperture in turn, each from a different place."""
    out = []
    for v in range(n):
        c = dict(cam)
        c["origin"] = (cam["origin"][0] + 0.07 * v, cam["origin"][1] + 0.03 * (v % 3), cam["origin"][2] - 0.02 * v)
        kind = v % 3
        c["aperture_kind"] = kind
        c["aperture_width"] = c["aperture_height"] = 0.0 if kind == 0 else 0.04 + 0.01 * v
        c["hex_ratio"] = 0.35 if kind == 2 else 0.0
        c["focal_plane_dist"] = 0.0 if kind == 0 else 3.0 + 0.1 * v
        out.append(c)
    return out


def _singles(gpu, cams, opt, seeds):
    return np.stack([gpu.process_job(c, opt, base_seed=s) for c, s in zip(cams, seeds)])


def _lit_room(n_point_lights=12):
    """A closed room with Lambertian, glass and mirror objects, point lights and two emitters (12 lights: 14 light samples per vertex, the
    kernel with the 64-bit slot word)."""
    sb = scenes.SceneBuilder()
    sb.triangles(scenes.make_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), sb.material((0.75, 0.7, 0.65, 1.0)))
    sb.sphere((0.35, -0.6, 0.1), 0.35, sb.material((1, 1, 1, 1), 1.5, bsdf=scenes.BSDF_GLASS))
    sb.sphere((-0.45, -0.7, -0.3), 0.28, sb.material((0.9, 0.9, 1.0, 1), bsdf=scenes.BSDF_MIRROR))
    sb.triangles(scenes.make_plane((-0.25, 0.97, -0.25), (0.25, 0.97, 0.25)), sb.material((1, 1, 1, 1), 1.0, (4, 3.5, 3, 1)), cull=True)
    sb.sphere((-0.6, 0.4, 0.5), 0.1, sb.material((1, 1, 1, 1), 1.0, (1, 2, 4, 1)))
    for k in range(n_point_lights):
        a = 2.0 * np.pi * k / max(n_point_lights, 1)
        sb.point_light((0.7 * np.cos(a), 0.3 + 0.05 * k, 0.7 * np.sin(a)), (0.2 + 0.05 * k, 0.3, 0.5 - 0.02 * k, 1.0))
    return sb.build(), scenes.camera((0, 0, -3), (0, 0, 0), (0, 1, 0), 1.0, 1.0, -1.0)


@pytest.fixture(scope="module")
def box():
    sc, cam = scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    yield sc, cam, gpu
    gpu.close()


@pytest.mark.parametrize("name", ["cornell", "box"])
@pytest.mark.parametrize("spp", [(4, 4), (2, 24)], ids=["fixed", "adaptive"])
def test_views_match_single_renders(name, spp):
    sc, cam = scenes.cornell_scene(40, 32) if name == "cornell" else scenes.box_scene()
    gpu = binding.Scene(sc, device=0)
    try:
        opt = scenes.options(40, 32, *spp)
        cams = _views(cam, 5)
        got, stats = gpu.process_views(cams, opt, base_seeds=SEEDS, want_stats=True)
        assert got.shape == (5, 32, 40, 4) and got.dtype == np.float32
        want = _singles(gpu, cams, opt, SEEDS)
        for v in range(5):
            assert_bits_equal(got[v], want[v], "%s view %d" % (name, v))
        assert stats["launches"] == 1 and stats["samples"] >= 5 * 32 * 40 * spp[0]
        assert not (got[0] == got[1]).all(), "the views differ"
    finally:
        gpu.close()


@pytest.mark.parametrize("variant", ["lds_window8", "lds_window4", "hbm_tree", "wide_word"])
def test_every_kernel_variant(variant):
    knobs = {}
    if variant == "lds_window8":
        sc, cam = scenes.cornell_scene(24, 20)
        knobs = {"PT_STACK_WINDOW": 8}
    elif variant == "lds_window4":
        sc, cam = scenes.box_scene()
        knobs = {"PT_STACK_WINDOW": 4}
    elif variant == "hbm_tree":
        mesh = scenes.bumpy_sphere_mesh(230, 230, scenes.DRAGON_BOX_TRANSFORM)
        assert len(mesh[0]) >= 100000
        sc, cam = scenes.dragon_box_scene(*mesh)
    else:
        sc, cam = _lit_room(12)
    with env(PT_DEBUG="0", **knobs):
        gpu = binding.Scene(sc, device=0)
        try:
            opt = scenes.options(24, 20, 2, 6)
            cams = _views(cam, 3)
            got = gpu.process_views(cams, opt, base_seeds=SEEDS[:3])
            want = _singles(gpu, cams, opt, SEEDS[:3])
            for v in range(3):
                assert_bits_equal(got[v], want[v], "%s view %d" % (variant, v))
        finally:
            gpu.close()


def test_ragged_sizes(box):
    _, cam, gpu = box
    opt = scenes.options(37, 23, 3, 3)  # tile size 5: clipped edge tiles; 851 pixels per view, not a multiple of 64
    cams = _views(cam, 3)
    got = gpu.process_views(cams, opt, base_seeds=SEEDS[:3])
    want = _singles(gpu, cams, opt, SEEDS[:3])
    for v in range(3):
        assert_bits_equal(got[v], want[v], "37x23 view %d" % v)
    opt = scenes.options(7, 3, 2, 2)  # tile size 1
    got = gpu.process_views(cams, opt, base_seeds=5)
    for v in range(3):
        assert_bits_equal(got[v], gpu.process_job(cams[v], opt, base_seed=5), "7x3 view %d" % v)


def test_one_view_is_process_job(box):
    _, cam, gpu = box
    opt = scenes.options(48, 40, 2, 12)
    c = _views(cam, 2)[1]
    got, stats = gpu.process_views([c], opt, base_seeds=[SEEDS[1]], want_stats=True)
    want, want_stats = gpu.process_job(c, opt, base_seed=SEEDS[1], want_stats=True)
    assert_bits_equal(got[0], want, "one view")
    for k in ("samples", "rays_traced", "shadow_rays_traced", "vertices", "shading_passes", "wavefronts", "slot_rows"):
        assert stats[k] == want_stats[k], (k, stats[k], want_stats[k])


def test_full_batch(box):
    _, cam, gpu = box
    n, size, spp = 64, 128, 2
    opt = scenes.options(size, size, spp, spp)
    cams = [dict(cam, origin=(0.6 * np.sin(2 * np.pi * v / n), 0.1, -3.0 + 0.6 * (1 - np.cos(2 * np.pi * v / n)))) for v in range(n)]
    seeds = [1000 + 7 * v for v in range(n)]
    got, stats = gpu.process_views(cams, opt, base_seeds=seeds, want_stats=True)
    assert got.shape == (n, size, size, 4)
    samples = 0
    for v in range(n):
        want, st = gpu.process_job(cams[v], opt, base_seed=seeds[v], want_stats=True)
        samples += st["samples"]
        if v % 9 == 0 or v == n - 1:
            assert_bits_equal(got[v], want, "view %d of %d" % (v, n))
    assert stats["samples"] == samples and stats["launches"] == 1
    print("64 x 128^2 x %d spp: %.2f ms in one launch (%.1f Msamples/s)" % (spp, stats["kernel_ms"], stats["samples"] / stats["kernel_ms"] / 1e3))


DEVICE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from cpupathtrace_amd import binding, scenes
from tests.test_gpu_views import SEEDS, _views
out = torch.full((4, 17, 33, 4), -1.0, dtype=torch.float32, device="cuda:0")
sc, cam = scenes.box_scene()
gpu = binding.Scene(sc, device=0)
opt = scenes.options(33, 17, 2, 8)
cams = _views(cam, 4)
want = gpu.process_views(cams, opt, base_seeds=SEEDS[:4])
stats = gpu.process_views_device(cams, opt, out.data_ptr(), torch.cuda.current_stream(0).cuda_stream, base_seeds=SEEDS[:4], want_stats=True)
torch.cuda.synchronize()
got = out.cpu().numpy()
same = got.view(np.uint32) == want.view(np.uint32)
print("launches %d, equal values %d of %d" % (stats["launches"], int(same.sum()), same.size))
sys.exit(0 if same.all() and stats["launches"] == 1 else 1)
"""


def test_device_output():
    """process_views_device into a [V, H, W, 4] torch tensor equals process_views.  In a fresh interpreter in which torch opens the device
    first (as for the RCCL tests: torch cannot take the device over from the library in the same process)."""
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", DEVICE_CHILD, ROOT], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]


def test_replicas(box):
    sc, cam, gpu = box
    other = binding.Scene(sc, device=0)
    try:
        opt = scenes.options(64, 64, 2, 6)  # 16 tiles of 16 per view
        cams = _views(cam, 3)
        want = gpu.process_views(cams, opt, base_seeds=SEEDS[:3])
        got, stats = binding.process_views_multi([gpu, other], cams, opt, base_seeds=SEEDS[:3], want_stats=True)
        assert_bits_equal(got, want, "two replicas")
        assert stats[0]["launches"] == 1 and stats[1]["launches"] == 1
    finally:
        other.close()


def test_progress(box):
    _, cam, gpu = box
    opt = scenes.options(64, 48, 2, 2)
    cams = _views(cam, 5)
    seen = []
    got = gpu.process_views(cams, opt, base_seeds=SEEDS, progress=lambda done, total: seen.append((done, total)))
    total = 5 * len(binding.job_tiles(64, 48))
    assert [d for d, _ in seen] == list(range(1, total + 1)) and all(t == total for _, t in seen)
    assert_bits_equal(got[4], gpu.process_job(cams[4], opt, base_seed=SEEDS[4]), "view 4 with progress")


def test_invalid_arguments(box):
    _, cam, gpu = box
    lib = binding.load()
    opt = scenes.options(16, 16, 2, 2)
    before = gpu.process_job(cam, opt, base_seed=3)
    cams = (binding.CameraParams * 2)(binding._camera(cam), binding._camera(cam))
    seeds = np.array([1, 2], np.uint64)
    sp = seeds.ctypes.data_as(C.POINTER(C.c_uint64))
    img = np.zeros((2, 16, 16, 4), np.float32)
    handles = (C.c_void_p * 1)(gpu._h)

    def views(cameras=cams, seed_ptr=sp, n=2, o=opt, out=img):
        op = binding._options(o)
        return lib.pt_render_views(handles, C.c_int(1), cameras, seed_ptr, C.c_int32(n), C.byref(op), binding._ptr(out), None, None, None)

    for rc in (views(n=0), views(n=-3), views(cameras=None), views(seed_ptr=None), views(out=None),
               views(o=scenes.options(16384, 8192, 1, 1)),  # 2 x 16384 x 8192 pixels: one more than a call may have
               views(o=scenes.options(16, 0, 1, 1))):
        assert rc == 1, (rc, lib.pt_last_error())  # PT_ERR_INVALID
    op = binding._options(opt)
    assert lib.pt_render_views_device(gpu._h, cams, sp, C.c_int32(0), C.byref(op), C.c_void_p(1), None, None) == 1
    assert lib.pt_render_views_device(gpu._h, cams, None, C.c_int32(2), C.byref(op), C.c_void_p(1), None, None) == 1
    with pytest.raises(binding.PtError) as e:
        binding.process_views_multi([gpu], [cam, cam], scenes.options(16, 0, 1, 1))
    assert e.value.code == 1
    assert_bits_equal(gpu.process_job(cam, opt, base_seed=3), before, "the scene after refused calls")


def test_cpp_views_program(tmp_path):
    exe = str(tmp_path / "views_test")
    build_host.compile_program([os.path.join(ROOT, "tests", "cpp", "views_test.cpp")], exe, extra_flags=["-O1"])
    path = [build_host.HERE] + [p for p in os.environ.get("LD_LIBRARY_PATH", "").split(os.pathsep) if p]
    r = subprocess.run([exe], env=dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join(path)), capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("[ OK ]") == 6, r.stdout
