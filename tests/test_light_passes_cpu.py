"""Light-group passes without a GPU (include/pt_light_passes.h): the host library's declarations, layout and refusals; the
yardstick tests/light_pass_ref.py against gather_ref.paths_from_rays -- its terms partition the radiance --; what the case tables and rays
hold; the mix, restated twice and computed by the library's host form; and a bound for the sum of the passes against the total."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build
from tests import light_pass_cases as cases, light_pass_ref as ref, pose_probe, query_cases, radiance_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, D = np.float32, np.float64
EPSILON = cases.OPTIONS["epsilon"]
SAMPLES = 4


# ---- 1. the host library -----------------------------------------------------------------------------------------------------------------------------

def test_light_passes_exports_declarations_and_layout():
    header = open(os.path.join(ROOT, "include", "pt_light_passes.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\(", header, re.M))
    assert declared == set(binding.LIGHT_PASSES_EXPORTS) and len(binding.LIGHT_PASSES_EXPORTS) == 7
    for name in dir(binding):
        if name.endswith("EXPORTS") and name != "LIGHT_PASSES_EXPORTS":
            assert not set(getattr(binding, name)) & declared, name
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h") and other != "pt_light_passes.h":
            assert not re.findall(r"\bpt_light_passes_[a-z_]*\s*\(", open(os.path.join(ROOT, "include", other)).read()), other
    # pt_hip.h reaches the header through pt_radiance.h, behind that file's own declarations
    radiance = open(os.path.join(ROOT, "include", "pt_radiance.h")).read()
    assert radiance.index('#include "pt_light_passes.h"') > radiance.index("int pt_radiance_capture_device(")
    flat = " ".join(header.replace(" * ", " ").split())
    for text in ("a pinhole or thin-lens model", "adaptive sampling", "resumable and checkpointed passes", "per-instance groups", "denoising of passes", "more than one device"):
        assert text in flat[flat.index("Left out:"):], text
    assert "do NOT in general add up to total bit for bit" in flat
    for name, value in (("PT_LIGHT_GROUPS_MAX", 8), ("PT_PASS_EMITTED", 0), ("PT_PASS_DIRECT", 1), ("PT_PASS_INDIRECT", 2)):
        assert re.search(r"^#define %s\s+%d$" % (name, value), header, re.M), name
    assert (binding.LIGHT_GROUPS_MAX, binding.PASS_EMITTED, binding.PASS_DIRECT, binding.PASS_INDIRECT) == (8, 0, 1, 2)
    assert binding.LightPass.itemsize == 16 and [binding.LightPass.fields[n][1] for n in ("value", "pad")] == [0, 12]
    g = binding.LightGroups
    assert C.sizeof(g) == 40 and [getattr(g, n).offset for n in ("n_groups", "split", "material_group", "n_materials", "point_light_group", "n_point_lights")] == [0, 4, 8, 16, 24, 32]
    assert "pt_light_passes.cpp" in build.SOURCES and "pt_light_pass_kernels.h" in build.HEADERS
    assert any(h.endswith(os.path.join("include", "pt_light_passes.h")) for h in build.HEADERS)
    lib = C.CDLL(build.build())
    for name in binding.LIGHT_PASSES_EXPORTS:
        assert hasattr(lib, name), name


def test_sizeof_the_structs_in_c(tmp_path):
    """40 and 16 bytes, by the compiler that builds the host side."""
    src = tmp_path / "size.c"
    src.write_text('#include "pt_hip.h"\n_Static_assert(sizeof(pt_light_groups) == 40, "groups");\n_Static_assert(sizeof(pt_light_pass) == 16, "pass");\n'
                   'int main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "size.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_count_of_passes():
    for n_groups in range(1, 9):
        for split in (False, True):
            assert binding.light_groups(n_groups, [], [], split).n_passes == n_groups * (3 if split else 1)
    lib = binding.load()
    n = C.c_uint32(77)
    ok = binding.light_groups(3, [], [])
    assert lib.pt_light_passes_count(None, C.byref(n)) == 1 and lib.pt_light_passes_count(C.byref(ok), None) == 1
    for n_groups, split in ((0, 0), (9, 0), (3, 2), (3, -1)):
        assert lib.pt_light_passes_count(C.byref(binding.light_groups(n_groups, [], [], split)), C.byref(n)) == 1 and n.value == 77


def test_refusals_that_need_no_device():
    """Every scene-independent refusal of the header's list comes before any device work and before the scene is locked, so this machine
    needs no GPU to see them.  The scene is a block of zero bytes."""
    lib = binding.load()
    scene = C.cast(C.create_string_buffer(1 << 20), C.c_void_p)
    p = binding._ptr
    rays, passes, total = np.zeros((4, 6), F), np.zeros((8, 24), binding.LightPass), np.zeros(8, binding.RadianceResult)
    ok = binding.radiance_params(4, 1e-3)
    view = ((0.0, 0.0, -1.6), (0.0, 0.0, 1.0), (0, 1, 0))
    desc = binding.capture_desc(binding.CAPTURE_EQUIRECT, 4, 2, *view)
    good = binding.light_groups(3, [0, 1, 2], [2, 0])

    def calls(g=good, rp=ok, scene=scene, r=p(rays), out=p(passes), n=4, d=desc, only=None):
        g = C.byref(g) if g is not None else None
        rp = C.byref(rp) if rp is not None else None
        d = C.byref(d) if d is not None else None
        n = C.c_size_t(n)
        ray = [lambda: lib.pt_light_passes_rays(scene, r, n, g, rp, out, p(total)), lambda: lib.pt_light_passes_rays_device(scene, r, n, g, rp, out, p(total), None)]
        capture = [lambda: lib.pt_light_passes_capture(scene, d, g, rp, out, p(total)), lambda: lib.pt_light_passes_capture_device(scene, d, g, rp, out, p(total), None)]
        return {"rays": ray, "capture": capture}.get(only, ray + capture)

    def refused(some, word):
        for call in some:
            assert call() == 1 and word in lib.pt_last_error(), lib.pt_last_error()  # PT_ERR_INVALID

    # every refusal of the corresponding radiance call
    refused(calls(scene=None) + calls(rp=None) + calls(r=None, only="rays") + calls(d=None, only="capture"), b"null")
    for samples in (0, -5):
        refused(calls(rp=binding.radiance_params(samples, 1e-3)), b"samples")
    refused(calls(rp=binding.radiance_params(1 << 29, 1e-3)), b"0x7fffffff")
    refused(calls(n=1 << 31, only="rays"), b"0x7fffffff")
    for epsilon in (-1e-3, float("nan")):
        refused(calls(rp=binding.radiance_params(4, epsilon)), b"epsilon")
    for bad in (dict(model=7), dict(width=0), dict(jitter=2)):
        d = binding.capture_desc(binding.CAPTURE_EQUIRECT, 4, 2, *view)
        for k, v in bad.items():
            setattr(d, k, v)
        refused(calls(d=d, only="capture"), {"model": b"model", "width": b"width", "jitter": b"jitter"}[list(bad)[0]])
    refused(calls(d=binding.capture_desc(binding.CAPTURE_CUBE, 13, 2, *view), only="capture"), b"6 * height")
    refused(calls(d=binding.capture_desc(binding.CAPTURE_FISHEYE, 4, 4, *view, fov=0.0), only="capture"), b"fov")
    refused(calls(d=binding.capture_desc(binding.CAPTURE_ORTHO, 4, 2, *view, extent=(0.0, 1.0)), only="capture"), b"extent")
    d = binding.capture_desc(binding.CAPTURE_EQUIRECT, 4, 2, *view)
    d.up[1] = float("inf")
    refused(calls(d=d, only="capture"), b"finite")
    # null groups or passes
    refused(calls(g=None) + calls(out=None), b"null")
    # (n == 0 needs no arrays and launches nothing -- but it needs the groups)
    assert lib.pt_light_passes_rays(scene, None, C.c_size_t(0), C.byref(good), C.byref(ok), None, None) == 0
    assert lib.pt_light_passes_rays_device(scene, None, C.c_size_t(0), C.byref(good), C.byref(ok), None, None, None) == 0
    assert lib.pt_light_passes_rays(scene, None, C.c_size_t(0), None, C.byref(ok), None, None) == 1
    # n_groups outside 1..8, a split other than 0 or 1
    for n_groups in (0, 9, 255):
        refused(calls(g=binding.light_groups(n_groups, [], [])), b"n_groups")
    for split in (2, -1):
        refused(calls(g=binding.light_groups(3, [0], [0], split)), b"split")
    # a null table with a non-zero count
    for field in ("material_group", "point_light_group"):
        bad = binding.light_groups(3, [0, 1, 2], [2, 0])
        setattr(bad, field, None)
        refused(calls(g=bad), b"null group table")
    # a table entry >= n_groups
    refused(calls(g=binding.light_groups(3, [0, 3, 2], [2, 0])), b"material's group")
    refused(calls(g=binding.light_groups(3, [0, 1, 2], [2, 255])), b"point light's group")
    refused(calls(g=binding.light_groups(1, [0, 0], [1])), b"point light's group")
    # n x samples x P above 0x7fffffff, with n x samples below it: 4 rays x 2^25 samples x 24 passes, 8 pixels x 2^24 samples x 24 passes
    refused(calls(g=binding.light_groups(8, [], [], True), rp=binding.radiance_params(1 << 25, 1e-3), only="rays"), b"passes above 0x7fffffff")
    refused(calls(g=binding.light_groups(8, [], [], True), rp=binding.radiance_params(1 << 24, 1e-3), only="capture"), b"passes above 0x7fffffff")
    # the mix: a null argument with n > 0, n_passes outside 1..24
    gains, out = np.ones((24, 3), F), np.zeros((8, 4), F)

    def mixes(a=p(passes), n=8, n_passes=24, g=p(gains), o=p(out), scene=scene):
        n, n_passes = C.c_size_t(n), C.c_uint32(n_passes)
        return [lambda: lib.pt_light_passes_mix(a, n, n_passes, g, None, o), lambda: lib.pt_light_passes_mix_device(scene, a, n, n_passes, g, None, o, None)]

    refused(mixes(a=None) + mixes(g=None) + mixes(o=None) + mixes(scene=None)[1:], b"null")
    for n_passes in (0, 25, 1 << 20):
        refused(mixes(n_passes=n_passes), b"n_passes")
    for call in mixes(a=None, g=None, o=None, n=0):
        assert call() == 0


# ---- 2. the yardstick ----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("light_pass_pose") / "libpose_probe.so")))


@pytest.fixture(scope="module")
def case(oracle_lib, assembler):
    """The case rays at 4 samples on the yardstick: computed once for the tests below."""
    scene, instances, shapes = cases.build()
    flat = query_cases.flatten(scene, instances, shapes, assembler)
    handle = oracle_lib.scene_create(flat["scene"])
    rays = cases.rays(flat)
    L, missed, terms = ref.ray_terms(handle, flat, rays, SAMPLES, EPSILON, cases.SEED)
    yield dict(flat=flat, handle=handle, rays=rays, L=L, missed=missed, terms=terms)
    handle.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_the_yardstick_partitions_the_radiance(case):
    """For every sample of the case rays, re-adding the recorded terms of all passes in the path's order into one accumulator gives
    gather_ref.paths_from_rays's rgb bit for bit; the alpha and the missed flags agree as well."""
    rays, n = case["rays"], len(case["rays"]) * SAMPLES
    assert rays.shape == (cases.N_RAYS, 6) and np.isfinite(rays).all()
    want, want_missed, _ = radiance_ref.ray_samples(case["handle"], case["flat"], rays, SAMPLES, EPSILON, cases.SEED)
    assert same_bits(case["L"], want).all() and (case["missed"] == want_missed).all()
    again = ref.readd(case["terms"], n).reshape(len(rays), SAMPLES, 4)
    assert same_bits(again[..., :3], want[..., :3]).all()
    assert (want[..., 3] == np.where(want_missed, 0.0, 1.0)).all()
    # a term's lanes are distinct (one addition per sample at each point of the loop), its scatterings are not negative
    for lanes, key, k, term in case["terms"]:
        assert len(np.unique(lanes)) == len(lanes) == len(key) == len(k) == len(term) and (k >= 0).all()
    # with one group and no split, the single accumulator IS out_spectrum's rgb
    one = dict(n_groups=1, split=False, material_group=np.zeros(len(cases.MATERIALS), np.uint8), point_light_group=np.zeros(cases.N_POINT_LIGHTS, np.uint8))
    acc, _ = ref.accumulate(case["terms"], n, one)
    assert same_bits(acc[:, 0], want.reshape(n, 4)[:, :3]).all()


def test_the_case_tables_hold_what_their_docstring_says(case):
    three, eight = cases.table("THREE", True), cases.table("EIGHT", True)
    assert cases.MATERIALS.index("lamp") == 5 and cases.MATERIALS.index("glow") == 6
    assert three["material_group"].tolist() == [0, 0, 0, 0, 0, 0, 1] and three["point_light_group"].tolist() == [2, 2] and three["n_groups"] == 3
    assert eight["material_group"].tolist() == [0, 1, 2, 3, 4, 5, 6] and eight["point_light_group"].tolist() == [7, 0] and eight["n_groups"] == 8
    assert [ref.n_passes(cases.table(name, split)) for name, split in cases.TABLES] == [3, 9, 8, 24]
    for name, split in cases.TABLES:
        assert cases.groups(cases.table(name, split)).n_passes == ref.n_passes(cases.table(name, split))
    # Every (group, component) pass of THREE that CAN receive a term receives a non-zero one from the case rays, so that no GPU test passes
    # on empty passes.  One of the nine cannot: a light sample has k = path_length >= 1 scatterings before it, and a point light is no
    # surface a ray could find, so (point lights, emitted) stays at +0 by the definition itself -- for any rays.
    acc, _ = ref.accumulate(case["terms"], len(case["rays"]) * SAMPLES, three)
    reached = (acc != 0).any(axis=(0, 2)).reshape(3, 3)
    print("passes of THREE that receive a term (group x component):\n%s" % reached.astype(int))
    assert reached[0].all() and reached[1].all() and reached[2].tolist() == [False, True, True]
    assert (acc[:, 2 * 3 + binding.PASS_EMITTED].view(np.uint32) == 0).all()
    # the two hand-made rays see their emitter along the ray itself
    first = acc.reshape(len(case["rays"]), SAMPLES, 9, 3)
    assert (first[0, :, 0 * 3 + binding.PASS_EMITTED] > 0).all() and (first[1, :, 1 * 3 + binding.PASS_EMITTED] > 0).all()
    # without the split a group's pass takes the terms of its three components
    flat, _ = ref.accumulate(case["terms"], len(case["rays"]) * SAMPLES, cases.table("THREE", False))
    assert ((flat != 0).any(axis=2) == (acc.reshape(-1, 3, 3, 3) != 0).any(axis=(2, 3))).all()


# ---- 3. the mix --------------------------------------------------------------------------------------------------------------------------------------------

def test_the_mix_restated_twice_and_on_the_host():
    rng = np.random.default_rng(5)
    for n_passes in (1, 3, 9, 24):
        passes = np.zeros((33, n_passes), binding.LightPass)
        passes["value"] = (rng.normal(size=(33, n_passes, 3)) * rng.uniform(1e-3, 1e3, (33, 1, 1))).astype(F)
        total = np.zeros(33, binding.RadianceResult)
        total["value"] = rng.uniform(0, 1, (33, 4)).astype(F)
        gains = rng.uniform(-2, 2, (n_passes, 3)).astype(F)
        gains[0, 0] = 0.0
        if n_passes > 1:
            gains[1] = (np.inf, np.nan, -0.0)  # any gain is taken as given
        for t in (None, total):
            a, b, c = ref.mix(passes, gains, t), ref.mix_naive(passes, gains, t), binding.mix_light_passes(passes, gains, t)
            assert same_bits(a, b).all() and same_bits(a, c).all(), n_passes
            assert (a[:, 3] == (0.0 if t is None else total["value"][:, 3])).all()
    # the products are rounded before they are added: a fused multiply-add would keep 2^-24 here
    passes = np.zeros((1, 2), binding.LightPass)
    passes["value"][0, :, 0] = (1.0 + 2.0 ** -12, -1.0)
    gains = np.array([[1.0 + 2.0 ** -12, 0, 0], [1.0 + 2.0 ** -11, 0, 0]], F)
    want = F(F(F(1.0 + 2.0 ** -12) * F(1.0 + 2.0 ** -12)) - F(1.0 + 2.0 ** -11))
    assert want == 0.0 and binding.mix_light_passes(passes, gains)[0, 0] == want == ref.mix(passes, gains)[0, 0]
    # shapes: a capture's passes
    image = np.zeros((3, 5, 4), binding.LightPass)
    image["value"] = rng.uniform(0, 1, (3, 5, 4, 3)).astype(F)
    assert same_bits(binding.mix_light_passes(image, np.ones((4, 3), F)), ref.mix(image, np.ones((4, 3), F))).all()


# ---- 4. the sum of the passes against the total -------------------------------------------------------------------------------------------------

def test_the_sum_of_the_passes_stays_near_the_total(case):
    """The passes of a ray do not add up to its total bit for bit, but nearly.  All terms are non-negative here, so a channel of the total
    and the sum of that channel over the passes are sums of the SAME non-negative numbers in different orders, each divided by `samples`.
    A term passes through at most T additions in its sample's accumulator (T: the most non-zero terms of any one sample, which the
    yardstick reports; adding zeros rounds nothing), ceil(samples / 64) additions in its lane's strided partial, 64 additions in lane
    order and one division: k = T + ceil(samples / 64) + 65 roundings of relative size U = 2^-24 at the most, in either sum.  Each sum
    is therefore within (1 + U)^k - 1 <= 1.01 k U of the exact one, relative to it (non-negative terms: no cancellation), and the two
    differ by at most 1.01 * (T + ceil(samples / 64) + 65) * 2^-23 times the exact sum.  The passes are added here in float64, which
    adds nothing worth counting (P - 1 roundings of 2^-53)."""
    n = len(case["rays"])
    for lanes, _, _, term in case["terms"]:
        assert (term[:, :3] >= 0).all()
    total = radiance_ref.records(case["L"], case["missed"])["value"][:, :3].astype(D)
    for name, split in cases.TABLES:
        acc, count = ref.accumulate(case["terms"], n * SAMPLES, cases.table(name, split))
        summed = ref.pass_records(acc, SAMPLES)["value"].astype(D).sum(axis=1)
        T = int(count.max())
        bound = ref.sum_bound(T, SAMPLES)
        worst = (np.abs(summed - total) / np.where(total > 0, total, 1.0)).max()
        print("%s split %d: T = %d, worst relative difference %.3g, bound %.3g" % (name, split, T, worst, bound))
        assert (np.abs(summed - total) <= bound * total).all()
    # (the strided sum itself, at more than one round per lane)
    rng = np.random.default_rng(3)
    acc = rng.uniform(0, 4, (5 * 130, 9, 3)).astype(F)
    exact = acc.astype(D).reshape(5, 130, 9, 3).sum(axis=(1, 2)) / 130
    got = ref.pass_records(acc, 130)["value"].astype(D).sum(axis=1)
    assert (np.abs(got - exact) <= ref.sum_bound(0, 130) * exact).all()
