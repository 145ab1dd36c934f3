"""Scene queries without a GPU (include/pt_query.h): the header's place in the ABI, the refusals that need no device, the
numpy restatement of the record (tests/query_ref.py) pinned against the oracle, and the product's own record function -- query_record of
pt_query_kernels.h, compiled for the host (tests/hip/query_probe.hip) -- against that restatement, bit for bit, on the oracle's hits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cpupathtrace_amd import binding, build
from tests import pose_probe, query_cases as cases, query_probe, query_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_query_exports_and_declarations():
    header = open(os.path.join(ROOT, "include", "pt_query.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\(", header, re.M))
    assert declared == set(binding.QUERY_EXPORTS) and len(binding.QUERY_EXPORTS) == 8
    others = [name for name in dir(binding) if name.endswith("EXPORTS") and name != "QUERY_EXPORTS"]
    assert "EXPORTS" in others and len(others) >= 15
    for name in others:
        assert not set(getattr(binding, name)) & declared, name
    # no other header declares them, and pt_hip.h takes the header in at its end, behind every other one
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h") and other != "pt_query.h":
            assert not re.findall(r"\b(pt_query_[a-z_]+|pt_occluded_[a-z_]+)\s*\(", open(os.path.join(ROOT, "include", other)).read()), other
    top = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert max(m.start() for m in re.finditer(r'#include "', top)) == top.index('#include "pt_query.h"')
    assert binding.Hit.itemsize == 64 and [binding.Hit.fields[n][1] for n in ("t", "position", "normal", "geometric_normal", "b2")] == [0, 16, 32, 48, 60]
    assert "pt_query.cpp" in build.SOURCES and "pt_query_kernels.h" in build.HEADERS
    lib = C.CDLL(build.build())
    for name in binding.QUERY_EXPORTS:
        assert hasattr(lib, name), name


def test_refusals_that_need_no_device():
    lib = binding.load()
    rays, hits, flags, xy = np.zeros((2, 7), F), np.zeros(2, binding.Hit), np.zeros(2, np.uint8), np.zeros((2, 2), np.int32)
    cam, opt = binding._camera(cases.CAMERA), binding._options(cases.OPTIONS)
    p = binding._ptr
    calls = [lambda: lib.pt_query_rays(None, p(rays), C.c_size_t(2), p(hits)), lambda: lib.pt_query_rays_device(None, p(rays), C.c_size_t(2), p(hits), None),
             lambda: lib.pt_occluded_rays(None, p(rays), C.c_size_t(2), p(flags)), lambda: lib.pt_occluded_rays_device(None, p(rays), C.c_size_t(2), p(flags), None),
             lambda: lib.pt_query_pixels(None, C.byref(cam), C.byref(opt), p(xy), C.c_size_t(2), p(hits)),
             lambda: lib.pt_query_pixels_device(None, C.byref(cam), C.byref(opt), p(xy), C.c_size_t(2), p(hits), None),
             lambda: lib.pt_query_frame(None, C.byref(cam), C.byref(opt), p(hits)), lambda: lib.pt_query_frame_device(None, C.byref(cam), C.byref(opt), p(hits), None),
             lambda: lib.pt_query_rays(None, None, C.c_size_t(0), None)]
    for call in calls:
        assert call() == 1 and b"null" in lib.pt_last_error()  # PT_ERR_INVALID


@pytest.fixture(scope="module")
def assembler(tmp_path_factory):
    return pose_probe.Probe(pose_probe.build_host(str(tmp_path_factory.mktemp("query_pose") / "libpose_probe.so")))


@pytest.fixture(scope="module", params=["S", "L"])
def case(request, oracle_lib, assembler):
    """A scene flattened for the oracle, its rays and the oracle's hits."""
    scene, instances, shapes = cases.build(request.param == "L")
    flat = cases.flatten(scene, instances, shapes, assembler)
    handle = oracle_lib.scene_create(flat["scene"])
    rays = cases.rays(flat)
    t, obj = handle.intersect(rays)
    yield dict(name=request.param, flat=flat, handle=handle, rays=rays, t=t, obj=obj)
    handle.close()


def test_inputs_meet_their_conditions(case, oracle_lib):
    flat = case["flat"]
    n_objects = len(flat["scene"]["obj_kind"])
    assert (n_objects < 1024) == (case["name"] == "S"), n_objects
    assert flat["count"][:3].tolist() == [72, 72, 35] and flat["n_faces"][:3] == [72, 72, 40]  # M2's instance lost its 5 degenerate faces
    assert not (flat["local_face"][144:179] == np.arange(35)).all()                              # ... so its triangles are not its faces
    hit = cases.check_conditions(flat, case["t"], case["obj"])
    assert not hit[40] and not hit[41]  # the NaN direction and the zero-length one
    if case["name"] == "L":
        # the slivers' run of overlapping boxes: deeper than the 8 entries of the stack's LDS window
        obj, _ = oracle_lib.bvh_dump(flat["scene"])
        depth, stack = 0, [1]
        for o in obj:
            d = stack.pop()
            depth = max(depth, d)
            if o < 0:
                stack += [d + 1, d + 1]
        assert depth > 10, depth
        sliver = (case["obj"] >= 5) & (case["obj"] < 5 + cases.N_SLIVERS)
        assert sliver.sum() >= 5, sliver.sum()
    # pixel rays hit as well: the frame is not empty
    t, obj = case["handle"].intersect(cases.pixel_rays(oracle_lib, cases.CAMERA, cases.FRAME_W, cases.FRAME_H, cases.frame_pixels(cases.FRAME_W, cases.FRAME_H)))
    assert ((obj >= 0).mean() >= 0.3) and len(np.unique(obj)) >= 20


def test_the_restatement_agrees_with_the_oracle(case):
    """(1 - b1 - b2) a + b1 b + b2 c reproduces the position to 1e-4 of the triangle's extent, the weights lie in [-1e-4, 1 + 1e-4], the
    geometric normal is a unit vector along the face normal, and the instance holds the object."""
    flat = case["flat"]
    want = query_ref.records(case["handle"], flat, case["rays"], with_table=True)
    hit = want["object"] >= 0
    assert (want["t"][~hit] == -1).all() and (want["face"][~hit] == query_ref.NO_FACE).all() and (want["position"][~hit] == 0).all()
    scene = flat["scene"]
    tri = (np.asarray(scene["obj_kind"])[want["object"]] == 0) & hit
    corners = np.asarray(scene["tri_pos"], np.float64).reshape(-1, 3, 3)[query_ref.triangle_of_object(scene)[want["object"][tri]]]
    b1, b2 = want["b1"][tri].astype(np.float64), want["b2"][tri].astype(np.float64)
    for b in (b1, b2, 1 - b1 - b2):
        assert (b >= -1e-4).all() and (b <= 1 + 1e-4).all(), (b.min(), b.max())
    again = (1 - b1 - b2)[:, None] * corners[:, 0] + b1[:, None] * corners[:, 1] + b2[:, None] * corners[:, 2]
    extent = (corners.max(axis=1) - corners.min(axis=1)).max(axis=1)
    assert (np.abs(again - want["position"][tri]).max(axis=1) <= 1e-4 * extent).all()
    g = want["geometric_normal"][tri].astype(np.float64)
    face = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    assert np.allclose(np.linalg.norm(g, axis=1), 1, atol=1e-5) and np.allclose(g, face / np.linalg.norm(face, axis=1, keepdims=True), atol=1e-4)
    assert (want["b1"][hit & ~tri] == 0).all() and (want["geometric_normal"][hit & ~tri] == want["normal"][hit & ~tri]).all()
    # both face rules agree where both apply (M1), and M2's faces come from the table alone
    plain = query_ref.records(case["handle"], flat, case["rays"], with_table=False)
    for i in (0, 1):
        sel = want["instance"] == i
        assert sel.any() and (want["face"][sel] == plain["face"][sel]).all() and (want["face"][sel] == flat["local_face"][want["object"][sel] - flat["n_desc"]]).all()
    sel = want["instance"] == 2
    assert sel.any() and (plain["face"][sel] == query_ref.NO_FACE).all() and (want["face"][sel] < 40).all()
    assert (want["instance"][hit & (want["object"] < flat["n_desc"])] == -1).all()


@pytest.fixture(scope="module")
def record_probe(tmp_path_factory):
    return query_probe.Probe(query_probe.build_host(str(tmp_path_factory.mktemp("query") / "libquery_probe.so")))


@pytest.mark.parametrize("with_table", [False, True])
def test_the_record_function_equals_the_restatement(case, record_probe, oracle_lib, with_table):
    """query_record, compiled for the host, on the oracle's hits of every ray and of every pixel of the frame: tests/query_ref.py's
    records bit for bit."""
    flat, handle = case["flat"], case["handle"]
    got = record_probe.records(flat, case["rays"], case["t"], case["obj"], with_table)
    query_ref.assert_records_equal(got, query_ref.records_of_hits(handle, flat, case["rays"], case["t"], case["obj"], with_table), "rays of %s" % case["name"])
    px = cases.pixel_rays(oracle_lib, cases.CAMERA, cases.FRAME_W, cases.FRAME_H, cases.frame_pixels(cases.FRAME_W, cases.FRAME_H))
    t, obj = handle.intersect(px)
    query_ref.assert_records_equal(record_probe.records(flat, px, t, obj, with_table), query_ref.records_of_hits(handle, flat, px, t, obj, with_table), "pixels of %s" % case["name"])
