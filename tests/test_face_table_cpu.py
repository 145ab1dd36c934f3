"""pt_face_table_kernel (pt_motion_shapes_kernels.h; include/pt_motion_shapes.h) behind the batched assembler, both
compiled for the host (tests/hip/face_table_probe.hip, built the way tests/pose_probe.py builds pose_probe.hip): under limits small enough
for three chunks, triangle t's nine coordinates are the transformed corners of face face_of[t], bit for bit.  This is the only place the
table is made over more than one chunk: no scene of test size reaches the product's limits on a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import build as product
from tests import motion_shapes_cases as cases
from tests import motion_shapes_ref as msr
from tests.pose_probe import ProbeInstance, ProbeMesh
from tests.util import assert_bits_equal

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("face_table") / "libface_table_probe.so")
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host_pose"), "-I", product.CSRC, "-x", "c++",
                    os.path.join(HERE, "hip", "face_table_probe.hip"), "-o", lib], check=True)
    return C.CDLL(lib)


def _run(probe, meshes, instances, limits):
    keep = [(np.ascontiguousarray(v, F).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)) for v, f in meshes]
    md = (ProbeMesh * len(keep))(*[ProbeMesh(len(v), v.ctypes.data, len(f), f.ctypes.data) for v, f in keep])
    inst = (ProbeInstance * len(instances))()
    for i, (mesh, matrix, smooth) in enumerate(instances):
        inst[i].mesh = mesh
        inst[i].transform[:] = [float(x) for x in np.asarray(matrix, F).reshape(16)]
        inst[i].smooth = int(smooth)
    room = sum(len(keep[mesh][1]) for mesh, _, _ in instances)
    pos, nrm = np.zeros((room, 9), F), np.zeros((room, 9), F)
    face_of = np.full(room, 0xA5A5A5A5, np.uint32)
    counts = np.zeros(len(instances), np.uint32)
    kept, chunks = C.c_uint64(), C.c_uint32()
    rc = probe.face_table_probe(md, inst, C.c_uint32(len(instances)), C.c_uint64(limits[0]), C.c_uint64(limits[1]), C.c_uint64(limits[2]), C.c_uint64(room),
                                C.c_void_p(pos.ctypes.data), C.c_void_p(nrm.ctypes.data), C.c_void_p(face_of.ctypes.data), C.c_void_p(counts.ctypes.data), C.byref(kept),
                                C.byref(chunks))
    assert rc == 0, rc
    return pos, face_of, counts, kept.value, chunks.value


@pytest.mark.parametrize("limits, chunks", [((0, 0, 0), 1), ((0, 90, 0), 3), ((62, 0, 0), 3)])
def test_face_of_names_the_face_of_every_triangle(probe, limits, chunks):
    patch, flat8 = cases.patch(), (cases.flat8_revived(), cases.flat8()[1])
    collapse = np.diag(np.array([0, 0, 0, 1], F))
    meshes = [patch, flat8]
    # flat8 first (its spliced degenerate face shifts the ranks), an instance without survivors between two that have, the patch twice
    instances = [(1, cases.place(0.0, -0.4, 0.3, 0.7), False), (0, cases.place(-0.4, 0.3, 0.45, 0.7), True), (1, collapse, False),
                 (0, cases.place(0.4, 0.3, 0.5, 0.7, degrees=15.0), True), (1, cases.place(0.2, 0.1, 0.6, 0.5), True)]
    pos, face_of, counts, kept, n_chunks = _run(probe, meshes, instances, limits)
    assert n_chunks == chunks, n_chunks
    want, face_first, want_counts = msr.face_table([(m, meshes[k][0], meshes[k][1]) for k, m, _ in instances])
    assert counts.tolist() == want_counts == [9, 72, 0, 72, 9] and kept == 162
    assert (face_of[:kept] == want).all() and (face_of[kept:] == 0xA5A5A5A5).all()  # (nothing is written for a rejected face)
    at = 0
    for i, (k, m, _) in enumerate(instances):
        v, f = meshes[k]
        local = face_of[at:at + counts[i]].astype(np.int64) - face_first[i]
        assert_bits_equal(pos[at:at + counts[i]].reshape(-1, 3, 3), msr.transform(m, v)[f[local]], "instance %d under limits %s" % (i, limits))
        at += counts[i]
    assert not (face_of[:9] == np.arange(9)).all()
