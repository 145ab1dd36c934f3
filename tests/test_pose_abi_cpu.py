"""The pose entry points of the C ABI (include/pt_pose.h) without a GPU: exported, declared, and every refusal that needs no scene
answered before a device is looked for; with the arguments in order and no device, PT_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np

from cpupathtrace_amd import binding, build, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_OK, PT_ERR_INVALID, PT_ERR_NO_DEVICE, PT_ERR_UNSUPPORTED = 0, 1, 2, 4
PT_MESH_MAX_FACES = 0x7FFFFFFF // 3
F = np.float32


def test_symbols_are_exported_and_declared():
    build.build()
    lib = C.CDLL(binding.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_pose.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(binding.POSE_EXPORTS) == {"pt_scene_pose", "pt_scene_get_pose", "pt_mesh_assemble_batch"}
    assert not declared & set(binding.EXPORTS) and not declared & set(binding.MESH_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    top = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert top.index('#include "pt_mesh.h"') < top.index('#include "pt_pose.h"')
    assert re.search(r"typedef struct pt_pose_info \{", header)
    fields = re.search(r"typedef struct pt_pose_info \{(.*?)\} pt_pose_info;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in binding.PoseInfo._fields_]
    assert C.sizeof(binding.PoseInfo) == 36


def _batch(lib, meshes, n_meshes, instances, n_instances, capacity, pos, nrm, n):
    return lib.pt_mesh_assemble_batch(C.c_int(0), meshes, C.c_uint32(n_meshes), instances, C.c_uint32(n_instances), C.c_uint64(capacity), binding._ptr(pos), binding._ptr(nrm),
                                      None, C.byref(n) if n is not None else None)


def test_refusals_come_before_any_device():
    lib = binding.load()
    v, f = scenes.bumpy_sphere_vertices(8, 4)
    md, arrays = binding._mesh_data(v, f)
    meshes = (binding.MeshData * 1)(md)
    ok = binding._mesh_instance(0, None, True)
    two = (binding.MeshInstance * 2)(ok, ok)
    n = C.c_uint64()
    pos, nrm = np.zeros((2 * len(f), 9), F), np.zeros((2 * len(f), 9), F)
    cap = 2 * len(f)
    # null arguments
    assert _batch(lib, meshes, 1, two, 2, cap, pos, nrm, None) == PT_ERR_INVALID
    assert _batch(lib, None, 1, two, 2, cap, pos, nrm, n) == PT_ERR_INVALID
    assert _batch(lib, meshes, 1, None, 2, cap, pos, nrm, n) == PT_ERR_INVALID
    # capacity > 0 with null outputs (capacity 0 needs none: that is the next test's, or a device's)
    assert _batch(lib, meshes, 1, two, 2, cap, None, nrm, n) == PT_ERR_INVALID
    assert _batch(lib, meshes, 1, two, 2, cap, pos, None, n) == PT_ERR_INVALID
    # a mesh index >= n_meshes
    assert _batch(lib, meshes, 1, (binding.MeshInstance * 2)(ok, binding._mesh_instance(1)), 2, cap, pos, nrm, n) == PT_ERR_INVALID
    assert b"mesh" in lib.pt_last_error()
    # a missing array
    assert _batch(lib, (binding.MeshData * 1)(binding.MeshData(len(v), None, len(f), md.faces)), 1, two, 2, cap, pos, nrm, n) == PT_ERR_INVALID
    assert _batch(lib, (binding.MeshData * 1)(binding.MeshData(len(v), md.vertices, len(f), None)), 1, two, 2, cap, pos, nrm, n) == PT_ERR_INVALID
    # more than PT_MESH_MAX_FACES faces in one mesh; more faces over all instances than references can name
    assert _batch(lib, (binding.MeshData * 1)(binding.MeshData(len(v), md.vertices, PT_MESH_MAX_FACES + 1, md.faces)), 1, two, 1, cap, pos, nrm, n) == PT_ERR_UNSUPPORTED
    assert _batch(lib, (binding.MeshData * 1)(binding.MeshData(len(v), md.vertices, 1 << 29, md.faces)), 1, two, 2, cap, pos, nrm, n) == PT_ERR_UNSUPPORTED
    # an unused mesh is not looked at
    unused = (binding.MeshData * 2)(md, binding.MeshData(5, None, PT_MESH_MAX_FACES + 1, None))
    assert _batch(lib, unused, 2, two, 2, cap, pos, nrm, n) in (PT_OK, PT_ERR_NO_DEVICE)
    # pt_scene_pose and pt_scene_get_pose without a scene
    m = np.eye(4, dtype=F).reshape(1, 16)
    info = binding.PoseInfo()
    assert lib.pt_scene_pose(None, None, C.c_uint32(1), binding._ptr(m), C.byref(info)) == PT_ERR_INVALID
    assert lib.pt_scene_pose(None, None, C.c_uint32(0), None, None) == PT_ERR_INVALID
    assert lib.pt_scene_get_pose(None, binding._ptr(m)) == PT_ERR_INVALID
    assert (pos == 0).all() and (nrm == 0).all() and n.value == 0
    del arrays


def test_without_a_device_there_is_no_assembly():
    """With every argument in order the answer depends on the machine: PT_ERR_NO_DEVICE without a GPU, the triangles with one."""
    lib = binding.load()
    v, f = scenes.bumpy_sphere_vertices(8, 4)
    md, arrays = binding._mesh_data(v, f)
    two = (binding.MeshInstance * 2)(binding._mesh_instance(0, None, True), binding._mesh_instance(0, None, False))
    n = C.c_uint64()
    pos, nrm = np.zeros((2 * len(f), 9), F), np.zeros((2 * len(f), 9), F)
    rc = _batch(lib, (binding.MeshData * 1)(md), 1, two, 2, 2 * len(f), pos, nrm, n)
    rc0 = _batch(lib, (binding.MeshData * 1)(md), 1, two, 2, 0, None, None, n)  # capacity 0: the count alone
    if binding.device_count() > 0:
        assert (rc, rc0) == (PT_OK, PT_OK) and n.value == 2 * len(f)
    else:
        assert (rc, rc0) == (PT_ERR_NO_DEVICE, PT_ERR_NO_DEVICE) and n.value == 0
        try:
            binding.mesh_assemble_batch([(v, f)], [(0, None, 1)])
            raise AssertionError("no error without a device")
        except binding.PtError as e:
            assert e.code == PT_ERR_NO_DEVICE
    del arrays
