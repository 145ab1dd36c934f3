"""The mesh entry points of the C ABI (include/pt_mesh.h) without a GPU: exported, declared, and every refusal answered before a device
is looked for; with the arguments in order and no device, PT_ERR_NO_DEVICE."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID, PT_ERR_NO_DEVICE, PT_ERR_UNSUPPORTED = 1, 2, 4
F = np.float32


def test_symbols_are_exported_and_declared():
    build.build()
    lib = C.CDLL(binding.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_mesh.h")).read()
    declared = set(re.findall(r"\b(pt_[a-z_0-9]+)\s*\(", header))
    assert declared == set(binding.MESH_EXPORTS) and len(declared) == 4
    assert not declared & set(binding.EXPORTS)  # (EXPORTS is what pt_hip.h itself declares)
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "pt_mesh.h"' in open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    for struct in ("pt_mesh_data", "pt_mesh_instance"):
        assert re.search(r"typedef struct %s \{" % struct, header)


def _desc(sc, keep):
    keep.update({k: np.ascontiguousarray(v) for k, v in sc.items() if isinstance(v, np.ndarray)})
    d = binding.SceneDesc()
    d.n_objects, d.obj_kind = len(keep["obj_kind"]), binding._ptr(keep["obj_kind"])
    d.n_triangles, d.tri_pos, d.tri_nrm = len(keep["tri_pos"]), binding._ptr(keep["tri_pos"]), binding._ptr(keep["tri_nrm"])
    d.tri_cull, d.tri_material = binding._ptr(keep["tri_cull"]), binding._ptr(keep["tri_material"])
    d.n_spheres, d.sph, d.sph_material = len(keep["sph"]), binding._ptr(keep["sph"]), binding._ptr(keep["sph_material"])
    d.n_materials, d.materials = len(keep["materials"]), binding._ptr(keep["materials"])
    d.n_point_lights, d.light_pos, d.light_spectrum = len(keep["light_pos"]), binding._ptr(keep["light_pos"]), binding._ptr(keep["light_spectrum"])
    return d


def _create(lib, d, meshes, n_meshes, instances, n_instances, out=True):
    h = C.c_void_p()
    rc = lib.pt_scene_create_meshes(C.c_int(0), C.byref(d) if d is not None else None, meshes, C.c_uint32(n_meshes), instances, C.c_uint32(n_instances),
                                    C.byref(h) if out else None)
    assert h.value is None or rc == 0
    if h.value is not None:
        lib.pt_scene_destroy(h)
    return rc


def test_refusals_come_before_any_device():
    lib = binding.load()
    keep = {}
    d = _desc(scenes.box_scene()[0], keep)  # 14 triangles, 1 material
    v, f = scenes.bumpy_sphere_vertices(8, 4)
    md, arrays = binding._mesh_data(v, f)
    meshes = (binding.MeshData * 1)(md)
    ok = binding._mesh_instance(0, None, True, True, 0)
    one = (binding.MeshInstance * 1)(ok)
    # null arrays
    assert _create(lib, None, meshes, 1, one, 1) == PT_ERR_INVALID
    assert _create(lib, d, meshes, 1, one, 1, out=False) == PT_ERR_INVALID
    assert _create(lib, d, None, 1, one, 1) == PT_ERR_INVALID
    assert _create(lib, d, meshes, 1, None, 1) == PT_ERR_INVALID
    assert _create(lib, d, (binding.MeshData * 1)(binding.MeshData(len(v), None, len(f), md.faces)), 1, one, 1) == PT_ERR_INVALID
    assert _create(lib, d, (binding.MeshData * 1)(binding.MeshData(len(v), md.vertices, len(f), None)), 1, one, 1) == PT_ERR_INVALID
    # a mesh index >= n_meshes; a material >= n_materials that is not PT_NO_MATERIAL
    assert _create(lib, d, meshes, 1, (binding.MeshInstance * 1)(binding._mesh_instance(1)), 1) == PT_ERR_INVALID
    assert _create(lib, d, meshes, 1, (binding.MeshInstance * 1)(binding._mesh_instance(0, material=1)), 1) == PT_ERR_INVALID
    assert b"material" in lib.pt_last_error()
    # more triangles than references can name, counted before any face is rejected: 3 instances of 2^29 faces + the box's 14
    huge = (binding.MeshData * 1)(binding.MeshData(len(v), md.vertices, 1 << 29, md.faces))
    two = (binding.MeshInstance * 2)(ok, ok)
    assert _create(lib, d, huge, 1, two, 2) == PT_ERR_UNSUPPORTED  # 2^30 + 14 > 2^30 - 1
    # pt_mesh_assemble
    n = C.c_uint64()
    pos = np.zeros((len(f), 9), F)
    assert lib.pt_mesh_assemble(C.c_int(0), None, C.byref(ok), C.c_uint64(len(f)), binding._ptr(pos), binding._ptr(pos), C.byref(n)) == PT_ERR_INVALID
    assert lib.pt_mesh_assemble(C.c_int(0), C.byref(md), None, C.c_uint64(len(f)), binding._ptr(pos), binding._ptr(pos), C.byref(n)) == PT_ERR_INVALID
    assert lib.pt_mesh_assemble(C.c_int(0), C.byref(md), C.byref(ok), C.c_uint64(len(f)), None, binding._ptr(pos), C.byref(n)) == PT_ERR_INVALID
    assert lib.pt_mesh_assemble(C.c_int(0), C.byref(md), C.byref(ok), C.c_uint64(len(f)), binding._ptr(pos), binding._ptr(pos), None) == PT_ERR_INVALID
    # the two queries
    assert lib.pt_scene_instance_ranges(None, None, None) == PT_ERR_INVALID
    assert lib.pt_scene_get_triangles(None, C.c_uint32(0), C.c_uint32(0), None, None, None, None) == PT_ERR_INVALID
    del arrays


def test_without_a_device_there_is_no_scene():
    if binding.device_count() > 0:
        pytest.skip("a GPU is present")
    lib = binding.load()
    keep = {}
    d = _desc(scenes.box_scene()[0], keep)
    v, f = scenes.bumpy_sphere_vertices(8, 4)
    md, arrays = binding._mesh_data(v, f)
    one = (binding.MeshInstance * 1)(binding._mesh_instance(0, None, True, True, 0))
    assert _create(lib, d, (binding.MeshData * 1)(md), 1, one, 1) == PT_ERR_NO_DEVICE
    assert _create(lib, d, None, 0, None, 0) == PT_ERR_NO_DEVICE  # no instances: the call is pt_scene_create
    n = C.c_uint64()
    pos = np.zeros((len(f), 9), F)
    assert lib.pt_mesh_assemble(C.c_int(0), C.byref(md), C.byref(one[0]), C.c_uint64(len(f)), binding._ptr(pos), binding._ptr(pos), C.byref(n)) == PT_ERR_NO_DEVICE
    sb = scenes.SceneBuilder()
    sb.mesh(v, f)
    with pytest.raises(binding.PtError) as e:
        binding.Scene(sb.build())
    assert e.value.code == PT_ERR_NO_DEVICE
    del arrays
