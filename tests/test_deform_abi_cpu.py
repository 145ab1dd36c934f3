"""The deform entry points of the C ABI (include/pt_deform.h) without a GPU: declared there and nowhere else, exported, laid out as the
binding says, and every refusal that needs no device answered before a device is looked for.  A scene needs a device, so the refusals
that compare a count with the scene's (a bone index equal to n_bones, a wrong vertex or bone count) are made here with a null scene --
PT_ERR_INVALID whatever the machine -- and against a live scene in tests/test_gpu_deform.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from cpupathtrace_amd import binding, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
F = np.float32
STRUCTS = (("pt_skin", "Skin"), ("pt_mesh_deform", "MeshDeform"), ("pt_deform_info", "DeformInfo"))


def test_symbols_are_exported_and_declared_in_their_own_header():
    build.build()
    lib = C.CDLL(binding.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_deform.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(binding.DEFORM_EXPORTS) == {"pt_scene_bind_skin", "pt_scene_deform", "pt_scene_get_mesh_vertices"}
    for other in (binding.EXPORTS, binding.NOISE_EXPORTS, binding.VARIANCE_EXPORTS, binding.FEATURES_EXPORTS, binding.MESH_EXPORTS, binding.POSE_EXPORTS,
                  binding.MOTION_EXPORTS, binding.RELIGHT_EXPORTS):
        assert not declared & set(other)
    for name in declared:
        assert hasattr(lib, name), name
    # no other header declares them, and pt_hip.h takes the header in behind pt_pose.h
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h") and other != "pt_deform.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert not re.findall(r"pt_scene_bind_skin\s*\(|pt_scene_deform\s*\(|pt_scene_get_mesh_vertices\s*\(", text), other
    top = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert top.index('#include "pt_mesh.h"') < top.index('#include "pt_pose.h"') < top.index('#include "pt_deform.h"')
    for struct, ctype in STRUCTS:
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s+", "", decl.strip()).split(",")]
        assert names == [n for n, _ in getattr(binding, ctype)._fields_], (struct, names)
    assert re.search(r"#define PT_SKIN_MAX_INFLUENCES 8\b", header) and binding.SKIN_MAX_INFLUENCES == 8
    for name, value in (("VERTICES", binding.DEFORM_VERTICES), ("BONES", binding.DEFORM_BONES), ("REST", binding.DEFORM_REST)):
        assert re.search(r"#define PT_DEFORM_%s %du\b" % (name, value), header), name
    # what stays out of scope is said where a user reads it
    prose = re.sub(r"\s+", " ", header.replace("\n *", " "))
    assert "OUT OF SCOPE: motion vectors of a deformed mesh" in prose and "pt_render_features_motion" in prose
    assert "ALL INSTANCES OF A MESH SHARE ITS DEFORMATION" in prose


def test_struct_layouts_match_a_compiled_c_program(tmp_path):
    import shutil
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler"
    lines = []
    for struct, ctype in STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (struct, struct))
        for name, _ in getattr(binding, ctype)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (struct, name, struct, name))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for struct, ctype in STRUCTS:
        ctype = getattr(binding, ctype)
        assert int(got[struct]) == C.sizeof(ctype), struct
        for name, _ in ctype._fields_:
            assert int(got["%s.%s" % (struct, name)]) == getattr(ctype, name).offset, (struct, name)
    # the pose's report keeps its pinned size; the deform's begins with the same fields
    assert C.sizeof(binding.PoseInfo) == 36 and C.sizeof(binding.DeformInfo) == 56
    assert binding.DeformInfo._fields_[:len(binding.PoseInfo._fields_)] == binding.PoseInfo._fields_


def _skin(mesh=0, n_bones=2, k=2, bone=None, weight=None):
    s = binding.Skin()
    s.mesh, s.n_bones, s.influences = mesh, n_bones, k
    s.bone = None if bone is None else bone.ctypes.data
    s.weight = None if weight is None else weight.ctypes.data
    return s


def _deform(lib, entries, n_entries=None, instances=None, n=0, transforms=None, info=None, scene=None):
    table = (binding.MeshDeform * max(len(entries), 1))(*entries) if entries is not None else None
    return lib.pt_scene_deform(scene, table, C.c_uint32(len(entries) if n_entries is None else n_entries), binding._ptr(instances), C.c_uint32(n),
                               binding._ptr(transforms), C.byref(info) if info is not None else None)


def test_refusals_come_before_any_device():
    lib = binding.load()
    err = lambda: lib.pt_last_error().decode()
    bone, weight = np.zeros((4, 2), np.uint32), np.ones((4, 2), F)
    # ---- pt_scene_bind_skin: nulls, K = 0 and 9, then the scene
    assert lib.pt_scene_bind_skin(None, None) == PT_ERR_INVALID and "null skin" in err()
    for k in (0, binding.SKIN_MAX_INFLUENCES + 1):
        s = _skin(k=k, bone=bone, weight=weight)
        assert lib.pt_scene_bind_skin(None, C.byref(s)) == PT_ERR_INVALID and "influences" in err(), k
    s = _skin(bone=bone, weight=None)
    assert lib.pt_scene_bind_skin(None, C.byref(s)) == PT_ERR_INVALID and "null weights" in err()
    for k in (1, binding.SKIN_MAX_INFLUENCES):
        s = _skin(k=k, bone=bone, weight=weight)
        assert lib.pt_scene_bind_skin(None, C.byref(s)) == PT_ERR_INVALID and "null scene" in err(), k
    bone[3, 1] = 2  # a bone index equal to n_bones
    s = _skin(n_bones=2, bone=bone, weight=weight)
    assert lib.pt_scene_bind_skin(None, C.byref(s)) == PT_ERR_INVALID
    s = _skin(n_bones=0)  # an unbind needs a scene too
    assert lib.pt_scene_bind_skin(None, C.byref(s)) == PT_ERR_INVALID and "null scene" in err()

    # ---- pt_scene_deform
    v, m = np.zeros((4, 3), F), np.zeros((2, 12), F)
    eye = np.eye(4, dtype=F).reshape(1, 16)
    info = binding.DeformInfo()
    info.n_instances = info.allocations = 7
    ok = binding.MeshDeform(0, binding.DEFORM_VERTICES, v.ctypes.data, 4)
    assert _deform(lib, [ok], info=info) == PT_ERR_INVALID and "null scene" in err()
    assert (info.n_instances, info.allocations) == (0, 0)  # (the info is cleared whatever happens)
    assert _deform(lib, None, n_entries=1) == PT_ERR_INVALID and "null deforms" in err()
    assert _deform(lib, [ok, binding.MeshDeform(0, 3, v.ctypes.data, 4)]) == PT_ERR_INVALID and "unknown kind 3 in deform 1" in err()
    assert _deform(lib, [binding.MeshDeform(0, 0xFFFFFFFF, None, 0)]) == PT_ERR_INVALID and "unknown kind" in err()
    assert _deform(lib, [binding.MeshDeform(0, binding.DEFORM_VERTICES, None, 4)]) == PT_ERR_INVALID and "null data" in err()
    assert _deform(lib, [binding.MeshDeform(0, binding.DEFORM_BONES, None, 2)]) == PT_ERR_INVALID and "null data" in err()
    assert _deform(lib, [binding.MeshDeform(0, binding.DEFORM_REST, None, 0)]) == PT_ERR_INVALID and "null scene" in err()  # (REST reads no data)
    assert _deform(lib, [ok], n=1, transforms=None) == PT_ERR_INVALID and "null transforms" in err()
    assert _deform(lib, [], n=1, transforms=eye) == PT_ERR_INVALID and "null scene" in err()
    # count mismatches are the scene's to find: without one the answer is the null scene's
    assert _deform(lib, [binding.MeshDeform(0, binding.DEFORM_VERTICES, v.ctypes.data, 5)]) == PT_ERR_INVALID
    assert _deform(lib, [binding.MeshDeform(0, binding.DEFORM_BONES, m.ctypes.data, 3)]) == PT_ERR_INVALID
    assert _deform(lib, [], n=0) == PT_ERR_INVALID and "null scene" in err()

    # ---- pt_scene_get_mesh_vertices
    n = C.c_uint32(5)
    assert lib.pt_scene_get_mesh_vertices(None, C.c_uint32(0), binding._ptr(v), C.byref(n)) == PT_ERR_INVALID and "null scene" in err()
    assert n.value == 5 and (v == 0).all()
