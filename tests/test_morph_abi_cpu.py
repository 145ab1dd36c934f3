"""The blend-shape entry points of the C ABI (include/pt_morph.h) without a GPU: declared there and nowhere else, exported, laid out as
the binding says, and every refusal that needs no scene answered before a device is looked for.  A scene needs a device, so the refusals
that compare with the scene's counts are made here with a null scene -- PT_ERR_INVALID whatever the machine -- and against a live scene
in tests/test_gpu_morph.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from cpupathtrace_amd import binding, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1
F = np.float32
STRUCTS = (("pt_morph_target", "MorphTarget"), ("pt_morph_set", "MorphSet"), ("pt_mesh_morph", "MeshMorph"), ("pt_morph_info", "MorphInfo"))
NAMES = {"pt_scene_bind_morphs", "pt_scene_morph", "pt_scene_get_morphs"}


def test_symbols_are_exported_and_declared_in_their_own_header():
    build.build()
    lib = C.CDLL(binding.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_morph.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(binding.MORPH_EXPORTS) == NAMES
    for other in (binding.EXPORTS, binding.NOISE_EXPORTS, binding.VARIANCE_EXPORTS, binding.FEATURES_EXPORTS, binding.MESH_EXPORTS, binding.POSE_EXPORTS,
                  binding.MOTION_EXPORTS, binding.RELIGHT_EXPORTS, binding.DEFORM_EXPORTS):
        assert not declared & set(other)
    for name in declared:
        assert hasattr(lib, name), name
    # no other header declares them, and pt_hip.h takes the header in behind pt_deform.h
    pattern = "|".join(r"%s\s*\(" % name for name in sorted(NAMES))
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.endswith(".h") and other != "pt_morph.h":
            assert not re.findall(pattern, open(os.path.join(ROOT, "include", other)).read()), other
    top = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert top.index('#include "pt_pose.h"') < top.index('#include "pt_deform.h"') < top.index('#include "pt_morph.h"')
    for struct, ctype in STRUCTS:
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s+", "", decl.strip()).split(",")]
        assert names == [n for n, _ in getattr(binding, ctype)._fields_], (struct, names)
    # what the arithmetic does with zero weights and signed zeros, and what stays out of scope, is said where a user reads it
    prose = re.sub(r"\s+", " ", header.replace("\n *", " "))
    assert "NO LISTED TARGET IS SKIPPED" in prose and "-0.0 becomes +0.0" in prose and "0 * inf and 0 * NaN are NaN" in prose
    assert "OUT OF SCOPE: motion vectors of a morphed mesh" in prose and "EVERY VERTEX INDEX INCLUDED" in prose


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
    # the morph's report begins with the deform's fields
    assert binding.MorphInfo._fields_[:len(binding.DeformInfo._fields_)] == binding.DeformInfo._fields_
    assert C.sizeof(binding.DeformInfo) == 56 and C.sizeof(binding.MorphInfo) == 72


def _set(targets, mesh=0, n_targets=None):
    table = (binding.MorphTarget * max(len(targets), 1))(*targets)
    s = binding.MorphSet(mesh, len(targets) if n_targets is None else n_targets, C.addressof(table) if targets else None)
    return s, table


def _morph(lib, entries, n_entries=None, instances=None, n=0, transforms=None, info=None, scene=None):
    table = (binding.MeshMorph * max(len(entries), 1))(*entries) if entries is not None else None
    return lib.pt_scene_morph(scene, table, C.c_uint32(len(entries) if n_entries is None else n_entries), binding._ptr(instances), C.c_uint32(n),
                              binding._ptr(transforms), C.byref(info) if info is not None else None)


def test_refusals_come_before_any_device():
    lib = binding.load()
    err = lambda: lib.pt_last_error().decode()
    idx, bad_idx, same_idx = np.array([0, 2, 3], np.uint32), np.array([0, 3, 2], np.uint32), np.array([1, 1], np.uint32)
    d = np.ones((4, 3), F)
    # ---- pt_scene_bind_morphs: nulls, the lists' own faults, then the scene
    assert lib.pt_scene_bind_morphs(None, None) == PT_ERR_INVALID and "null morph set" in err()
    s, keep = _set([binding.MorphTarget(3, idx.ctypes.data, None)])
    assert lib.pt_scene_bind_morphs(None, C.byref(s)) == PT_ERR_INVALID and "null deltas in target 0" in err()
    s, keep = _set([binding.MorphTarget(3, idx.ctypes.data, d.ctypes.data), binding.MorphTarget(3, bad_idx.ctypes.data, d.ctypes.data)])
    assert lib.pt_scene_bind_morphs(None, C.byref(s)) == PT_ERR_INVALID and "target 1 are not strictly ascending" in err()
    s, keep = _set([binding.MorphTarget(2, same_idx.ctypes.data, d.ctypes.data)])
    assert lib.pt_scene_bind_morphs(None, C.byref(s)) == PT_ERR_INVALID and "not strictly ascending" in err()  # (a vertex listed twice by one target)
    for targets in ([binding.MorphTarget(3, idx.ctypes.data, d.ctypes.data)], [binding.MorphTarget(4, None, d.ctypes.data)], [binding.MorphTarget(0, None, None)], []):
        s, keep = _set(targets)  # sparse, dense, empty, and an unbind: the scene's to judge
        assert lib.pt_scene_bind_morphs(None, C.byref(s)) == PT_ERR_INVALID and "null scene" in err()
    s = binding.MorphSet(0, 3, None)  # (null targets unbind, whatever the count)
    assert lib.pt_scene_bind_morphs(None, C.byref(s)) == PT_ERR_INVALID and "null scene" in err()

    # ---- pt_scene_morph
    w, m = np.zeros(2, F), np.zeros((2, 12), F)
    eye = np.eye(4, dtype=F).reshape(1, 16)
    info = binding.MorphInfo()
    info.n_instances = info.allocations = info.n_vertices_morphed = 7
    info.n_entries_read = 7
    ok = binding.MeshMorph(0, w.ctypes.data, 2, None, 0)
    assert _morph(lib, [ok], info=info) == PT_ERR_INVALID and "null scene" in err()
    assert (info.n_instances, info.allocations, info.n_vertices_morphed, info.n_entries_read) == (0, 0, 0, 0)  # (the info is cleared whatever happens)
    assert _morph(lib, None, n_entries=1) == PT_ERR_INVALID and "null morphs" in err()
    assert _morph(lib, [ok, binding.MeshMorph(0, None, 2, None, 0)]) == PT_ERR_INVALID and "null weights in morph 1" in err()
    assert _morph(lib, [binding.MeshMorph(0, None, 0, m.ctypes.data, 2)]) == PT_ERR_INVALID and "null weights" in err()
    assert _morph(lib, [ok], n=1, transforms=None) == PT_ERR_INVALID and "null transforms" in err()
    assert _morph(lib, [], n=1, transforms=eye) == PT_ERR_INVALID and "null scene" in err()
    # count mismatches are the scene's to find: without one the answer is the null scene's
    assert _morph(lib, [binding.MeshMorph(0, w.ctypes.data, 5, m.ctypes.data, 3)]) == PT_ERR_INVALID and "null scene" in err()
    assert _morph(lib, [], n=0) == PT_ERR_INVALID and "null scene" in err()

    # ---- pt_scene_get_morphs
    n_targets, n_entries = C.c_uint32(5), C.c_uint64(6)
    assert lib.pt_scene_get_morphs(None, C.c_uint32(0), C.byref(n_targets), C.byref(n_entries)) == PT_ERR_INVALID and "null scene" in err()
    assert (n_targets.value, n_entries.value) == (5, 6)
