"""The relight entry points of the C ABI (include/pt_relight.h) without a GPU: declared, exported, laid out as the binding says, every
refusal that needs no scene -- and the condition under which the large case of tests/test_gpu_relight.py says anything, asserted on the
CPU oracle's leaf order."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cpupathtrace_amd import binding, build, build_host
from tests import relight_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID = 1


def test_symbols_are_exported_and_declared():
    build.build()
    lib = C.CDLL(binding.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pt_relight.h")).read()
    declared = set(re.findall(r"^int (pt_[a-z_0-9]+)\s*\(", header, re.M))
    assert declared == set(binding.RELIGHT_EXPORTS) == {"pt_scene_relight", "pt_scene_get_materials", "pt_scene_get_point_lights"}
    for other in (binding.EXPORTS, binding.NOISE_EXPORTS, binding.VARIANCE_EXPORTS, binding.FEATURES_EXPORTS, binding.MESH_EXPORTS, binding.POSE_EXPORTS,
                  binding.MOTION_EXPORTS):
        assert not declared & set(other)
    for name in declared:
        assert hasattr(lib, name), name
    top = open(os.path.join(ROOT, "include", "pt_hip.h")).read()
    assert top.index('#include "pt_motion.h"') < top.index('#include "pt_relight.h"')
    for struct, ctype in (("pt_relight", binding.Relight), ("pt_relight_info", binding.RelightInfo)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
        names = [n.strip(" *") for decl in fields.split(";") if decl.strip() for n in re.sub(r"^(const\s+)?\w+\s+", "", decl.strip()).split(",")]
        assert names == [n for n, _ in ctype._fields_], (struct, names)


def test_struct_layouts_match_a_compiled_c_program(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    lines = []
    for struct, ctype in (("pt_relight", binding.Relight), ("pt_relight_info", binding.RelightInfo)):
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (struct, struct))
        for name, _ in ctype._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (struct, name, struct, name))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pt_hip.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for struct, ctype in (("pt_relight", binding.Relight), ("pt_relight_info", binding.RelightInfo)):
        assert int(got[struct]) == C.sizeof(ctype), struct
        for name, _ in ctype._fields_:
            assert int(got["%s.%s" % (struct, name)]) == getattr(ctype, name).offset, (struct, name)
    assert C.sizeof(binding.RelightInfo) == 28


def test_null_arguments_are_refused_without_a_device():
    lib = binding.load()
    look, info = binding.Relight(), binding.RelightInfo()
    info.n_emissive = 7
    assert lib.pt_scene_relight(None, C.byref(look), C.byref(info)) == PT_ERR_INVALID
    assert info.n_emissive == 0  # (the info is cleared whatever happens)
    assert lib.pt_scene_relight(None, None, None) == PT_ERR_INVALID
    n = C.c_uint32(5)
    m = np.zeros(2, binding.MATERIAL_DTYPE)
    pos, spectrum = np.zeros((2, 3), np.float32), np.zeros((2, 4), np.float32)
    assert lib.pt_scene_get_materials(None, binding._ptr(m), C.c_uint32(2), C.byref(n)) == PT_ERR_INVALID
    assert lib.pt_scene_get_point_lights(None, binding._ptr(pos), binding._ptr(spectrum), C.c_uint32(2), C.byref(n)) == PT_ERR_INVALID
    assert b"null" in lib.pt_last_error() and n.value == 5


def test_large_case_shares(oracle_lib):
    """The large case's flags alternate along the leaf order: lit and unlit objects are each at least a quarter of the objects and the
    flag changes at least 1,000 times -- on the ORACLE's order of the flat scene (the tree the library must reproduce), so the
    compaction's scan has carries to get wrong in every workgroup and across its trips."""
    host = C.CDLL(build_host.build())
    instances, matrices = rc.large_instances()
    triangles = rc.loaded(host, instances, matrices)
    flat = rc.flat_scene(triangles, instances, rc.large_look(True))
    topology, _ = oracle_lib.bvh_dump(flat)
    order = topology[topology >= 0]
    n = len(flat["obj_kind"])
    assert sorted(order.tolist()) == list(range(n))
    lit = np.zeros(n, bool)
    lit[rc.N_DESC_OBJECTS:rc.N_DESC_OBJECTS + triangles[0][0]] = True
    share, changes = rc.share_conditions(order, lit)
    print("large case: %d objects, %.3f lit, %d changes of the flag along the order" % (n, share, changes))
