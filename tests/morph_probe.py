"""Builds and loads the host form of tests/hip/morph_probe.hip: the blend-shape kernel's own source (pt_morph_kernels.h of the product,
behind pt_deform_kernels.h) and the host transposition of a morph set (pt_morph_rows.h), compiled with the host compiler against
tests/hip/host_deform.  TEST INFRASTRUCTURE ONLY; no GPU, no hipcc.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from cpupathtrace_amd import binding
from cpupathtrace_amd import build as product

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "morph_probe.hip")
F = np.float32


def build_host(lib):
    """-ffp-contract=off as the product."""
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host_deform"), "-I", product.CSRC, "-x", "c++", SOURCE,
           "-o", lib]
    subprocess.run(cmd, check=True)
    return lib


def target_table(targets):
    """(pt_morph_target array, the arrays it points into) for a list of (indices or None, deltas)."""
    table, keep = (binding.MorphTarget * max(len(targets), 1))(), []
    for t, (indices, deltas) in enumerate(targets):
        d = np.ascontiguousarray(deltas, F).reshape(-1, 3)
        backing = d if len(d) > 0 else np.zeros((1, 3), F)
        keep += [d, backing]
        table[t].n_deltas, table[t].delta = len(d), backing.ctypes.data
        if indices is not None:
            idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
            assert len(idx) == len(d)
            backing = idx if len(idx) > 0 else np.zeros(1, np.uint32)
            keep += [idx, backing]
            table[t].vertex = backing.ctypes.data
    return table, keep


class Probe:
    def __init__(self, lib):
        self.lib = C.CDLL(lib)
        self.lib.morph_probe_lds_targets.restype = C.c_uint32
        self.lib.morph_probe_rows.restype = None
        self.lds_targets = self.lib.morph_probe_lds_targets()

    def rows(self, n_vertices, targets):
        """The product's transposition: (row_start (n + 1,), target of every entry, delta (entries, 3))."""
        table, keep = target_table(targets)
        n_entries = sum(len(np.asarray(d).reshape(-1, 3)) for _, d in targets)
        row_start, target, delta = np.zeros(n_vertices + 1, np.uint32), np.zeros(max(n_entries, 1), np.uint32), np.zeros((max(n_entries, 1), 3), F)
        self.lib.morph_probe_rows(C.c_uint32(n_vertices), table, C.c_uint32(len(targets)), C.c_void_p(row_start.ctypes.data), C.c_void_p(target.ctypes.data),
                                  C.c_void_p(delta.ctypes.data))
        del keep
        return row_start, target[:n_entries], delta[:n_entries]

    def morph(self, rest, targets, weights, skin=None, lds_targets=None, lds_bones=256):
        """The kernel over one mesh: rest (n, 3), targets [(indices or None, deltas)], weights (T,); skin: None (K = 0) or
        (bone (n, K), weight (n, K), bones (n_bones, 3, 4)) -> (n, 3).  lds_targets: the launch's LDS budget in weights (None = the
        product's, 0 = the cache form); lds_bones: the same for the bone table."""
        rest = np.ascontiguousarray(rest, F).reshape(-1, 3)
        weights = np.ascontiguousarray(weights, F).reshape(-1)
        assert len(weights) == len(targets)
        table, keep = target_table(targets)
        k, n_bones, bone, weight, bones = 0, 0, None, None, None
        if skin is not None:
            bone = np.ascontiguousarray(skin[0], np.uint32).reshape(len(rest), -1)
            weight = np.ascontiguousarray(skin[1], F).reshape(bone.shape)
            bones = np.ascontiguousarray(skin[2], F).reshape(-1, 12)
            k, n_bones = bone.shape[1], len(bones)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        out = np.zeros((len(rest), 3), F)
        rc = self.lib.morph_probe_morph(C.c_uint32(len(rest)), ptr(rest), table, C.c_uint32(len(targets)), ptr(weights),
                                        C.c_uint32(self.lds_targets if lds_targets is None else lds_targets), C.c_uint32(k), ptr(bone), ptr(weight), ptr(bones),
                                        C.c_uint32(n_bones), C.c_uint32(lds_bones), ptr(out))
        del keep
        assert rc == 0, rc
        return out
