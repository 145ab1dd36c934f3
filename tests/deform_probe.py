"""Builds and loads the host form of tests/hip/deform_probe.hip: the skinning kernel's own source (pt_deform_kernels.h of the product)
compiled with the host compiler against tests/hip/host_deform.  TEST INFRASTRUCTURE ONLY; no GPU, no hipcc.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from cpupathtrace_amd import build as product

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "deform_probe.hip")
F = np.float32


def build_host(lib):
    """-ffp-contract=off as the product."""
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host_deform"), "-I", product.CSRC, "-x", "c++", SOURCE,
           "-o", lib]
    subprocess.run(cmd, check=True)
    return lib


class Probe:
    def __init__(self, lib):
        self.lib = C.CDLL(lib)
        self.lib.deform_probe_lds_bones.restype = C.c_uint32
        self.lds_bones = self.lib.deform_probe_lds_bones()

    def skin(self, rest, bone, weight, bones, lds_bones=None):
        """The kernel over one mesh: rest (n, 3), bone / weight (n, K), bones (n_bones, 3, 4) -> (n, 3).  lds_bones: the launch's LDS
        budget in bones (None = the product's, 0 = the cache form)."""
        rest = np.ascontiguousarray(rest, F).reshape(-1, 3)
        bone = np.ascontiguousarray(bone, np.uint32).reshape(len(rest), -1)
        weight = np.ascontiguousarray(weight, F).reshape(bone.shape)
        table = np.ascontiguousarray(bones, F).reshape(-1, 12)
        out = np.zeros((len(rest), 3), F)
        rc = self.lib.deform_probe_skin(C.c_uint32(len(rest)), C.c_void_p(rest.ctypes.data), C.c_uint32(bone.shape[1]), C.c_void_p(bone.ctypes.data),
                                        C.c_void_p(weight.ctypes.data), C.c_void_p(table.ctypes.data), C.c_uint32(len(table)),
                                        C.c_uint32(self.lds_bones if lds_bones is None else lds_bones), C.c_void_p(out.ctypes.data))
        assert rc == 0, rc
        return out
