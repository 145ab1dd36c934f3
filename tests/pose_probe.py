"""Builds and loads the host form of tests/hip/pose_probe.hip: the batched mesh assembler's own source (pt_mesh_batch_kernels.h of the
product) compiled with the host compiler against tests/hip/host_pose.  TEST INFRASTRUCTURE ONLY; no GPU, no hipcc.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from cpupathtrace_amd import build as product

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "pose_probe.hip")
F = np.float32


def build_host(lib):
    """-ffp-contract=off as the product; division and square root are IEEE on the host anyway."""
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host_pose"), "-I", product.CSRC, "-x", "c++", SOURCE,
           "-o", lib]
    subprocess.run(cmd, check=True)
    return lib


class ProbeMesh(C.Structure):
    _fields_ = [("n_vertices", C.c_uint32), ("vertices", C.c_void_p), ("n_faces", C.c_uint32), ("faces", C.c_void_p)]


class ProbeInstance(C.Structure):
    _fields_ = [("mesh", C.c_uint32), ("transform", C.c_float * 16), ("smooth", C.c_int32)]


class Range(C.Structure):  # PtBatchRange
    _fields_ = [("first_tri", C.c_uint32), ("count", C.c_uint32), ("material", C.c_uint32), ("cull", C.c_uint32)]


class Probe:
    def __init__(self, lib):
        self.lib = C.CDLL(lib)

    def assemble(self, meshes, instances, room, out_pos, out_nrm, limits=(0, 0, 0)):
        """meshes: [(vertices, faces)]; instances: [(mesh index, matrix, smooth)].  Returns (total, counts, chunks, scans, sorts); the
        triangles are written to out_pos / out_nrm (room rows at least)."""
        keep = [(np.ascontiguousarray(v, F).reshape(-1, 3), np.ascontiguousarray(f, np.int32).reshape(-1, 3)) for v, f in meshes]
        md = (ProbeMesh * max(len(keep), 1))(*[ProbeMesh(len(v), v.ctypes.data, len(f), f.ctypes.data) for v, f in keep])
        inst = (ProbeInstance * max(len(instances), 1))()
        for i, (mesh, matrix, smooth) in enumerate(instances):
            inst[i].mesh = mesh
            inst[i].transform[:] = [float(x) for x in np.asarray(matrix, F).reshape(16)]
            inst[i].smooth = int(smooth)
        counts = np.zeros(len(instances), np.uint32)
        kept, chunks, scans, sorts = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.lib.pose_probe_assemble(md, inst, C.c_uint32(len(instances)), C.c_uint64(limits[0]), C.c_uint64(limits[1]), C.c_uint64(limits[2]), C.c_uint64(room),
                                          C.c_void_p(out_pos.ctypes.data), C.c_void_p(out_nrm.ctypes.data), C.c_void_p(counts.ctypes.data), C.byref(kept),
                                          C.byref(chunks), C.byref(scans), C.byref(sorts))
        assert rc == 0, rc
        return kept.value, counts, chunks.value, scans.value, sorts.value

    def fill_ranges(self, ranges, first_tri, n, first_obj):
        """ranges: [(first_tri, count, material, cull)]; returns (cull, material, object) arrays of first_tri + n entries, 0xA5 where nothing was written."""
        table = (Range * max(len(ranges), 1))(*[Range(*r) for r in ranges])
        cull = np.full(first_tri + n, 0xA5, np.uint8)
        material, obj = np.full(first_tri + n, 0xA5A5A5A5, np.uint32), np.full(first_tri + n, 0xA5A5A5A5, np.uint32)
        rc = self.lib.pose_probe_fill_ranges(table, C.c_uint32(len(ranges)), C.c_uint32(first_tri), C.c_uint32(n), C.c_uint32(first_obj), C.c_void_p(cull.ctypes.data),
                                             C.c_void_p(material.ctypes.data), C.c_void_p(obj.ctypes.data))
        assert rc == 0, rc
        return cull, material, obj
