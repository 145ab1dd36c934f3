"""Builds and loads the host form of tests/hip/nearest_probe.hip: the device functions of the nearest-surface queries
(pt_nearest_kernels.h of the product) compiled with the host compiler against tests/hip/host_query.  TEST INFRASTRUCTURE ONLY; no GPU,
no hipcc.  The leaf records it reads are laid out here as pt_types.h describes them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from cpupathtrace_amd import binding
from cpupathtrace_amd import build as product
from tests import query_probe

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "nearest_probe.hip")
F = np.float32


def build_host(lib):
    """-ffp-contract=off as the product; division and square root are IEEE on the host anyway."""
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host_query"), "-I", product.CSRC, "-x", "c++", SOURCE,
           "-o", lib]
    subprocess.run(cmd, check=True)
    return lib


def leaf_records(scene):
    """recs of a flat scene's leaves, [n_tris + 1 + n_spheres][16] floats: the geometry words of the shading records, a spare record,
    (origin, radius) per sphere."""
    shade = query_probe.tri_shade(scene)
    sph = np.asarray(scene["sph"], F).reshape(-1, 4)
    recs = np.zeros((len(shade) + 1 + len(sph), 16), F)
    recs[:len(shade), :12] = shade[:, :12]
    recs[len(shade) + 1:, :4] = sph
    return recs


def _p(a):
    return C.c_void_p(a.ctypes.data)


class Probe:
    def __init__(self, lib):
        self.lib = C.CDLL(lib)

    def sizes(self):
        record, grid, offsets = C.c_uint32(), C.c_uint32(), np.zeros(12, np.uint32)
        assert self.lib.nearest_probe_sizes(C.byref(record), C.byref(grid), _p(offsets)) == 0
        return record.value, grid.value, offsets.tolist()

    def triangles(self, p, a, ab, ac):
        """(d2, v, w, feature, diff) of n pairs, row by row."""
        p, a, ab, ac = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (p, a, ab, ac))
        out = np.zeros((len(p), 8), F)
        assert self.lib.nearest_probe_triangles(C.c_uint64(len(p)), _p(p), _p(a), _p(ab), _p(ac), _p(out)) == 0
        return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy().view(np.uint32), out[:, 4:7].copy()

    def spheres(self, p, sph):
        """(d2, len, dist, feature) of n pairs."""
        p, sph = np.ascontiguousarray(p, F).reshape(-1, 3), np.ascontiguousarray(sph, F).reshape(-1, 4)
        out = np.zeros((len(p), 4), F)
        assert self.lib.nearest_probe_spheres(C.c_uint64(len(p)), _p(p), _p(sph), _p(out)) == 0
        return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy().view(np.uint32)

    def bounds(self, p, lo, hi, m):
        p, lo, hi = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (p, lo, hi))
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(m, F), (len(p),)))
        out = np.zeros(len(p), F)
        assert self.lib.nearest_probe_bounds(C.c_uint64(len(p)), _p(p), _p(lo), _p(hi), _p(m), _p(out)) == 0
        return out

    def margins(self, p, root_lo, root_hi):
        p = np.ascontiguousarray(p, F).reshape(-1, 3)
        lo, hi = np.ascontiguousarray(root_lo, F), np.ascontiguousarray(root_hi, F)
        out = np.zeros(len(p), F)
        assert self.lib.nearest_probe_margins(C.c_uint64(len(p)), _p(p), _p(lo), _p(hi), _p(out)) == 0
        return out

    def records(self, flat, points, max_distance=np.inf, with_table=False, order=None):
        """The kernel's leaf code and take rule over every leaf in `order` (default: ascending record index), then nearest_record."""
        scene = flat["scene"]
        recs = leaf_records(scene)
        n_tris = len(np.asarray(scene["tri_pos"], F).reshape(-1, 9))
        sph = np.asarray(scene["sph"], F).reshape(-1, 4)
        sphere_objects = np.nonzero(np.asarray(scene["obj_kind"]) == 1)[0]
        meta = np.ascontiguousarray(np.stack([np.asarray(scene["sph_material"], np.uint32), sphere_objects.astype(np.uint32)], axis=1)) if len(sph) else np.zeros((1, 2), np.uint32)
        table = np.array([[first, count, flat["face_first"][i], flat["n_faces"][i], i, 0, 0, 0] for i, (first, count) in enumerate(zip(flat["first"], flat["count"])) if count > 0],
                         np.uint32).reshape(-1, 8)
        face_of = np.ascontiguousarray(flat["face_of"], np.uint32) if with_table else None
        if order is None:
            order = np.concatenate([np.arange(n_tris), n_tris + 1 + np.arange(len(sph))])
        order = np.ascontiguousarray(order, np.uint32)
        assert sorted(order.tolist()) == list(range(n_tris)) + [n_tris + 1 + i for i in range(len(sph))]
        pts = np.asarray(points, F).reshape(-1, 3)
        q = np.empty((len(pts), 4), F)
        q[:, :3], q[:, 3] = pts, np.asarray(max_distance, F)
        out = np.zeros(len(q), binding.Nearest)
        rc = self.lib.nearest_probe_records(C.c_uint32(n_tris), C.c_uint32(len(sph)), _p(recs), _p(meta), _p(table) if len(table) else None, C.c_uint32(len(table)),
                                            C.c_uint32(flat["n_desc"]), _p(face_of) if face_of is not None else None, _p(order), C.c_uint64(len(q)), _p(q), _p(out))
        assert rc == 0, rc
        return out
