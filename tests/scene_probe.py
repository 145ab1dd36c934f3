"""Builds and loads tests/hip/libscene_probe.so: sample_emissive (pt_shading.h) and object_normal / tri_shade_normal (pt_device.h) on the
device tables of a scene the product created (tests/hip/scene_probe.hip).  TEST INFRASTRUCTURE ONLY; not part of libpathtrace_hip.so.

Built like tests/unit_probe.py: the product's hipcc and flags, one compile under a lock into a temporary file that is renamed into place,
rebuilt when the probe source or a product header is newer than the library.  `SceneProbe` takes a cpupathtrace_amd.binding.Scene: the
probe runs in the same process on the same device and reads the scene's own device memory through its handle.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from cpupathtrace_amd import build as product
from oracle import _f32, _ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "scene_probe.hip")
LIB = os.path.join(HERE, "hip", "libscene_probe.so")


def _deps():
    headers = [os.path.join(product.CSRC, f) for f in os.listdir(product.CSRC) if f.endswith(".h")]
    return [SOURCE, os.path.join(HERE, "hip", "guard_band.h"), os.path.abspath(__file__), os.path.abspath(product.__file__), os.path.join(product.CSRC, "..", "..", "include", "pt_hip.h")] + headers


def up_to_date(lib=LIB):
    if not os.path.exists(lib):
        return False
    t = os.path.getmtime(lib)
    return all(os.path.getmtime(d) <= t for d in _deps())


def build(force=False, verbose=False, lib=LIB):
    """Compile the probe for gfx950 unless it is up to date (no GPU needed).  Safe when several processes call it at once."""
    if not force and up_to_date(lib):
        return lib
    import fcntl
    with open(lib + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and up_to_date(lib):
                return lib
            tmp = "%s.%d.tmp" % (lib, os.getpid())
            cmd = [product.hipcc()] + product.FLAGS + ["-x", "hip", SOURCE, "-o", tmp]
            if verbose:
                print(" ".join(cmd))
            try:
                subprocess.run(cmd, check=True)
                os.replace(tmp, lib)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return lib


class ProbeError(RuntimeError):
    pass


class SceneProbe:
    """The device side of oracle.SceneHandle.sample_lights / .normal for one binding.Scene."""

    def __init__(self, scene, lib=None):
        self.lib = C.CDLL(lib or build())
        self.lib.pts_error_string.restype = C.c_char_p
        self.scene = scene  # (kept alive: the probe reads its device memory)
        counts = np.zeros(4, np.uint32)
        self._call("scene_counts", C.c_void_p(_ptr(counts)))
        self.n_emis, self.n_object_samples, self.n_lights, self.device_built = (int(v) for v in counts)
        self.lds_table_max = int(self.lib.pts_lds_table_max())

    def _call(self, name, *args):
        rc = getattr(self.lib, "pts_" + name)(self.scene._h, *args)
        if rc != 0:
            raise ProbeError("pts_%s: error %d (%s)" % (name, rc, self.lib.pts_error_string(rc).decode()))

    def emis_cdf(self):
        out = np.zeros(max(self.n_emis, 1), np.float32)
        self._call("emis_cdf", C.c_void_p(_ptr(out)))
        return out[:self.n_emis]

    def sample_emissive(self, form, pos, states):
        """n_object_samples draws of sample_emissive per case, in order.  form 0: the tables in global memory, 1: in LDS.  Returns
        valid [n][S], light_pos [n][S][3], spectrum [n][S][4], pd [n][S] and the engine state after every draw [n][S]."""
        pos = _f32(pos, (-1, 3))
        states = np.ascontiguousarray(states, dtype=np.uint64)
        n, s = len(pos), self.n_object_samples
        assert len(states) == n
        valid, lp = np.empty((n, s), np.uint8), np.empty((n, s, 3), np.float32)
        rgba, pd, st = np.empty((n, s, 4), np.float32), np.empty((n, s), np.float32), np.empty((n, s), np.uint64)
        self._call("sample_emissive", C.c_int(form), C.c_uint64(n), C.c_void_p(_ptr(pos)), C.c_void_p(_ptr(states)), C.c_void_p(_ptr(valid)),
                   C.c_void_p(_ptr(lp)), C.c_void_p(_ptr(rgba)), C.c_void_p(_ptr(pd)), C.c_void_p(_ptr(st)))
        return valid, lp, rgba, pd, st

    def sample_lights(self, form, pos, states, light_pos, light_spectrum, max_lights=16):
        """The draws of sample_emissive arranged as Scene::sampleLights returns them (oracle.SceneHandle.sample_lights): the point lights
        first (pd 1), then the valid draws, compacted; the engine state after the last draw."""
        valid, lp, rgba, pd, st = self.sample_emissive(form, pos, states)
        n, s = valid.shape
        light_pos, light_spectrum = _f32(light_pos, (-1, 3)), _f32(light_spectrum, (-1, 4))
        k = len(light_pos)
        assert k + s <= max_lights
        cnt = (k + valid.sum(axis=1)).astype(np.int32)
        out_lp, out_rgba, out_pd = np.zeros((n, max_lights, 3), np.float32), np.zeros((n, max_lights, 4), np.float32), np.zeros((n, max_lights), np.float32)
        out_lp[:, :k], out_rgba[:, :k], out_pd[:, :k] = light_pos, light_spectrum, 1.0
        at = np.full(n, k)
        for j in range(s):
            rows = np.nonzero(valid[:, j])[0]
            out_lp[rows, at[rows]], out_rgba[rows, at[rows]], out_pd[rows, at[rows]] = lp[rows, j], rgba[rows, j], pd[rows, j]
            at[rows] += 1
        return cnt, out_lp, out_rgba, out_pd, (st[:, -1] if s > 0 else np.ascontiguousarray(states, dtype=np.uint64)), valid

    def object_normal(self, obj, pos, lds=False):
        """object_normal of object obj[i] (construction index) at pos[i]: (normal, material index); with lds also (found, normal, material)
        through tri_shade_normal on the LDS record, found = 1 where the object is an emissive triangle."""
        obj = np.ascontiguousarray(obj, dtype=np.int32)
        pos = _f32(pos, (-1, 3))
        n = len(pos)
        assert len(obj) == n
        nrm, mat = np.empty((n, 3), np.float32), np.empty(n, np.uint32)
        found, lnrm, lmat = np.empty(n, np.uint8), np.empty((n, 3), np.float32), np.empty(n, np.uint32)
        self._call("object_normal", C.c_int(1 if lds else 0), C.c_uint64(n), C.c_void_p(_ptr(obj)), C.c_void_p(_ptr(pos)), C.c_void_p(_ptr(nrm)),
                   C.c_void_p(_ptr(mat)), C.c_void_p(_ptr(found)), C.c_void_p(_ptr(lnrm)), C.c_void_p(_ptr(lmat)))
        return (nrm, mat, found, lnrm, lmat) if lds else (nrm, mat)


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
