"""Builds and loads tests/hip/libfollow_probe.so: bsdf_follow of pt_device.h behind one entry point (tests/hip/follow_probe.hip).
TEST INFRASTRUCTURE ONLY; the probe is not part of libpathtrace_hip.so.  Built like tests/unit_probe.py builds its probe: the product's
hipcc and flags, one compile under a lock into a temporary file that is renamed into place, rebuilt when a source is newer."""
import ctypes as C
import os
import subprocess

import numpy as np

from cpupathtrace_amd import build as product
from oracle import _f32, _ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "follow_probe.hip")
LIB = os.path.join(HERE, "hip", "libfollow_probe.so")
HEADERS = ["pt_device.h", "pt_libm.h", "pt_types.h"]


def up_to_date(lib=LIB):
    if not os.path.exists(lib):
        return False
    t = os.path.getmtime(lib)
    deps = [SOURCE, os.path.join(HERE, "hip", "guard_band.h"), os.path.abspath(__file__), os.path.abspath(product.__file__)] + [os.path.join(product.CSRC, h) for h in HEADERS]
    return all(os.path.getmtime(d) <= t for d in deps)


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


class Probe:
    def __init__(self, lib=None):
        self.lib = C.CDLL(lib or build())
        self.lib.ptf_error_string.restype = C.c_char_p

    def device_count(self):
        return int(self.lib.ptf_device_count())

    def bsdf_follow(self, kind, one_way, rays, pos, nrm, epsilon, ior):
        """bsdf_follow for n cases: (rays (n, 6), reflected (n,) bool)."""
        rays, pos, nrm, ior = _f32(rays, (-1, 6)), _f32(pos, (-1, 3)), _f32(nrm, (-1, 3)), _f32(ior)
        n = len(rays)
        assert len(pos) == len(nrm) == len(ior) == n
        out_ray, refl = np.empty((n, 6), np.float32), np.empty(n, np.int32)
        rc = self.lib.ptf_bsdf_follow(C.c_int(kind), C.c_int(one_way), C.c_uint64(n), C.c_void_p(_ptr(rays)), C.c_void_p(_ptr(pos)), C.c_void_p(_ptr(nrm)),
                                      C.c_float(epsilon), C.c_void_p(_ptr(ior)), C.c_void_p(_ptr(out_ray)), C.c_void_p(_ptr(refl)))
        if rc != 0:
            raise ProbeError("ptf_bsdf_follow: error %d (%s)" % (rc, self.lib.ptf_error_string(rc).decode()))
        return out_ray, refl != 0
