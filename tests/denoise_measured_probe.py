"""Builds and loads tests/hip/libdenoise_measured_probe.so: the measured form of the denoiser (pt_denoise_measured_run) on caller-given
frames and planes, whole runs and one kernel at a time (tests/hip/denoise_measured_probe.hip).  TEST INFRASTRUCTURE ONLY; the probe is not
part of libpathtrace_hip.so.

Built as tests/denoise_probe.py builds its probe (the product's hipcc and flags, under a lock, rebuilt when a source is newer); the probe
includes that one, so Probe here has every method of denoise_probe.Probe (the existing filter, from the same library) and adds the measured
ones, in the layout of the numpy restatement (tests/denoise_measured_ref.py).  A written guard band raises GuardError.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from cpupathtrace_amd import build as product
from tests import denoise_probe as dp
from tests.denoise_probe import GuardError, ProbeError  # noqa: F401 (what the probe raises)

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "denoise_measured_probe.hip")
LIB = os.path.join(HERE, "hip", "libdenoise_measured_probe.so")
F = np.float32


def up_to_date(lib=LIB):
    if not os.path.exists(lib):
        return False
    t = os.path.getmtime(lib)
    deps = [SOURCE, dp.SOURCE, os.path.abspath(__file__), os.path.abspath(product.__file__)] + [os.path.join(product.CSRC, h) for h in dp.HEADERS]
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


def build_host(lib):
    """The probe and the kernels it includes compiled for the host against tests/hip/host (no GPU, no hipcc), as denoise_probe.build_host."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host"), "-I", product.CSRC, "-x", "c++", SOURCE,
           "-o", lib]
    subprocess.run(cmd, check=True)
    return lib


class Probe(dp.Probe):
    def __init__(self, lib=None):
        super().__init__(lib or build())

    def _callm(self, name, *args):
        rc = getattr(self.lib, "ptm_" + name)(*args)
        if rc >= self.guard_code:
            raise GuardError("ptm_%s: the guard band of buffer %d was written" % (name, rc - self.guard_code))
        if rc != 0:
            raise ProbeError("ptm_%s: HIP error %d (%s)" % (name, rc, self.lib.ptd_error_string(rc).decode()))

    def denoise_measured(self, rgba, features, plane, samples, params, in_place=False):
        """pt_denoise_measured_run; params: the restatement's dict (DenoiseParams' fields and sigma_measured)."""
        rgba = dp._f(rgba)
        h, w = rgba.shape[:2]
        s = None if samples is None else dp._i(samples)
        assert s is None or s.shape == (h, w)
        out = np.empty_like(rgba)
        par = dp.denoise_params(params)
        self._callm("run", C.c_int32(w), C.c_int32(h), dp._p(rgba), dp._p(dp._f(features, (h, w, 3, 4))), dp._p(dp._f(plane, (h, w, 4))), dp._p(s), C.byref(par),
                    C.c_float(params["sigma_measured"]), C.c_int(1 if in_place else 0), dp._p(out))
        return out

    def variance_measured(self, c, l, guide, cls, features, plane, sigma_normal, sigma_depth, masked=False):
        """-> gx, gy, var"""
        h, w = np.asarray(l).shape
        grad, var = np.empty((h, w, 2), F), np.empty((h, w), F)
        self._callm("variance", C.c_int(1 if masked else 0), C.c_int32(w), C.c_int32(h), dp._p(dp._col4(c, l)), dp._p(dp._f(guide, (h, w, 4))), dp._p(dp._u(cls)),
                    dp._p(dp._f(features, (h, w, 3, 4))), dp._p(dp._f(plane, (h, w, 4))), C.c_float(sigma_normal), C.c_float(sigma_depth), dp._p(grad), dp._p(var))
        return grad[..., 0].copy(), grad[..., 1].copy(), var

    def atrous_measured(self, c, l, var, guide, cls, gx, gy, plane, step, sigma_luminance, sigma_normal, sigma_depth, sigma_measured, masked=False):
        """One launch -> c, l, var"""
        h, w = np.asarray(l).shape
        col_out, var_out = np.empty((h, w, 4), F), np.empty((h, w), F)
        grad = np.ascontiguousarray(np.stack([np.asarray(gx, F), np.asarray(gy, F)], axis=-1), dtype=F)
        self._callm("atrous", C.c_int(1 if masked else 0), C.c_int32(w), C.c_int32(h), dp._p(dp._col4(c, l)), dp._p(dp._f(var, (h, w))), dp._p(dp._f(guide, (h, w, 4))),
                    dp._p(dp._u(cls)), dp._p(grad), dp._p(dp._f(plane, (h, w, 4))), C.c_int32(step), C.c_float(sigma_luminance), C.c_float(sigma_normal),
                    C.c_float(sigma_depth), C.c_float(sigma_measured), dp._p(col_out), dp._p(var_out))
        return col_out[..., :3].copy(), col_out[..., 3].copy(), var_out


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
