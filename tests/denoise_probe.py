"""Builds and loads tests/hip/libdenoise_probe.so: the denoiser kernels of pt_denoise.hip on caller-given frames, whole runs and one
kernel at a time (tests/hip/denoise_probe.hip).  TEST INFRASTRUCTURE ONLY; the probe is not part of libpathtrace_hip.so.

Built like tests/unit_probe.py: the product's hipcc and flags, one compile under a lock into a temporary file that is renamed into place,
rebuilt when the probe source or pt_denoise.hip / pt_denoise.h is newer than the library.  Every method takes and returns the arrays of the
numpy restatements (tests/denoise_ref.py, preview_ref.py, temporal_ref.py) in their layout: colour (H, W, 3) and luminance (H, W) apart,
classes int32.  A written guard band raises GuardError.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from cpupathtrace_amd import build as product

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "denoise_probe.hip")
LIB = os.path.join(HERE, "hip", "libdenoise_probe.so")
HEADERS = ["pt_denoise.hip", "pt_denoise.h"]
F = np.float32


def up_to_date(lib=LIB, source=SOURCE):
    if not os.path.exists(lib):
        return False
    t = os.path.getmtime(lib)
    deps = [source, os.path.abspath(__file__), os.path.abspath(product.__file__)] + [os.path.join(product.CSRC, h) for h in HEADERS]
    return all(os.path.getmtime(d) <= t for d in deps)


def build(force=False, verbose=False, lib=LIB, source=SOURCE):
    """Compile the probe for gfx950 unless it is up to date (no GPU needed).  Safe when several processes call it at once."""
    if not force and up_to_date(lib, source):
        return lib
    import fcntl
    with open(lib + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and up_to_date(lib, source):
                return lib
            tmp = "%s.%d.tmp" % (lib, os.getpid())
            cmd = [product.hipcc()] + product.FLAGS + ["-x", "hip", source, "-o", tmp]
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
    """The probe and the kernels it includes compiled for the host against tests/hip/host (no GPU, no hipcc): for tests that run the
    kernels' source on the CPU.  -ffp-contract=off as the product; division and square root are IEEE on the host anyway."""
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    cmd = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host"), "-I", product.CSRC, "-x", "c++", SOURCE,
           "-o", lib]
    subprocess.run(cmd, check=True)
    return lib


class ProbeError(RuntimeError):
    pass


class GuardError(ProbeError):
    """A kernel wrote into the guard band of a buffer (or into the sentinel view of a batch)."""


class DenoiseParams(C.Structure):  # PtDenoiseParams
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float)]


class TemporalParams(C.Structure):  # PtTemporalParams
    _fields_ = [("spatial", DenoiseParams), ("alpha_color", C.c_float), ("alpha_moments", C.c_float), ("max_history", C.c_int32),
                ("moments_min_history", C.c_int32), ("sigma_luminance_temporal", C.c_float), ("normal_min", C.c_float), ("position_tolerance", C.c_float)]


class Reprojection(C.Structure):  # PtReprojection
    _fields_ = [("origin", C.c_float * 3), ("row", (C.c_float * 3) * 3), ("footprint", C.c_float), ("mode", C.c_int32)]


def denoise_params(p):
    return DenoiseParams(int(p["iterations"]), float(p["sigma_luminance"]), float(p["sigma_normal"]), float(p["sigma_depth"]))


def temporal_params(p):
    return TemporalParams(denoise_params(p["spatial"]), p["alpha_color"], p["alpha_moments"], int(p["max_history"]), int(p["moments_min_history"]),
                          p["sigma_luminance_temporal"], p["normal_min"], p["position_tolerance"])


def reprojection(mode, origin=(0, 0, 0), rows=((1, 0, 0), (0, 1, 0), (0, 0, 1)), footprint=0.0):
    rp = Reprojection()
    rp.origin[:] = [float(v) for v in origin]
    for i in range(3):
        rp.row[i][:] = [float(v) for v in rows[i]]
    rp.footprint = float(footprint)
    rp.mode = int(mode)
    return rp


def _f(a, shape=None):
    a = np.ascontiguousarray(a, dtype=F)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _p(a):
    p = C.c_void_p(None if a is None else a.ctypes.data)
    p.array = a  # (the array lives as long as the argument)
    return p


def _col4(c, l):
    """(H, W, 3) colour and (H, W) luminance as the kernels' float4."""
    return np.ascontiguousarray(np.concatenate([np.asarray(c, F), np.asarray(l, F)[..., None]], axis=-1), dtype=F)


def _pad4(a):
    a = np.asarray(a, F)
    return np.ascontiguousarray(np.concatenate([a, np.zeros(a.shape[:-1] + (1,), F)], axis=-1), dtype=F)


def _u(a):
    return np.ascontiguousarray(np.asarray(a).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def prev_state(h, w, col=None, lum=None, mom=None, length=None, pos=None, nrm=None, cls=None):
    """A previous state as temporal_ref keeps it (zeros where not given)."""
    z = lambda *s: np.zeros((h, w) + s, F)
    col = z(3) if col is None else np.asarray(col, F)
    return {"col": col, "lum": z() if lum is None else np.asarray(lum, F), "mom": z(2) if mom is None else np.asarray(mom, F),
            "len": np.zeros((h, w), np.int32) if length is None else _i(length), "pos": z(3) if pos is None else np.asarray(pos, F),
            "nrm": z(3) if nrm is None else np.asarray(nrm, F), "cls": np.zeros((h, w), np.int32) if cls is None else _i(cls)}


class Probe:
    def __init__(self, lib=None):
        self.lib = C.CDLL(lib or build())
        self.lib.ptd_error_string.restype = C.c_char_p
        self.guard_code = int(self.lib.ptd_guard_code())

    def device_count(self):
        return int(self.lib.ptd_device_count())

    def _call(self, name, *args):
        rc = getattr(self.lib, "ptd_" + name)(*args)
        if rc >= self.guard_code:
            raise GuardError("ptd_%s: the guard band of buffer %d was written" % (name, rc - self.guard_code))
        if rc != 0:
            raise ProbeError("ptd_%s: HIP error %d (%s)" % (name, rc, self.lib.ptd_error_string(rc).decode()))

    # ---- whole runs ----
    def _run(self, form, rgba, features, samples, params, n_views, split, in_place):
        rgba = _f(rgba)
        h, w = rgba.shape[-3:-1]
        features = _f(features, rgba.shape[:-1] + (3, 4))
        samples = None if samples is None else _i(samples)
        assert samples is None or samples.shape == rgba.shape[:-1]
        out = np.empty_like(rgba)
        dp = denoise_params(params)
        self._call("run", C.c_int(form), C.c_int32(w), C.c_int32(h), C.c_int32(n_views), C.c_int32(split), _p(rgba), _p(features), _p(samples), C.byref(dp),
                   C.c_int(1 if in_place else 0), _p(out))
        return out

    def denoise(self, rgba, features, params, in_place=False):
        return self._run(0, rgba, features, None, params, 1, 0, in_place)

    def denoise_masked(self, rgba, features, samples, params, in_place=False):
        return self._run(1, rgba, features, samples, params, 1, 0, in_place)

    def denoise_views(self, rgba, features, samples, params, split=0, in_place=False):
        """(V, H, W, 4) frames through pt_denoise_views_run; 0 < split < V puts a sentinel view between views split - 1 and split."""
        return self._run(2, rgba, features, samples, params, len(rgba), split, in_place)

    def temporal(self, rgba, features, params, rp, prev, in_place=False):
        """One pt_temporal_run from the previous state `prev` (prev_state()).  Returns out and this push's state as a dict like prev."""
        rgba = _f(rgba)
        h, w = rgba.shape[:2]
        out, hist, mom = np.empty_like(rgba), np.empty((h, w, 4), F), np.empty((h, w, 2), F)
        ln, pos, nrm, cls = np.empty((h, w), np.int32), np.empty((h, w, 4), F), np.empty((h, w, 4), F), np.empty((h, w), np.uint32)
        tp = temporal_params(params)
        pc, pm, pl, pp, pn, pcl = _col4(prev["col"], prev["lum"]), _f(prev["mom"], (h, w, 2)), _i(prev["len"]), _pad4(prev["pos"]), _pad4(prev["nrm"]), _u(prev["cls"])
        self._call("temporal", C.c_int32(w), C.c_int32(h), _p(rgba), _p(_f(features, (h, w, 3, 4))), C.byref(tp), C.byref(rp), _p(pc), _p(pm), _p(pl), _p(pp),
                   _p(pn), _p(pcl), C.c_int(1 if in_place else 0), _p(out), _p(hist), _p(mom), _p(ln), _p(pos), _p(nrm), _p(cls))
        return out, {"col": hist[..., :3], "lum": hist[..., 3], "mom": mom, "len": ln, "pos": pos[..., :3], "nrm": nrm[..., :3], "cls": cls.astype(np.int32),
                     "pos_w": pos[..., 3], "nrm_w": nrm[..., 3]}

    # ---- single stages ----
    def prepare(self, rgba, features, samples=None):
        """-> c (H, W, 3), l (H, W), guide (H, W, 4), cls (H, W) int32"""
        rgba = _f(rgba)
        h, w = rgba.shape[:2]
        col, guide, cls = np.empty((h, w, 4), F), np.empty((h, w, 4), F), np.empty((h, w), np.uint32)
        s = None if samples is None else _i(samples)
        self._call("prepare", C.c_int(0 if s is None else 1), C.c_int32(w), C.c_int32(h), _p(rgba), _p(_f(features, (h, w, 3, 4))), _p(s), _p(col), _p(guide), _p(cls))
        return col[..., :3].copy(), col[..., 3].copy(), guide, cls.astype(np.int32)

    def variance(self, c, l, guide, cls, sigma_normal, sigma_depth, masked=False, temporal=None):
        """-> gx, gy, var.  temporal = (len, moments, min_history) selects the kTemporal form."""
        h, w = np.asarray(l).shape
        grad, var = np.empty((h, w, 2), F), np.empty((h, w), F)
        form = 2 if temporal is not None else (1 if masked else 0)
        ln, mom, mh = (None, None, 0) if temporal is None else (_i(temporal[0]), _f(temporal[1], (h, w, 2)), int(temporal[2]))
        self._call("variance", C.c_int(form), C.c_int32(w), C.c_int32(h), _p(_col4(c, l)), _p(_f(guide, (h, w, 4))), _p(_u(cls)), C.c_float(sigma_normal),
                   C.c_float(sigma_depth), _p(ln), _p(mom), C.c_int32(mh), _p(grad), _p(var))
        return grad[..., 0].copy(), grad[..., 1].copy(), var

    def atrous(self, c, l, var, guide, cls, gx, gy, step, sigma_luminance, sigma_normal, sigma_depth, masked=False, temporal=None):
        """One launch -> c, l, var.  temporal = (len, moments, min_history, sigma_luminance_temporal)."""
        h, w = np.asarray(l).shape
        col_out, var_out = np.empty((h, w, 4), F), np.empty((h, w), F)
        form = 2 if temporal is not None else (1 if masked else 0)
        ln, mom, mh, slt = (None, None, 0, 0.0) if temporal is None else (_i(temporal[0]), _f(temporal[1], (h, w, 2)), int(temporal[2]), float(temporal[3]))
        grad = np.ascontiguousarray(np.stack([np.asarray(gx, F), np.asarray(gy, F)], axis=-1), dtype=F)
        self._call("atrous", C.c_int(form), C.c_int32(w), C.c_int32(h), _p(_col4(c, l)), _p(_f(var, (h, w))), _p(_f(guide, (h, w, 4))), _p(_u(cls)), _p(grad),
                   C.c_int32(step), C.c_float(sigma_luminance), C.c_float(sigma_normal), C.c_float(sigma_depth), _p(ln), _p(mom), C.c_int32(mh), C.c_float(slt),
                   _p(col_out), _p(var_out))
        return col_out[..., :3].copy(), col_out[..., 3].copy(), var_out

    def accumulate(self, features, c, l, cls, rp, prev, params):
        """-> col (H, W, 3), lum, moments (H, W, 2), len, pos (H, W, 4), nrm (H, W, 4)"""
        h, w = np.asarray(l).shape
        col_out, mom, ln = np.empty((h, w, 4), F), np.empty((h, w, 2), F), np.empty((h, w), np.int32)
        pos, nrm = np.empty((h, w, 4), F), np.empty((h, w, 4), F)
        pc, pm, pl, pp, pn, pcl = _col4(prev["col"], prev["lum"]), _f(prev["mom"], (h, w, 2)), _i(prev["len"]), _pad4(prev["pos"]), _pad4(prev["nrm"]), _u(prev["cls"])
        self._call("accumulate", C.c_int32(w), C.c_int32(h), _p(_f(features, (h, w, 3, 4))), _p(_col4(c, l)), _p(_u(cls)), C.byref(rp), _p(pc), _p(pm), _p(pl),
                   _p(pp), _p(pn), _p(pcl), C.c_float(params["alpha_color"]), C.c_float(params["alpha_moments"]), C.c_int32(params["max_history"]),
                   C.c_float(params["normal_min"]), C.c_float(params["position_tolerance"]), _p(col_out), _p(mom), _p(ln), _p(pos), _p(nrm))
        return col_out[..., :3].copy(), col_out[..., 3].copy(), mom, ln, pos, nrm

    def finish(self, c, l, rgba, features, cls=None, var=None, in_place=False):
        """cls and var given: the kMasked form."""
        rgba = _f(rgba)
        h, w = rgba.shape[:2]
        out = np.empty_like(rgba)
        masked = cls is not None
        self._call("finish", C.c_int(1 if masked else 0), C.c_int32(w), C.c_int32(h), _p(_col4(c, l)), _p(rgba), _p(_f(features, (h, w, 3, 4))),
                   _p(_u(cls) if masked else None), _p(_f(var, (h, w)) if masked else None), C.c_int(1 if in_place else 0), _p(out))
        return out


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
