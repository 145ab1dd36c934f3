"""Builds and loads tests/hip/libunit_probe.so: the device functions of pt_device.h / pt_libm.h behind one entry point each
(tests/hip/unit_probe.hip).  TEST INFRASTRUCTURE ONLY; the probe is not part of libpathtrace_hip.so.

Built like the product (cpupathtrace_amd/build.py): the same hipcc, the same flags, one compile under a lock into a temporary file that
is renamed into place, and rebuilt when the probe source or a product header is newer than the library.  `Probe` has the methods of
oracle.Checker for the units it covers, with the same arguments and results, so a test hands one set of arrays to both.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from cpupathtrace_amd import build as product
from oracle import _f32, _ptr, camera_params

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "unit_probe.hip")
LIB = os.path.join(HERE, "hip", "libunit_probe.so")
HEADERS = ["pt_device.h", "pt_shading.h", "pt_kernels.h", "pt_libm.h", "pt_types.h", os.path.join("..", "..", "include", "pt_hip.h"), os.path.join("..", "..", "include", "pt_frame_noise.h")]


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


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


class Probe:
    """The device side of oracle.Checker: same methods, same arrays, computed by the product's device functions on GPU 0."""

    def __init__(self, lib=None):
        self.lib = C.CDLL(lib or build())
        self.lib.ptu_error_string.restype = C.c_char_p

    def device_count(self):
        return int(self.lib.ptu_device_count())

    def _call(self, name, *args):
        rc = getattr(self.lib, "ptu_" + name)(*args)
        if rc != 0:
            raise ProbeError("ptu_%s: HIP error %d (%s)" % (name, rc, self.lib.ptu_error_string(rc).decode()))

    # ---- RNG (each also returns the engine's state after the last draw) ----
    def rng_draws(self, seed, n):
        out, st = np.empty(n, dtype=np.uint32), C.c_uint64(0)
        self._call("rng_draws", C.c_uint64(seed), C.c_uint64(n), C.c_void_p(_ptr(out)), C.byref(st))
        return out, st.value

    def uniform_floats(self, seed, a, b, n):
        out, st = np.empty(n, dtype=np.float32), C.c_uint64(0)
        self._call("uniform_floats", C.c_uint64(seed), C.c_float(a), C.c_float(b), C.c_uint64(n), C.c_void_p(_ptr(out)), C.byref(st))
        return out, st.value

    def bernoulli(self, seed, p, n):
        out, st = np.empty(n, dtype=np.uint8), C.c_uint64(0)
        self._call("bernoulli", C.c_uint64(seed), C.c_double(p), C.c_uint64(n), C.c_void_p(_ptr(out)), C.byref(st))
        return out, st.value

    # ---- primitives ----
    def _slab(self, name, boxes, rays):
        boxes, rays = _f32(boxes, (-1, 6)), _f32(rays, (-1, 6))
        assert len(boxes) == len(rays)
        out = np.empty(len(rays), dtype=np.float32)
        self._call(name, C.c_uint64(len(rays)), C.c_void_p(_ptr(boxes)), C.c_void_p(_ptr(rays)), C.c_void_p(_ptr(out)))
        return out

    def aabb_intersect(self, boxes, rays):
        """slab_test, the restated AABB::getIntersection."""
        return self._slab("aabb_intersect", boxes, rays)

    def slab_walk(self, boxes, rays):
        """slab_walk, the min/max variant the traversal uses."""
        return self._slab("slab_walk", boxes, rays)

    def tri_intersect(self, tri, cull, rays):
        tri, rays = _f32(tri, (-1, 9)), _f32(rays, (-1, 6))
        cull = np.ascontiguousarray(cull, dtype=np.uint8)
        assert len(tri) == len(rays) == len(cull)
        out = np.empty(len(rays), dtype=np.float32)
        self._call("tri_intersect", C.c_uint64(len(rays)), C.c_void_p(_ptr(tri)), C.c_void_p(_ptr(cull)), C.c_void_p(_ptr(rays)),
                   C.c_void_p(_ptr(out)))
        return out

    def tri_normal(self, tri, nrm, pos):
        tri, nrm, pos = _f32(tri, (-1, 9)), _f32(nrm, (-1, 9)), _f32(pos, (-1, 3))
        assert len(tri) == len(nrm) == len(pos)
        out = np.empty((len(pos), 3), dtype=np.float32)
        self._call("tri_normal", C.c_uint64(len(pos)), C.c_void_p(_ptr(tri)), C.c_void_p(_ptr(nrm)), C.c_void_p(_ptr(pos)), C.c_void_p(_ptr(out)))
        return out

    def sphere_intersect(self, sph, rays):
        sph, rays = _f32(sph, (-1, 4)), _f32(rays, (-1, 6))
        assert len(sph) == len(rays)
        out = np.empty(len(rays), dtype=np.float32)
        self._call("sphere_intersect", C.c_uint64(len(rays)), C.c_void_p(_ptr(sph)), C.c_void_p(_ptr(rays)), C.c_void_p(_ptr(out)))
        return out

    # ---- BSDF ----
    def bsdf_propagate(self, kind, one_way, rays, pos, nrm, epsilon, ior, states):
        rays, pos, nrm, ior = _f32(rays, (-1, 6)), _f32(pos, (-1, 3)), _f32(nrm, (-1, 3)), _f32(ior)
        states = np.ascontiguousarray(states, dtype=np.uint64)
        n = len(rays)
        assert len(pos) == len(nrm) == len(ior) == len(states) == n
        out_ray, fac, pd, st = np.empty((n, 6), np.float32), np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.uint64)
        self._call("bsdf_propagate", C.c_int(kind), C.c_int(one_way), C.c_uint64(n), C.c_void_p(_ptr(rays)), C.c_void_p(_ptr(pos)),
                   C.c_void_p(_ptr(nrm)), C.c_float(epsilon), C.c_void_p(_ptr(ior)), C.c_void_p(_ptr(states)), C.c_void_p(_ptr(out_ray)),
                   C.c_void_p(_ptr(fac)), C.c_void_p(_ptr(pd)), C.c_void_p(_ptr(st)))
        return out_ray, fac, pd, st

    def bsdf_spectrum(self, kind, one_way, from_dir, to_dir, nrm, light, diffuse, specular, synthetic):
        from_dir, to_dir, nrm = _f32(from_dir, (-1, 3)), _f32(to_dir, (-1, 3)), _f32(nrm, (-1, 3))
        light, diffuse, specular = _f32(light, (-1, 4)), _f32(diffuse, (-1, 4)), _f32(specular, (-1, 4))
        n = len(from_dir)
        assert len(to_dir) == len(nrm) == len(light) == len(diffuse) == len(specular) == n
        rgba, shade, p = np.empty((n, 4), np.float32), np.empty(n, np.float32), np.empty(n, np.float32)
        self._call("bsdf_spectrum", C.c_int(kind), C.c_int(one_way), C.c_uint64(n), C.c_void_p(_ptr(from_dir)), C.c_void_p(_ptr(to_dir)),
                   C.c_void_p(_ptr(nrm)), C.c_void_p(_ptr(light)), C.c_void_p(_ptr(diffuse)), C.c_void_p(_ptr(specular)),
                   C.c_int(1 if synthetic else 0), C.c_void_p(_ptr(rgba)), C.c_void_p(_ptr(shade)), C.c_void_p(_ptr(p)))
        return rgba, shade, p

    # ---- camera ----
    def _camera(self, name, cam, xy, pixel_width, pixel_height, states):
        xy = _f32(xy, (-1, 2))
        states = np.ascontiguousarray(states, dtype=np.uint64)
        n = len(xy)
        assert len(states) == n
        rays, st = np.empty((n, 6), np.float32), np.empty(n, np.uint64)
        cp = camera_params(cam)  # (oracle.CameraParams has the layout of pt_camera_params)
        self._call(name, C.byref(cp), C.c_uint64(n), C.c_void_p(_ptr(xy)), C.c_float(pixel_width), C.c_float(pixel_height),
                   C.c_void_p(_ptr(states)), C.c_void_p(_ptr(rays)), C.c_void_p(_ptr(st)))
        return rays, st

    def camera_shoot(self, cam, xy, pixel_width, pixel_height, states):
        return self._camera("camera_shoot", cam, xy, pixel_width, pixel_height, states)

    def camera_shoot_lane(self, cam, xy, pixel_width, pixel_height, states):
        return self._camera("camera_shoot_lane", cam, xy, pixel_width, pixel_height, states)

    # ---- per-pixel estimator (pt_shading.h) ----
    def max_candidates(self):
        return int(self.lib.ptu_max_candidates())

    def estimator_run(self, min_sample_count, max_sample_count, stop_bound, contrib, collected):
        """oracle.Checker.estimator_run on the device (cand_cap = PT_MAX_CANDIDATES), plus "overlap" [n][len]: estimator_safe_to_overlap
        before every consumed sample."""
        contrib = _f32(contrib)
        n, length = contrib.shape[0], contrib.shape[1]
        assert contrib.shape == (n, length, 4)
        collected = np.ascontiguousarray(collected, dtype=np.uint8)
        assert collected.shape == (n, length)
        cap = self.max_candidates()
        out = {"value": np.empty((n, 4), np.float32), "accepted": np.empty(n, np.uint8), "consumed": np.empty(n, np.int32),
               "est_f": np.empty((n, 24), np.float32), "est_i": np.empty((n, 8), np.int32),
               "cand_f": np.empty((n, cap, 8), np.float32), "cand_count": np.empty((n, cap), np.int32),
               "overlap": np.empty((n, length), np.uint8)}
        self._call("estimator_run", C.c_int(min_sample_count), C.c_int(max_sample_count), C.c_int(stop_bound), C.c_uint64(n), C.c_int(length),
                   C.c_void_p(_ptr(contrib)), C.c_void_p(_ptr(collected)), C.c_void_p(_ptr(out["value"])), C.c_void_p(_ptr(out["accepted"])),
                   C.c_void_p(_ptr(out["consumed"])), C.c_void_p(_ptr(out["est_f"])), C.c_void_p(_ptr(out["est_i"])),
                   C.c_void_p(_ptr(out["cand_f"])), C.c_void_p(_ptr(out["cand_count"])), C.c_void_p(_ptr(out["overlap"])))
        return out

    # ---- libm: device header against the same header compiled for the host: (mismatch count, first mismatching inputs, count of inputs
    # on which the host compile differs from the running C library) ----
    def libm_sincos(self, bits):
        bits = _u32(bits)
        bad, first = C.c_uint64(0), np.zeros(16, np.uint32)
        libc = C.c_uint64(0)
        self._call("libm_sincos", C.c_uint64(len(bits)), C.c_void_p(_ptr(bits)), C.byref(bad), C.c_void_p(_ptr(first)), C.byref(libc))
        return bad.value, first[:min(bad.value, 16)], libc.value

    def libm_acos(self, bits):
        bits = _u32(bits)
        bad, first = C.c_uint64(0), np.zeros(16, np.uint32)
        libc = C.c_uint64(0)
        self._call("libm_acos", C.c_uint64(len(bits)), C.c_void_p(_ptr(bits)), C.byref(bad), C.c_void_p(_ptr(first)), C.byref(libc))
        return bad.value, first[:min(bad.value, 16)], libc.value

    def libm_pow(self, x_bits, y_bits, full=True, paired=False):
        """paired: powf(x[i], y[i]); otherwise every x with every y."""
        x_bits, y_bits = _u32(x_bits), _u32(y_bits)
        assert not paired or len(x_bits) == len(y_bits)
        bad, first, libc = C.c_uint64(0), np.zeros((16, 2), np.uint32), C.c_uint64(0)
        self._call("libm_pow", C.c_int(1 if full else 0), C.c_uint64(len(x_bits)), C.c_void_p(_ptr(x_bits)), C.c_uint64(len(y_bits)),
                   C.c_void_p(_ptr(y_bits)), C.c_int(1 if paired else 0), C.byref(bad), C.c_void_p(_ptr(first)), C.byref(libc))
        return bad.value, first[:min(bad.value, 16)], libc.value


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
