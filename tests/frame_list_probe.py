"""Builds and loads tests/hip/libframe_list_probe.so: the launchers of pt_frame.hip, one at a time, on caller-given work lists, statuses,
park records, tile tables and maps (tests/hip/frame_list_probe.hip).  TEST INFRASTRUCTURE ONLY; the probe is not part of
libpathtrace_hip.so.

Built like tests/denoise_probe.py: the product's hipcc and flags, one compile under a lock into a temporary file that is renamed into place,
rebuilt when the probe source, pt_frame.hip, pt_kernels.h, pt_noise.h or pt_types.h is newer than the library.  Every method takes and
returns the arrays of tests/frame_list_ref.py in their layout: lists (n, 2) uint32, records (R, 132) uint32, tiles (T, 4) int32.  An array
a launcher writes is handed over WITH its initial contents and comes back as the device left it, so what a kernel left alone shows as
well as what it wrote.  A written guard band raises GuardError, a written const input InputChangedError."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

from cpupathtrace_amd import build as product

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "frame_list_probe.hip")
LIB = os.path.join(HERE, "hip", "libframe_list_probe.so")
HEADERS = ["pt_frame.hip", "pt_kernels.h", "pt_noise.h", "pt_types.h"]
RECORD_WORDS = 132
SIZE_NAMES = ("sizeof_park_record", "sizeof_estimator", "PT_COMPACT_WORDS", "PT_NOISE_SUMMARY_WORDS", "PT_COMPACT_FIRST", "PT_COMPACT_SECOND", "PT_COMPACT_LOST",
              "PT_COMPACT_CARRIED", "PT_COMPACT_WITH_CANDIDATES", "PT_COMPACT_MIN_INVERTED", "PT_COMPACT_MAX", "PT_COMPACT_WITH_RECORD", "PT_COMPACT_WRITTEN",
              "PT_COMPACT_NO_ROOM", "PT_COMPACT_HELD", "PT_NOISE_RATED", "PT_NOISE_UNRATED", "PT_NOISE_HELD", "PT_NOISE_MAX_BITS", "PT_NOISE_FIRST_BIN",
              "sizeof_noise_rule", "sizeof_dev_options", "offsetof_stats_sample_count", "offsetof_rule_target", "offsetof_rule_floor", "offsetof_record_est",
              "PT_STREAM_UNTOUCHED", "PT_STREAM_FINISHED", "PT_STREAM_PARKED", "PT_NO_PARK", "entries_per_block", "carry_mark")


def up_to_date(lib=LIB, source=SOURCE):
    if not os.path.exists(lib):
        return False
    t = os.path.getmtime(lib)
    deps = [source, os.path.join(HERE, "hip", "guard_band.h"), os.path.abspath(__file__), os.path.abspath(product.__file__)] + [os.path.join(product.CSRC, h) for h in HEADERS]
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


class ProbeError(RuntimeError):
    pass


class GuardError(ProbeError):
    """A kernel wrote into the guard band of an array."""


class InputChangedError(ProbeError):
    """An array a launcher takes as const came back with other bytes."""


class DevOptions(C.Structure):  # PtDevOptions
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("min_sample_count", C.c_int32), ("max_sample_count", C.c_int32), ("epsilon", C.c_float),
                ("pixel_width", C.c_float), ("pixel_height", C.c_float), ("stats_sample_count", C.c_int32), ("candidate_batch_count", C.c_int32),
                ("check_sample_count", C.c_int32), ("overlap_bound", C.c_int32)]


class NoiseRule(C.Structure):  # PtNoiseRule
    _fields_ = [("opt", DevOptions), ("target", C.c_float), ("floor", C.c_float)]


def dev_options(per_batch):
    """Only stats_sample_count is read by the kernels of pt_frame.hip; the other fields get values of their own so that a kernel reading
    the wrong one shows."""
    return DevOptions(640, 480, 16, 256, 1e-4, 1.0 / 640, 1.0 / 480, int(per_batch), 3, 5, 256)


def noise_rule(per_batch, target=0.0, floor=1e-5):
    """target and floor: floats, taken to fp32 as the C ABI takes them"""
    return NoiseRule(dev_options(per_batch), float(np.float32(target)), float(np.float32(floor)))


def _u32(a, shape):
    a = np.array(a, dtype=np.uint32, order="C", copy=True)
    return a.reshape(shape)


def _p(a):
    p = C.c_void_p(a.ctypes.data if a.size else None)
    p.array = a  # (the array lives as long as the argument)
    return p


class Probe:
    def __init__(self, lib=None):
        self.lib = C.CDLL(lib or build())
        self.lib.frame_list_probe_error_string.restype = C.c_char_p
        self.guard_code = int(self.lib.frame_list_probe_guard_code())
        self.changed_code = int(self.lib.frame_list_probe_changed_code())

    def device_count(self):
        return int(self.lib.frame_list_probe_device_count())

    def sizes(self):
        out = np.zeros(64, np.uint32)
        n = int(self.lib.frame_list_probe_sizes(_p(out)))
        assert n == len(SIZE_NAMES), n
        return dict(zip(SIZE_NAMES, out[:n].tolist()))

    def _call(self, name, *args):
        rc = getattr(self.lib, "frame_list_probe_" + name)(*args)
        if rc >= self.changed_code:
            raise InputChangedError("%s: const array %d was written" % (name, rc - self.changed_code))
        if rc >= self.guard_code:
            raise GuardError("%s: the guard band of array %d was written" % (name, rc - self.guard_code))
        if rc != 0:
            raise ProbeError("%s: HIP error %d (%s)" % (name, rc, self.lib.frame_list_probe_error_string(rc).decode()))

    def compact(self, todo, status, parked, park_in, park_out, park_count, target, rule, resort, todo_out_fill=0xDEADBEEF, place_only=False):
        """pt_launch_frame_compact (place_only: the count and place kernels alone).  parked None: the launcher's `parked` is park_out, as
        the frame passes it (park_in under resort).  park_out (cap, 132) with its initial records, park_count its initial value.  Returns a
        dict: todo_out (n, 2) (entries the kernels did not write keep todo_out_fill), status, block_counts, result (16,) uint64, park_out,
        park_count, and todo, parked, park_in as they were on the device afterwards."""
        todo = _u32(todo, (-1, 2))
        n = len(todo)
        status = _u32(status, (-1,))
        alias = parked is None
        parked = np.zeros((0, RECORD_WORDS), np.uint32) if alias else _u32(parked, (-1, RECORD_WORDS))
        park_in, park_out = _u32(park_in, (-1, RECORD_WORDS)), _u32(park_out, (-1, RECORD_WORDS))
        assert not (not alias and len(parked) == 0), "an empty `parked` cannot be told from `parked is park_out`"
        # every index a kernel will form stays inside its array: checked here, before anything runs
        records_read = park_in if (alias and resort) else (park_out if alias else parked)
        assert n == 0 or todo[:, 0].max() < len(status), "a stream outside `status`"
        st = status[todo[:, 0]]
        assert (st[st >= 2] - 2 < len(records_read)).all(), "a status names a record outside `parked`"
        if target > 0:
            unclaimed = (st == 0) & (todo[:, 1] != 0xFFFFFFFF)
            assert (todo[unclaimed, 1] < len(park_in)).all(), "an entry names a record outside `park_in`"
        assert resort or park_count <= len(park_out)
        todo_out = np.full((n, 2), todo_out_fill, np.uint32)
        blocks = np.full(3 * ((n + 1023) // 1024), 0xABCD1234, np.uint32)
        result = np.full(16, 0x0123456789ABCDEF, np.uint64)
        count = np.array([park_count], np.uint32)
        todo_after, parked_after, park_in_after = np.empty_like(todo), np.empty_like(parked), np.empty_like(park_in)
        self._call("compact", C.c_int(1 if place_only else 0), _p(todo), C.c_uint32(n), _p(status), C.c_uint32(len(status)), _p(parked), C.c_uint32(len(parked)),
                   _p(todo_out), _p(blocks), _p(result), C.c_int32(target), _p(park_in), C.c_uint32(len(park_in)), _p(park_out), _p(count), C.c_uint32(len(park_out)),
                   C.byref(rule), C.c_int(1 if resort else 0), _p(todo_after), _p(parked_after), _p(park_in_after))
        return dict(todo_out=todo_out, status=status, block_counts=blocks.reshape(-1, 3), result=result, park_out=park_out, park_count=int(count[0]), todo=todo_after,
                    parked=None if alias else parked_after, park_in=park_in_after)

    @staticmethod
    def _tiles(tiles, tile_offset):
        tiles = np.array(tiles, dtype=np.int32, order="C").reshape(-1, 4)
        tile_offset = _u32(tile_offset, (-1,))
        assert len(tiles) == len(tile_offset) >= 1
        return tiles, tile_offset

    def gather(self, todo, n_parked, park, tiles, tile_offset, width, fill=-7.0):
        """-> rgba (n, 4) float32, at (n, 2) int32: (pixel, samples)"""
        todo, park = _u32(todo, (-1, 2)), _u32(park, (-1, RECORD_WORDS))
        tiles, tile_offset = self._tiles(tiles, tile_offset)
        n = len(todo)
        assert ((todo[:, 1] == 0xFFFFFFFF) | (todo[:, 1] < len(park))).all(), "an entry names a record outside `park`"
        rgba, at = np.full((n, 4), fill, np.float32), np.full((n, 2), -77, np.int32)
        self._call("gather", _p(todo), C.c_uint32(n), C.c_uint32(n_parked), _p(park), C.c_uint32(len(park)), _p(tiles), _p(tile_offset), C.c_uint32(len(tiles)),
                   C.c_int32(width), _p(rgba), _p(at))
        return rgba, at

    def preview_base(self, view, samples, cover):
        view, samples = np.array(view, np.float32, order="C").reshape(-1, 4), np.array(samples, np.int32, order="C").reshape(-1)
        cover = np.array(cover, np.uint8, order="C").reshape(-1)
        assert len(view) == len(samples) == len(cover)
        self._call("preview_base", _p(view), _p(samples), _p(cover), C.c_uint32(len(cover)))
        return view, samples

    def scatter(self, rgba, at, view, samples):
        rgba, at = np.array(rgba, np.float32, order="C").reshape(-1, 4), np.array(at, np.int32, order="C").reshape(-1, 2)
        view, samples = np.array(view, np.float32, order="C").reshape(-1, 4), np.array(samples, np.int32, order="C").reshape(-1)
        assert len(rgba) == len(at) and len(view) == len(samples)
        assert len(at) == 0 or (at[:, 0].min() >= 0 and at[:, 0].max() < len(view)), "a pixel outside the view"
        self._call("scatter", _p(rgba), _p(at), C.c_uint32(len(at)), _p(view), _p(samples), C.c_uint32(len(view)))
        return view, samples

    def rate(self, todo, park, tiles, tile_offset, width, rule):
        """-> out (n, 2) uint32: (pixel, bits of the error), summary (68,) uint32"""
        todo, park = _u32(todo, (-1, 2)), _u32(park, (-1, RECORD_WORDS))
        tiles, tile_offset = self._tiles(tiles, tile_offset)
        n = len(todo)
        assert ((todo[:, 1] == 0xFFFFFFFF) | (todo[:, 1] < len(park))).all(), "an entry names a record outside `park`"
        out, summary = np.full((n, 2), 0xDEADBEEF, np.uint32), np.full(68, 0xABCD1234, np.uint32)
        self._call("rate", _p(todo), C.c_uint32(n), _p(park), C.c_uint32(len(park)), _p(tiles), _p(tile_offset), C.c_uint32(len(tiles)), C.c_int32(width), C.byref(rule),
                   _p(out), _p(summary))
        return out, summary

    def noise_base(self, error_map, cover):
        error_map, cover = np.array(error_map, np.float32, order="C").reshape(-1), np.array(cover, np.uint8, order="C").reshape(-1)
        assert len(error_map) == len(cover)
        self._call("noise_base", _p(error_map), _p(cover), C.c_uint32(len(cover)))
        return error_map

    def noise_scatter(self, rated, error_map):
        rated, error_map = _u32(rated, (-1, 2)), np.array(error_map, np.float32, order="C").reshape(-1)
        assert len(rated) == 0 or rated[:, 0].max() < len(error_map), "a pixel outside the map"
        self._call("noise_scatter", _p(rated), C.c_uint32(len(rated)), _p(error_map), C.c_uint32(len(error_map)))
        return error_map

    def variance(self, todo, park, tiles, tile_offset, width, opt):
        """-> var (n, 4) float32, at (n,) int32"""
        todo, park = _u32(todo, (-1, 2)), _u32(park, (-1, RECORD_WORDS))
        tiles, tile_offset = self._tiles(tiles, tile_offset)
        n = len(todo)
        assert ((todo[:, 1] == 0xFFFFFFFF) | (todo[:, 1] < len(park))).all(), "an entry names a record outside `park`"
        var, at = np.full((n, 4), -7.0, np.float32), np.full(n, -77, np.int32)
        self._call("variance", _p(todo), C.c_uint32(n), _p(park), C.c_uint32(len(park)), _p(tiles), _p(tile_offset), C.c_uint32(len(tiles)), C.c_int32(width),
                   C.byref(opt), _p(var), _p(at))
        return var, at

    def variance_scatter(self, var, at, var_map):
        var, at = np.array(var, np.float32, order="C").reshape(-1, 4), np.array(at, np.int32, order="C").reshape(-1)
        var_map = np.array(var_map, np.float32, order="C").reshape(-1, 4)
        assert len(var) == len(at)
        assert len(at) == 0 or (at.min() >= 0 and at.max() < len(var_map)), "a pixel outside the map"
        self._call("variance_scatter", _p(var), _p(at), C.c_uint32(len(at)), _p(var_map), C.c_uint32(len(var_map)))
        return var_map


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
