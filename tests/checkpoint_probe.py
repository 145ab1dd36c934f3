"""Builds and loads the host form of tests/hip/checkpoint_probe.hip: the per-stream functions of the checkpoint kernels
(pt_checkpoint_kernels.h of the product) and the blob's writer and parser (pt_checkpoint_format.cpp), compiled with the host compiler
against tests/hip/host_checkpoint.  TEST INFRASTRUCTURE ONLY; no GPU, no hipcc."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from cpupathtrace_amd import binding
from cpupathtrace_amd import build as product
from tests import checkpoint_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "hip", "checkpoint_probe.hip")
FORMAT = os.path.join(product.CSRC, "pt_checkpoint_format.cpp")
PT_ERR_INVALID = 1


def build_host(lib):
    cxx = shutil.which("g++") or shutil.which("c++") or "g++"
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-fPIC", "-shared", "-I", os.path.join(HERE, "hip", "host_checkpoint"), "-I", product.CSRC, "-x", "c++", SOURCE, FORMAT,
           "-o", lib]
    subprocess.run(cmd, check=True)
    return lib


def _p(a):
    return None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)


class Probe:
    def __init__(self, lib):
        self.lib = C.CDLL(lib)
        self.lib.checkpoint_probe_last_error.restype = C.c_char_p
        sizes = [C.c_uint32() for _ in range(3)]
        self.lib.checkpoint_probe_sizes(*[C.byref(s) for s in sizes])
        assert [s.value for s in sizes] == [ref.HEADER.itemsize, C.sizeof(binding.CheckpointInfo), 4 * ref.RECORD_WORDS], [s.value for s in sizes]

    def error(self):
        return self.lib.checkpoint_probe_last_error().decode()

    def write(self, state, the_map, pixels, records, capacity=None):
        """The library's writer over plain arrays: (status, blob or None, needed size)."""
        h = ref.header_of(state)
        v = int(state["n_views"])
        cams = np.ascontiguousarray(state["cameras"], np.float32).reshape(v, 17)
        seeds = np.ascontiguousarray(state["seeds"], np.uint64)
        tiles = np.ascontiguousarray(state["tiles"], np.int32).reshape(-1, 4)
        the_map = np.ascontiguousarray(the_map, np.uint8)
        pixels = np.ascontiguousarray(pixels, np.float32)
        records = np.ascontiguousarray(records, np.uint32)
        header = np.frombuffer(h.tobytes(), np.uint8).copy()
        written = C.c_size_t()
        args = (_p(header), _p(cams), _p(seeds), _p(tiles), _p(the_map), _p(pixels), _p(records), C.c_uint64(records.nbytes))
        if capacity is None:
            rc = self.lib.checkpoint_probe_write(*args, None, C.c_size_t(0), C.byref(written))
            assert rc == PT_ERR_INVALID and "capacity" in self.error()
            capacity = written.value
        blob = np.zeros(max(capacity, 1), np.uint8)
        rc = self.lib.checkpoint_probe_write(*args, _p(blob), C.c_size_t(capacity), C.byref(written))
        return rc, (blob[:written.value] if rc == 0 else None), written.value

    def inspect(self, blob):
        """pt_checkpoint_inspect of the probe's own copy of the format code: (status, dict or None)."""
        b = np.ascontiguousarray(np.frombuffer(bytes(blob), np.uint8))
        info = binding.CheckpointInfo()
        rc = self.lib.pt_checkpoint_inspect(_p(b), C.c_size_t(len(b)), C.byref(info))
        return rc, (info.as_dict() if rc == 0 else None)

    def parse(self, blob, n_tiles):
        b = np.ascontiguousarray(np.frombuffer(bytes(blob), np.uint8))
        offsets = np.zeros(7, np.uint64)
        per_tile = [np.zeros(n_tiles + 1, np.uint64) for _ in range(3)]
        rc = self.lib.checkpoint_probe_parse(_p(b), C.c_size_t(len(b)), _p(offsets), *[C.c_void_p(a.ctypes.data) for a in per_tile], C.c_size_t(n_tiles))
        return rc, offsets, per_tile

    def pack(self, todo, park, n_streams, image, tiles, sizes_only=False):
        """Pack of one replica: todo (n, 2) uint32, park (R, 132) uint32, image (rows, width, 4) float32, tiles (T, 4) int32 (the
        replica's, in its order).  -> map, pixels (F, 4), records (uint32 words), tile_finished, tile_units, totals."""
        todo = np.ascontiguousarray(todo, np.uint32).reshape(-1, 2)
        park = np.ascontiguousarray(park, np.uint32).reshape(-1, ref.RECORD_WORDS)
        tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1, 4)
        image = np.ascontiguousarray(image, np.float32)
        offsets = np.concatenate([[0], np.cumsum(tiles[:, 2].astype(np.int64) * tiles[:, 3])])[:-1].astype(np.uint32)
        slot = np.zeros(max(n_streams, 1), np.uint32)
        the_map = np.zeros(max(n_streams, 1), np.uint8)
        pixels = np.zeros((max(n_streams, 1), 4), np.float32)
        records = np.zeros(max(len(park), 1) * ref.RECORD_WORDS, np.uint32)
        tile_finished, tile_units, totals = np.zeros(len(tiles), np.uint64), np.zeros(len(tiles), np.uint64), np.zeros(3, np.uint64)
        rc = self.lib.checkpoint_probe_pack(_p(todo), C.c_uint32(len(todo)), _p(park), C.c_uint32(len(park)), C.c_uint32(n_streams), _p(slot), _p(image),
                                            _p(tiles), _p(offsets), C.c_uint32(len(tiles)), C.c_int32(image.shape[1]), _p(the_map), _p(pixels),
                                            None if sizes_only else _p(records), _p(tile_finished), _p(tile_units), _p(totals))
        assert rc == 0
        return the_map[:n_streams], pixels[:int(totals[0])], records[:4 * int(totals[1])], tile_finished, tile_units, totals

    def unpack(self, the_map, trimmed):
        """Unpack of one replica: -> todo (n, 2), park (R, 132), summary (4,)."""
        the_map = np.ascontiguousarray(the_map, np.uint8)
        trimmed = np.ascontiguousarray(trimmed, np.uint32)
        n = len(the_map)
        n_rec = int(((the_map & 3) == ref.RECORD).sum())
        n_todo = int(((the_map & 3) != ref.FINISHED).sum())
        todo = np.zeros((max(n, 1), 2), np.uint32)
        park = np.full((max(n_rec, 1), ref.RECORD_WORDS), 0xDEADBEEF, np.uint32)
        summary = np.zeros(4, np.uint64)
        rc = self.lib.checkpoint_probe_unpack(_p(the_map), C.c_uint32(n), _p(trimmed), _p(todo), _p(park), _p(summary))
        assert rc == 0
        return todo[:n_todo], park[:n_rec], summary
