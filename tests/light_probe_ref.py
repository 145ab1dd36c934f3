"""The yardstick of include/pt_light_probes.h in numpy: directions from gather_ref's engine with sinf / cosf of the running
glibc through ctypes (tests/test_libm_sincos.py pins the device's sincosf_glibc to that glibc, and the oracle calls it as well), radiance
from gather_ref.paths_from_rays (pinned to the compiled reference's getSample by tests/test_gather_cpu.py), `missed` from the first
intersect, `backfacing` from the checker's normal, and the strided sums and the lookup in float32, operation by operation in the header's
order."""
import ctypes as C
import ctypes.util

import numpy as np

from cpupathtrace_amd import binding
from tests import gather_ref

F, D, U64 = np.float32, np.float64, np.uint64
PI_F = F(np.pi)
LANES = 64
A = np.array([1.0] + [F(2.0) / F(3.0)] * 3 + [0.25] * 5, F)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = C.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [C.c_float]


def sincosf(phi):
    """glibc's sinf and cosf of every float of phi."""
    phi = np.asarray(phi, F)
    sn = np.array([_libm.sinf(float(v)) for v in phi.ravel()], F).reshape(phi.shape)
    cs = np.array([_libm.cosf(float(v)) for v in phi.ravel()], F).reshape(phi.shape)
    return sn, cs


def directions(states):
    """The direction of every engine: (d (n, 3) float32, the states behind the two draws)."""
    u1, states = gather_ref.uniform01(states)
    u2, states = gather_ref.uniform01(states)
    z = (F(1.0) - F(2.0) * u1).astype(F)
    r = np.sqrt((F(1.0) - (z * z).astype(F)).astype(F)).astype(F)
    phi = ((F(2.0) * PI_F) * u2).astype(F)
    sn, cs = sincosf(phi)
    return np.stack([(r * cs).astype(F), (r * sn).astype(F), z], axis=1).astype(F), states


def basis(d):
    """Y_0 .. Y_8 at d (n, 3): (n, 9) float32, in the header's association."""
    d = np.asarray(d, F).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        Y = [np.full(len(d), 0.282095, F), F(0.488603) * y, F(0.488603) * z, F(0.488603) * x, (F(1.092548) * x).astype(F) * y, (F(1.092548) * y).astype(F) * z,
             F(0.315392) * ((F(3.0) * (z * z).astype(F)).astype(F) - F(1.0)).astype(F), (F(1.092548) * x).astype(F) * z, F(0.546274) * ((x * x).astype(F) - (y * y).astype(F)).astype(F)]
    return np.stack([np.asarray(v, F) for v in Y], axis=1)


def samples_of(handle, flat, positions, samples, epsilon, base_seed=0, first_probe=0):
    """Every sample of every probe: (d (n, samples, 3), L (n, samples, 4), missed (n, samples) bool, backfacing (n, samples) bool,
    paths_from_vertex's dict)."""
    positions = np.asarray(positions, F).reshape(-1, 3)
    n = len(positions)
    states = gather_ref.sample_states(base_seed, n, samples, first_probe).reshape(-1)
    d, states = directions(states)
    rays = np.concatenate([np.repeat(positions, samples, axis=0), d], axis=1).astype(F)
    t, obj = handle.intersect(rays)
    missed = t < F(0.0)
    hit = np.nonzero(~missed)[0]
    backfacing = np.zeros(len(rays), bool)
    with np.errstate(all="ignore"):
        pos = (rays[hit, :3] + rays[hit, 3:] * t[hit, None]).astype(F)
        nrm = handle.normal(obj[hit], pos)[0].astype(F)
        backfacing[hit] = gather_ref._dot(nrm, rays[hit, 3:]) > F(0.0)
    rgba, _, _, info = gather_ref.paths_from_rays(handle, flat, rays, states, epsilon)
    return d.reshape(n, samples, 3), rgba.reshape(n, samples, 4), missed.reshape(n, samples), backfacing.reshape(n, samples), info


def project(d, L, missed, backfacing):
    """The records of n probes from their samples: term, the 64 strided partials in increasing s, the partials in lane order."""
    n, samples = d.shape[:2]
    out = np.zeros(n, binding.LightProbe)
    out["samples"], out["missed"], out["backfacing"] = samples, missed.sum(axis=1), backfacing.sum(axis=1)
    with np.errstate(all="ignore"):
        Y = basis(d.reshape(-1, 3)).reshape(n, samples, 9)
        term = (Y[:, :, :, None] * L[:, :, None, :3]).astype(F)  # (n, samples, 9, 3)
        partial = np.zeros((n, LANES, 9, 3), F)
        for s in range(samples):
            partial[:, s % LANES] = (partial[:, s % LANES] + term[:, s]).astype(F)
        total = np.zeros((n, 9, 3), F)
        for j in range(LANES):
            total = (total + partial[:, j]).astype(F)
        out["sh"] = ((total * (F(4.0) * PI_F)).astype(F) / F(samples)).astype(F)
    return out


def light_probes(handle, flat, positions, samples, epsilon, base_seed=0):
    """pt_light_probes_points: (n,) records of dtype binding.LightProbe."""
    d, L, missed, backfacing, _ = samples_of(handle, flat, positions, samples, epsilon, base_seed)
    return project(d, L, missed, backfacing)


def grid_positions(grid):
    """The positions of a grid's probes in index order, x fastest: origin + (float)i * step in float32."""
    grid = binding.light_probe_grid(grid, None, None)
    nx, ny, nz = (int(c) for c in grid["count"])
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    idx = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1).astype(F)
    return (grid["origin"].astype(F) + (idx * grid["step"].astype(F)).astype(F)).astype(F)


def shade(grid, probes, points, normals, max_backfacing=0.25):
    """pt_light_probes_shade: (n, 4) float32."""
    grid = binding.light_probe_grid(grid, None, None)
    probes = np.asarray(probes).reshape(-1)
    P, N = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    n = len(P)
    count = [int(c) for c in grid["count"]]
    cell, f = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            g = ((P[:, a] - grid["origin"][a]).astype(F) / grid["step"][a]).astype(F)
            g = np.fmin(np.fmax(g, F(0.0)), F(count[a] - 1)).astype(F)
            i = np.minimum(np.floor(g).astype(np.int64), count[a] - 2)
            if count[a] == 1:
                i = np.zeros(n, np.int64)
            cell.append(i)
            f.append((g - i.astype(F)).astype(F))
        excluded = probes["backfacing"].astype(F) > (F(max_backfacing) * probes["samples"].astype(F)).astype(F)
        wsum = np.zeros(n, F)
        b = np.zeros((n, 9, 3), F)
        for c in range(8):
            up = (c & 1, (c >> 1) & 1, c >> 2)
            exists = all(not (up[a] and count[a] == 1) for a in range(3))
            at = [cell[a] + (up[a] if not (up[a] and count[a] == 1) else 0) for a in range(3)]
            index = (at[2] * count[1] + at[1]) * count[0] + at[0]
            w3 = [f[a] if up[a] else (F(1.0) - f[a]).astype(F) for a in range(3)]
            w = ((w3[0] * w3[1]).astype(F) * w3[2]).astype(F)
            if not exists:
                w = np.zeros(n, F)
            w = np.where(excluded[index], F(0.0), w).astype(F)
            wsum = (wsum + w).astype(F)
            b = (b + (w[:, None, None] * probes["sh"][index]).astype(F)).astype(F)
        b = (b / wsum[:, None, None]).astype(F)
        ay = (A[None, :] * basis(N)).astype(F)
        v = np.zeros((n, 3), F)
        for k in range(9):
            v = (v + (ay[:, k, None] * b[:, k]).astype(F)).astype(F)
        out = np.zeros((n, 4), F)
        out[:, :3] = np.fmax(v, F(0.0))
        out[:, 3] = wsum
        out[wsum == F(0.0)] = 0
    return out


def assert_probes_equal(got, want, what=""):
    """Bit for bit; two NaNs of any payload compare equal (gather_ref.assert_records_equal's rule)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    for name in ("samples", "missed", "backfacing", "pad"):
        bad = got[name] != want[name]
        assert not bad.any(), "%s: %s differs for %d records, first at %s: got %s want %s" % (what, name, bad.sum(), np.argwhere(bad)[0].tolist(), got[name][bad][0], want[name][bad][0])
    assert_floats_equal(got["sh"], want["sh"], what + ": sh")


def assert_floats_equal(got, want, what=""):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    assert not bad.any(), "%s differs for %d numbers, first at %s: got %r want %r" % (what, bad.sum(), np.argwhere(bad)[0].tolist(), g[bad][0], w[bad][0])
