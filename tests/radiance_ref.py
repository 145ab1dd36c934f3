"""The yardstick of include/pt_radiance.h in numpy: engines from gather_ref.sample_states, the jitter from
gather_ref.uniform01, sinf / cosf of the running glibc through light_probe_ref.sincosf, the four capture generators in float32, operation by
operation in the header's order, radiance from gather_ref.paths_from_rays (pinned to the compiled reference's getSample by
tests/test_gather_cpu.py), and the strided sums of the record."""
import numpy as np

from cpupathtrace_amd import binding
from tests import gather_ref
from tests.light_probe_ref import sincosf

F, D = np.float32, np.float64
PI_F = F(np.pi)
LANES = 64
EQUIRECT, CUBE, FISHEYE, ORTHO = binding.CAPTURE_EQUIRECT, binding.CAPTURE_CUBE, binding.CAPTURE_FISHEYE, binding.CAPTURE_ORTHO


def basis_of(desc):
    """(origin, right, up, forward) of a binding.CaptureDesc as float32 arrays of three."""
    return tuple(np.array(list(getattr(desc, name)), F) for name in ("origin", "right", "up", "forward"))


def cube_local(face, a, b):
    """The local direction of a cube face at (a, b): the header's table, (n, 3) float32."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    one = np.ones_like(a)
    table = [(one, b, -a), (-one, b, a), (a, one, -b), (a, -one, b), (a, b, one), (-a, b, -one)]
    return np.stack(table[int(face)], axis=-1).astype(F)


def world(desc, l):
    """d[k] = ((right[k] * lx) + (up[k] * ly)) + (forward[k] * lz)"""
    _, right, up, forward = basis_of(desc)
    l = np.asarray(l, F)
    lx, ly, lz = l[..., 0, None], l[..., 1, None], l[..., 2, None]
    return (((right * lx).astype(F) + (up * ly).astype(F)).astype(F) + (forward * lz).astype(F)).astype(F)


def equirect_local(sx, sy):
    phi = ((F(2.0) * PI_F) * (sx - F(0.5)).astype(F)).astype(F)
    theta = (PI_F * sy).astype(F)
    sp, cp = sincosf(phi)
    st, ct = sincosf(theta)
    return np.stack([(st * sp).astype(F), ct, (st * cp).astype(F)], axis=-1).astype(F)


def fisheye_local(a, b, fov):
    """(local directions, outside): rr > 1 has no ray (its direction is left zero)."""
    rr = np.sqrt(((a * a).astype(F) + (b * b).astype(F)).astype(F)).astype(F)
    outside = rr > F(1.0)
    theta = (rr * (F(0.5) * F(fov))).astype(F)
    st, ct = sincosf(theta)
    with np.errstate(all="ignore"):
        l = np.stack([((st * a).astype(F) / rr).astype(F), ((st * b).astype(F) / rr).astype(F), ct], axis=-1).astype(F)
    l[rr == F(0.0)] = (0.0, 0.0, 1.0)
    l[outside] = 0.0
    return l, outside


def capture_rays(desc, pixels, u1, u2):
    """The ray of every (pixel index, u1, u2): (rays (n, 6) float32, outside (n,) bool)."""
    pixels = np.asarray(pixels, np.int64)
    u1, u2 = np.asarray(u1, F), np.asarray(u2, F)
    width, height = int(desc.width), int(desc.height)
    px, py = pixels % width, pixels // width
    origin, right, up, forward = basis_of(desc)
    o = np.repeat(origin[None], len(pixels), axis=0)
    outside = np.zeros(len(pixels), bool)
    if desc.model == CUBE:
        N = height
        face = px // N
        a = (F(2.0) * ((((px - face * N).astype(F) + u1).astype(F)) / F(N)).astype(F) - F(1.0)).astype(F)
        b = (F(1.0) - (F(2.0) * ((py.astype(F) + u2).astype(F) / F(N)).astype(F)).astype(F)).astype(F)
        l = np.zeros((len(pixels), 3), F)
        for k in range(6):
            sel = face == k
            l[sel] = cube_local(k, a[sel], b[sel])
        return np.concatenate([o, gather_ref._normalize(world(desc, l))], axis=1).astype(F), outside
    sx = ((px.astype(F) + u1).astype(F) / F(width)).astype(F)
    sy = ((py.astype(F) + u2).astype(F) / F(height)).astype(F)
    a = ((F(2.0) * sx).astype(F) - F(1.0)).astype(F)
    b = (F(1.0) - (F(2.0) * sy).astype(F)).astype(F)
    if desc.model == EQUIRECT:
        d = world(desc, equirect_local(sx, sy))
    elif desc.model == FISHEYE:
        l, outside = fisheye_local(a, b, desc.fov)
        d = world(desc, l)
        d[outside] = 0.0
    else:
        ax, by = (a * F(desc.extent[0])).astype(F), (b * F(desc.extent[1])).astype(F)
        o = ((origin + (right * ax[:, None]).astype(F)).astype(F) + (up * by[:, None]).astype(F)).astype(F)
        d = np.repeat(forward[None], len(pixels), axis=0)
    return np.concatenate([o, d], axis=1).astype(F), outside


def centre_rays(desc):
    """The rays of a capture without jitter: (rays (height * width, 6), outside)."""
    n = int(desc.width) * int(desc.height)
    half = np.full(n, 0.5, F)
    return capture_rays(desc, np.arange(n), half, half)


def ray_samples(handle, flat, rays, samples, epsilon, base_seed=0):
    """Every sample of every ray of pt_radiance_rays: (L (n, samples, 4) with getSample's alpha, missed (n, samples) bool,
    paths_from_vertex's dict)."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    n = len(rays)
    states = gather_ref.sample_states(base_seed, n, samples).reshape(-1)
    rgba, collected, _, info = gather_ref.paths_from_rays(handle, flat, np.repeat(rays, samples, axis=0), states, epsilon)
    return rgba.reshape(n, samples, 4), (collected == 0).reshape(n, samples), info


def capture_samples(handle, flat, desc, samples, epsilon, base_seed=0):
    """Every sample of every pixel of pt_radiance_capture: (L (n, samples, 4), missed, outside (n, samples) bool, the rays (n, samples, 6))."""
    n = int(desc.width) * int(desc.height)
    states = gather_ref.sample_states(base_seed, n, samples).reshape(-1)
    u1 = u2 = np.full(n * samples, 0.5, F)
    if desc.jitter:
        u1, states = gather_ref.uniform01(states)
        u2, states = gather_ref.uniform01(states)
    rays, outside = capture_rays(desc, np.repeat(np.arange(n), samples), u1, u2)
    traced = np.nonzero(~outside)[0]
    L = np.zeros((n * samples, 4), F)
    missed = np.zeros(n * samples, bool)
    rgba, collected, _, _ = gather_ref.paths_from_rays(handle, flat, rays[traced], states[traced], epsilon)
    L[traced], missed[traced] = rgba, collected == 0
    return L.reshape(n, samples, 4), missed.reshape(n, samples), outside.reshape(n, samples), rays.reshape(n, samples, 6)


def strided_sum(term):
    """(n, samples, c) -> (n, c): the 64 strided partials in increasing s, then the partials in lane order, all from +0 in float32."""
    n, samples = term.shape[:2]
    with np.errstate(all="ignore"):
        partial = np.zeros((n, LANES) + term.shape[2:], F)
        for s in range(samples):
            partial[:, s % LANES] = (partial[:, s % LANES] + term[:, s]).astype(F)
        total = np.zeros((n,) + term.shape[2:], F)
        for j in range(LANES):
            total = (total + partial[:, j]).astype(F)
    return total


def records(L, missed, outside=None):
    """The records of n rays or pixels from their samples."""
    n, samples = L.shape[:2]
    out = np.zeros(n, binding.RadianceResult)
    out["samples"], out["missed"] = samples, missed.sum(axis=1)
    if outside is not None:
        out["outside"] = outside.sum(axis=1)
    with np.errstate(all="ignore"):
        out["value"] = (strided_sum(np.asarray(L, F)) / F(samples)).astype(F)
    return out


def radiance(handle, flat, rays, samples, epsilon, base_seed=0):
    """pt_radiance_rays: (n,) records of dtype binding.RadianceResult."""
    L, missed, _ = ray_samples(handle, flat, rays, samples, epsilon, base_seed)
    return records(L, missed)


def capture(handle, flat, desc, samples, epsilon, base_seed=0):
    """pt_radiance_capture: (height, width) records."""
    L, missed, outside, _ = capture_samples(handle, flat, desc, samples, epsilon, base_seed)
    return records(L, missed, outside).reshape(int(desc.height), int(desc.width))


def assert_records_equal(got, want, what=""):
    """Bit for bit; two NaNs of any payload compare equal (gather_ref.assert_records_equal's rule)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    for name in ("samples", "missed", "outside", "pad"):
        bad = got[name] != want[name]
        assert not bad.any(), "%s: %s differs for %d records, first at %s: got %s want %s" % (what, name, bad.sum(), np.argwhere(bad)[0].tolist(), got[name][bad][0], want[name][bad][0])
    g, w = np.ascontiguousarray(got["value"]), np.ascontiguousarray(want["value"])
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    assert not bad.any(), "%s: value differs for %d numbers, first at %s: got %r want %r" % (what, bad.sum(), np.argwhere(bad)[0].tolist(), g[bad][0], w[bad][0])
