"""The case families of the skinning tests, shared by tests/test_deform_cases_cpu.py (the kernel's source compiled for the host) and
tests/test_gpu_deform.py (the kernel): the smallest shapes at which the kernel can still go wrong.  TEST INFRASTRUCTURE ONLY.

  vertex counts   1, 255, 256, 257, 1000: the edges of a block of 256 threads, a last partial block
  influences K    1, 3, 4, 8: an odd K allows only 4-byte loads of a vertex's indices and weights, 4 and 8 take 16-byte loads
  bone counts     1, 2, the largest table staged in LDS, that + 1 (the first one read through the cache), one several times beyond
  weights         a partition of 1; all zero; negative and > 1; a partition with denormal entries
  poison          one bone with a NaN entry and one with infinite entries, referenced with ordinary and with ZERO weights
"""
import itertools

import numpy as np

F = np.float32
LDS_BONES = 256  # PT_SKIN_LDS_BONES of cpupathtrace_amd/csrc/pt_skin.h (tests/test_deform_cases_cpu.py holds the two equal)
VERTEX_COUNTS = (1, 255, 256, 257, 1000)
INFLUENCES = (1, 3, 4, 8)
BONE_COUNTS = (1, 2, LDS_BONES, LDS_BONES + 1, 5 * LDS_BONES + 3)
WEIGHT_KINDS = ("partition", "zero", "wild", "denormal")
DENORMAL = F(1.0e-41)
assert 0 < DENORMAL < np.finfo(F).tiny


def rest_vertices(n, seed=1):
    """n points of the stand-in mesh's neighbourhood (around (0, 50, 0), y > 0)."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-40.0, 40.0, (n, 3)) + np.array([0.0, 50.0, 0.0])).astype(F)


def bone_matrices(n_bones, seed=2, scale=0.2, shift=5.0):
    """(n_bones, 3, 4): rows 0 .. 2 of affine matrices near the identity."""
    rng = np.random.default_rng(seed)
    m = np.zeros((n_bones, 3, 4))
    m[:, :, :3] = np.eye(3) + rng.uniform(-scale, scale, (n_bones, 3, 3))
    m[:, :, 3] = rng.uniform(-shift, shift, (n_bones, 3))
    return m.astype(F)


def rig(n_vertices, n_bones, k, kind, seed=3):
    """(bone (n, K) uint32, weight (n, K) float32).  The first and the last bone are both used."""
    rng = np.random.default_rng(seed + 1000 * k + n_bones)
    bone = rng.integers(0, n_bones, (n_vertices, k)).astype(np.uint32)
    bone[0, 0] = n_bones - 1
    bone[-1, -1] = 0
    if kind == "zero":
        weight = np.zeros((n_vertices, k))
    elif kind == "wild":
        weight = rng.uniform(-2.0, 3.0, (n_vertices, k))
    else:
        weight = rng.dirichlet(np.ones(k), n_vertices)
    weight = weight.astype(F)
    if kind == "denormal":
        weight[::3, 0] = DENORMAL
    return bone, weight


def case(n_vertices, k, n_bones, kind):
    bone, weight = rig(n_vertices, n_bones, k, kind)
    return {"rest": rest_vertices(n_vertices), "bone": bone, "weight": weight, "bones": bone_matrices(n_bones)}


def all_cases():
    """(name, case) over the full product of the families."""
    for n, k, b, kind in itertools.product(VERTEX_COUNTS, INFLUENCES, BONE_COUNTS, WEIGHT_KINDS):
        yield "%d vertices, K=%d, %d bones, %s weights" % (n, k, b, kind), case(n, k, b, kind)


NAN_BONE, INF_BONE = 1, 2


def poison(bones, cancelling=True):
    """A copy of the table with a NaN entry in bone NAN_BONE and infinite entries in bone INF_BONE.  cancelling: every row of INF_BONE has
    +inf in column 1 and -inf in column 3, so that a vertex with y > 0 becomes NaN in every component whatever its weight (inf - inf);
    otherwise one +inf entry, which leaves infinite coordinates."""
    out = np.array(bones, F)
    assert len(out) > max(NAN_BONE, INF_BONE)
    out[NAN_BONE, 1, 2] = np.nan
    if cancelling:
        out[INF_BONE, :, 1] = np.inf
        out[INF_BONE, :, 3] = -np.inf
    else:
        out[INF_BONE, 0, 0] = np.inf
    return out


def poisoned_rig(n_vertices, n_bones, k, rest=None, seed=4):
    """A partition rig over the healthy bones in which every 4th vertex references NAN_BONE with an ordinary weight, the next one
    INF_BONE with an ordinary weight, the next one NAN_BONE with weight ZERO and the next one INF_BONE with weight ZERO, in its last
    influence.  Returns (bone, weight, poisoned): poisoned marks the vertices that reference a poisoned bone -- all of them are NaN
    under poison(cancelling=True), the zero weights included (0 * inf and 0 * NaN are NaN)."""
    assert n_bones > 3
    rng = np.random.default_rng(seed + k)
    bone = (3 + rng.integers(0, n_bones - 3, (n_vertices, k))).astype(np.uint32)
    weight = rng.dirichlet(np.ones(k), n_vertices).astype(F)
    poisoned = np.zeros(n_vertices, bool)
    for offset, (which, zero) in enumerate(((NAN_BONE, False), (INF_BONE, False), (NAN_BONE, True), (INF_BONE, True))):
        rows = np.arange(offset, n_vertices, 8)  # (every 8th, so that half of the vertices stay healthy)
        bone[rows, k - 1] = which
        if zero:
            weight[rows, k - 1] = 0
        poisoned[rows] = True
    return bone, weight, poisoned


def truncated(vertices, faces, n):
    """The first n vertices of an indexed mesh and the faces that use no other."""
    f = np.asarray(faces)
    return np.ascontiguousarray(vertices[:n]), np.ascontiguousarray(f[(f < n).all(axis=1)])
