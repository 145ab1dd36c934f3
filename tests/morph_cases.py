"""The case families of the blend-shape tests, shared by tests/test_morph_cases_cpu.py (the kernel's source compiled for the host) and
tests/test_gpu_morph.py (the kernel): the smallest shapes at which the kernel can still go wrong.  TEST INFRASTRUCTURE ONLY.

  vertex counts   1, 255, 256, 257, 1000: the edges of a block of 256 threads, a last partial block
  target counts   1, 2, 3, the most weights staged in LDS, that + 1 (the first set whose weights are read through the cache)
  target forms    "dense":  every target dense (of many targets the first and the last; the others sparse)
                  "sparse": every target sparse, about 5 % of the vertices each; one vertex is listed by EVERY target (a row of length T),
                            the vertex before it by none (length 0) and the vertex behind it by the last target only (length 1): the three
                            stand next to each other in one wavefront
                  "mixed":  dense and sparse targets and one EMPTY target (of a single target: the empty one alone)
  weights         all zero; a partition of 1; negative and > 1; a partition with denormal entries
  poison          one target with a NaN and one with an infinite delta, referenced with an ordinary and with a ZERO weight
  signed zero     rest vertices of -0.0 that a zero-weight target lists, and that no target lists
  skin            K = 0 (the morph alone), 1, 4, 8, with 2 and 257 bones (the table in LDS, and read through the cache)
"""
import itertools

import numpy as np

from tests import deform_cases

F = np.float32
LDS_TARGETS = 2048  # PT_MORPH_LDS_TARGETS of cpupathtrace_amd/csrc/pt_morph_skin.h (tests/test_morph_cases_cpu.py holds the two equal)
VERTEX_COUNTS = deform_cases.VERTEX_COUNTS
TARGET_COUNTS = (1, 2, 3, LDS_TARGETS, LDS_TARGETS + 1)
FORMS = ("dense", "sparse", "mixed")
WEIGHT_KINDS = ("zero", "partition", "wild", "denormal")
SKINS = ((0, 0), (1, 2), (4, 2), (8, 2), (1, 257), (4, 257), (8, 257))  # (K, bones)
DENORMAL = deform_cases.DENORMAL


def row_vertices(n_vertices):
    """(none, every, last): the vertex no target of a "sparse" set lists, the one every target lists and the one only the last target
    lists -- neighbours inside one wavefront where the mesh has three vertices to spare."""
    every = min(n_vertices - 1, 70)
    return (every - 1 if every >= 1 else None), every, (every + 1 if every + 1 < n_vertices else None)


def _deltas(rng, k):
    return rng.uniform(-3.0, 3.0, (k, 3)).astype(F)


def _sparse(rng, n_vertices, t, n_targets):
    none, every, last = row_vertices(n_vertices)
    listed = rng.random(n_vertices) < 0.05
    listed[every] = True
    if none is not None:
        listed[none] = False
    if last is not None:
        listed[last] = t == n_targets - 1
    idx = np.flatnonzero(listed).astype(np.uint32)
    return idx, _deltas(rng, len(idx))


def target_set(n_vertices, n_targets, form, seed=1):
    """A list of (indices or None, deltas): see the module's text."""
    rng = np.random.default_rng(seed + 7 * n_vertices + 13 * n_targets)
    out = []
    for t in range(n_targets):
        if form == "dense":
            dense = n_targets <= 3 or t in (0, n_targets - 1)
        elif form == "sparse":
            dense = False
        else:
            if t == (n_targets // 2 if n_targets >= 3 else 0):
                out.append((np.zeros(0, np.uint32), np.zeros((0, 3), F)))  # the empty target
                continue
            dense = (len(out) - (t > n_targets // 2)) % 2 == 0  # the others in turn: dense, sparse, dense ..
        out.append((None, _deltas(rng, n_vertices)) if dense else _sparse(rng, n_vertices, t, n_targets))
    return out


def weights(n_targets, kind, seed=5):
    rng = np.random.default_rng(seed + n_targets)
    if kind == "zero":
        w = np.zeros(n_targets)
    elif kind == "wild":
        w = rng.uniform(-2.0, 3.0, n_targets)
    else:
        w = rng.dirichlet(np.ones(n_targets))
    w = w.astype(F)
    if kind == "denormal":
        w[::3] = DENORMAL
    return w


def skin(n_vertices, k, n_bones):
    """None for K = 0, else (bone, weight, bones) of tests/deform_cases.py's partition rig."""
    if k == 0:
        return None
    bone, weight = deform_cases.rig(n_vertices, n_bones, k, "partition")
    return bone, weight, deform_cases.bone_matrices(n_bones)


def all_sets():
    """(name, n_vertices, rest, targets) over vertices x targets x forms."""
    for n, t, form in itertools.product(VERTEX_COUNTS, TARGET_COUNTS, FORMS):
        yield "%d vertices, %d %s targets" % (n, t, form), n, deform_cases.rest_vertices(n), target_set(n, t, form)


NAN_TARGET, INF_TARGET = 1, 2


def poisoned_set(n_vertices, n_targets=5, seed=9):
    """Dense healthy targets but for NAN_TARGET and INF_TARGET, sparse: vertices 0, 8, 16 .. are listed by NAN_TARGET (a NaN in its y
    delta), vertices 1, 9, .. by INF_TARGET (+inf in x).  Returns (targets, poisoned): poisoned marks the vertices either lists -- all
    of them are NaN or infinite under an ordinary weight, and NaN in the poisoned component under a ZERO weight (0 * inf, 0 * NaN)."""
    rng = np.random.default_rng(seed)
    targets = [(None, _deltas(rng, n_vertices)) for _ in range(n_targets)]
    poisoned = np.zeros(n_vertices, bool)
    for which, offset, (component, value) in ((NAN_TARGET, 0, (1, np.nan)), (INF_TARGET, 1, (0, np.inf))):
        idx = np.arange(offset, n_vertices, 8).astype(np.uint32)
        d = _deltas(rng, len(idx))
        d[:, component] = value
        targets[which] = (idx, d)
        poisoned[idx] = True
    return targets, poisoned


def signed_zero_case(n_vertices=257):
    """(rest, targets, weights, listed): every rest component is -0.0; target 0 (weight 0) lists the even vertices with ordinary deltas,
    target 1 (weight 0 as well) is empty.  Listed vertices become +0.0 (-0.0 + 0 * d), the others stay -0.0."""
    rest = np.full((n_vertices, 3), -0.0, F)
    idx = np.arange(0, n_vertices, 2).astype(np.uint32)
    targets = [(idx, np.full((len(idx), 3), 1.5, F)), (np.zeros(0, np.uint32), np.zeros((0, 3), F))]
    listed = np.zeros(n_vertices, bool)
    listed[idx] = True
    return rest, targets, np.zeros(2, F), listed
