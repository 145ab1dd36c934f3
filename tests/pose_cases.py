"""The batches of the batched mesh assembler's tests (include/pt_pose.h; tests/test_pose_batch_cpu.py on the host, tests/test_gpu_pose.py
on the device) and their expected answers, which come from tests/golden/mesh_assembly.npz alone: the compiled reference's io::loadMesh
per (mesh, transform, smooth), laid end to end in instance order."""
import os

import numpy as np

from tests import mesh_cases

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_assembly.npz")
MESH_NAMES = list(mesh_cases.MESHES)
TRANSFORM_NAMES = list(mesh_cases.TRANSFORMS)
MESH_LIST = [mesh_cases.MESHES[m] for m in MESH_NAMES]


def batch_uniform(transform):
    """18 instances: the nine meshes x smooth 0 / 1, interleaved, all under one transform.  Entries are (mesh name, transform name, smooth)."""
    return [(m, transform, s) for m in MESH_NAMES for s in (0, 1)]


def batch_rotating():
    """The same 18 instances, instance i under transform i mod 7: a table-lookup bug hides when all matrices are equal."""
    return [(m, TRANSFORM_NAMES[i % len(TRANSFORM_NAMES)], s) for i, (m, _, s) in enumerate(batch_uniform("identity"))]


def instances_of(batch):
    """(mesh index, matrix, smooth) per entry, for the probes and binding.mesh_assemble_batch."""
    return [(MESH_NAMES.index(m), mesh_cases.TRANSFORMS[t], s) for m, t, s in batch]


def expected(golden, batch):
    """(counts, positions (total, 9), normals (total, 9)) of the batch from the golden file."""
    keys = [mesh_cases.case_key(m, t, s) for m, t, s in batch]
    counts = [int(golden["count__" + k]) for k in keys]
    pos = np.concatenate([golden["pos__" + k].view(F).reshape(-1, 9) for k in keys])
    nrm = np.concatenate([golden["nrm__" + k].view(F).reshape(-1, 9) for k in keys])
    assert len(pos) == len(nrm) == sum(counts)
    return counts, pos, nrm


def total_faces(batch):
    return sum(len(mesh_cases.MESHES[m][1]) for m, _, _ in batch)


def has_empty_between_survivors(counts):
    alive = [i for i, c in enumerate(counts) if c > 0]
    return any(c == 0 and alive and alive[0] < i < alive[-1] for i, c in enumerate(counts))
