"""Linear blend skinning as include/pt_deform.h states it, restated in NumPy float32: every product and every sum is rounded to float32
on its own, in the stated order.  TEST INFRASTRUCTURE ONLY: the expected values of tests/test_deform_cases_cpu.py and
tests/test_gpu_deform.py; it shares no code with the kernel (cpupathtrace_amd/csrc/pt_deform_kernels.h).
"""
import numpy as np

F = np.float32


def bone_rows(bones):
    """(n_bones, 3, 4) float32 from (n_bones, 12), (n_bones, 3, 4) or (n_bones, 4, 4): rows 0 .. 2 of every bone's matrix."""
    b = np.asarray(bones, F)
    if b.ndim == 3 and b.shape[1:] == (4, 4):
        b = b[:, :3, :]
    return np.ascontiguousarray(b).reshape(-1, 3, 4)


def skin(rest, bone, weight, bones):
    """rest (n, 3), bone (n, K) indices, weight (n, K), bones as bone_rows takes them -> (n, 3) float32.
        acc = 0;  for k in order:  d = 0; d += B[c][0]*x; d += B[c][1]*y; d += B[c][2]*z; d += B[c][3]*1;  acc += weight * d
    No influence is skipped, nothing is normalised or divided."""
    rest = np.ascontiguousarray(rest, F).reshape(-1, 3)
    bone = np.ascontiguousarray(bone, np.uint32).reshape(len(rest), -1)
    weight = np.ascontiguousarray(weight, F).reshape(bone.shape)
    table = bone_rows(bones)
    x, y, z = rest[:, 0], rest[:, 1], rest[:, 2]
    one = np.ones(len(rest), F)
    acc = np.zeros((len(rest), 3), F)
    with np.errstate(all="ignore"):
        for k in range(bone.shape[1]):
            b = table[bone[:, k]]  # (n, 3, 4)
            for c in range(3):
                d = np.zeros(len(rest), F)
                d = d + b[:, c, 0] * x
                d = d + b[:, c, 1] * y
                d = d + b[:, c, 2] * z
                d = d + b[:, c, 3] * one
                acc[:, c] = acc[:, c] + weight[:, k] * d
    assert acc.dtype == F
    return acc
