#!/usr/bin/env python3
"""Generate tests/golden/mesh_assembly.npz from the compiled, unmodified reference's io::loadMesh (ref_load_mesh of oracle/_ref/libptref.so).

Run in the build container only (it needs the reference to build oracle/_ref):

    python tests/golden/make_mesh_golden.py

For every mesh x transform x smooth flag of tests/mesh_cases.py the file holds the INPUTS (vertices, faces, matrix, flag) and the
OUTPUTS the reference's loader produced for the mesh's OBJ text: the number of surviving triangles, their positions and normals.
Nothing of the reference's source text is stored.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
from tests import mesh_cases  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mesh_assembly.npz")


def main():
    ref = oracle.Checker("ref").lib
    arrays = {}
    for name, (v, f) in mesh_cases.MESHES.items():
        arrays["vertices__" + name], arrays["faces__" + name] = v, f
    for name, m in mesh_cases.TRANSFORMS.items():
        arrays["matrix__" + name] = m
    for mesh, transform, smooth in mesh_cases.CASES:
        v, f = mesh_cases.MESHES[mesh]
        n, pos, nrm = mesh_cases.load_mesh(ref, "ref_", v, f, mesh_cases.TRANSFORMS[transform], smooth)
        key = mesh_cases.case_key(mesh, transform, smooth)
        arrays["count__" + key] = np.int64(n)
        arrays["pos__" + key] = pos.view(np.uint32)  # bits: NaN payloads stay what the reference wrote
        arrays["nrm__" + key] = nrm.view(np.uint32)
        if mesh == "degenerate":
            print("%-44s kept %d of %d" % (key, n, len(f)))
    np.savez_compressed(OUT, **arrays)
    print("%s %.1f KiB" % (os.path.basename(OUT), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
