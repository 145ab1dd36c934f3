"""Host restatement of the motion plane of pt_render_features_motion_marked (include/pt_motion_shapes.h), built from
tests/motion_ref.py: the feature rays, the oracle's closest hits and normals on the FLAT scene, pt_motion_table's kinds for instances
whose mesh kept its shape, and for an instance of kind DEFORMED the contract's formulas in numpy float32, operation for operation, so the
device must agree bit for bit.  The face a surviving triangle came from is found by a numpy restatement of the assembler's transform and
keep test (pt_mesh_batch_kernels.h: kb_transform, kb_face_keep), not asked of the device."""
import numpy as np

from tests import denoise_ref as dr
from tests.motion_ref import MOVED, NONE, STATIC, _dot3, flat_scene  # noqa: F401 (flat_scene: for the callers)

F = np.float32
DEFORMED = 3


def _dot_from_zero(a, b):
    """dot() of detail/linear.h: from zero, in index order, every product and sum rounded to float."""
    d = F(0.0) + a[..., 0] * b[..., 0]
    d = d + a[..., 1] * b[..., 1]
    return (d + a[..., 2] * b[..., 2]).astype(F)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]],
                    axis=-1).astype(F)


def _len2(v):
    """motion_dot3(v, v): (x x + y y) + z z"""
    return ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(F)


def transform(matrix, vertices):
    """kb_transform: M * (x, y, z, 1) row by row from zero, then * (1 / w)."""
    m, v = np.asarray(matrix, F).reshape(4, 4), np.asarray(vertices, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        h = []
        for r in range(4):
            d = F(0.0) + m[r, 0] * v[:, 0]
            d = d + m[r, 1] * v[:, 1]
            d = d + m[r, 2] * v[:, 2]
            h.append((d + m[r, 3] * F(1.0)).astype(F))
        inv = (F(1.0) / h[3]).astype(F)
        return np.stack([h[0] * inv, h[1] * inv, h[2] * inv], axis=1).astype(F)


def kept_faces(matrix, vertices, faces):
    """kb_face_keep on the transformed vertices: the indices of the faces that stay, ascending."""
    tv = transform(matrix, vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    inside = ((f >= 0) & (f < len(tv))).all(axis=1)
    g = np.where(inside[:, None], f, 0)
    with np.errstate(all="ignore"):
        a, b, c = tv[g[:, 0]], tv[g[:, 1]], tv[g[:, 2]]
        ab, ac, bc = (b - a).astype(F), (c - a).astype(F), (c - b).astype(F)
        cr = _cross(ab, ac)
        keep = inside & (_dot_from_zero(ab, ab) > 0) & (_dot_from_zero(ac, ac) > 0) & (_dot_from_zero(bc, bc) > 0) & ~(_dot_from_zero(cr, cr) <= 0)
    return np.nonzero(keep)[0]


def face_table(instances):
    """instances: [(matrix, current vertices, faces)] in instance order.  (face_of, face_first, counts): for every surviving triangle the
    scene-wide face it came from, the scene-wide number of every instance's face 0, and the survivors per instance."""
    face_of, face_first, counts, base = [], [], [], 0
    for matrix, vertices, faces in instances:
        k = kept_faces(matrix, vertices, faces)
        face_of.append(base + k)
        face_first.append(base)
        counts.append(len(k))
        base += len(np.asarray(faces).reshape(-1, 3))
    return np.concatenate(face_of).astype(np.uint32) if face_of else np.zeros(0, np.uint32), face_first, counts


def shape_motion(tri_pos, pos, nrm, faces, marked_vertices, marked_matrix):
    """The contract's DEFORMED arithmetic for n hits: tri_pos (n, 9) the hit triangles' corners, pos / nrm (n, 3) the hits and their
    shading normals, faces (n, 3) the vertex indices of the faces they came from.  Returns (pp, pn, none)."""
    tri_pos, pos, nrm = np.asarray(tri_pos, F).reshape(-1, 9), np.asarray(pos, F), np.asarray(nrm, F)
    q = transform(marked_matrix, marked_vertices)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        qa, qb, qc = q[f[:, 0]], q[f[:, 1]], q[f[:, 2]]
        a = tri_pos[:, 0:3]
        ab, ac = (tri_pos[:, 3:6] - a).astype(F), (tri_pos[:, 6:9] - a).astype(F)  # the record's edges (Triangle::Triangle)
        ap = (pos - a).astype(F)
        d00, d01, d11 = _dot_from_zero(ab, ab), _dot_from_zero(ab, ac), _dot_from_zero(ac, ac)
        d20, d21 = _dot_from_zero(ap, ab), _dot_from_zero(ap, ac)
        inv_d = (F(1.0) / (d00 * d11 - d01 * d01)).astype(F)
        v = ((d11 * d20 - d01 * d21) * inv_d).astype(F)
        w = ((d00 * d21 - d01 * d20) * inv_d).astype(F)
        u = (F(1.0) - v - w).astype(F)
        pp = ((qa * u[:, None] + qb * v[:, None]) + qc * w[:, None]).astype(F)
        cp, cc = _cross((qb - qa).astype(F), (qc - qa).astype(F)), _cross(ab, ac)
        lp, lc = _len2(cp), _len2(cc)
        none = ~(lp > 0) | ~(lc > 0) | ~np.isfinite(pp).all(axis=1)
        ngp = (cp * (F(1.0) / np.sqrt(lp)).astype(F)[:, None]).astype(F)
        ng = (cc * (F(1.0) / np.sqrt(lc)).astype(F)[:, None]).astype(F)
        vv = ((nrm - ng) + ngp).astype(F)
        len2 = _len2(vv)
        inv = (F(1.0) / np.sqrt(len2)).astype(F)
        pn = np.where((len2 > 0)[:, None], vv * inv[:, None], F(0.0)).astype(F)
    pp[none], pn[none] = 0, 0
    return pp, pn, none


def host_motion(checker, scene, cam, width, height, first, count, kind, back, normal, inst_pos, shapes):
    """tests/motion_ref.py's host_motion with the fourth kind.  inst_pos: (instance triangles, 9), the positions of the instances'
    triangles in object order; shapes[i] for an instance of kind DEFORMED: (faces (n_faces, 3), marked vertices, marked matrix,
    local face (count[i],): the face of the instance's mesh every one of its triangles came from).  counts also has "deformed" (rays on
    such an instance) and "no previous" (those of them without a previous position)."""
    handle = checker.scene_create(scene)
    okind = np.asarray(scene["obj_kind"])
    n_pix = width * height
    acc = np.zeros((2, n_pix, 4), F)
    counts = {"hit": 0, "description": 0, "sphere": 0, "static": 0, "moved": 0, "none": 0, "deformed": 0, "no previous": 0}
    live = [i for i in range(len(first)) if count[i] > 0]
    first_instance_object = min([int(first[i]) for i in live], default=0)
    inst_pos = np.asarray(inst_pos, F).reshape(-1, 9)
    try:
        for rays in dr.feature_rays(checker, cam, width, height):
            t, obj = handle.intersect(rays)
            hit = (obj >= 0) & (t >= 0)
            idx = np.nonzero(hit)[0]
            th = t[idx]
            pos = (rays[idx, :3] + rays[idx, 3:] * th[:, None]).astype(F)
            o = obj[idx].astype(np.int64)
            nrm, _ = handle.normal(o, pos)
            nrm = nrm.astype(F)
            pp, pn = pos.copy(), nrm.copy()
            moved, none = np.zeros(len(idx), F), np.zeros(len(idx), F)
            inst = np.full(len(idx), -1)
            for i in live:
                inst[(o >= int(first[i])) & (o < int(first[i]) + int(count[i]))] = i
            counts["hit"] += len(idx)
            counts["sphere"] += int((okind[o] != 0).sum())
            counts["description"] += int(((okind[o] == 0) & (inst < 0)).sum())
            for i in live:
                sel = inst == i
                if kind[i] == MOVED:
                    b, m = np.asarray(back[i], F), np.asarray(normal[i], F)
                    P, N = pos[sel], nrm[sel]
                    for k in range(3):
                        pp[sel, k] = _dot3(b[k], P) + b[k, 3]
                    v = np.stack([_dot3(m[k], N) for k in range(3)], axis=1).astype(F)
                    len2 = _len2(v)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        inv = (F(1.0) / np.sqrt(len2)).astype(F)
                        pn[sel] = np.where((len2 > 0)[:, None], v * inv[:, None], F(0.0))
                    moved[sel] = 1
                    counts["moved"] += int(sel.sum())
                elif kind[i] == NONE:
                    pp[sel], pn[sel], moved[sel], none[sel] = 0, 0, 1, 1
                    counts["none"] += int(sel.sum())
                elif kind[i] == DEFORMED:
                    faces, marked_vertices, marked_matrix, local_face = shapes[i]
                    tri = o[sel] - first_instance_object
                    hit_faces = np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(local_face, np.int64)[o[sel] - int(first[i])]]
                    pp[sel], pn[sel], gone = shape_motion(inst_pos[tri], pos[sel], nrm[sel], hit_faces, marked_vertices, marked_matrix)
                    moved[sel] = 1
                    none[sel] = gone
                    counts["deformed"] += int(sel.sum())
                    counts["no previous"] += int(gone.sum())
                else:
                    counts["static"] += int(sel.sum())
            v = np.zeros((2, n_pix, 4), F)
            v[0, idx, :3], v[0, idx, 3] = pp, moved
            v[1, idx, :3], v[1, idx, 3] = pn, none
            acc = (acc + v).astype(F)
    finally:
        handle.close()
    out = (acc * F(0.25)).astype(F)
    return np.ascontiguousarray(out.transpose(1, 0, 2).reshape(height, width, 2, 4)), counts
