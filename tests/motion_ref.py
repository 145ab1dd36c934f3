"""Host restatement of the motion plane of pt_render_features_motion (include/pt_motion.h) from the CPU oracle: the
feature rays of tests/denoise_ref.py, their closest hits by the oracle's intersect on a FLAT scene (the description's objects, then the
instances' surviving triangles as objects first .. first + count - 1), the oracle's normals, and the per-instance table of
pt_motion_table.  Every operation is fp32 in the kernel's order, so the device must agree bit for bit.  Also: numpy float64 answers for
pt_motion_table itself."""
import numpy as np

from tests import denoise_ref as dr

F = np.float32
STATIC, MOVED, NONE = 0, 1, 2


def _dot3(row, v):
    return (row[0] * v[:, 0] + row[1] * v[:, 1]) + row[2] * v[:, 2]


def flat_scene(description, pos, nrm, cull, material):
    """`description` (a scene dict without instances, every triangle with explicit normals) with the instances' triangles appended as
    objects len(obj_kind) ..."""
    sc = dict(description)
    sc.pop("instances", None)
    sc.pop("meshes", None)
    n = len(pos)
    base_nrm = description.get("tri_nrm")
    assert base_nrm is not None
    sc["obj_kind"] = np.concatenate([np.asarray(description["obj_kind"], np.uint8), np.zeros(n, np.uint8)])
    sc["tri_pos"] = np.concatenate([np.asarray(description["tri_pos"], F).reshape(-1, 9), np.asarray(pos, F).reshape(-1, 9)])
    sc["tri_nrm"] = np.concatenate([np.asarray(base_nrm, F).reshape(-1, 9), np.asarray(nrm, F).reshape(-1, 9)])
    sc["tri_cull"] = np.concatenate([np.asarray(description["tri_cull"], np.uint8), np.asarray(cull, np.uint8)])
    sc["tri_material"] = np.concatenate([np.asarray(description["tri_material"], np.uint32), np.asarray(material, np.uint32)])
    return sc


def host_motion(checker, scene, cam, width, height, first, count, kind, back, normal):
    """((H, W, 2, 4) float32 motion, counts): per pixel the sum in ray order, then * 0.25, of [previous position, moved], [previous normal,
    no previous position] over the 4 feature rays; counts of the rays by what they hit (hit, description triangles, spheres, static /
    moved / none instances)."""
    handle = checker.scene_create(scene)
    okind = np.asarray(scene["obj_kind"])
    n_pix = width * height
    acc = np.zeros((2, n_pix, 4), F)
    counts = {"hit": 0, "description": 0, "sphere": 0, "static": 0, "moved": 0, "none": 0}
    live = [i for i in range(len(first)) if count[i] > 0]  # an instance without survivors shares its first with a neighbour: never selected
    try:
        for rays in dr.feature_rays(checker, cam, width, height):
            t, obj = handle.intersect(rays)
            hit = (obj >= 0) & (t >= 0)
            idx = np.nonzero(hit)[0]
            th = t[idx]
            pos = (rays[idx, :3] + rays[idx, 3:] * th[:, None]).astype(F)
            o = obj[idx].astype(np.int64)
            nrm, _ = handle.normal(o, pos)
            pp, pn = pos.copy(), nrm.astype(F).copy()
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
                    len2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        inv = (F(1.0) / np.sqrt(len2)).astype(F)
                        pn[sel] = np.where((len2 > 0)[:, None], v * inv[:, None], F(0.0))
                    moved[sel] = 1
                    counts["moved"] += int(sel.sum())
                elif kind[i] == NONE:
                    pp[sel], pn[sel], moved[sel], none[sel] = 0, 0, 1, 1
                    counts["none"] += int(sel.sum())
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


# ---- pt_motion_table in numpy float64 ------------------------------------------------------------------------------------------------------

def classify(c, p):
    """The kind of one instance by the contract's words, on fp32 matrices (4, 4)."""
    c, p = np.asarray(c, F), np.asarray(p, F)
    if c.tobytes() == p.tobytes():
        return STATIC
    if not (np.isfinite(c).all() and np.isfinite(p).all()):
        return NONE
    last = np.array([0, 0, 0, 1], F)
    if not ((c[3] == last).all() and (p[3] == last).all()):
        return NONE
    for m in (c, p):
        d = np.linalg.det(m[:3, :3].astype(np.float64))
        if not np.isfinite(d) or d == 0:
            return NONE
    return MOVED


def table64(c, p):
    """(back (3, 4), normal (3, 3)) of a moved instance in float64 (numpy's inverse), not rounded."""
    c, p = np.asarray(c, np.float64), np.asarray(p, np.float64)
    a, b = c[:3, :3], p[:3, :3]
    l = b @ np.linalg.inv(a)
    back = np.concatenate([l, (p[:3, 3] - l @ c[:3, 3])[:, None]], axis=1)
    return back, (a @ np.linalg.inv(b)).T
