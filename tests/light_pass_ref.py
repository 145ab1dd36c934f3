"""The yardstick of include/pt_light_passes.h in numpy: gather_ref.paths_from_vertex / paths_from_rays restated so that
every term the loop adds to out_spectrum is also written down with where it came from -- the material of the emitting vertex, the material
of the registry object an emitter sample chose, or the point light -- and with the number of scatterings before it.  From that list the
accumulators of any group table, with or without the split, are made by adding the terms in the path's order; the records are
radiance_ref's strided sums, and the mix is restated twice.

The emitter a light sample chose is found by replaying the selection draw: the first of the three numbers a sample draws, lower_bound over
handle.emissive()'s CDF in float32.  The checker returns only the samples it kept; the ones it dropped are aligned by checking that every
returned position lies on the object chosen for it, and the module asserts that this alignment is unambiguous for every sample it
processes (and that the replayed engine ends where the checker's does)."""
import itertools

import numpy as np

from cpupathtrace_amd import binding
from tests import gather_ref, radiance_ref
from tests.gather_ref import D, F, U64, MAX_LIGHTS, NO_MATERIAL, _fmin_std, _len, _normalize, _propagate, _spectrum, draw, material_of_object, material_rows, uniform01

# (the records this module makes are the binding's: without the feature the module does not import)
LIGHT_PASS, EXPORTS = binding.LightPass, binding.LIGHT_PASSES_EXPORTS

ON_OBJECT = 1e-4  # a sampled position lies this close to its object (gather_cases.emitter_kinds' tolerance)
NO_KEY = -1       # the key of PT_NO_MATERIAL: group 0


def object_samples(n_emissive):
    """scene.cpp:226"""
    return min(2 + int(np.log10(n_emissive + 1)), n_emissive)


def lies_on(scene, obj, pos):
    """Does pos[i] (n, 3) lie on object `obj` (construction index) of a flat scene?  In float64, within ON_OBJECT."""
    kind = np.asarray(scene["obj_kind"])
    which = int((kind[:obj] == kind[obj]).sum())
    p = np.asarray(pos, D)
    if kind[obj] == 1:
        s = np.asarray(scene["sph"], D).reshape(-1, 4)[which]
        return np.abs(np.linalg.norm(p - s[:3], axis=-1) - s[3]) < ON_OBJECT
    a, b, c = np.asarray(scene["tri_pos"], D).reshape(-1, 3, 3)[which]
    nrm = np.cross(b - a, c - a)
    area2 = np.linalg.norm(nrm)
    nrm = nrm / area2
    off = (p - a) @ nrm
    q = p - off[..., None] * nrm
    # barycentric coordinates as signed areas
    u = np.cross(c - b, q - b) @ nrm / area2
    v = np.cross(a - c, q - c) @ nrm / area2
    w = 1.0 - u - v
    tol = ON_OBJECT / np.sqrt(area2)
    return (np.abs(off) < ON_OBJECT) & (u > -tol) & (v > -tol) & (w > -tol)


def chosen_emitters(handle, scene, states, light_pos, count, n_point_lights):
    """The registry entry of every emitter sample the checker returned for these lanes: (n, n_object_samples) int64, -1 where there is no
    such sample; and the engines behind the replayed draws.  states: the engines before sample_lights."""
    obj, cdf = handle.emissive()
    k = object_samples(len(obj))
    n = len(states)
    chosen = np.zeros((n, k), np.int64)
    st = np.array(states, U64)
    for c in range(k):
        u, st = uniform01(st)
        chosen[:, c] = np.searchsorted(np.asarray(cdf, F), u, side="left")  # std::lower_bound
        _, st = draw(st)
        _, st = draw(st)
    assert k == 0 or (chosen < len(obj)).all()
    m = np.asarray(count, np.int64) - n_point_lights
    assert (m >= 0).all() and (m <= k).all()
    resolved = np.full((n, k), -1, np.int64)
    if k == 0:
        return resolved, st
    # on[e][lane, r]: returned position r lies on registry entry e
    on = np.stack([lies_on(scene, int(o), light_pos[:, n_point_lights:n_point_lights + k]) for o in obj])
    for kept in range(1, k + 1):
        lanes = np.nonzero(m == kept)[0]
        if len(lanes) == 0:
            continue
        first, found = None, np.zeros(len(lanes), bool)
        for combo in itertools.combinations(range(k), kept):
            entries = chosen[lanes][:, list(combo)]  # (lanes, kept)
            ok = np.ones(len(lanes), bool)
            for r in range(kept):
                ok &= on[entries[:, r], lanes, r]
            if first is None:
                first = np.full((len(lanes), kept), -1, np.int64)
            new = ok & ~found
            first[new] = entries[new]
            # every other consistent alignment names the same objects: the alignment is unambiguous in what it is used for
            again = ok & found
            assert (first[again] == entries[again]).all(), "an emitter sample could lie on two chosen objects"
            found |= ok
        assert found.all(), "a returned emitter sample lies on no object the replay chose"
        resolved[lanes, :kept] = first
    return resolved, st


def terms_from_vertex(handle, flat, ray_dir, pos, nrm, material, states, epsilon, path_length0=0):
    """gather_ref.paths_from_vertex (its default mode), restated: returns (out_spectrum (n, 4), end states, terms), terms a list in the
    path's order of (lanes, key, k, rgba): the lanes that add a term at this point of the loop, where each came from -- a material index,
    NO_KEY for the default material, n_materials + j for point light j --, the scatterings before it, and the term."""
    checker, scene = handle.c, flat["scene"]
    eps = F(epsilon)
    n = len(pos)
    states = np.array(states, U64).reshape(n)
    out, spectrum = np.zeros((n, 4), F), np.ones((n, 4), F)
    contribution_unweighted = np.ones(n, F)
    divisor, bounce_pd = np.ones(n, D), np.ones(n, D)
    path_length = np.full(n, int(path_length0), np.int64)
    of_object = material_of_object(scene)
    n_materials = len(np.asarray(scene["materials"]))
    n_point_lights = len(np.asarray(scene["light_pos"]).reshape(-1, 3))
    emissive_obj, _ = handle.emissive()
    terms = []
    live = np.arange(n)
    ray_dir, pos, nrm, material = (np.array(ray_dir, F).reshape(n, 3), np.array(pos, F).reshape(n, 3), np.array(nrm, F).reshape(n, 3),
                                   np.array(material, np.uint32).reshape(n))

    def key_of(mat):
        mat = np.asarray(mat, np.uint32)
        return np.where(mat == NO_MATERIAL, NO_KEY, mat.astype(np.int64))

    with np.errstate(all="ignore"):
        while len(live) > 0:
            path_length[live] += 1
            diffuse, specular, emission, ior, bsdf, one_way = material_rows(scene, material)
            # :62-64
            w = (divisor[live] * bounce_pd[live]).astype(F)
            term = ((spectrum[live] * emission).astype(F) / w[:, None]).astype(F)
            out[live] = (out[live] + term).astype(F)
            terms.append((live.copy(), key_of(material), path_length[live] - 1, term))
            # :67-70
            sp = spectrum[live]
            contribution = (((sp[:, 0] + sp[:, 1]).astype(F) + sp[:, 2]).astype(F) / F(3.0)).astype(F)
            probability = (F(0.1) + F(0.1) * _fmin_std((contribution_unweighted[live] * contribution).astype(F), F(1.0))).astype(F)
            probability = np.where(path_length[live] <= 4, F(1.0), probability).astype(F)
            u, states[live] = uniform01(states[live])
            do_bounce = u < probability
            # :74-103
            before = states[live].copy()
            count, light_pos, light_rgba, light_pd, states[live] = handle.sample_lights(pos, before, MAX_LIGHTS)
            assert (count <= MAX_LIGHTS).all()
            entry, replayed = chosen_emitters(handle, scene, before, light_pos, count, n_point_lights)
            assert (replayed == states[live]).all(), "the replayed selection draws and the checker's engine part ways"
            for j in range(int(count.max()) if len(count) else 0):
                sel = np.nonzero(j < count)[0]
                if j < n_point_lights:
                    key = np.full(len(sel), n_materials + j, np.int64)
                else:
                    key = key_of(of_object[emissive_obj[entry[sel, j - n_point_lights]]])
                to_light = (light_pos[sel, j] - pos[sel]).astype(F)
                light_dir = _normalize(to_light)
                origin = (pos[sel] + light_dir * eps).astype(F)
                light_t, _ = handle.intersect(np.concatenate([origin, light_dir], axis=1))
                visible = (light_t < F(0.0)) | (light_t >= (_len(to_light) - eps).astype(F))
                base, shading_factor, shadow_ray_pd = _spectrum(checker, bsdf[sel], one_way[sel], ray_dir[sel], light_dir, nrm[sel], light_rgba[sel, j], diffuse[sel],
                                                                specular[sel], True)
                lanes = live[sel]
                combined = ((base * shading_factor[:, None]).astype(F) * spectrum[lanes]).astype(F)
                weight = (divisor[lanes] * bounce_pd[lanes] * light_pd[sel, j].astype(D) * shadow_ray_pd.astype(D)).astype(F)
                weighed = (combined / weight[:, None]).astype(F)
                add = visible & (shadow_ray_pd > F(0.0))
                out[lanes[add]] = (out[lanes[add]] + weighed[add]).astype(F)
                terms.append((lanes[add], key[add], path_length[lanes[add]], weighed[add]))
            # :106-114
            bounce_pd[live] = np.where(do_bounce, bounce_pd[live] * probability.astype(D), bounce_pd[live] * (F(1.0) - probability).astype(F).astype(D))
            go = np.nonzero(do_bounce & ~(bounce_pd[live] <= 1E-20))[0]
            if len(go) == 0:
                break
            live, ray_dir, pos, nrm = live[go], ray_dir[go], pos[go], nrm[go]
            diffuse, specular, ior, bsdf, one_way = diffuse[go], specular[go], ior[go], bsdf[go], one_way[go]
            # :117-136
            next_ray, ray_factor, ray_pd, states[live] = _propagate(checker, bsdf, one_way, ray_dir, pos, nrm, float(eps), ior, states[live])
            divisor[live] = divisor[live] * ray_pd.astype(D)
            divisor[live] = divisor[live] / ray_factor.astype(D)
            contribution_unweighted[live] = (contribution_unweighted[live] * ray_factor).astype(F)
            shaded, shading_factor, shading_pd = _spectrum(checker, bsdf, one_way, ray_dir, next_ray[:, 3:], nrm, spectrum[live], diffuse, specular, False)
            divisor[live] = divisor[live] * shading_pd.astype(D)
            divisor[live] = divisor[live] / shading_factor.astype(D)
            contribution_unweighted[live] = (contribution_unweighted[live] * shading_factor).astype(F)
            spectrum[live] = shaded
            # :134-138, :45-49
            t, obj = handle.intersect(next_ray)
            go = np.nonzero(~(divisor[live] <= 1E-20) & ~(t < F(0.0)))[0]
            live, next_ray, t, obj = live[go], next_ray[go], t[go], obj[go]
            if len(live) == 0:
                break
            ray_dir = next_ray[:, 3:].astype(F)
            pos = (next_ray[:, :3] + ray_dir * t[:, None]).astype(F)
            nrm = handle.normal(obj, pos)[0].astype(F)
            material = of_object[obj]
    return out, states, terms


def terms_from_rays(handle, flat, rays, states, epsilon):
    """gather_ref.paths_from_rays restated: (rgba with getSample's alpha (n, 4), collected (n,), terms with lanes that index `rays`)."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    states = np.array(states, U64).reshape(-1)
    t, obj = handle.intersect(rays)
    hit = np.nonzero(~(t < F(0.0)))[0]
    rgba = np.zeros((len(rays), 4), F)
    pos = (rays[hit, :3] + rays[hit, 3:] * t[hit, None]).astype(F)
    nrm = handle.normal(obj[hit], pos)[0].astype(F)
    out, _, terms = terms_from_vertex(handle, flat, rays[hit, 3:], pos, nrm, material_of_object(flat["scene"])[obj[hit]], states[hit], epsilon, 0)
    rgba[hit] = out
    rgba[hit, 3] = F(1.0)
    collected = np.zeros(len(rays), np.uint8)
    collected[hit] = 1
    return rgba, collected, [(hit[lanes], key, k, term) for lanes, key, k, term in terms]


def n_passes(table):
    return int(table["n_groups"]) * (3 if table["split"] else 1)


def pass_of(table, key, k):
    """p = group * C + component for terms with these keys and scatterings."""
    full = np.concatenate([np.asarray(table["material_group"], np.int64), np.asarray(table["point_light_group"], np.int64)])
    group = np.where(key == NO_KEY, 0, full[np.maximum(key, 0)])
    return group * 3 + np.minimum(k, 2) if table["split"] else group


def accumulate(terms, n, table):
    """The accumulators of n samples: (n, P, 3) float32, every one from +0, acc = acc + term in the path's order; and per sample the
    number of terms that are not all zeros (adding zeros rounds nothing)."""
    acc, count = np.zeros((n, n_passes(table), 3), F), np.zeros(n, np.int64)
    with np.errstate(all="ignore"):
        for lanes, key, k, term in terms:
            p = pass_of(table, key, k)
            acc[lanes, p] = (acc[lanes, p] + term[:, :3]).astype(F)
            count[lanes] += (term[:, :3] != 0).any(axis=1)
    return acc, count


def readd(terms, n):
    """All the terms of every sample added in the path's order into ONE accumulator: (n, 4) -- what out_spectrum holds."""
    out = np.zeros((n, 4), F)
    with np.errstate(all="ignore"):
        for lanes, _, _, term in terms:
            out[lanes] = (out[lanes] + term).astype(F)
    return out


def ray_terms(handle, flat, rays, samples, epsilon, base_seed=0):
    """Every sample of every ray of pt_light_passes_rays: (L (n, samples, 4), missed (n, samples), terms over n * samples lanes,
    sample-fastest)."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    n = len(rays)
    states = gather_ref.sample_states(base_seed, n, samples).reshape(-1)
    rgba, collected, terms = terms_from_rays(handle, flat, np.repeat(rays, samples, axis=0), states, epsilon)
    return rgba.reshape(n, samples, 4), (collected == 0).reshape(n, samples), terms


def capture_terms(handle, flat, desc, samples, epsilon, base_seed=0):
    """Every sample of every pixel of pt_light_passes_capture (radiance_ref.capture_samples' arrangement): (L, missed, outside, terms)."""
    n = int(desc.width) * int(desc.height)
    states = gather_ref.sample_states(base_seed, n, samples).reshape(-1)
    u1 = u2 = np.full(n * samples, 0.5, F)
    if desc.jitter:
        u1, states = uniform01(states)
        u2, states = uniform01(states)
    rays, outside = radiance_ref.capture_rays(desc, np.repeat(np.arange(n), samples), u1, u2)
    traced = np.nonzero(~outside)[0]
    L, missed = np.zeros((n * samples, 4), F), np.zeros(n * samples, bool)
    rgba, collected, terms = terms_from_rays(handle, flat, rays[traced], states[traced], epsilon)
    L[traced], missed[traced] = rgba, collected == 0
    return L.reshape(n, samples, 4), missed.reshape(n, samples), outside.reshape(n, samples), [(traced[lanes], key, k, term) for lanes, key, k, term in terms]


def first_samples(terms, total_samples, samples):
    """The terms of the first `samples` samples of every ray, re-indexed: sample s of ray i has its own engine, so they are the terms of
    a call with fewer samples."""
    out = []
    for lanes, key, k, term in terms:
        keep = lanes % total_samples < samples
        out.append(((lanes[keep] // total_samples) * samples + lanes[keep] % total_samples, key[keep], k[keep], term[keep]))
    return out


def pass_records(acc, samples):
    """(n * samples, P, 3) accumulators -> (n, P) records of dtype binding.LightPass by the strided sum."""
    n = len(acc) // samples
    out = np.zeros((n, acc.shape[1]), LIGHT_PASS)
    with np.errstate(all="ignore"):
        out["value"] = (radiance_ref.strided_sum(acc.reshape(n, samples, acc.shape[1], 3)) / F(samples)).astype(F)
    return out


def mix(passes, gains, total=None):
    """The header's mix, pass by pass over all rays at once."""
    gains = np.asarray(gains, F).reshape(passes.shape[-1], 3)
    out = np.zeros(passes.shape[:-1] + (4,), F)
    with np.errstate(all="ignore"):
        for p in range(passes.shape[-1]):
            out[..., :3] = (out[..., :3] + (passes["value"][..., p, :] * gains[p]).astype(F)).astype(F)
    if total is not None:
        out[..., 3] = total["value"][..., 3]
    return out


def mix_naive(passes, gains, total=None):
    """The same, one number at a time."""
    gains = np.asarray(gains, F).reshape(passes.shape[-1], 3)
    flat = passes.reshape(-1, passes.shape[-1])
    out = np.zeros((len(flat), 4), F)
    with np.errstate(all="ignore"):
        for i in range(len(flat)):
            for c in range(3):
                acc = F(0.0)
                for p in range(flat.shape[1]):
                    acc = F(acc + F(flat["value"][i, p, c] * gains[p, c]))
                out[i, c] = acc
    out = out.reshape(passes.shape[:-1] + (4,))
    if total is not None:
        out[..., 3] = total["value"][..., 3]
    return out


def sum_bound(T, samples):
    """The relative difference allowed between the sum of a ray's passes and its total: tests/test_light_passes_cpu.py derives it."""
    return 1.01 * (T + -(-samples // 64) + 65) * 2.0 ** -23


def assert_passes_equal(got, want, what=""):
    """Bit for bit; two NaNs of any payload compare equal."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert (got["pad"] == 0).all(), what
    g, w = np.ascontiguousarray(got["value"]), np.ascontiguousarray(want["value"])
    bad = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    assert not bad.any(), "%s: %d numbers differ, first at %s: got %r want %r" % (what, bad.sum(), np.argwhere(bad)[0].tolist(), g[bad][0], w[bad][0])
