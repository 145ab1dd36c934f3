// pt_sample_walk.h -- one lane's path sample, from a given start to its end: the loop that light gathered at points
// (pt_gather_kernels.h), the light probes (pt_light_probe_kernels.h), radiance along free rays (pt_radiance_kernels.h) and the light-group
// passes (pt_light_pass_kernels.h) all run.  Included by exactly one translation unit, pt_walks.hip, ahead of those four and behind
// pt_trace.h, bind_lane and dispatch_route.
//
// The loop is getSample (worker.cpp:37-138) restated for one lane.  A lane runs its sample's walks one after another on its Tracer through
// ONE tr.start / tr.step site (pt_follow_kernel's arrangement): a turn of the loop advances the lane's vertex -- light sample by light
// sample, then the roulette and the bounce -- until it has a ray to trace, and traces it; lanes on a shadow walk and lanes on a closest
// walk step together, the destination word tells them apart.  The vertex is the path kernel's (pt_path.hip), operation for operation: the
// emission term and the two double-precision weights are formed as there, a light sample whose weight is +-0 in all three channels or
// whose threshold is not positive needs no ray, and a shadow walk is Tracer::begin's with the threshold in the origin's w.
//
// What a kernel chooses, all of it at compile time: where the sample starts (AT_VERTEX), whether it bounces (BOUNCES), and a sink whose
// hooks see the two events that set a kernel's flags and the three places where a term is added to out_spectrum.  A hook that does
// nothing leaves no instruction behind.
#ifndef PT_SAMPLE_WALK_H
#define PT_SAMPLE_WALK_H

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"

namespace {

using namespace ptd;

// RandomEngine(seed), base.h:26
PT_D uint64_t gather_engine(uint64_t seed) {
    return seed ^ (~seed << 32);
}

// The scene's root box as Tracer::start takes it.  (pt_gather_kernels.h fills its boxes by hand: with this helper the compiler scheduled
// the occlusion kind and pt_gather_frame_points_kernel differently -- pt_walks.hip's head has the same finding --, and those are to stay.)
PT_D void scene_root(const PtDevScene &sc, RootBox &root) {
    root.ref = sc.root_ref;
    for(int k = 0; k < 3; k++) {
        root.lo[k] = sc.root_lo[k];
        root.hi[k] = sc.root_hi[k];
    }
}

// sample_emissive (pt_shading.h) that also hands out the registry index it chose.  The selection -- the first of the sample's three
// numbers, std::lower_bound over the CDF -- is replayed on a COPY of the engine; the sample itself is then sample_emissive's, untouched:
// every draw and every number are its own by construction.
template<typename Tables>
PT_D bool sample_emissive_indexed(const PtDevScene &sc, const Tables &tb, V3 pos, uint64_t &rng, V3 &light_pos, C4 &spectrum, float &pd, uint32_t &object_index) {
    uint64_t peek = rng;
    const float r = rng_uniform01(peek);
    int lo = 0, n = (int)sc.n_emis;
    while(n > 0) {
        const int half = n >> 1;
        if(tb.cdf(lo + half) < r) {
            lo = lo + half + 1;
            n = n - half - 1;
        }
        else {
            n = half;
        }
    }
    object_index = (uint32_t)lo;
    return sample_emissive(sc, tb, pos, rng, light_pos, spectrum, pd);
}

// The sink that ignores everything: what a kernel's own sink derives from, and the gather kernel's as it is.
struct SampleSink {
    // true: the loop finds out which emissive object a light sample chose (sample_emissive_indexed) and hands its material to material()
    static constexpr bool kEmitters = false;
    // What the sink keeps of a term's emitter (nothing here)
    struct Emitter {};
    PT_D Emitter point_light(uint32_t) const { return {}; } // of point light j
    PT_D Emitter material(uint32_t) const { return {}; }    // of an emissive object's, or an emitting vertex's, material
    // The very first walk hit nothing
    PT_D void first_miss() {}
    // The first vertex has been reached along rd; n is its normal
    PT_D void first_vertex(V3, V3) {}
    // A light sample's term has been added to out_spectrum, with no ray or after an unoccluded shadow walk; path_length scatterings lie before it
    PT_D void direct(const C4 &, Emitter, int) {}
    // A new vertex's emitted term has been added; path_length - 1 scatterings lie before it
    PT_D void emitted(const C4 &, Emitter, int) {}
};

// One sample's out_spectrum.  AT_VERTEX: the sample starts at the vertex p with the normal v, reached along -v, that has no material
// (PT_NO_MATERIAL: the receiver) -- getSample at a first vertex that is already there, path_length = 1; BOUNCES draws its roulette here,
// !BOUNCES ends the sample behind the vertex's light samples.  !AT_VERTEX: the sample starts with the ray (p, v) -- getSample entered at
// its real top (worker.cpp:44, path_length = 0).  alive == false: there is no sample, nothing is traced and no hook is called.  The
// engine comes by value: no kernel draws from it behind its sample.
template<bool AT_VERTEX, bool BOUNCES, typename TracerT, typename Sink>
PT_D C4 sample_walk(TracerT &tr, const PtDevScene &sc, const RootBox &root, float epsilon, uint64_t rng, bool alive, V3 p, V3 v, Sink &sink) {
    const uint32_t n_light_samples = sc.n_lights + sc.n_object_samples;
    // getSample's state (worker.cpp:37-43)
    float contribution_unweighted = 1.0f;
    double divisor = 1.0, bounce_pd = 1.0;
    C4 spectrum = c4(1.0f, 1.0f, 1.0f, 1.0f);
    C4 out = c4(0.0f, 0.0f, 0.0f, 0.0f);
    int path_length = AT_VERTEX ? 1 : 0;
    // worker.cpp:64 adds 0 at the receiver; :67-70
    float bounce_probability = 1.0f;
    bool do_bounce = false;
    if constexpr(AT_VERTEX && BOUNCES) {
        do_bounce = rng_uniform01(rng) < bounce_probability;
    }
    uint32_t j = 0;
    uint32_t material_index = 0xFFFFFFFFu; // PT_NO_MATERIAL
    V3 pos = p, n = AT_VERTEX ? v : v3(0.0f, 1.0f, 0.0f), rd = AT_VERTEX ? neg(v) : v;
    bool need = !AT_VERTEX; // the first ray is there
    float4 ro = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rdv = ro;
    if constexpr(!AT_VERTEX) {
        ro = make_float4(p.x, p.y, p.z, 0.0f);
        rdv = make_float4(v.x, v.y, v.z, __uint_as_float(0u));
    }
    C4 pending = c4(0.0f, 0.0f, 0.0f, 0.0f);
    typename Sink::Emitter pending_emitter{}; // the emitter of `pending`
    while(alive) {
        // ---- advance the vertex until it has a ray to trace -------------------------------------------------------------------------------------
        while(alive && !need) {
            if(j < n_light_samples) {
                // worker.cpp:76-103, light sample j
                V3 light_pos;
                C4 light_spectrum;
                float lpd;
                bool valid;
                typename Sink::Emitter emitter{};
                if(j < sc.n_lights) {
                    const float4 lp = sc.lights[2 * j];
                    light_pos = v3(lp.x, lp.y, lp.z);
                    light_spectrum = c4(sc.lights[2 * j + 1]);
                    lpd = 1.0f;
                    valid = true;
                    emitter = sink.point_light(j);
                }
                else if constexpr(Sink::kEmitters) {
                    uint32_t object_index;
                    valid = sample_emissive_indexed(sc, EmisGlobal{sc}, pos, rng, light_pos, light_spectrum, lpd, object_index);
                    if(valid) {
                        emitter = sink.material(__float_as_uint(sc.emis[4 * (size_t)object_index + 2].w));
                    }
                }
                else {
                    valid = sample_emissive(sc, EmisGlobal{sc}, pos, rng, light_pos, light_spectrum, lpd);
                }
                j += 1;
                if(valid) {
                    const Material mat = material_load(sc.materials, material_index);
                    const V3 to_light = light_pos - pos;
                    const V3 light_dir = normalize(to_light);
                    float shading_factor, shadow_ray_pd;
                    const C4 base_spectrum = bsdf_spectrum(mat, rd, light_dir, n, light_spectrum, true, shading_factor, shadow_ray_pd);
                    if(shadow_ray_pd > 0.0f) {
                        const C4 combined = (base_spectrum * shading_factor) * spectrum;
                        const C4 weighed = combined / (float)(divisor * bounce_pd * lpd * shadow_ray_pd);
                        // adding +-0 never changes out_spectrum (which is never -0), so such a sample needs no ray
                        if(!(weighed.r == 0.0f && weighed.g == 0.0f && weighed.b == 0.0f)) {
                            const float threshold = len(to_light) - epsilon;
                            if(threshold <= 0.0f) {
                                out = out + weighed; // light_t < 0 || light_t >= threshold holds for every light_t
                                sink.direct(weighed, emitter, path_length);
                            }
                            else {
                                need = true;
                                pending = weighed;
                                pending_emitter = emitter;
                                const V3 o2 = pos + light_dir * epsilon;
                                ro = make_float4(o2.x, o2.y, o2.z, threshold);
                                rdv = make_float4(light_dir.x, light_dir.y, light_dir.z, __uint_as_float(PT_DEST_SHADOW));
                            }
                        }
                    }
                }
            }
            else if(!BOUNCES || !do_bounce) {
                alive = false; // worker.cpp:106-109 (the direct light of one vertex ends here as well)
            }
            else {
                // worker.cpp:110-138
                bounce_pd *= bounce_probability;
                if(bounce_pd <= 1E-20) {
                    alive = false;
                }
                else {
                    const Material mat = material_load(sc.materials, material_index);
                    float ray_factor, ray_pd;
                    const Ray next_ray = bsdf_propagate(mat, rd, pos, n, epsilon, rng, ray_factor, ray_pd);
                    divisor *= ray_pd;
                    divisor /= ray_factor;
                    contribution_unweighted *= ray_factor;
                    float shading_factor, shading_pd;
                    const C4 shaded = bsdf_spectrum(mat, rd, next_ray.d, n, spectrum, false, shading_factor, shading_pd);
                    divisor *= shading_pd;
                    divisor /= shading_factor;
                    contribution_unweighted *= shading_factor;
                    spectrum = shaded;
                    if(divisor <= 1E-20) {
                        alive = false;
                    }
                    else {
                        need = true;
                        ro = make_float4(next_ray.o.x, next_ray.o.y, next_ray.o.z, 0.0f);
                        rdv = make_float4(next_ray.d.x, next_ray.d.y, next_ray.d.z, __uint_as_float(0u));
                    }
                }
            }
        }
        if(!alive) {
            break;
        }
        // ---- the walk: the first ray's, a shadow ray's or a bounce's --------------------------------------------------------------------------
        Walk w;
        typename TracerT::Rec rec;
        rec.r0 = rec.r1 = rec.r2 = rec.r3 = (f4v){0.0f, 0.0f, 0.0f, 0.0f};
        tr.start(w, rec, root, ro, rdv);
        uint32_t n_nodes = 0, n_leaves = 0;
        while(tr.step(w, rec, 1, n_nodes, n_leaves)) {
        }
        need = false;
        if(w.dest & PT_DEST_SHADOW) {
            if(!w.occluded) {
                out = out + pending; // worker.cpp:100
                sink.direct(pending, pending_emitter, path_length);
            }
        }
        else if(w.best_ref == PT_REF_NONE) {
            alive = false; // worker.cpp:47-49
            if(path_length == 0) {
                sink.first_miss();
            }
        }
        else {
            // the next vertex, up to the roulette draw (worker.cpp:50-70)
            path_length++;
            rd = v3(rdv.x, rdv.y, rdv.z);
            pos = v3(ro.x, ro.y, ro.z) + rd * w.best_t;
            n = object_normal(sc, w.best_ref, pos, material_index);
            if(path_length == 1) {
                sink.first_vertex(n, rd);
            }
            const Material mat = material_load(sc.materials, material_index);
            const C4 emitted = (spectrum * mat.emission) / (float)(divisor * bounce_pd);
            out = out + emitted;
            sink.emitted(emitted, sink.material(material_index), path_length);
            bounce_probability = path_length <= 4 ? 1.0f : 0.1f + 0.1f * fmin_std(contribution_unweighted * get_contribution(spectrum), 1.0f);
            do_bounce = rng_uniform01(rng) < bounce_probability;
            j = 0;
        }
    }
    return out;
}

} // namespace

#endif
