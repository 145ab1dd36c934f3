// pt_trace.h -- the traversal machinery of one lane: Walk (a ray and where it stands in the tree), Tracer (record fetch, the common step
// for inner nodes, the rare step for leaves and pops, the stack window in LDS with its HBM spill area) and the two stack-window sizes.
// pt_path.hip's header comment describes the traversal; the persistent path kernel there and the one-walk-per-lane kernels of
// pt_walks.hip are its users.  The code generation of the path kernel reacts to harmless-looking moves of this text:
// compare builds with tools/kernel_diff.py after any edit.
#ifndef PT_TRACE_H
#define PT_TRACE_H

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_shading.h"

#define PT_PATH_STACK_LDS 8 /* entries of a lane's traversal stack kept in LDS (16 KB per workgroup: four workgroups share a CU); deeper ones spill to HBM */
// A scene staged in LDS whose records leave no room for four workgroups per CU beside an 8-entry window gets a 4-entry one (its tree has at most
// 384 records: few walks go deeper, and those spill as on any tree).  176 / 98 / 72 triangles in the benchmark's box: 600 -> 757, 855 -> 949, 802 -> 862
// Msamples/s; where four workgroups fit anyway the small window costs 2-4 % (Cornell 718 -> 705), and on trees in HBM 9 % (profiles/r03_stack_window_ab.txt).
#define PT_PATH_STACK_LDS_SMALL 4

namespace ptd {

typedef float f2v __attribute__((ext_vector_type(2)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
typedef const f4v __attribute__((address_space(1))) *glb_f4_cptr;
typedef u2v __attribute__((address_space(3))) *lds_u2_ptr;
typedef u2v __attribute__((address_space(1))) *glb_u2_ptr;
typedef unsigned int __attribute__((address_space(3))) *lds_u32_ptr;
typedef const PtPathArgs __attribute__((address_space(4))) *args_c4;

template<bool IN_LDS>
struct RecPtr {
    typedef glb_f4_cptr type;
};
template<>
struct RecPtr<true> {
    typedef lds_f4_cptr type;
};

// The root of the tree: its box is tested before anything else (Scene::getIntersection, scene.cpp:211-219)
struct RootBox {
    float lo[3], hi[3];
    uint32_t ref;
};

// One walk (one ray) in a lane.
//
// `cur` is where the walk stands: the reference of an inner node (bits 31, 30 = 00) or of a leaf (bit 31 set, pt_types.h), PT_REF_NONE when
// the walk is over, or PT_REF_POPPING when it has to return to a parked node but the entry on top of its stack has already been
// discarded (see Tracer::node_step).  The stack of parked nodes has a SENTINEL as entry 0 -- (PT_REF_NONE, -1) -- so "the stack is
// empty" needs no test anywhere: popping the sentinel ends the walk, and its distance passes every pruning test.
#define PT_REF_POPPING 0xfffffffeu
struct Walk {
    V3 o, d, inv;
    f2v o_xy, o_zx, o_yz, i_xy, i_zx, i_yz; // origin and inverse direction again, as the register pairs of the packed slab arithmetic
    float thr;       // shadow threshold |to_light| - epsilon (worker.cpp:86)
    uint32_t dest;   // destination word of the ray
    float best_t;
    uint32_t best_ref;
    float t_max;     // pruning distance: the smallest hit distance so far (scene.cpp:124,137)
    float t_lim;     // the largest float below t_max: x < t_max  <=>  x <= t_lim, which lets min() fold the pruning test into the box test
    uint32_t cur;
    uint32_t sp;     // entries on the stack, the sentinel included
    bool occluded;   // shadow ray: a leaf closer than the light was found

    PT_D void pack() {
        o_xy = (f2v){o.x, o.y};
        o_zx = (f2v){o.z, o.x};
        o_yz = (f2v){o.y, o.z};
        i_xy = (f2v){inv.x, inv.y};
        i_zx = (f2v){inv.z, inv.x};
        i_yz = (f2v){inv.y, inv.z};
    }
    // t_max is never negative (hit distances are >= 0; it may be -0): below zero there is nothing, and every entry distance is >= 0
    PT_D void set_t_max(float t) {
        t_max = t;
        t_lim = t > 0.0f ? __uint_as_float(__float_as_uint(t) - 1u) : -1.0f;
    }
};

// The traversal machinery of one lane: record arrays (LDS or HBM), the stack window in LDS and its HBM spill area.
//
// What a step costs on this chip (tools/issue_probe.hip, profiles/r03_issue_probe.txt): a wavefront that is alone on its SIMD issues one
// instruction per 4.5 cycles whatever the instruction; a taken branch costs 22 cycles, a not-taken one 13, a wave-uniform branch on a
// ballot (v_cmp into an SGPR pair, s_cmp, s_cbranch) 35-52, a lane mask that goes through the scalar unit on its way to a v_cndmask
// 16 more than one that stays in vcc, an LDS round trip 55, an L1 hit 112.  A stream's samples are sequential, so at the end of every
// launch -- and for the whole of a strong-scaling share -- the frame time is the length of a few such lonely chains.  Hence:
//   * node_step is STRAIGHT-LINE code for all 64 lanes, no branch and no exec mask but the one around the record loads.  Conditions
//     never meet in scalar registers: a child that is not entered gets the entry distance +inf, and min / max / compare-with-inf on
//     the two distances yield near child, far child, "both" and "none" (each v_cmp feeds the v_cndmask or the add-with-carry behind
//     it through vcc).  The far child is written ABOVE the top of the stack by every lane (it only becomes an entry where the stack
//     pointer moves) and the top entry is read by every lane ahead of the arithmetic, so the first pop of the recursion's return
//     (scene.cpp:137) costs no trip to LDS;
//   * everything rare -- leaves, a popped entry that fails the distance test, a stack deeper than its LDS window -- is left to
//     slow_step, which the traversal loop enters through ONE wave-uniform branch per step.
// Diagnostic build (-DPT_STEP_STAMPS, tools/step_timing.py): s_memtime stamps inside the step; segment k collects the cycles from the
// previous stamp to stamp k, each inflated by the round trip of the previous stamp itself (segment 7 = two stamps back to back: that price)
#ifdef PT_STEP_STAMPS
#define PT_STAMP(k)                                                      \
    do {                                                                 \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime();     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");               \
        stamp_acc[k] += now_ - stamp_last;                               \
        stamp_last = now_;                                               \
    } while(0)
#else
#define PT_STAMP(k) do { } while(0)
#endif

// (PATH_KERNEL: which form of the triangle test slow_step takes -- pt_device.h: tri_intersect)
template<int STACK_LDS, bool IN_LDS, bool PATH_KERNEL = false>
struct Tracer {
    static_assert((STACK_LDS & (STACK_LDS - 1)) == 0, "the stack window is indexed with a mask");
#ifdef PT_STEP_STAMPS
    mutable unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_last = 0;
#endif
#ifdef PT_PATH_TIMING
    // diagnostic build: what slow_step costs a wavefront (the same values in every lane) -- shader-clock cycles inside it, its invocations, the
    // lanes it served (leaves + walks that came to pop) and the trips of its pop loop.  (No request of this step is in flight while it
    // runs and it issues none: its cycles are its instructions, its LDS trips and the spill reloads of its pop loop.)
    mutable unsigned long long slow_cycles = 0;
    mutable uint32_t slow_calls = 0, slow_served = 0, slow_trips = 0;
#endif
    typedef typename RecPtr<IN_LDS>::type rec_ptr;
    rec_ptr recs;         // the 64-byte records the tree's references index: leaves, then pairs (pt_types.h)
    lds_u2_ptr stack_l;   // this thread's column: entry e at stack_l[(e mod STACK_LDS) * 256]
    glb_u2_ptr my_spill;  // entries that have left the window: entry e at my_spill[e]

    // The 64-byte record a walk stands on, requested as soon as the walk knows where it goes next: a node's pair of child boxes, a
    // triangle, or a sphere's (origin, radius).  A reference's low 30 bits ARE the record's index: one mask, one shift-add.
    struct Rec {
        f4v r0, r1, r2, r3;
    };
    PT_D void fetch(uint32_t cur, Rec &R) const {
        rec_ptr p = recs + 4 * (size_t)(cur & PT_REF_INDEX);
        R.r0 = p[0];
        R.r1 = p[1];
        R.r2 = p[2];
        R.r3 = p[3];
    }
    // Registers that a load fills and nobody reads (the last two words of a record) become the compiler's scratch registers, and their
    // first use then has to wait for the load: a full memory latency at the end of every step.  Every consumer of a record calls this.
    static PT_D void whole(const Rec &R) {
        asm volatile("" ::"v"(R.r0), "v"(R.r1), "v"(R.r2), "v"(R.r3));
    }

    // Where a walk stands, classified with one comparison each: a reference below 2^30 = an inner node (node_step moves it); at or above,
    // except PT_REF_NONE = it waits for slow_step (a leaf, or a walk that has to go on popping).
    static PT_D unsigned long long node_lanes(uint32_t cur) { return __builtin_amdgcn_uicmp(cur, 0x40000000u, 36); }       // cur < 2^30
    static PT_D unsigned long long slow_lanes(uint32_t cur) { return __builtin_amdgcn_uicmp(cur + 1u, 0x40000000u, 34); }  // 2^30 <= cur < NONE

    // Start a walk: Scene::getIntersection tests the root box first (scene.cpp:211-219).  begin() is the walk's side of it -- afterwards
    // w.cur is the root, or PT_REF_NONE where the ray misses the root box -- and start() also requests the root's record.  (The path kernel
    // calls the two apart: see its hand-out.)
    PT_D void begin(Walk &w, const RootBox &root, float4 ro, float4 rd) const {
        w.o = v3(ro.x, ro.y, ro.z);
        w.d = v3(rd.x, rd.y, rd.z);
        w.thr = ro.w;
        w.dest = __float_as_uint(rd.w);
        w.inv = slab_inverse(w.d);
        w.pack();
        w.best_ref = PT_REF_NONE;
        w.best_t = -1.0f;
        // A shadow ray is a closest-hit query like any other in the reference (worker.cpp:83-86) and must be pruned like one: starting it
        // with the light's distance as pruning distance is NOT the same thing in floating point.  The sampled point lies on an emitter,
        // the ray starts epsilon in front of the vertex and the threshold is |to_light| - epsilon: the emitter's own hit distance and
        // the threshold are the same number up to rounding, and the reference finds "occluded" whenever the hit comes out an ulp
        // below.  A box around a flat, axis-aligned emitter is entered at that very distance (again up to rounding, of the slab test
        // this time), so pruning at the threshold skipped the emitter in cases where the reference tested it and found t < threshold.
        // The walk still ends at the first hit below the threshold (the closest hit can only be nearer).
        w.set_t_max(FLT_MAX);
        // (the sentinel pair is made where it is stored: as a constant it was hoisted out of the path kernel's loops and kept in scratch)
        uint32_t sent_ref, sent_t;
        asm volatile("v_mov_b32 %0, -1\n\tv_mov_b32 %1, -1.0" : "=v"(sent_ref), "=v"(sent_t)); // PT_REF_NONE, bits of -1.0f
        const u2v sentinel = {sent_ref, sent_t};
        stack_l[0] = sentinel;
        w.sp = 1;
        w.occluded = false;
        // (one select, no branch: an empty scene's root box is never entered whatever the test says)
        const float t_root = slab_walk(ld3(root.lo), ld3(root.hi), w.o, w.inv);
        w.cur = ((root.ref != PT_REF_NONE) & (t_root >= 0.0f)) ? root.ref : PT_REF_NONE;
    }
    PT_D void start(Walk &w, Rec &R, const RootBox &root, float4 ro, float4 rd) const {
        begin(w, root, ro, rd);
        if(w.cur != PT_REF_NONE) {
            fetch(w.cur, R);
        }
    }

    // One step of every walk that stands on an inner node (`node_mask`); the record of where a walk stands next is requested.
    // AABB::getIntersection of both children (bounding_box.cpp:38-73): a box is hit iff t_max >= 0 and t_min <= t_max -- the
    // same as max(t_min, 0) <= t_max -- and its entry distance is max(t_min, 0) (0 = origin inside, :68-70).
    // impl::getChildIntersection (scene.cpp:113-146): a child is entered iff it is hit and its entry distance is below the pruning
    // distance (entry < t_max <=> entry <= t_lim, so both tests are ONE comparison with min(box exit, t_lim)); with both entered the
    // nearer one comes first -- on equal distances the RIGHT one (scene.cpp:120-121): "left first" is a strict less-than -- and the other
    // is parked with its entry distance; with none entered the walk returns to the node on top of its stack if that one's entry
    // distance is still below the pruning distance (scene.cpp:137), and goes on popping in slow_step otherwise.
    // The stack: the top STACK_LDS entries of a lane live in LDS (slot = index mod STACK_LDS), older ones in the lane's HBM spill area.
    // `deep_mask`: the lanes whose stack has left the window -- for them a push first moves the entry it overwrites to the spill area and
    // a pop brings the entry that left the window last back into the slot that has become free; if there is no such lane (one scalar
    // branch) the far child is simply written ABOVE the top of the stack by every lane: it only becomes an entry where the pointer moves.
    // `request_below` (a scalar): the lanes whose new reference is below it request their record here.  PT_REF_POPPING in a step that the
    // rare step does not follow -- every lane that moved onto a record, AHEAD of the deep-stack reload, whose wait the request shares --
    // and 0 in one that it follows: step() then requests once, behind the rare step (see there).
    PT_D void node_step(Walk &w, Rec &R, unsigned long long node_mask, unsigned long long deep_mask, uint32_t request_below) const {
        if(!__builtin_amdgcn_inverse_ballot_w64(node_mask)) {
            return; // (the one exec mask of the step; the caller knows the mask is not empty)
        }
#ifdef PT_STEP_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        PT_STAMP(2); // waiting for the record
        whole(R);
        const f4v q0 = R.r0, q1 = R.r1, q2 = R.r2;
        const uint32_t sp = w.sp;
        const u2v top = stack_l[((sp - 1u) & (uint32_t)(STACK_LDS - 1)) * 256u]; // read ahead of the arithmetic that decides whether it is needed
        // twelve differences and products, two per instruction (v_pk_add_f32 with a negated operand is the IEEE subtraction,
        // v_pk_mul_f32 the IEEE product: nothing is fused, every result is the reference's)
        const f2v a0 = ((f2v){q0.x, q0.y} - w.o_xy) * w.i_xy; // L.lo.x, L.lo.y
        const f2v a1 = ((f2v){q0.z, q0.w} - w.o_zx) * w.i_zx; // L.lo.z, L.hi.x
        const f2v a2 = ((f2v){q1.x, q1.y} - w.o_yz) * w.i_yz; // L.hi.y, L.hi.z
        const f2v a3 = ((f2v){q1.z, q1.w} - w.o_xy) * w.i_xy; // R.lo.x, R.lo.y
        const f2v a4 = ((f2v){q2.x, q2.y} - w.o_zx) * w.i_zx; // R.lo.z, R.hi.x
        const f2v a5 = ((f2v){q2.z, q2.w} - w.o_yz) * w.i_yz; // R.hi.y, R.hi.z
        const float l1 = a0.x, l2 = a1.y, l3 = a0.y, l4 = a2.x, l5 = a1.x, l6 = a2.y;
        const float r1 = a3.x, r2 = a4.y, r3 = a3.y, r4 = a5.x, r5 = a4.x, r6 = a5.y;
        const float l_min = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(l1, l2), __builtin_fminf(l3, l4)), __builtin_fminf(l5, l6));
        const float l_max = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(l1, l2), __builtin_fmaxf(l3, l4)), __builtin_fmaxf(l5, l6));
        const float r_min = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(r1, r2), __builtin_fminf(r3, r4)), __builtin_fminf(r5, r6));
        const float r_max = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(r1, r2), __builtin_fmaxf(r3, r4)), __builtin_fmaxf(r5, r6));
        const float left_t = __builtin_fmaxf(l_min, 0.0f), right_t = __builtin_fmaxf(r_min, 0.0f);
        const float inf = __builtin_inff();
        const float t_lim = w.t_lim;
        const float tl = left_t <= __builtin_fminf(l_max, t_lim) ? left_t : inf;   // entry distance of a child that is entered, else +inf
        const float tr = right_t <= __builtin_fminf(r_max, t_lim) ? right_t : inf;
        const bool left_first = tl < tr;
        const uint32_t left_ref = __float_as_uint(R.r3.x), right_ref = __float_as_uint(R.r3.y);
        const uint32_t near_ref = left_first ? left_ref : right_ref;
        const float near_t = __builtin_fminf(tl, tr), far_t = __builtin_fmaxf(tl, tr);
        const u2v far = {left_first ? right_ref : left_ref, __float_as_uint(far_t)};
        const bool both = far_t < inf, entered = near_t < inf;
        const uint32_t slot = (sp & (uint32_t)(STACK_LDS - 1)) * 256u;
        if(deep_mask == 0ULL) {
            stack_l[slot] = far;
        }
        else if(both) {
            if(sp >= (uint32_t)STACK_LDS) {
                my_spill[sp - STACK_LDS] = stack_l[slot];
            }
            stack_l[slot] = far;
        }
        const uint32_t popped = __uint_as_float(top.y) <= t_lim ? top.x : PT_REF_POPPING;
        const uint32_t next = entered ? near_ref : popped;
        w.sp = entered ? sp + (both ? 1u : 0u) : sp - 1u;
        w.cur = next;
        asm volatile("" ::"v"(w.sp), "v"(w.cur)); // (the walk's new state is complete before the record is requested: nothing is left to do behind the loads)
        PT_STAMP(3); // slab tests, decision, stack
        // the lanes that moved onto a record (not the ones whose walk ended or that go on popping: the two codes at the top)
        if(next < request_below) {
            fetch(next, R);
        }
        PT_STAMP(4); // address and request of the next record (none in a step that the rare step follows, and none for records in LDS: see step())
        if(deep_mask != 0ULL) {
            if(!entered & (sp - 1u >= (uint32_t)STACK_LDS)) {
                stack_l[((sp - 1u) & (uint32_t)(STACK_LDS - 1)) * 256u] = my_spill[sp - 1u - STACK_LDS]; // the window moves down
            }
        }
    }

    // Everything that is not the common step: the leaves in `leaf_mask` (Object::getIntersection) and the walks that must (go on) pop(ping).
    // n_leaves counts visits for the whole wavefront (the same value in every lane).
    // It runs for the lanes that wait for it while the others stand still, and on the flagship it is a fifth of a wavefront's life
    // (profiles/slow_step_share.txt), so it is shaped like node_step: ONE divergent region around the leaf test, whose
    // result is applied with selects on lane predicates, and a pop loop that carries nothing but `sp` and `cur` -- "has to pop" IS
    // cur == PT_REF_POPPING, a leaf lane that goes on popping takes that code -- with one test at its bottom and one way out.  (With a
    // flag beside cur and the test on top, every trip copied cur and sp to other registers and back and carried four lane masks
    // through the scalar unit; the early returns of the triangle test and the nested tests behind it were sixteen divergent regions.)
    // It requests no record: step() does, behind it, and node_step requests none ahead of it, so the leaf block opens without a wait for
    // other lanes' records.
    PT_D void slow_step(Walk &w, Rec &R, unsigned long long leaf_mask, uint32_t &n_leaves) const {
        uint32_t cur = w.cur;
#ifdef PT_PATH_TIMING
        const unsigned long long t_slow = __builtin_amdgcn_s_memtime();
        slow_calls++;
        slow_served += (uint32_t)__popcll(leaf_mask) + (uint32_t)__popcll(__ballot(cur == PT_REF_POPPING));
#endif
        if(leaf_mask != 0ULL) {
            n_leaves += (uint32_t)__popcll(leaf_mask);
            if(__builtin_amdgcn_inverse_ballot_w64(leaf_mask)) {
                // a leaf reports Object::getIntersection unconditionally (scene.cpp:105-109); among the non-negative hits the smallest wins and a
                // later-visited leaf wins ties (scene.cpp:141-146); a shadow walk ends at its first hit below the threshold (worker.cpp:86)
                const float4 q0 = to_f4(R.r0), q1 = to_f4(R.r1), q2 = to_f4(R.r2);
                // (the triangle test is straight-line code and runs on a sphere's record too, where its result is replaced: a wavefront
                // without a lane on a sphere skips the sphere's code as a whole, and no scene pays for a branch around the triangle's)
                const TriRec tr = tri_unpack(q0, q1, q2);
                float t_leaf = tri_intersect<!PATH_KERNEL>(tr.a, tr.ab, tr.ac, (tr.obj_cull >> 31) != 0, w.o, w.d);
                if(cur & PT_REF_SPHERE) {
                    t_leaf = sphere_intersect(v3(q0.x, q0.y, q0.z), q0.w, w.o, w.d);
                }
                const bool hit = t_leaf >= 0.0f;
                const bool ends = hit & ((w.dest & PT_DEST_SHADOW) != 0u) & (t_leaf < w.thr); // the shadow walk is over: occluded
                const bool counts = hit & !ends;
                const bool best = counts & ((w.best_ref == PT_REF_NONE) | !(w.best_t < t_leaf));
                w.best_t = best ? t_leaf : w.best_t;
                w.best_ref = best ? cur : w.best_ref;
                w.set_t_max((counts & (t_leaf < w.t_max)) ? t_leaf : w.t_max); // std::min(t_max, t_leaf); t_lim of an unchanged t_max is the value it had
                w.occluded = w.occluded | ends;
                cur = ends ? PT_REF_NONE : PT_REF_POPPING;
            }
        }
        // pop: the first parked node whose entry distance is still below t_max (scene.cpp:137: re-tested against the then-current distance);
        // the sentinel at the bottom passes the test and ends the walk.  Every lane reads the entry below ITS top (a slot of its own column
        // whatever sp is: the index is masked) and only the popping ones take it; the one divergent region of a trip is the window moving down.
        const bool popper = cur == PT_REF_POPPING;
        if(__ballot(popper) != 0ULL) {
            uint32_t sp = w.sp;
            const float t_max = w.t_max;
            do {
#ifdef PT_PATH_TIMING
                slow_trips++;
#endif
                const bool popping = cur == PT_REF_POPPING;
                const uint32_t below = sp - 1u;
                const uint32_t slot = (below & (uint32_t)(STACK_LDS - 1)) * 256u;
                const u2v e = stack_l[slot];
                if(popping & (below >= (uint32_t)STACK_LDS)) {
                    stack_l[slot] = my_spill[below - STACK_LDS]; // the window moves down: the entry that left it last comes back
                }
                sp = popping ? below : sp;
                cur = (popping & (__uint_as_float(e.y) < t_max)) ? e.x : cur;
            } while(__ballot(cur == PT_REF_POPPING) != 0ULL);
            w.sp = sp;
        }
        w.cur = cur;
#ifdef PT_PATH_TIMING
        slow_cycles += __builtin_amdgcn_s_memtime() - t_slow;
#endif
    }

    // One step of the wavefront: the common step for the lanes on inner nodes; then, if no lane is left on one or `leaf_min` lanes wait for
    // it, the rare one.  Returns false when no lane of the wavefront stands anywhere any more.
    PT_D bool step(Walk &w, Rec &R, int leaf_min, uint32_t &n_nodes, uint32_t &n_leaves) const {
        PT_STAMP(0); // loop back, the caller's code between two steps
        PT_STAMP(7); // (nothing: what a stamp costs)
        const unsigned long long nodes = node_lanes(w.cur), slow = slow_lanes(w.cur);
        if((nodes | slow) == 0ULL) {
            return false;
        }
        PT_STAMP(1); // classification
        if constexpr(IN_LDS) {
            // Records in LDS: ONE request at the end of the step, for every lane that either half has moved, kept as a scalar lane mask
            // (remembering `cur` in a vector register to compare afterwards cost 21 moves and 24 branches in the burst loop).  A node lane
            // is in `nodes` whether it entered a child, took the top of its stack or was served by the pop loop in this very step; a served
            // leaf or popping lane is in `slow`; a leaf lane that still waits is in neither and keeps the record it has.  (Why the two
            // locations of the tree take different forms: the measurements of DESIGN.md 5.8.)
            unsigned long long moved = 0ULL;
            if(nodes != 0ULL) {
                n_nodes += (uint32_t)__popcll(nodes);
                node_step(w, R, nodes, nodes & __builtin_amdgcn_uicmp(w.sp, (uint32_t)STACK_LDS, 35), 0u);
                moved = nodes;
            }
            PT_STAMP(5); // the deep-stack reload (or the test for it), leaving the common step
            if(slow != 0ULL && (nodes == 0ULL || __popcll(slow) >= leaf_min)) {
                slow_step(w, R, slow & __builtin_amdgcn_uicmp(w.cur, PT_REF_POPPING, 36), n_leaves);
                moved |= slow;
            }
            PT_STAMP(6); // the rare step (or the test for it)
            if(__builtin_amdgcn_inverse_ballot_w64(moved & __builtin_amdgcn_uicmp(w.cur, PT_REF_POPPING, 36))) {
                fetch(w.cur, R);
            }
            return true;
        }
        // Records in HBM.  Whether the rare step follows is known before the common one runs (`slow` was taken ahead of it).  Where it follows, node_step
        // requests nothing and ONE request behind slow_step serves every lane either half has moved: the compiler tracks the record
        // registers, not lanes, so with node_step's request in flight the leaf block opened with s_waitcnt vmcnt(0) -- the few leaf lanes
        // waited a full memory latency for records only the node lanes need -- and the poppers' own request at slow_step's end was a second
        // latency in the same step.  Where it does not follow, the request stays where it was, ahead of the deep-stack reload: moved behind
        // it, every step with a deep pop paid the reload's latency and the record's one after the other.
        const bool rare = slow != 0ULL && (nodes == 0ULL || __popcll(slow) >= leaf_min);
        if(nodes != 0ULL) {
            n_nodes += (uint32_t)__popcll(nodes);
            node_step(w, R, nodes, nodes & __builtin_amdgcn_uicmp(w.sp, (uint32_t)STACK_LDS, 35), rare ? 0u : PT_REF_POPPING);
        }
        PT_STAMP(5); // the deep-stack reload (or the test for it), leaving the common step
        // The rare step, for the leaves and the walks that have to go on popping: its code is long (a triangle test is 100 instructions,
        // a division among them), so the waiting lanes share it -- not before `leaf_min` of them wait, unless no lane stands on a node any
        // more.  (Serving the popping walks at once instead of letting them wait with the leaves: 422 against 430 Msamples/s.)
        if(rare) {
            // (slow was taken before the common step: a lane that has just reached a leaf is not in it, its record is not requested yet)
            slow_step(w, R, slow & __builtin_amdgcn_uicmp(w.cur, PT_REF_POPPING, 36), n_leaves);
            // `nodes` and `slow` together are every lane with a walk, and in this step every one of them has moved (a node lane that node_step
            // sent popping was served by the pop loop just now), so no lane mask is needed: the lanes that stand on a record request it --
            // not the ones whose walk is over (no lane is left popping: the loop ran until none was)
            if(w.cur < PT_REF_POPPING) {
                fetch(w.cur, R);
            }
        }
        PT_STAMP(6); // the rare step with the request behind it (or the test for it)
        return true;
    }
};

} // namespace ptd

#endif
