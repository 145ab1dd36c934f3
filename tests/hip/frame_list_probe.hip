// frame_list_probe.hip -- TEST ONLY: the work-list kernels of cpupathtrace_amd/csrc/pt_frame.hip, one launcher at a time, on caller-given
// lists, statuses, records, tile tables and maps.
//
// Built by tests/frame_list_probe.py into tests/hip/libframe_list_probe.so with the product's compiler flags; not part of
// libpathtrace_hip.so.  pt_frame.hip is included unchanged, so the kernels of its anonymous namespace are in reach.  Every entry point
// frame_list_probe_* takes host arrays, puts every device array, input, output or unused, into a Guarded<> (guard_band.h) with a band
// on both sides, calls the product's own launcher on a stream of its own, waits, copies everything back and returns GuardStatus::code():
// the HIP error, or PT_GUARD_TOUCHED + the number of the array whose band was written, or PT_INPUT_CHANGED + the number of the array a
// launcher takes as const that came back with other bytes, or 0.  An array a launcher writes is given with its initial bytes by the
// caller, so what a kernel left alone is seen as well as what it wrote.
#include "../../cpupathtrace_amd/csrc/pt_frame.hip"

#include <cstddef>
#include <cstring>
#include <vector>

#include "guard_band.h"

namespace {

constexpr int PT_INPUT_CHANGED = 200000;
constexpr size_t kBand = 64;      // elements either side of an array of words, pairs or pixels
constexpr size_t kBandRecords = 2; // ... and of an array of 528-byte records

struct Probe {
    GuardStatus st;
    hipStream_t stream = nullptr;
    int changed = 0; // 1 + the number of the first const array that came back changed
    Probe() {
        st(hipSetDevice(0));
        if(st.ok()) {
            st(hipStreamCreate(&stream));
        }
    }
    ~Probe() {
        if(stream != nullptr) {
            (void)hipStreamDestroy(stream);
        }
    }
    void launched(int rc) {
        if(rc != 0) {
            st(hipGetLastError());
            st(hipErrorLaunchFailure);
        }
    }
    void wait() {
        if(stream != nullptr) {
            st(hipStreamSynchronize(stream));
        }
        st(hipGetLastError());
    }
    // an array the launcher takes as const: its bands, and its bytes against the caller's
    template<typename T>
    void same(Guarded<T> &a, const void *src) {
        std::vector<T> back(a.n);
        a.get(back.data());
        if(st.ok() && a.n > 0 && std::memcmp(back.data(), src, a.n * sizeof(T)) != 0 && changed == 0) {
            changed = a.id + 1;
        }
    }
    int code() const {
        const int c = st.code();
        return c != 0 ? c : (changed != 0 ? PT_INPUT_CHANGED + changed - 1 : 0);
    }
};

const PtParkRecord *records(const uint32_t *words) {
    return reinterpret_cast<const PtParkRecord *>(words);
}

} // namespace

extern "C" {

int frame_list_probe_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int frame_list_probe_guard_code() {
    return PT_GUARD_TOUCHED;
}

int frame_list_probe_changed_code() {
    return PT_INPUT_CHANGED;
}

const char *frame_list_probe_error_string(int code) {
    return code >= PT_INPUT_CHANGED ? "a const input was written" : (code >= PT_GUARD_TOUCHED ? "a guard band was written" : hipGetErrorString(static_cast<hipError_t>(code)));
}

// What the Python side restates, for it to assert: out[0 .. 32)
int frame_list_probe_sizes(uint32_t *out) {
    const uint32_t v[32] = {static_cast<uint32_t>(sizeof(PtParkRecord)),
                            static_cast<uint32_t>(sizeof(PtEstimator)),
                            static_cast<uint32_t>(PT_COMPACT_WORDS),
                            static_cast<uint32_t>(PT_NOISE_SUMMARY_WORDS),
                            PT_COMPACT_FIRST,
                            PT_COMPACT_SECOND,
                            PT_COMPACT_LOST,
                            PT_COMPACT_CARRIED,
                            PT_COMPACT_WITH_CANDIDATES,
                            PT_COMPACT_MIN_INVERTED,
                            PT_COMPACT_MAX,
                            PT_COMPACT_WITH_RECORD,
                            PT_COMPACT_WRITTEN,
                            PT_COMPACT_NO_ROOM,
                            PT_COMPACT_HELD,
                            PT_NOISE_RATED,
                            PT_NOISE_UNRATED,
                            PT_NOISE_HELD,
                            PT_NOISE_MAX_BITS,
                            PT_NOISE_FIRST_BIN,
                            static_cast<uint32_t>(sizeof(PtNoiseRule)),
                            static_cast<uint32_t>(sizeof(PtDevOptions)),
                            static_cast<uint32_t>(offsetof(PtDevOptions, stats_sample_count)),
                            static_cast<uint32_t>(offsetof(PtNoiseRule, target)),
                            static_cast<uint32_t>(offsetof(PtNoiseRule, floor)),
                            static_cast<uint32_t>(offsetof(PtParkRecord, est)),
                            PT_STREAM_UNTOUCHED,
                            PT_STREAM_FINISHED,
                            PT_STREAM_PARKED,
                            PT_NO_PARK,
                            kPerBlock,
                            kCarry};
    std::memcpy(out, v, sizeof(v));
    return 32;
}

// pt_launch_frame_compact.  status [n_status], todo_out [n], block_counts [3 * ceil(n / 1024)], result [PT_COMPACT_WORDS], park_out [cap] and
// park_count [1] are given with their initial contents and come back as the device left them.  n_parked == 0: `parked` is park_out itself,
// as the frame passes it (under resort: park_in, and the launcher gets no park_out and no park_count, as from the frame).  todo_after,
// parked_after and park_in_after: the const inputs as they were on the device afterwards.
// place_only != 0: the count and place kernels alone, launched as the launcher launches them, without the carry: the list as the place
// kernel leaves it.
int frame_list_probe_compact(int place_only, const uint32_t *todo, uint32_t n, uint32_t *status, uint32_t n_status, const uint32_t *parked, uint32_t n_parked,
                             uint32_t *todo_out, uint32_t *block_counts, unsigned long long *result, int32_t target, const uint32_t *park_in, uint32_t n_park_in,
                             uint32_t *park_out, uint32_t *park_count, uint32_t cap, const PtNoiseRule *noise, int resort, uint32_t *todo_after,
                             uint32_t *parked_after, uint32_t *park_in_after) {
    Probe pr;
    GuardStatus &st = pr.st;
    const uint32_t n_blocks = (n + kPerBlock - 1) / kPerBlock;
    Guarded<uint2> d_todo(st, n, kBand, reinterpret_cast<const uint2 *>(todo)), d_todo_out(st, n, kBand, reinterpret_cast<const uint2 *>(todo_out));
    Guarded<uint32_t> d_status(st, n_status, kBand, status), d_blocks(st, 3 * static_cast<size_t>(n_blocks), kBand, block_counts), d_count(st, 1, kBand, park_count);
    Guarded<unsigned long long> d_result(st, PT_COMPACT_WORDS, kBand, result);
    Guarded<PtParkRecord> d_parked(st, n_parked, kBandRecords, records(parked)), d_park_in(st, n_park_in, kBandRecords, records(park_in));
    Guarded<PtParkRecord> d_park_out(st, cap, kBandRecords, records(park_out));
    if(st.ok()) {
        const PtParkRecord *p_parked = n_parked != 0 ? d_parked.p() : (resort != 0 ? d_park_in.p() : d_park_out.p());
        PtParkRecord *p_out = resort != 0 ? nullptr : d_park_out.p();
        uint32_t *p_count = resort != 0 ? nullptr : d_count.p();
        if(place_only == 0) {
            pr.launched(pt_launch_frame_compact(pr.stream, d_todo.p(), n, d_status.p(), p_parked, d_todo_out.p(), d_blocks.p(), d_result.p(), target, d_park_in.p(), p_out,
                                                p_count, cap, *noise, resort));
        }
        else {
            st(hipMemsetAsync(d_result.p(), 0, PT_COMPACT_WORDS * sizeof(unsigned long long), pr.stream));
            if(n != 0 && st.ok()) {
                pt_frame_count_kernel<<<n_blocks, kThreads, 0, pr.stream>>>(d_todo.p(), n, d_status.p(), d_blocks.p(), target, p_parked, d_park_in.p(), *noise);
                pt_frame_place_kernel<<<n_blocks, kThreads, 0, pr.stream>>>(d_todo.p(), n, d_status.p(), d_blocks.p(), n_blocks, p_parked, d_todo_out.p(), d_result.p(), target,
                                                                            d_park_in.p(), *noise, resort);
            }
        }
    }
    pr.wait();
    d_todo.get(reinterpret_cast<uint2 *>(todo_after));
    d_todo_out.get(reinterpret_cast<uint2 *>(todo_out));
    d_status.get(status);
    d_blocks.get(block_counts);
    d_count.get(park_count);
    d_result.get(result);
    d_parked.get(reinterpret_cast<PtParkRecord *>(parked_after));
    d_park_in.get(reinterpret_cast<PtParkRecord *>(park_in_after));
    d_park_out.get(reinterpret_cast<PtParkRecord *>(park_out));
    return pr.code();
}

// pt_launch_frame_gather: out_rgba [n][4] and out_at [n][2] given with their initial contents
int frame_list_probe_gather(const uint32_t *todo, uint32_t n, uint32_t n_parked, const uint32_t *park, uint32_t n_park, const int32_t *tiles, const uint32_t *tile_offset,
                            uint32_t n_tiles, int32_t width, float *out_rgba, int32_t *out_at) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<uint2> d_todo(st, n, kBand, reinterpret_cast<const uint2 *>(todo));
    Guarded<PtParkRecord> d_park(st, n_park, kBandRecords, records(park));
    Guarded<int4> d_tiles(st, n_tiles, kBand, reinterpret_cast<const int4 *>(tiles));
    Guarded<uint32_t> d_offset(st, n_tiles, kBand, tile_offset);
    Guarded<float4> d_rgba(st, n, kBand, reinterpret_cast<const float4 *>(out_rgba));
    Guarded<int2> d_at(st, n, kBand, reinterpret_cast<const int2 *>(out_at));
    if(st.ok()) {
        pr.launched(pt_launch_frame_gather(pr.stream, d_todo.p(), n, n_parked, d_park.p(), d_tiles.p(), d_offset.p(), n_tiles, width, d_rgba.p(), d_at.p()));
    }
    pr.wait();
    d_rgba.get(reinterpret_cast<float4 *>(out_rgba));
    d_at.get(reinterpret_cast<int2 *>(out_at));
    pr.same(d_todo, todo);
    pr.same(d_park, park);
    pr.same(d_tiles, tiles);
    pr.same(d_offset, tile_offset);
    return pr.code();
}

// pt_launch_frame_preview_base: view [n_pixels][4] and samples [n_pixels] given with their initial contents
int frame_list_probe_preview_base(float *view, int32_t *samples, const uint8_t *cover, uint32_t n_pixels) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<float4> d_view(st, n_pixels, kBand, reinterpret_cast<const float4 *>(view));
    Guarded<int32_t> d_samples(st, n_pixels, kBand, samples);
    Guarded<uint8_t> d_cover(st, n_pixels, kBand, cover);
    if(st.ok()) {
        pr.launched(pt_launch_frame_preview_base(pr.stream, d_view.p(), d_samples.p(), d_cover.p(), n_pixels));
    }
    pr.wait();
    d_view.get(reinterpret_cast<float4 *>(view));
    d_samples.get(samples);
    pr.same(d_cover, cover);
    return pr.code();
}

// pt_launch_frame_scatter: n entries into view [n_pixels][4] and samples [n_pixels], both given with their initial contents
int frame_list_probe_scatter(const float *rgba, const int32_t *at, uint32_t n, float *view, int32_t *samples, uint32_t n_pixels) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<float4> d_rgba(st, n, kBand, reinterpret_cast<const float4 *>(rgba)), d_view(st, n_pixels, kBand, reinterpret_cast<const float4 *>(view));
    Guarded<int2> d_at(st, n, kBand, reinterpret_cast<const int2 *>(at));
    Guarded<int32_t> d_samples(st, n_pixels, kBand, samples);
    if(st.ok()) {
        pr.launched(pt_launch_frame_scatter(pr.stream, d_rgba.p(), d_at.p(), n, d_view.p(), d_samples.p()));
    }
    pr.wait();
    d_view.get(reinterpret_cast<float4 *>(view));
    d_samples.get(samples);
    pr.same(d_rgba, rgba);
    pr.same(d_at, at);
    return pr.code();
}

// pt_launch_frame_rate: out [n][2] and summary [PT_NOISE_SUMMARY_WORDS] given with their initial contents
int frame_list_probe_rate(const uint32_t *todo, uint32_t n, const uint32_t *park, uint32_t n_park, const int32_t *tiles, const uint32_t *tile_offset, uint32_t n_tiles,
                          int32_t width, const PtNoiseRule *noise, uint32_t *out, uint32_t *summary) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<uint2> d_todo(st, n, kBand, reinterpret_cast<const uint2 *>(todo)), d_out(st, n, kBand, reinterpret_cast<const uint2 *>(out));
    Guarded<PtParkRecord> d_park(st, n_park, kBandRecords, records(park));
    Guarded<int4> d_tiles(st, n_tiles, kBand, reinterpret_cast<const int4 *>(tiles));
    Guarded<uint32_t> d_offset(st, n_tiles, kBand, tile_offset), d_summary(st, PT_NOISE_SUMMARY_WORDS, kBand, summary);
    if(st.ok()) {
        pr.launched(pt_launch_frame_rate(pr.stream, d_todo.p(), n, d_park.p(), d_tiles.p(), d_offset.p(), n_tiles, width, *noise, d_out.p(), d_summary.p()));
    }
    pr.wait();
    d_out.get(reinterpret_cast<uint2 *>(out));
    d_summary.get(summary);
    pr.same(d_todo, todo);
    pr.same(d_park, park);
    pr.same(d_tiles, tiles);
    pr.same(d_offset, tile_offset);
    return pr.code();
}

// pt_launch_frame_noise_base: map [n_pixels] given with its initial contents
int frame_list_probe_noise_base(float *map, const uint8_t *cover, uint32_t n_pixels) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<float> d_map(st, n_pixels, kBand, map);
    Guarded<uint8_t> d_cover(st, n_pixels, kBand, cover);
    if(st.ok()) {
        pr.launched(pt_launch_frame_noise_base(pr.stream, d_map.p(), d_cover.p(), n_pixels));
    }
    pr.wait();
    d_map.get(map);
    pr.same(d_cover, cover);
    return pr.code();
}

// pt_launch_frame_noise_scatter: n entries into map [n_pixels], given with its initial contents
int frame_list_probe_noise_scatter(const uint32_t *rated, uint32_t n, float *map, uint32_t n_pixels) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<uint2> d_rated(st, n, kBand, reinterpret_cast<const uint2 *>(rated));
    Guarded<float> d_map(st, n_pixels, kBand, map);
    if(st.ok()) {
        pr.launched(pt_launch_frame_noise_scatter(pr.stream, d_rated.p(), n, d_map.p()));
    }
    pr.wait();
    d_map.get(map);
    pr.same(d_rated, rated);
    return pr.code();
}

// pt_launch_frame_variance: out_var [n][4] and out_at [n] given with their initial contents
int frame_list_probe_variance(const uint32_t *todo, uint32_t n, const uint32_t *park, uint32_t n_park, const int32_t *tiles, const uint32_t *tile_offset, uint32_t n_tiles,
                              int32_t width, const PtDevOptions *opt, float *out_var, int32_t *out_at) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<uint2> d_todo(st, n, kBand, reinterpret_cast<const uint2 *>(todo));
    Guarded<PtParkRecord> d_park(st, n_park, kBandRecords, records(park));
    Guarded<int4> d_tiles(st, n_tiles, kBand, reinterpret_cast<const int4 *>(tiles));
    Guarded<uint32_t> d_offset(st, n_tiles, kBand, tile_offset);
    Guarded<float4> d_var(st, n, kBand, reinterpret_cast<const float4 *>(out_var));
    Guarded<int32_t> d_at(st, n, kBand, out_at);
    if(st.ok()) {
        pr.launched(pt_launch_frame_variance(pr.stream, d_todo.p(), n, d_park.p(), d_tiles.p(), d_offset.p(), n_tiles, width, *opt, d_var.p(), d_at.p()));
    }
    pr.wait();
    d_var.get(reinterpret_cast<float4 *>(out_var));
    d_at.get(out_at);
    pr.same(d_todo, todo);
    pr.same(d_park, park);
    pr.same(d_tiles, tiles);
    pr.same(d_offset, tile_offset);
    return pr.code();
}

// pt_launch_frame_variance_scatter: n entries into map [n_pixels][4], given with its initial contents
int frame_list_probe_variance_scatter(const float *var, const int32_t *at, uint32_t n, float *map, uint32_t n_pixels) {
    Probe pr;
    GuardStatus &st = pr.st;
    Guarded<float4> d_var(st, n, kBand, reinterpret_cast<const float4 *>(var)), d_map(st, n_pixels, kBand, reinterpret_cast<const float4 *>(map));
    Guarded<int32_t> d_at(st, n, kBand, at);
    if(st.ok()) {
        pr.launched(pt_launch_frame_variance_scatter(pr.stream, d_var.p(), d_at.p(), n, d_map.p()));
    }
    pr.wait();
    d_map.get(reinterpret_cast<float4 *>(map));
    pr.same(d_var, var);
    pr.same(d_at, at);
    return pr.code();
}

} // extern "C"
