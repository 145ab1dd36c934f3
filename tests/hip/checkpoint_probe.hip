// TEST ONLY: the per-stream and per-unit functions of the checkpoint kernels (pt_checkpoint_kernels.h of the product, PT_CHECKPOINT_HOST)
// compiled for the HOST against tests/hip/host_checkpoint, as tests/hip/query_probe.hip compiles query_record, together with the blob's
// writer and parser (pt_checkpoint_format.cpp, which has no HIP in it).  checkpoint_probe_pack / _unpack are pack and unpack of one
// replica with the kernels' decisions and a serial scan in place of the workgroup scans; tests/test_checkpoint_cpu.py runs them on
// synthetic replicas.
#define PT_CHECKPOINT_HOST
#include "pt_checkpoint_kernels.h"

#include "pt_checkpoint_format.h"

#include <cstring>
#include <string>

namespace {
thread_local std::string g_error;
}

namespace pth {
int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
} // namespace pth

extern "C" {

const char *checkpoint_probe_last_error() {
    return g_error.c_str();
}

int checkpoint_probe_sizes(uint32_t *header, uint32_t *info, uint32_t *record) {
    *header = sizeof(pt_checkpoint_header);
    *info = sizeof(pt_checkpoint_info);
    *record = sizeof(PtParkRecord);
    return 0;
}

// ptc::write over plain arrays
int checkpoint_probe_write(const pt_checkpoint_header *h, const pt_camera_params *cams, const uint64_t *seeds, const pt_tile *tiles, const uint8_t *map, const void *pixels,
                           const void *records, uint64_t record_bytes, void *blob, size_t capacity, size_t *written) {
    return ptc::write(blob, capacity, *h, cams, seeds, tiles, map, pixels, records, record_bytes, written);
}

// ptc::parse: the per-tile tables ([n_tiles + 1] each, may be null) and the sections' offsets (7 words: tables, seeds, tiles, map, pixels, records, trailer)
int checkpoint_probe_parse(const void *blob, size_t bytes, uint64_t *offsets, uint64_t *tile_stream, uint64_t *tile_finished, uint64_t *tile_record_bytes, size_t n_tiles) {
    ptc::Parsed p;
    const int rc = ptc::parse(blob, bytes, &p, true);
    if(rc != PT_OK) {
        return rc;
    }
    const uint64_t at[7] = {p.at.tables, p.at.seeds, p.at.tiles, p.at.map, p.at.pixels, p.at.records, p.at.trailer};
    memcpy(offsets, at, sizeof(at));
    if(tile_stream != nullptr && n_tiles + 1 == p.tile_stream.size()) {
        memcpy(tile_stream, p.tile_stream.data(), (n_tiles + 1) * 8);
        memcpy(tile_finished, p.tile_finished.data(), (n_tiles + 1) * 8);
        memcpy(tile_record_bytes, p.tile_record_bytes.data(), (n_tiles + 1) * 8);
    }
    return PT_OK;
}

// Pack of one replica, as pt_launch_checkpoint_pack: slot is n_streams words of scratch; out_records may be null (the sizes only)
int checkpoint_probe_pack(const uint2 *todo, uint32_t n_todo, const PtParkRecord *park, uint32_t park_cap, uint32_t n_streams, uint32_t *slot, const float4 *image,
                          const int4 *tiles, const uint32_t *tile_offset, uint32_t n_tiles, int32_t width, uint8_t *map, float4 *out_pixels, uint4 *out_records,
                          unsigned long long *tile_finished, unsigned long long *tile_units, unsigned long long *totals) {
    memset(totals, 0, PT_CKPT_TOTALS * sizeof(unsigned long long));
    memset(slot, 0, (size_t)n_streams * sizeof(uint32_t));
    for(uint32_t i = 0; i < n_todo; i++) {
        if(todo[i].x < n_streams) {
            slot[todo[i].x] = ptd::ckpt_slot(todo[i]);
        }
    }
    unsigned long long fin = 0, units = 0;
    for(uint32_t s = 0; s < n_streams; s++) {
        uint32_t bad = 0;
        const uint8_t m = ptd::ckpt_map_byte(slot[s], park, park_cap, &bad);
        totals[PT_CKPT_TOTAL_BAD] |= bad;
        map[s] = m;
        const uint32_t tile = ptd::ckpt_stream_tile(s, tile_offset, n_tiles);
        if(tile_offset[tile] == s) {
            tile_finished[tile] = fin;
            tile_units[tile] = units;
        }
        if((m & 3u) == PT_CKPT_FINISHED) {
            if(out_records != nullptr) {
                out_pixels[fin] = image[ptd::ckpt_stream_pixel(s, tile, tiles, tile_offset, width)];
            }
            fin++;
        }
        const uint32_t n = ptd::ckpt_units(m);
        for(uint32_t j = 0; j < n && out_records != nullptr; j++) {
            out_records[units + j] = ptd::ckpt_pack_unit(park + (slot[s] - PT_CKPT_RECORD), j);
        }
        units += n;
    }
    totals[PT_CKPT_TOTAL_FINISHED] = fin;
    totals[PT_CKPT_TOTAL_UNITS] = units;
    return 0;
}

// Unpack of one replica, as pt_launch_checkpoint_unpack; summary: the PT_CKPT_PARTIALS words over the whole replica
int checkpoint_probe_unpack(const uint8_t *map, uint32_t n_streams, const uint4 *trimmed, uint2 *todo, PtParkRecord *park, unsigned long long *summary) {
    uint32_t n_records = 0;
    for(uint32_t s = 0; s < n_streams; s++) {
        n_records += (map[s] & 3u) == PT_CKPT_RECORD ? 1u : 0u;
    }
    unsigned long long units = 0, carried = 0, with_candidates = 0, least = 0xffffffffull, most = 0;
    uint32_t rec = 0, unt = 0;
    for(uint32_t s = 0; s < n_streams; s++) {
        const uint8_t m = map[s];
        if((m & 3u) == PT_CKPT_FINISHED) {
            continue;
        }
        unsigned long long samples = 0;
        if((m & 3u) == PT_CKPT_RECORD) {
            todo[rec] = make_uint2(s, rec);
            samples = (uint32_t)ptd::ckpt_samples(trimmed + units);
            with_candidates += (m >> 2) != 0 ? 1 : 0;
            for(uint32_t j = 0; j < PT_CKPT_FULL_UNITS; j++) {
                reinterpret_cast<uint4 *>(park + rec)[j] = ptd::ckpt_unpack_unit(trimmed + units, (uint32_t)(m >> 2) & 15u, s, j);
            }
            rec++;
            units += ptd::ckpt_units(m);
        }
        else {
            todo[n_records + unt] = make_uint2(s, PT_NO_PARK);
            unt++;
        }
        carried += samples;
        least = samples < least ? samples : least;
        most = samples > most ? samples : most;
    }
    summary[PT_CKPT_CARRIED] = carried;
    summary[PT_CKPT_WITH_CANDIDATES] = with_candidates;
    summary[PT_CKPT_MIN] = least;
    summary[PT_CKPT_MAX] = most;
    return 0;
}

} // extern "C"
