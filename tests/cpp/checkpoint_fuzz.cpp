// TEST ONLY: a stand-alone program that feeds the parser of a frame checkpoint's blob (pt_checkpoint_format.cpp, which has no HIP in it)
// truncated and damaged blobs.  Built with -fsanitize=address,undefined as an ordinary host program by tests/test_checkpoint_cpu.py; every
// blob it tries lives in a heap buffer of exactly its size, so a read past the end is a sanitizer report.  The blobs it starts from are
// its own writer's: a plain frame and a frame of three views, with every class of stream and every candidate count.
#include "pt_checkpoint_format.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {
std::string g_error;
uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t next() { // xorshift64: a fixed-seed sample
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}
} // namespace

namespace pth {
int fail(int code, const std::string &msg) {
    g_error = msg;
    return code;
}
} // namespace pth

static std::vector<uint8_t> make_blob(int32_t n_views) {
    pt_checkpoint_header h{};
    h.n_views = n_views;
    h.options.image_width = 40;
    h.options.image_height = 12;
    h.options.min_sample_count = 4;
    h.options.max_sample_count = 64;
    h.options.epsilon = 1e-4f;
    h.noise_floor = 1e-5f;
    h.noise_fraction = 1.0f;
    h.quantum = 8;
    h.target = 16;
    std::vector<pt_tile> tiles;
    for(int32_t v = 0; v < n_views; v++) {
        tiles.push_back(pt_tile{0, 12 * v, 32, 12});
        tiles.push_back(pt_tile{32, 12 * v, 8, 12});
    }
    h.n_tiles = tiles.size();
    h.n_streams = static_cast<uint64_t>(n_views) * 40 * 12;
    std::vector<uint8_t> map(h.n_streams);
    std::vector<uint8_t> pixels, records;
    for(uint64_t i = 0; i < h.n_streams; i++) {
        const unsigned cls = static_cast<unsigned>(next() % 3), k = static_cast<unsigned>(next() % 9);
        map[i] = static_cast<uint8_t>(cls == PT_CHECKPOINT_RECORD ? cls | (k << 2) : cls);
        if(cls == PT_CHECKPOINT_FINISHED) {
            for(int b = 0; b < 16; b++) {
                pixels.push_back(static_cast<uint8_t>(next()));
            }
        }
        else if(cls == PT_CHECKPOINT_RECORD) {
            const size_t at = records.size();
            for(unsigned b = 0; b < PT_CHECKPOINT_RECORD_BYTES + k * PT_CHECKPOINT_CANDIDATE_BYTES; b++) {
                records.push_back(static_cast<uint8_t>(next()));
            }
            const int32_t n_candidates = static_cast<int32_t>(k);
            std::memcpy(records.data() + at + 16 + 116, &n_candidates, 4);
        }
    }
    std::vector<pt_camera_params> cams(static_cast<size_t>(n_views));
    std::vector<uint64_t> seeds(static_cast<size_t>(n_views), 1234);
    size_t written = 0;
    (void)ptc::write(nullptr, 0, h, cams.data(), seeds.data(), tiles.data(), map.data(), pixels.data(), records.data(), records.size(), &written);
    std::vector<uint8_t> blob(written);
    if(ptc::write(blob.data(), blob.size(), h, cams.data(), seeds.data(), tiles.data(), map.data(), pixels.data(), records.data(), records.size(), &written) != PT_OK) {
        std::printf("checkpoint_fuzz: the writer failed: %s\n", g_error.c_str());
        std::exit(2);
    }
    return blob;
}

// The parser and pt_checkpoint_inspect on a copy of exactly `n` bytes: PT_OK or PT_ERR_INVALID, and both agree
static int attempt(const uint8_t *bytes, size_t n, const char *what, size_t where) {
    std::unique_ptr<uint8_t[]> copy(new uint8_t[n > 0 ? n : 1]);
    if(n > 0) {
        std::memcpy(copy.get(), bytes, n);
    }
    ptc::Parsed parsed;
    const int a = ptc::parse(copy.get(), n, &parsed, true);
    pt_checkpoint_info info;
    const int b = pt_checkpoint_inspect(copy.get(), n, &info);
    if((a != PT_OK && a != PT_ERR_INVALID) || a != b || (a == PT_ERR_INVALID && g_error.empty())) {
        std::printf("checkpoint_fuzz: %s at %zu: parse %d, inspect %d (%s)\n", what, where, a, b, g_error.c_str());
        std::exit(1);
    }
    return a;
}

int main() {
    size_t tried = 0, accepted = 0;
    for(int32_t n_views : {1, 3}) {
        const std::vector<uint8_t> blob = make_blob(n_views);
        if(attempt(blob.data(), blob.size(), "the writer's blob", 0) != PT_OK) {
            std::printf("checkpoint_fuzz: the writer's blob is refused: %s\n", g_error.c_str());
            return 1;
        }
        // truncated at every length up to the end of the header, and at a stride beyond
        for(size_t n = 0; n < blob.size(); n += n <= sizeof(pt_checkpoint_header) + 16 ? 1 : 97) {
            tried++;
            if(attempt(blob.data(), n, "truncation", n) == PT_OK) {
                std::printf("checkpoint_fuzz: a blob truncated to %zu bytes is accepted\n", n);
                return 1;
            }
        }
        // every bit of the header, alone; the checksum stays, then is made right again so that the field itself is judged
        std::vector<uint8_t> work = blob;
        ptc::Layout at;
        pt_checkpoint_header h;
        std::memcpy(&h, blob.data(), sizeof(h));
        if(ptc::layout(h, &at) != PT_OK) {
            return 1;
        }
        for(size_t bit = 0; bit < 8 * sizeof(pt_checkpoint_header); bit++) {
            work[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
            tried += 2;
            if(attempt(work.data(), work.size(), "header bit", bit) == PT_OK) {
                std::printf("checkpoint_fuzz: header bit %zu flipped and the checksum holds\n", bit);
                return 1;
            }
            const uint64_t sum = ptc::checksum(work.data(), at.trailer);
            std::memcpy(work.data() + at.trailer, &sum, 8);
            accepted += attempt(work.data(), work.size(), "header bit, checksum mended", bit) == PT_OK ? 1 : 0;
            work = blob;
        }
        // a fixed-seed sample of bits elsewhere, one to four at a time, with and without a mended checksum
        for(int round = 0; round < 4000; round++) {
            const int flips = 1 + static_cast<int>(next() % 4);
            for(int f = 0; f < flips; f++) {
                const size_t bit = sizeof(pt_checkpoint_header) * 8 + static_cast<size_t>(next() % ((blob.size() - sizeof(pt_checkpoint_header)) * 8));
                work[bit / 8] ^= static_cast<uint8_t>(1u << (bit % 8));
            }
            tried++;
            if(round % 2 == 1) {
                const uint64_t sum = ptc::checksum(work.data(), at.trailer);
                std::memcpy(work.data() + at.trailer, &sum, 8);
            }
            accepted += attempt(work.data(), work.size(), "body bits", static_cast<size_t>(round)) == PT_OK ? 1 : 0;
            work = blob;
        }
    }
    std::printf("checkpoint_fuzz: ok, %zu blobs tried, %zu of the damaged ones still valid checkpoints\n", tried, accepted);
    return 0;
}
