/* pt_checkpoint.h -- checkpoints of a resumable frame.  Part of the C ABI of libpathtrace_hip.so: include/pt_hip.h
 * includes this file, which is not meant to be included on its own.
 *
 * A checkpoint is one contiguous little-endian BLOB in caller memory: everything a pt_frame needs to be finished later, by another
 * process, on another machine or on another number of replicas, bit-identically to an uninterrupted render.  It is a pure function of
 * the frame's state: it depends neither on how many replicas rendered the frame nor on the order in which its streams got there, so two
 * blobs of the same state are the same bytes.  The library does no file I/O; the scene is not in the blob.
 *
 * THE FORMAT (version 1).  Every section starts at a multiple of 16 bytes from the blob's start; the bytes between the end of a section
 * and the next multiple of 16 are 0.  In this order:
 *   header    one pt_checkpoint_header (below; 352 bytes, no implicit padding).  The sizes it states are those of the build that wrote it:
 *             a blob whose sizes differ from the reader's is refused, never reinterpreted.  camera / base_seed: a plain frame's; for a view
 *             frame (n_views > 1) those of view 0.  tile rectangles lie in the image of n_views * image_height rows.
 *   tables    n_views > 1 only: n_views pt_camera_params, then (at the next multiple of 16) n_views uint64 base seeds.  bytes_tables is
 *             the distance from the section's start to the end of the seeds.  n_views == 1: empty.
 *   tiles     n_tiles pt_tile, in the frame's order.
 *   map       one byte per stream in FRAME STREAM ORDER: tile after tile in the tile list, row-major inside a tile (the frame's own
 *             numbering, not a replica's).  Bits 0-1: the class, PT_CHECKPOINT_FINISHED / _UNTOUCHED / _RECORD (3 is invalid).  Bits 2-5:
 *             the record's est.n_candidates, 0..8 (0 unless the class is _RECORD).  Bits 6-7: 0.  Every later offset follows from the map.
 *   pixels    16 bytes (the rgba of the caller's image) per FINISHED stream, in stream order.
 *   records   one TRIMMED record per _RECORD stream, in stream order, 144 + 48 k bytes for a record with k candidates:
 *               int32 cursor, uint32 rng[2], 4 bytes of 0;  the 128-byte estimator with its `pad` word 0;  k candidates of 48 bytes
 *               (float mean[4], float m2[4], int32 count, 12 bytes of 0).
 *             Candidate slots a record has not written never reach the blob.
 *   trailer   uint64 checksum of every byte before it (their count is a multiple of 16), read as little-endian uint64 words w[0], w[1], ...
 *             in eight interleaved lanes, so that a reader is not bound by one chain of multiplications.  With
 *               step(h, v):  h ^= v;  h *= 0x100000001b3;  h ^= h >> 32      (64-bit, wrapping)
 *             lane l starts as h[l] = 0xcbf29ce484222325 + l and takes every word with i % 8 == l in order: h[l] = step(h[l], w[i]);
 *             the checksum is h[0] after h[0] = step(h[0], h[l]) for l = 1 .. 7 in order.
 *             total_bytes counts the trailer.
 * The FINGERPRINT is made of what a scene keeps on the host anyway: six counts and the bits of the root box.  It guards against loading
 * a blob onto the wrong scene by mistake and promises nothing more: two different scenes with equal counts and root box pass it.
 *
 * THE CALLS
 *   - pt_checkpoint_inspect: validates a blob and reports what it holds; needs no device.  PT_ERR_INVALID, naming the field, for a
 *     null argument, a wrong magic, version or size, any count that does not fit `bytes` (checked without overflow), a tile outside the
 *     image, tiles whose pixels are not n_streams, a map byte outside the rules above, section sizes other than the map implies, a record whose
 *     n_candidates is not its map byte's, padding that is not 0, or a wrong checksum.  No byte outside [blob, blob + bytes) is read.
 *   - pt_frame_checkpoint_size: the bytes pt_frame_checkpoint_save would write now.
 *   - pt_frame_checkpoint_save: `image` is the buffer the caller passes to pt_frame_render.  Only between two pt_frame_render calls (it
 *     takes the frame's lock).  *written (may be NULL) receives the blob's size; a capacity below it returns PT_ERR_INVALID with the
 *     needed size there.  A failed frame returns its code.  A frame that never launched saves (every stream untouched), a complete one
 *     too (every stream finished).  Saving changes nothing observable: the frame goes on and finishes bit-identically, and a second save
 *     at once gives the same bytes.
 *   - pt_frame_checkpoint_load: inspects the blob, compares its fingerprint with every scene (PT_ERR_INVALID naming the field), deals its
 *     tiles to the n_scenes replicas exactly as pt_frame_create does -- the replica count is free --, writes the finished pixels into
 *     out_image ([rows][width][4] floats) and leaves every other pixel of it alone, restores mode and counters.  The result is an ordinary
 *     pt_frame under every existing contract.  Any failure leaves no frame and no leak; *out is NULL then.
 * Not in a checkpoint: the scene, compression beyond trimming, blobs of another version, the history of a temporal denoiser, and
 * pt_render_tiles_ctl jobs (they never park). */
#ifndef PT_CHECKPOINT_H
#define PT_CHECKPOINT_H

#ifdef __cplusplus
extern "C" {
#endif

#define PT_CHECKPOINT_VERSION 1u
#define PT_CHECKPOINT_MAGIC "PTFRAME\x1a" /* 8 bytes */
#define PT_CHECKPOINT_FINISHED 0u
#define PT_CHECKPOINT_UNTOUCHED 1u
#define PT_CHECKPOINT_RECORD 2u
#define PT_CHECKPOINT_RECORD_BYTES 144u    /* a trimmed record without candidates */
#define PT_CHECKPOINT_CANDIDATE_BYTES 48u

typedef struct pt_checkpoint_fingerprint {
    uint64_t triangles, spheres, materials, point_lights, emitters, tree_nodes;
    uint32_t root_box[6]; /* the bits of the root box: lo.xyz, hi.xyz */
} pt_checkpoint_fingerprint;

typedef struct pt_checkpoint_header {
    uint8_t magic[8];
    uint32_t version;
    uint32_t header_bytes; /* sizeof(pt_checkpoint_header) */
    uint64_t total_bytes;
    uint32_t size_estimator, size_candidate, max_candidates, size_camera, size_options;
    int32_t n_views;
    uint64_t n_tiles, n_streams;
    uint64_t base_seed;
    pt_options options;
    pt_camera_params camera;
    int32_t quantum, max_passes_per_call, passes_completed, target, pass_in_progress;
    float noise_target, noise_floor, noise_fraction;
    int32_t follow_features;
    pt_feature_params feature_params;
    int32_t launches;
    uint64_t samples_lost;
    pt_checkpoint_fingerprint fingerprint;
    uint64_t streams_finished, streams_untouched, streams_with_record;
    uint64_t bytes_tables, bytes_tiles, bytes_map, bytes_pixels, bytes_records; /* without the padding behind them */
} pt_checkpoint_header;

typedef struct pt_checkpoint_info {
    uint64_t total_bytes, n_tiles, n_streams;
    uint64_t streams_finished, streams_untouched, streams_with_record, streams_with_candidates;
    uint64_t bytes_header, bytes_tables, bytes_tiles, bytes_map, bytes_pixels, bytes_records;
    uint64_t samples_lost;
    pt_checkpoint_fingerprint fingerprint;
    pt_options options;
    uint32_t version;
    int32_t n_views;
    int32_t quantum, max_passes_per_call, passes_completed, target, pass_in_progress;
    float noise_target, noise_floor, noise_fraction;
    int32_t follow_features;
    int32_t launches;
} pt_checkpoint_info;

int pt_checkpoint_inspect(const void *blob, size_t bytes, pt_checkpoint_info *out);
int pt_frame_checkpoint_size(pt_frame *frame, size_t *bytes);
int pt_frame_checkpoint_save(pt_frame *frame, const float *image, void *blob, size_t capacity, size_t *written);
int pt_frame_checkpoint_load(pt_scene *const *scenes, int n_scenes, const void *blob, size_t bytes, float *out_image, pt_frame **out);

#ifdef __cplusplus
}
#endif

#endif
