/*
 * clay.h -- C ABI of the MI355X-native Clay (Coupled-Layer MSR) erasure-code engine.
 *
 * Drop-in boundary for the `ClayCode` API of spool-labs/clay (crate clay-codes
 * 0.1.2).  Every entry point names the reference interface it replaces.  The
 * signatures use plain pointers and sizes only (no torch / HIP types): a Rust
 * `extern "C"` block, ctypes, JNI or cgo binds them directly.
 *
 * Conventions
 *   - Return value: 0 on success, otherwise the error kind (enum clay_error_kind);
 *     if `err` is non-NULL it receives kind, payload fields and the Display text
 *     of the reference's ClayError (error.rs:26-54).
 *   - All buffers are caller-allocated; size-query helpers replace Rust's owned
 *     Vec returns.  `HashMap<usize, Vec<u8>>` arguments become parallel arrays
 *     (ids[i], bufs[i], lens[i]); where the reference depends on HashMap
 *     iteration order (decode.rs:54-56, repair.rs:225) this ABI uses array order.
 *   - Thread safety: like the reference (ClayCode is immutable, lib.rs:58), all
 *     functions may be called concurrently, from any thread, on any stream.  There is
 *     no process-wide lock: plan caches and per-device buffer pools are locked only
 *     for bookkeeping, never across a launch or a wait on the caller's stream.
 *   - Device buffers the library needs (U workspaces of decode/repair/staged encode,
 *     staging buffers of the host API) come from a per-device pool; a buffer is reused
 *     once the event recorded after its last use has completed, so streams that come
 *     and go do not grow device memory.  Buffers and pointer tables first used inside
 *     a stream capture stay reserved for the captured graph.
 *   - Host-buffer functions (clay_encode / clay_decode / clay_repair) copy to the
 *     GPU, run the HIP kernels and copy back.  *_device functions take device
 *     pointers and a hipStream_t (passed as void*) and are asynchronous.
 *   - There is no CPU fallback: without a usable GPU, compute entry points fail
 *     with CLAY_ERR_DEVICE.
 */
#ifndef CLAY_H
#define CLAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLAY_ABI_VERSION 4

/* ClayCode public fields (lib.rs:59-82) + the two private RS counts (lib.rs:79-81). */
typedef struct clay_code {
    size_t k, m, n, d, q, t, nu, sub_chunk_no, beta;
    size_t original_count, recovery_count;
} clay_code_t;

/* ClayError (error.rs:5-24).  Payload fields a,b,c follow declaration order:
 *   InsufficientHelpers{needed, provided}           -> a, b
 *   InvalidChunkSize{expected, actual}              -> a, b
 *   InsufficientHelperData{helper, expected, actual}-> a, b, c
 *   InconsistentChunkSizes{first_size, mismatched_idx, mismatched_size} -> a, b, c
 *   TooManyErasures{max, actual}                    -> a, b
 *   MissingYSectionHelper{lost_node, missing_helper}-> a, b
 * String variants carry their text in msg only. */
enum clay_error_kind {
    CLAY_OK = 0,
    CLAY_ERR_INVALID_PARAMETERS = 1,
    CLAY_ERR_INSUFFICIENT_HELPERS = 2,
    CLAY_ERR_INVALID_CHUNK_SIZE = 3,
    CLAY_ERR_INSUFFICIENT_HELPER_DATA = 4,
    CLAY_ERR_INCONSISTENT_CHUNK_SIZES = 5,
    CLAY_ERR_TOO_MANY_ERASURES = 6,
    CLAY_ERR_RECONSTRUCTION_FAILED = 7,
    CLAY_ERR_MISSING_Y_SECTION_HELPER = 8,
    CLAY_ERR_OVERFLOW = 9,
    /* not in the reference: HIP runtime / device failure, unsupported device shape */
    CLAY_ERR_DEVICE = 100,
};

typedef struct clay_error {
    int kind;
    size_t a, b, c;
    char msg[256];
} clay_error_t;

/* ------------------------------------------------------------------ */
/* Parameters                                                          */
/* ------------------------------------------------------------------ */

/* ClayCode::new(k, m, d)            -- lib.rs:94-147 */
int clay_new(size_t k, size_t m, size_t d, clay_code_t *out, clay_error_t *err);
/* ClayCode::new_default(k, m)       -- lib.rs:150-152 (d = k + m - 1) */
int clay_new_default(size_t k, size_t m, clay_code_t *out, clay_error_t *err);
/* ClayCode::normalized_repair_bandwidth -- lib.rs:239-241 */
double clay_normalized_repair_bandwidth(const clay_code_t *code);
/* Chunk size ClayCode::encode produces for `data_len` bytes -- encode.rs:33-42 */
size_t clay_encoded_chunk_size(const clay_code_t *code, size_t data_len);

/* ------------------------------------------------------------------ */
/* Host-buffer API (mirrors the reference semantics)                   */
/* ------------------------------------------------------------------ */

/* ClayCode::encode(data) -> Vec<Vec<u8>>   -- lib.rs:176-178, encode.rs:30-80.
 * out_chunks: n host buffers of chunk_size bytes (chunk_size must equal
 * clay_encoded_chunk_size(code, len)); [0,k) receive the zero-padded data
 * chunks, [k,n) the parity chunks.  The reference panics on an internal error
 * (encode.rs:67-68); this ABI returns CLAY_ERR_RECONSTRUCTION_FAILED instead. */
int clay_encode(const clay_code_t *code, const uint8_t *data, size_t len,
                uint8_t *const *out_chunks, size_t chunk_size, clay_error_t *err);

/* ClayCode::decode(available, erasures) -> Vec<u8> -- lib.rs:188-194, decode.rs:31-161.
 * available: n_avail entries (ids, bufs, lens).  out receives k*chunk bytes
 * (the first k internal chunks, padding included, decode.rs:155-158);
 * *out_len = k*chunk (0 for the empty/empty case).  out_cap < k*chunk ->
 * CLAY_ERR_INVALID_PARAMETERS. */
int clay_decode(const clay_code_t *code, const size_t *ids, const uint8_t *const *bufs,
                const size_t *lens, size_t n_avail, const size_t *erasures, size_t n_erasures,
                uint8_t *out, size_t out_cap, size_t *out_len, clay_error_t *err);

/* ClayCode::minimum_to_repair(lost, available) -- lib.rs:207-213, repair.rs:61-126.
 * Every helper needs the same sub-chunk list (repair.rs:102,113), so the result
 * is helpers_out[0..*n_helpers) (capacity >= d) plus one index list
 * subchunks_out[0..*n_subchunks) (capacity >= beta). */
int clay_minimum_to_repair(const clay_code_t *code, size_t lost_node, const size_t *available,
                           size_t n_available, size_t *helpers_out, size_t *n_helpers,
                           size_t *subchunks_out, size_t *n_subchunks, clay_error_t *err);

/* ClayCode::repair(lost, helper_data, chunk_size) -- lib.rs:226-233, repair.rs:140-421.
 * helper i: ids[i], bufs[i] (lens[i] bytes = the beta sub-chunks concatenated in
 * minimum_to_repair order).  out receives chunk_size bytes. */
int clay_repair(const clay_code_t *code, size_t lost_node, const size_t *ids,
                const uint8_t *const *bufs, const size_t *lens, size_t n_helpers,
                size_t chunk_size, uint8_t *out, clay_error_t *err);

/* ------------------------------------------------------------------ */
/* Device-resident API (HBM in, HBM out; asynchronous on `stream`)      */
/* ------------------------------------------------------------------ */

/* Encode one stripe already resident in HBM.  data_chunks: k device pointers
 * (chunk_size bytes each, chunk_size % sub_chunk_no == 0), parity_chunks: m
 * device pointers.  Pointer arrays themselves are host memory.  Same bytes as
 * clay_encode's parity for the same (padded) data.  stream: hipStream_t or NULL. */
int clay_encode_device(const clay_code_t *code, const uint8_t *const *data_chunks,
                       uint8_t *const *parity_chunks, size_t chunk_size, int device,
                       void *stream, clay_error_t *err);

/* Batched encode: `n_stripes` independent stripes, stripe s uses
 * data_chunks[s*k .. s*k+k) and parity_chunks[s*m .. s*m+m).
 * (10,4,13) and (9,4,12), 2 or more stripes whose chunks are rows of one buffer (one
 * stride for all data chunks, one for all parity chunks), every chunk and both strides
 * 8-byte aligned, sub-chunk a multiple of 8 and at least 16 bytes: ONE launch of the
 * batched streaming kernel (clay_last_encode_path "stream-batch-k10m4-w256-l4" /
 * "stream-batch-k9m4-w256-l4", clay_last_launch_count 1) under encode path auto for stripes
 * of more than 4 MiB of data with sub-chunks up to 262,152 bytes, and under "stream"
 * (variant 0 or 4) at any size.  It allocates nothing and uploads no pointer table, so it
 * can be captured without a warm call.  Everything else runs as before: smaller stripes
 * the staged batch, other layouts one launch per stripe. */
int clay_encode_device_batch(const clay_code_t *code, const uint8_t *const *data_chunks,
                             uint8_t *const *parity_chunks, size_t n_stripes, size_t chunk_size,
                             int device, void *stream, clay_error_t *err);

/* Host-streaming encode (host memory in, host memory out; blocking).  data_chunks:
 * k host pointers, parity_chunks: m host pointers (chunk_size bytes each; pin
 * them, e.g. hipHostMalloc / hipHostRegister, for overlap).  The stripe is cut
 * into pieces of piece_bytes (0 = auto, ~128 MiB of input per piece) of every
 * sub-chunk; each piece is copied in with one 2D copy per node, encoded on the
 * device and its parity copied out, round-robin over n_streams (0 = 2) streams
 * so H2D, encode and D2H of consecutive pieces overlap.  Same parity bytes as
 * clay_encode / clay_encode_device.  Replaces the host-side entry of
 * ClayCode::encode (lib.rs:165-167 -> encode.rs:30-80) for callers that hold
 * the data chunks in host memory. */
int clay_encode_host_pipelined(const clay_code_t *code, const uint8_t *const *data_chunks,
                               uint8_t *const *parity_chunks, size_t chunk_size, int device,
                               size_t piece_bytes, int n_streams, clay_error_t *err);

/* Batched encode of n_stripes stripes laid out at fixed strides in device memory
 * (the reference encodes one stripe per call, encode.rs:30-80):
 * data node i of stripe s at data + s*data_stripe_stride + i*data_node_stride, parity
 * node j at parity + s*parity_stripe_stride + j*parity_node_stride (bytes; e.g. a
 * contiguous [n_stripes][k][chunk] buffer has node stride chunk, stripe stride k*chunk).
 * Same results as clay_encode_device_batch with the equivalent pointer arrays, with O(1)
 * host work per call.  Asynchronous on `stream`.
 * (10,4,13) and (9,4,12) with base pointers and all four strides 8-byte aligned and the
 * sub-chunk a multiple of 8 (at least 16): 2 or more stripes are ONE launch of the batched
 * streaming kernel ("stream-batch-k10m4-w256-l4" / "stream-batch-k9m4-w256-l4"), under auto
 * for stripes of more than 4 MiB of data with sub-chunks up to 262,152 bytes and under
 * "stream" (variant 0 or 4) at any size; see clay_encode_device_batch. */
int clay_encode_device_strided(const clay_code_t *code, const uint8_t *data, int64_t data_node_stride,
                               int64_t data_stripe_stride, uint8_t *parity, int64_t parity_node_stride,
                               int64_t parity_stripe_stride, size_t n_stripes, size_t chunk_size, int device,
                               void *stream, clay_error_t *err);

/* Scrub: do the stored chunks of a stripe still form a codeword?  (reed-solomon-erasure,
 * the crate under the reference, ships `verify`; the reference's Clay layer has no
 * counterpart.)  data_chunks: k device pointers, parity_chunks: m device pointers
 * (chunk_size bytes each), all read only: nothing is ever written to them.  result:
 * device memory of one uint32_t, defined by the call (the caller need not clear it): bit j
 * is set iff parity chunk j (node k + j) differs, at any byte, from the parity
 * clay_encode_device gives for the data chunks.  A mismatch is a result, not an error: the
 * call returns CLAY_OK.  Asynchronous on `stream`: the clear of `result`, then one launch of
 * the compare-ending variant of the bit-sliced encode, which loads the stored parity where
 * the encode stores it.  (The clear is a small launch of the same kernel in its clear mode,
 * not a hipMemsetAsync -- a captured memset node has been seen to replay a stale fill value --
 * and like a memset it is not counted in clay_last_launch_count.)  No scratch memory, no
 * allocation, so the call may be captured unprepared.
 * Any sub-chunk size and alignment.  Codes: (4,2,5), (6,3,8), (8,4,11), (9,3,11) and
 * (10,4,13); any other code is CLAY_ERR_INVALID_PARAMETERS.  Validation is
 * clay_encode_device's; a NULL result is CLAY_ERR_INVALID_PARAMETERS.  Last exec path
 * "bs-scrub1" ((4,2,5); k_bs_encode1) or "bs-scrub" (k_bs_encode; (4,2,5) under exec modes
 * 1 / 2).  clay_set_encode_path has no effect.
 * (10,4,13) at streaming speed: a stripe on 8-byte rows -- sub-chunk size a multiple of 8 and at
 * least 16 (and 256 x sub-chunk < 2^32), every data and parity chunk 8-byte aligned -- runs the
 * compare-ending variant of the streaming encode k_stream_encode, last exec path "stream-scrub":
 * under exec mode 3 stream at any such sub-chunk, under 0 auto, 5 and 6 from a sub-chunk of
 * 65,536 bytes (one full round of 256-byte tiles on every CU; below it v1 is faster).  Exec
 * modes 1 / 2 keep v1 ("bs-scrub"), its A/B partner, and so does every stripe off 8-byte rows in
 * every mode.  The 1 GiB stripe: 0.32 ms against 0.70 on v1 (the encode: 0.33). */
int clay_scrub_device(const clay_code_t *code, const uint8_t *const *data_chunks,
                      const uint8_t *const *parity_chunks, size_t chunk_size, uint32_t *result,
                      int device, void *stream, clay_error_t *err);

/* Batched scrub: `n_stripes` independent stripes, stripe s uses data_chunks[s*k .. s*k+k)
 * and parity_chunks[s*m .. s*m+m); result: n_stripes uint32_t in device memory, result[s]
 * the mask of stripe s, every word defined by the call.  Stripes that sit at one data and
 * one parity stride (rows of one buffer) run in ONE launch at any sub-chunk size (last exec
 * path "bs-scrub1-batch" / "bs-scrub-batch"); any other arrangement takes one launch per
 * stripe ("bs-scrub1" / "bs-scrub", clay_last_launch_count = n_stripes).  (10,4,13) on the
 * streaming kernel (see clay_scrub_device; EVERY stripe of the call must be on 8-byte rows,
 * else none takes it: one path per call): 2 or more stripes at one data and one parity stripe
 * stride (a data stride of 0 included) can run in ONE launch of its batch variant, last exec path
 * "stream-scrub-batch", clay_last_launch_count = 1 -- for every such call under
 * clay_set_scrub_path(1); by default (scrub path 0 auto, exec modes 0 / 5 / 6) for sub-chunks of
 * 2,048 to 66,176 bytes when the first stripes of the batch's workgroup groups give every XCD at
 * least 20 full 256-byte tiles (min(G, n_stripes) x the XCD's share of a row >= 5,120 bytes, G =
 * the groups of one stripe's workgroups an XCD holds; e.g. 20 stripes at 2,048, 5 at 8,192, 2 from
 * 20,480): there it beat the path below in every measured case, 2.0-2.2x for 1 GiB of stripes of
 * 5 to 80 MiB.  Every other call on the streaming kernel ("stream-scrub": exec
 * mode 3 stream with scrub path auto, sub-chunks from 65,536 bytes outside the gate, stripes off
 * the stride) is one launch per stripe in the batch and strided forms too, clay_last_launch_count
 * = n_stripes.  n_stripes = 0 returns CLAY_OK and touches nothing. */
int clay_scrub_device_batch(const clay_code_t *code, const uint8_t *const *data_chunks,
                            const uint8_t *const *parity_chunks, uint32_t *result, size_t n_stripes,
                            size_t chunk_size, int device, void *stream, clay_error_t *err);

/* Batched scrub of stripes at fixed strides, the layout of clay_encode_device_strided: data
 * node i of stripe s at data + s*data_stripe_stride + i*data_node_stride, parity node j at
 * parity + s*parity_stripe_stride + j*parity_node_stride.  One launch, O(1) host work --
 * also for (10,4,13) on the streaming kernel's batch variant ("stream-scrub-batch": both bases
 * and all four strides multiples of 8; see clay_scrub_device_batch and clay_set_scrub_path for
 * when it is taken); "stream-scrub" is one launch per stripe.  Bytes between the chunks are never
 * read into the answer. */
int clay_scrub_device_strided(const clay_code_t *code, const uint8_t *data, int64_t data_node_stride,
                              int64_t data_stripe_stride, const uint8_t *parity, int64_t parity_node_stride,
                              int64_t parity_stripe_stride, uint32_t *result, size_t n_stripes,
                              size_t chunk_size, int device, void *stream, clay_error_t *err);

/* Host-buffer scrub, in the spirit of reed-solomon-erasure's `verify`: chunks = the n host
 * chunks of a stripe (k data, then m parity; chunk_size bytes each, chunk_size %
 * sub_chunk_no == 0).  Copies them to the current device (one pooled buffer), scrubs, and
 * returns the mask of clay_scrub_device in *mask_out (host memory) once its own work is
 * done; 0 = a codeword.  Validates as clay_encode_host_pipelined; same codes as
 * clay_scrub_device. */
int clay_verify(const clay_code_t *code, const uint8_t *const *chunks, size_t chunk_size,
                uint32_t *mask_out, clay_error_t *err);

/* Y-grouped chunk layout ("Option C" of the reference's
 * docs/clay-practical-implementation.md:416-582, in the crate's MSB-first digit order):
 * for y-section y, the chunk's alpha sub-chunks reordered as blocks x = 0..q-1 of beta
 * sub-chunks, block x = the layers z with digit_y(z) == x in ascending order
 * (= get_repair_subchunk_indices of node (y, x), repair.rs:22-49).  A helper stored this
 * way serves the repair of node (y, x) from ONE contiguous range, group + x*beta*sc, which
 * can be passed straight to clay_repair_device.  Device buffers of chunk_size bytes, not
 * in place; asynchronous on `stream`. */
int clay_chunk_to_ygroup(const clay_code_t *code, size_t y, const uint8_t *chunk, uint8_t *group,
                         size_t chunk_size, int device, void *stream, clay_error_t *err);
int clay_ygroup_to_chunk(const clay_code_t *code, size_t y, const uint8_t *group, uint8_t *chunk,
                         size_t chunk_size, int device, void *stream, clay_error_t *err);

/* Decode / rebuild on device.  chunks: n device pointers, NULL for every erased
 * node (validation as decode.rs:36-126 with available = the non-NULL entries).
 * out_chunks: n device pointers; for every erased DATA node out_chunks[i] must
 * be non-NULL and receives the rebuilt chunk; for an erased PARITY node a
 * non-NULL out_chunks[i] also receives the rebuilt parity chunk (the value the
 * reference computes internally, decode.rs:213-253); other entries are ignored. */
int clay_decode_device(const clay_code_t *code, const uint8_t *const *chunks,
                       const size_t *erasures, size_t n_erasures, uint8_t *const *out_chunks,
                       size_t chunk_size, int device, void *stream, clay_error_t *err);

/* clay_decode_device for callers whose chunks are ONE CODEWORD (the crate's own usage: chunks
 * that ClayCode::encode produced), chosen per call.  A decode of one erased node with every other
 * node present, in a q = m code with a streaming repair kernel ((9,3,11), (10,4,13), (4,2,5)),
 * rebuilds the node with the repair of repair.rs:140-421 from the whole chunks (last exec path
 * "bs-repair-stream", when the sub-chunk gives every CU a tile): it reads only the alpha / q layers
 * of the node's repair plane (repair.rs:61-126) instead of every layer ((10,4,13) 1 GiB {0}:
 * 0.137 ms vs 0.350 on the local decode).  On a codeword the bytes equal decode.rs:31-161's (the
 * codeword through the k data chunks is unique); on chunks that are NOT one codeword they differ,
 * which is why clay_decode_device never takes this route.  Every other pattern runs exactly as
 * clay_decode_device.  The choice is an argument of the call, not process state: concurrent
 * clay_decode_device calls are unaffected.  The repair route is taken under exec modes auto and
 * "stream" only (as clay_repair_device's kernel choice); under "grouped" / "tile" the call runs
 * as clay_decode_device.  No reference counterpart (decode.rs has one path). */
int clay_decode_device_codeword(const clay_code_t *code, const uint8_t *const *chunks,
                                const size_t *erasures, size_t n_erasures, uint8_t *const *out_chunks,
                                size_t chunk_size, int device, void *stream, clay_error_t *err);

/* Batched decode of n_stripes stripes with the SAME erasure set, laid out at fixed strides in
 * device memory (the reference decodes one stripe per call, decode.rs:31-161; its benchmark,
 * benches/clay_bench.rs:58-93, decodes 1 KiB - 1 MiB stripes, which are launch-bound on a GPU;
 * after a node failure every stripe has the same erasure pattern).  Node i (external index,
 * 0..n-1) of stripe s is at chunks + s*stripe_stride + i*node_stride; the slots of erased nodes are
 * never read.  Every node not listed in `erasures` is available.  Every erased node e (data or
 * parity) of stripe s is rebuilt at out + s*out_stripe_stride + e*out_node_stride.  out may equal
 * chunks with the same strides (rebuild in place into the erased slots); otherwise output regions
 * must not overlap any region that is read.  Validation runs once, before any device work, exactly
 * as clay_decode_device's (decode.rs:36-126); n_stripes == 0 returns CLAY_OK and launches nothing.
 * Each stripe's output bytes are those of clay_decode_device for that stripe alone, on any input.
 * Paths (clay_set_exec_mode): stripes of <= 4 MiB of data each run as a batch -- (4,2,5) with one
 * erasure as ONE launch of the batched k_bs_decode1 for any number of stripes (last exec path
 * "bs-decode1-batch", any sub-chunk size and alignment; allocates nothing, so it may be captured
 * unprepared), anything else, from 4 stripes, as one k_gexec launch per level of the decode plan
 * ("grouped-batch"; inside a stream capture it must have been prepared by one call of the same
 * shape, like clay_decode_device); fewer or larger stripes run stripe by stripe as
 * clay_decode_device.
 * The streaming batch: (10,4,13) stripes whose pattern runs on the local decode on 256-byte row
 * runs can run as ONE launch of that kernel's batch variant for any number of stripes (last exec
 * path "stream-local256-batch", clay_last_launch_count() 1).  A call is eligible when
 *   - the code is (10,4,13) and n_stripes >= 2;
 *   - stripe 0's pattern is one the one-stripe call runs on k_stream_local256 on 8-byte rows: every
 *     1-erasure and every 2-erasure pattern, a sub-chunk that is a multiple of 8 with
 *     512 <= sub-chunk < 2^24, every chunk 8-byte aligned;
 *   - every present node's input sits at one stripe stride and every rebuilt output at one (the
 *     strided form by construction; pointer arrays that are rows of one buffer);
 *   - both stripe strides are multiples of 8, so every stripe is on 8-byte rows.
 * The overlap rule above applies unchanged; out == chunks in place is allowed (erased slots are
 * never read).  Which exec modes take it:
 *   "stream"         every eligible call at any eligible size, stripes of <= 4 MiB included
 *   auto             only calls that would run stripe by stripe (more than 4 MiB of data per
 *                    stripe), for sub-chunks up to the measured gate kDecodeStreamBatchMaxSc =
 *                    262,152 bytes: above it (the 1 GiB stripe's 419,432) the batch lost to the
 *                    loop and auto keeps one launch per stripe
 *   "stream-local"   never: one launch per stripe ("stream-local256"), the A/B partner
 *   "grouped", "tile"  never
 *   "stream-fused2"  unchanged
 * The pattern's table is uploaded once per pattern: inside a stream capture the call needs one warm
 * call of the same pattern first (else the "not prepared" error, nothing launched); nothing else is
 * allocated.  (9,4,12) and rows off 8-byte alignment keep the paths above.
 * Three and four erasures -- the batch of the fused decode v2 (k_stream_fused2, last exec path
 * "stream-fused2-batch", clay_last_launch_count() 1): the same conditions, with a pattern that exec
 * mode "stream" runs on k_stream_fused2 in the one-stripe call (at most two erasures per y-section
 * and within the kernel's round capacity: 352 of the 364 three-erasure and 878 of the 1,001
 * four-erasure patterns of (10,4,13)).  Every stripe keeps the one-stripe cut of 64-byte tiles; the
 * workgroups left over run further stripes side by side.  Which exec modes take it:
 *   "stream"         every eligible call at any eligible size, stripes of <= 4 MiB included
 *   auto             only calls that would run stripe by stripe (more than 4 MiB of data per
 *                    stripe), for sub-chunks up to the measured gate kDecodeFused2BatchMaxSc
 *                    = 419,432 bytes, the largest sub-chunk of the sweep: the batch beat the loop in
 *                    every swept cell (profiles/r15/batch_decode_fused2_gate.txt); above it
 *                    nothing was measured and auto keeps one launch per stripe
 *   "stream-fused2"  never: one launch per stripe ("stream-fused2"), the A/B partner
 *   "stream-local", "grouped", "tile"  never
 * Warm call before a capture and allocation as above.  (9,4,12), the patterns outside the kernel
 * and rows off 8-byte alignment keep the paths above.
 * Asynchronous on `stream`. */
int clay_decode_device_strided(const clay_code_t *code, const uint8_t *chunks, int64_t node_stride,
                               int64_t stripe_stride, const size_t *erasures, size_t n_erasures,
                               uint8_t *out, int64_t out_node_stride, int64_t out_stripe_stride,
                               size_t n_stripes, size_t chunk_size, int device, void *stream,
                               clay_error_t *err);

/* Pointer-array form of clay_decode_device_strided (decode.rs:31-161 per stripe; the stripe sizes
 * of benches/clay_bench.rs:58-93): stripe s uses chunks[s*n .. s*n+n) and
 * out_chunks[s*n .. s*n+n) with the NULL conventions of clay_decode_device; the NULL pattern must
 * be identical in every stripe (else CLAY_ERR_INVALID_PARAMETERS).  Pointer arrays that are rows of
 * one buffer (uniform stripe strides) take the same paths as the strided form; others run the
 * batch through a cached device pointer table ("grouped-batch"). */
int clay_decode_device_batch(const clay_code_t *code, const uint8_t *const *chunks,
                             const size_t *erasures, size_t n_erasures, uint8_t *const *out_chunks,
                             size_t n_stripes, size_t chunk_size, int device, void *stream,
                             clay_error_t *err);

/* Repair on device: helper buffers are device pointers (beta*sub-chunk bytes),
 * out is a device buffer of chunk_size bytes. */
int clay_repair_device(const clay_code_t *code, size_t lost_node, const size_t *helper_ids,
                       const uint8_t *const *helper_bufs, size_t n_helpers, size_t chunk_size,
                       uint8_t *out, int device, void *stream, clay_error_t *err);

/* Repair on device from WHOLE helper chunks (device pointers, chunk_size bytes
 * each): the kernels read the beta repair layers of repair.rs:22-49 in place, so
 * callers holding full chunks in HBM skip the gather/concat that
 * minimum_to_repair's index lists imply (repair.rs:61-126).
 * Same output bytes as clay_repair on the gathered sub-chunks. */
int clay_repair_device_full_chunks(const clay_code_t *code, size_t lost_node, const size_t *helper_ids,
                                   const uint8_t *const *helper_chunks, size_t n_helpers,
                                   size_t chunk_size, uint8_t *out, int device, void *stream,
                                   clay_error_t *err);

/* Batched repair of n_stripes stripes with the SAME lost node and helper set, laid out at fixed
 * strides in device memory (the reference repairs one stripe per call, repair.rs:140-421; after a
 * node failure a store of small stripes rebuilds the same node in every one of them, at the
 * launch-bound stripe sizes of benches/clay_bench.rs).  The helper buffer of external node
 * id = helper_ids[h] of stripe s is at helpers + s*stripe_stride + id*node_stride: it is indexed by
 * node id, not by h, so a [n_stripes][n][...] buffer is passed as it is; the slots of nodes not in
 * helper_ids (the lost node's included) are never read.  full_chunks == 0: a helper buffer holds
 * the beta repair sub-chunks concatenated in minimum_to_repair order (clay_repair_device's layout);
 * full_chunks != 0: it is the whole chunk (clay_repair_device_full_chunks's layout).  The rebuilt
 * chunk of stripe s goes to out + s*out_stripe_stride.  With full_chunks, out may be
 * helpers + lost_node*node_stride with out_stripe_stride == stripe_stride (rebuild into the lost
 * slot); otherwise output regions must not overlap any region that is read.  Validation runs once,
 * before any device work, exactly as clay_repair_device's (repair.rs:140-211), plus a NULL check of
 * the base pointers; n_stripes == 0 validates, returns CLAY_OK and launches nothing.  Each stripe's
 * output bytes are those of clay_repair_device / clay_repair_device_full_chunks for that stripe
 * alone, on any input (helpers need not come from a codeword).
 * Paths (clay_set_exec_mode): stripes of <= 4 MiB of data each run as a batch -- q = m codes with
 * a k_bs_repair instantiation ((4,2,5), (9,3,11), (10,4,13)) repaired from all n - 1 other nodes
 * as ONE launch of the batched k_bs_repair for any number of stripes (last exec path
 * "bs-repair-batch", any sub-chunk size and alignment, both layouts; allocates nothing, so it may
 * be captured unprepared), anything else, from 4 stripes, as one k_gexec launch per level of the
 * repair plan ("grouped-batch"; inside a stream capture it must have been prepared by one call of
 * the same shape); fewer or larger stripes run stripe by stripe as clay_repair_device.
 * Asynchronous on `stream`. */
int clay_repair_device_strided(const clay_code_t *code, size_t lost_node, const size_t *helper_ids,
                               size_t n_helpers, const uint8_t *helpers, int64_t node_stride,
                               int64_t stripe_stride, int full_chunks, uint8_t *out,
                               int64_t out_stripe_stride, size_t n_stripes, size_t chunk_size,
                               int device, void *stream, clay_error_t *err);

/* Pointer-array form of clay_repair_device_strided: stripe s uses helper_bufs[s*n_helpers + h] for
 * helper_ids[h], and outs[s]; a NULL entry is CLAY_ERR_INVALID_PARAMETERS.  Pointer arrays that are
 * rows of one buffer (uniform stripe strides) take the same paths as the strided form; others run
 * the batch through a cached device pointer table ("grouped-batch"). */
int clay_repair_device_batch(const clay_code_t *code, size_t lost_node, const size_t *helper_ids,
                             const uint8_t *const *helper_bufs, size_t n_helpers, int full_chunks,
                             uint8_t *const *outs, size_t n_stripes, size_t chunk_size, int device,
                             void *stream, clay_error_t *err);

/* ------------------------------------------------------------------ */
/* Engine control / introspection                                      */
/* ------------------------------------------------------------------ */

/* Pre-allocate an idle pooled workspace for chunk_size (any stream may take it) and
 * build + upload the code's encode plan, so that a later call allocates nothing --
 * e.g. before stream capture.  The workspace is q x t x chunk_size bytes, the grouped
 * executor's U workspace for that chunk size, held per in-flight call (the streaming
 * kernels need none).  Decode/repair plans and the
 * streaming decode's pattern tables depend on the erasure pattern: run one call per
 * pattern before capturing it (a capture that needs an unprepared one fails with
 * CLAY_ERR_DEVICE rather than allocating). */
int clay_reserve_workspace(const clay_code_t *code, size_t chunk_size, int device,
                           clay_error_t *err);

/* Free the device's idle pooled buffers (waiting for their last users' events) and
 * its unpinned batch pointer tables.  Buffers in use or owned by captured graphs stay. */
int clay_release_workspace(int device, clay_error_t *err);

/* Reclaim what calls made inside stream captures left to their graphs: the pointer tables of
 * captured batch calls (a 4 MiB per-device arena; a captured batch of n stripes takes
 * n x 130 x 8 bytes, so about a dozen 300-stripe captures fill it, after which capturing
 * such calls fails with CLAY_ERR_DEVICE) and the pooled workspaces pinned to graphs.
 * The caller MUST first synchronise every stream that replays those graphs and destroy the
 * graphs: the released workspaces are handed to the next call at once, with no event to wait
 * on, so a replay still running would race that call.  It does not synchronise the device
 * itself (that would invalidate another thread's capture in global mode), so it is safe while
 * other threads capture unrelated work; it fails (nothing released) while one of this
 * library's calls runs inside a capture, or while a capture that took a workspace or a table
 * from this library is still open.  No reference counterpart. */
int clay_release_captured(int device, clay_error_t *err);

/* Bytes of device memory held by the device's buffer pool (tests / monitoring). */
size_t clay_workspace_bytes(int device);

/* Encode path selection (process-wide; tests and benchmarks).  Low byte = path:
 *   0 auto      -- the streaming kernel for q = 4, t = 4 codes with k = 9 / 10 (the
 *                  BASELINE (10,4,13)) and for (9,3,11) (k_stream_encode3: any sub-chunk
 *                  size >= 16 and any alignment); (4,2,5): the line-local bit-sliced kernel
 *                  (k_bs_encode1, "bitsliced-line-k4m2-w2048", any sub-chunk and alignment);
 *                  else the bit-sliced v1 kernel if the code has a
 *                  compiled instantiation; else the byte-sliced fused kernel when the
 *                  parity is one y-section; else the staged plan executor.  Batches of
 *                  >= 4 stripes of <= 4 MiB of data run as one staged launch per level.
 *                  The LDS-DMA kernel (stream) needs sub-chunks that are
 *                  multiples of 8 bytes and 8-byte aligned chunk pointers (else auto
 *                  falls through); the v1 kernel takes any sub-chunk size and alignment.
 *   1 staged    -- the plan executor (k_gexec), any code
 *   2 fused     -- byte-sliced fused kernel (q == m <= 4)
 *   3 bitsliced -- bit-sliced v1 (register loads); variant = lanes per column group
 *                  for (10,4,13): 0 (2), 1, 4; (4,2,5) runs v1 here, not the line kernel
 *   5 stream    -- the streaming kernel (stream_encode.hpp); variant = loader waves
 *                  for (10,4,13): 0 (= 4, the default), 1, 2, 4; (9,4,12) always runs
 *                  4 loader waves (its variant is accepted and ignored); (9,3,11): 7 loader
 *                  waves for variant 7, else 2 (stream_encode3.hpp)
 * (4, the v6 kernel of round 1, is retired.)  Bits 8..15 = variant.  Every accepted (path, variant) produces the reference's
 * parity bytes; any other value returns -1 and leaves the setting unchanged.
 * Returns the previous setting (path | variant << 8). */
int clay_set_encode_path(int mode);

/* Plan executor for decode, repair and the staged encode (process-wide tuning knob; no
 * reference counterpart -- the crate has one CPU path).  A mode only chooses kernels: every
 * mode returns the reference's bytes on any input.
 *   0 auto    -- the tile-fused executor (one launch, U workspace in LDS) for small plans
 *                (<= 32 op groups) whose U slots fit the LDS budget, else the grouped
 *                per-level executor; for q = 4, t = 4 codes ((10,4,13), (9,4,12)) with
 *                sc >= 512: decodes whose erasures lie in one y-section plus at most one
 *                erasure in one other section ({0}, {0,4}, {0,1}, {0,1,4}, {0,1,2,3}, ...) run
 *                a single-launch local decode: one erasure in its section plus at most one
 *                more, or two in one section ({0}, {12}, {0,4}, {0,1}), on 256-byte row runs
 *                (k_stream_local256, last path "stream-local256", any sub-chunk), the others
 *                on 64-byte tiles (k_stream_local, "stream-local", sc % 8 == 0) -- except
 *                three erasures as two in one section and one in another ({0,1,4}), which
 *                take the fused decode v2 first; 3 or 4 erasures with at most two per
 *                y-section (sc % 8 == 0; the BASELINE {0,4,8,12} and the (2,1,1) / (2,2)
 *                patterns included) the fused decode v2 (k_stream_fused2, "stream-fused2");
 *                (4,2,5) with one erasure and every other chunk present: the single-erasure
 *                bit-sliced decode (k_bs_decode1, "bs-decode1", any sub-chunk and alignment);
 *                batched decodes (clay_decode_device_strided / _batch, stripes of <= 4 MiB of
 *                data): (4,2,5) with one erasure at uniform stripe strides in one launch of
 *                the batched k_bs_decode1 ("bs-decode1-batch"), every other code, pattern or
 *                layout, from 4 stripes, one k_gexec launch per plan level for the whole batch
 *                ("grouped-batch"; larger (10,4,13) stripes with one or two erasures: the streaming
 *                batch, "stream-local256-batch", up to the gate of clay_decode_device_strided;
 *                with three or four erasures "stream-fused2-batch" up to its gate there);
 *                batched repairs (clay_repair_device_strided / _batch, same
 *                stripe sizes): q = m codes with a k_bs_repair instantiation from all n - 1 other
 *                nodes at uniform stripe strides in one launch of the batched k_bs_repair
 *                ("bs-repair-batch"), every other code, helper set or layout, from 4 stripes,
 *                "grouped-batch"
 *   1 grouped -- always the grouped executor (k_gexec, one launch per level); batched decodes
 *                and repairs always "grouped-batch" (the A/B partner of the line / repair batch)
 *   2 tile    -- the tile executor wherever its U slots fit, whatever the plan size; batched
 *                decodes and repairs as under grouped ("grouped-batch": the tile executor has no
 *                batch form)
 *   (auto and stream: repair of (9,3,11), (10,4,13), (4,2,5) from all n - 1 other nodes runs
 *    the bit-sliced repair kernels: k_bs_repair_stream (LDS-DMA streaming, one workgroup per
 *    CU; auto when the sub-chunk gives every CU a tile, stream for any sub-chunk >= 16 bytes
 *    of (9,3,11) / (10,4,13); last path "bs-repair-stream"), else k_bs_repair ("bs-repair"))
 *   (scrubs, clay_scrub_device*: (4,2,5) on the line kernel, "bs-scrub1" / "bs-scrub1-batch",
 *    except under 1 grouped and 2 tile, which keep v1, "bs-scrub" / "bs-scrub-batch", its A/B
 *    partner; (10,4,13) on 8-byte rows on the streaming kernel, "stream-scrub", under 3 stream
 *    at any sub-chunk and under 0 auto / 5 / 6 from a sub-chunk of 65,536 bytes, v1 under 1 / 2;
 *    batches of it in one launch, "stream-scrub-batch", as clay_set_scrub_path says -- never
 *    under 1 / 2, and under 3 stream only with scrub path 1; everything else on v1 in every mode)
 *   3 stream  -- every decode a streaming kernel takes on it: the local decode where it takes
 *                the pattern (the (2,1) patterns: the fused decode v2 first), else the fused
 *                decode v2 (2-4 erasures, at most two per section); batched decodes of (10,4,13)
 *                eligible for the streaming batch (clay_decode_device_strided) in one launch,
 *                "stream-local256-batch" or, on the fused decode v2, "stream-fused2-batch", at any
 *                eligible size; everything else as auto
 *   5 stream-local -- every decode a local kernel takes on it ("stream-local256" /
 *                "stream-local", the (2,1) patterns included); every other decode on auto's
 *                plan executors (no fused decode v2, no k_bs_decode1); never the streaming batch
 *                (one launch per stripe: its A/B partner)
 *   6 stream-fused2 -- decodes of 2-4 erasures with at most two per y-section on the fused
 *                decode v2 (k_stream_fused2, "stream-fused2"; ring of 10 - e node buffers: a
 *                section's surviving real nodes fit it, two neighbouring sections that do not
 *                run as a split step; the loader waves' round items fit their registers);
 *                every other decode, one erasure included, on auto's plan executors (no local
 *                decode, no k_bs_decode1); batched decodes keep one launch per stripe (the A/B
 *                partner of "stream-fused2-batch")
 * (4 and 7 are retired: the single-launch decode of round 3 and the process-wide "codeword"
 * mode, now the per-call clay_decode_device_codeword.)
 * No CLAY_* environment variable is read on a call path; the measurement knobs (planner and
 * executor tuning, CLAY_LOCAL_W64 = the 64-byte local kernel for every local pattern) are read
 * once when the library is loaded.
 * Returns the previous mode, or -1 for an unknown mode (setting unchanged). */
int clay_set_exec_mode(int mode);
/* Path of the batched scrubs of (10,4,13), clay_scrub_device_batch / _strided (process-wide tuning
 * knob, like the two above).  It only chooses kernels: every value gives the same result words.
 * A call is ELIGIBLE for the streaming batch -- ONE launch of k_stream_encode's compare-ending
 * batch variant for all its stripes, last exec path "stream-scrub-batch", clay_last_launch_count
 * 1 -- when it has 2 or more stripes, every stripe is on 8-byte rows (clay_scrub_device), the
 * stripes sit at one data and one parity stripe stride (a data stride of 0, every stripe on the
 * same data chunks, included), the exec mode is not 1 grouped / 2 tile, and one workgroup's steps
 * fit the kernel's 31-bit counter.  A call that is not eligible runs as without this setter.
 *   0 auto         -- under exec mode 3 stream: never (one launch per stripe, "stream-scrub": the
 *                     batch's A/B partner).  Under exec modes 0 auto, 5 and 6: the streaming batch
 *                     by the measured gate (see clay_scrub_device_batch), never below a sub-chunk
 *                     of 2,048 bytes; else as without this setter
 *   1 stream-batch -- the streaming batch for every eligible call, at any sub-chunk size from 16
 *                     bytes and any stripe count from 2, under exec modes 0, 3, 5 and 6
 * Returns the previous value, or -1 for any other value (setting unchanged). */
int clay_set_scrub_path(int path);
/* Plan executor the calling thread's last decode / repair / staged encode ran on:
 * "tile" (k_texec), "grouped" (k_gexec), "stream-local256" (k_stream_local256), "stream-local"
 * (k_stream_local), "stream-fused2"
 * (k_stream_fused2), "bs-decode1" (k_bs_decode1), "bs-repair-stream" (k_bs_repair_stream),
 * "bs-repair" (k_bs_repair), the batched decodes' "bs-decode1-batch" (k_bs_decode1 over many
 * stripes), the batched repairs' "bs-repair-batch" (k_bs_repair over many stripes), both batches'
 * "grouped-batch" (k_gexec over many stripes), the scrubs' "bs-scrub1" (k_bs_encode1's compare
 * ending) / "bs-scrub" (k_bs_encode's) with one launch per stripe and "bs-scrub1-batch" /
 * "bs-scrub-batch" (a batch in one launch), "stream-scrub" (k_stream_encode's compare ending,
 * (10,4,13): one launch per stripe in every entry point) and "stream-scrub-batch" (the same
 * kernel's batch variant: many stripes in one launch, clay_set_scrub_path), or "none". */
const char *clay_last_exec_path(void);

/* Name of the path the last encode on this thread used ("fused-q4w128p8", "staged", ...). */
const char *clay_last_encode_path(void);

/* Number of kernel launches the last device call on this thread issued. */
size_t clay_last_launch_count(void);

/* Introspection (tests / tooling): export the staged-engine plan -- the
 * reference's layered algorithm replayed into GF(2^8) region ops
 * "dst = XOR coef*src" -- for kind 0 = encode, 1 = decode (mask = erased
 * internal nodes, want = erased nodes whose C is wanted), 2 = repair (mask =
 * helper internal nodes, lost = external lost node).  Records are uint32:
 * ops_out[4*i..] = {dst_base, dst_slot, src_begin, nsrc}, srcs_out[4*j..] =
 * {base, slot, coef, 0}, stages_out = stage begin offsets (n_stages+1).  Base
 * index b: b < tn -> C[node b]; tn <= b < 2tn -> helper H[node b-tn]; 2tn -> U
 * workspace (slot = node*alpha + z); 2tn+1 -> repaired chunk.  counts[] =
 * {n_ops, n_srcs, n_stages+1}.  Capacities too small -> only counts filled. */
int clay_plan_export(const clay_code_t *code, int kind, const uint8_t *mask, const uint8_t *want,
                     size_t lost_node, uint32_t *ops_out, size_t ops_cap, uint32_t *srcs_out,
                     size_t srcs_cap, uint32_t *stages_out, size_t stages_cap, size_t counts[3],
                     clay_error_t *err);

/* ABI version (CLAY_ABI_VERSION) and build string. */
int clay_abi_version(void);
const char *clay_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* CLAY_H */
