/* kirag_sparse.h - C ABI of libkirag_sparse.so: a doc-range-blocked inverted index over learned sparse vectors (SPLADE rows, bge-m3 lexical weights) and an
 * exact top-k over it, on the AMD Instinct MI355X (gfx950).
 *
 * A small library of its own next to libkirag_amd.so and libkirag_late.so, which it neither links nor shares an object file with: it links the HIP runtime
 * only.  Conventions as in kirag_late.h:
 *   - every function returns KS_OK (0) or a negative error code; ks_last_error() gives a thread-local message.  The codes carry the values of the KR_E* codes
 *     they mirror.
 *   - there is NO CPU fallback: without a gfx950 device every compute call fails with KS_ENODEV.  EVERY argument check comes before a device is asked for, so
 *     a call that would be refused for its arguments is refused the same way on a machine without a device.
 *   - device pointers must be aligned to their element (4 bytes; out_row 8; weights 2).  A misaligned pointer is KS_EINVAL naming it.
 *   - the compute calls select `device` for their own work and put the caller's current device back before they return; so does ks_release_scratch.
 *   - host index arrays (offsets, query CSR, skip lists) are copied into the library's own pinned staging buffer and from there to its device workspace: the
 *     kernels never read the caller's host arrays.
 *   - every compute call waits for the work it enqueued on `stream` before it returns (one pinned staging buffer per device, no events to track): results are
 *     ready and the caller's host arrays may be reused at once.  Calls for one device from several threads are serialised.
 *
 * INDEX LAYOUT.  Rows (passages) are numbered 0 .. N-1 in insertion order.  Block b owns the rows b*R .. min(N, (b+1)*R) - 1, R = KS_BLOCK_ROWS
 * (ks_block_rows() tells what the built library uses).  Per block there are two arrays:
 *   ptr   uint32[V + 1]  the block's term-pointer table, block b's at ptr + b * (V + 1)
 *   post  uint32[...]    the block's postings, block b's at post + post_off[b], post_off[b + 1] - post_off[b] of them: the block-local row in the high 16
 *                        bits, the IEEE binary16 weight in the low 16 bits
 * The postings of term t in block b are post[post_off[b] + ptr_b[t]] .. post[post_off[b] + ptr_b[t + 1] - 1], in ascending local row; a row appears at most
 * once under a term.  Weights are binary16, finite and > 0.
 *
 * RESULT DEFINITION (exact).  The score of row r for a query with terms t_1 < ... < t_m and fp32 weights q_1 .. q_m is
 *     s = 0;  for i = 1 .. m: if r holds t_i with weight d: s = fl32(s + fl32(q_i * float(d)))
 * - one fp32 multiply and one fp32 add per shared term, NOT fused, in ascending term order.  The result of a query is the first k of the rows with s > 0
 * ordered by (score descending, row ascending); missing places hold row -1 and score +0.0.  A row's score is a function of the row and the query alone: not
 * of N, of the block the row lies in, of the other queries of the call or of k.
 *
 * ROBUSTNESS.  The scan kernel masks every local row to R - 1 and clamps every segment [ptr[t], ptr[t + 1]) to the block's posting count, so no content of
 * the device arrays can make it read or write outside the arrays and the LDS it was given; no workgroup waits for another.
 */
#ifndef KIRAG_SPARSE_H
#define KIRAG_SPARSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef KS_API
#define KS_API
#endif

#define KS_OK 0
#define KS_EINVAL (-22)   /* bad argument; the message names the field */
#define KS_ENOMEM (-12)   /* hipMalloc failed */
#define KS_ENODEV (-19)   /* no usable HIP device */
#define KS_EHIP (-5)      /* a HIP runtime call failed; see ks_last_error() */
#define KS_ERANGE (-34)   /* ks_count_positive / ks_compact_rows met an element that is NaN, +-Inf, or +-Inf once rounded to binary16 */

#define KS_ABI_VERSION 1

#ifndef KS_BLOCK_ROWS
#define KS_BLOCK_ROWS 16384   /* R: rows per block, 16384 or 32768 (one fp32 accumulator per row in LDS: 64 or 128 KiB).  16384 measured faster at every
                               * shape of profiles/sparse/measurements.txt (two workgroups per CU); -DKS_BLOCK_ROWS=32768 builds the other */
#endif
#define KS_MAX_K 1024         /* 1 <= k <= KS_MAX_K */
#define KS_MAX_QUERIES 65535  /* nq <= KS_MAX_QUERIES per call */
#define KS_MAX_SKIP 64        /* ns <= KS_MAX_SKIP skipped terms */
/* Bound of the candidate workspace, in candidates of 8 bytes (128 MiB): ks_search slices the queries of a call so that queries * blocks * k stays within
 * it; one query's blocks * k must fit (KS_EINVAL otherwise).  The environment variable KIRAG_SPARSE_MAX_CANDIDATES, read at every call, lowers it (tests). */
#define KS_MAX_CANDIDATES (1 << 24)

KS_API int ks_abi_version(void);
KS_API const char* ks_last_error(void);
/* frees the per-device workspaces; synchronises the devices that have one */
KS_API void ks_release_scratch(void);
KS_API int ks_block_rows(void);

/* Exact top-k of nq sparse queries over the index (see RESULT DEFINITION).
 *   post, ptr   DEVICE, the index arrays described above (ptr: blocks * (V + 1) entries, blocks = ceil(N / R))
 *   post_off    HOST int64[blocks + 1]: starts at 0, non-decreasing, a block holds fewer than 2^32 postings
 *   N, V        0 <= N <= 2^31, 1 <= V <= 2^24
 *   q_off       HOST int64[nq + 1]: starts at 0, non-decreasing.  A query without terms is allowed: it has no results
 *   q_term      HOST int32[q_off[nq]]: strictly ascending within a query, 0 <= term < V
 *   q_w         HOST fp32[q_off[nq]]: finite and > 0
 *   k           1 <= k <= KS_MAX_K
 *   out_score   DEVICE fp32[nq * k], out_row DEVICE int64[nq * k]: query i's results at i * k */
KS_API int ks_search(const uint32_t* post, const uint32_t* ptr, const int64_t* post_off, int64_t N, int V, const int64_t* q_off, int nq,
                     const int32_t* q_term, const float* q_w, int k, float* out_score, int64_t* out_row, int device, void* stream);

/* The ingest path from a [B, V] fp32 block on the device (a KR_POOL_SPLADE forward), two calls.  An element is KEPT iff its value rounded to binary16
 * (nearest even) is > 0 and its term is not in skip_terms.  Any element of the block that is NaN or +-Inf, or +-Inf once rounded, makes either call return
 * KS_ERANGE.
 *   block       DEVICE fp32[B * V]
 *   skip_terms  HOST int32[ns], each in [0, V); ns <= KS_MAX_SKIP
 * ks_count_positive fills HOST counts[B] with the number of kept elements per row.
 * ks_compact_rows takes HOST row_off[B + 1] (starts at 0, row_off[r + 1] - row_off[r] = counts[r]) and fills DEVICE terms int32[row_off[B]] and DEVICE
 * weights binary16[row_off[B]]: row r's kept elements at row_off[r], in ascending term.  It counts again: a row whose count disagrees with row_off makes it
 * return KS_EINVAL, and nothing is written outside that row's slot. */
KS_API int ks_count_positive(const float* block, int B, int V, const int32_t* skip_terms, int ns, int64_t* counts, int device, void* stream);
KS_API int ks_compact_rows(const float* block, int B, int V, const int32_t* skip_terms, int ns, const int64_t* row_off, int32_t* terms,
                           uint16_t* weights, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
