/* kirag_pairs.h - C ABI of libkirag_pairs.so: the exact sparse score of given (query, row) pairs over the forward form of a sparse index (the rows' own
 * (term, binary16 weight) lists), on the AMD Instinct MI355X (gfx950).  It scores the candidates another retriever found without scanning the inverted index.
 *
 * A small library of its own next to libkirag_amd.so, libkirag_late.so and libkirag_sparse.so, none of which it links or shares an object file with: it links
 * the HIP runtime only.  Conventions as in kirag_sparse.h:
 *   - every function returns KP_OK (0) or a negative error code; kp_last_error() gives a thread-local message.  The codes carry the values of the KR_E* codes
 *     they mirror.
 *   - there is NO CPU fallback: without a gfx950 device a well-formed call with pairs fails with KP_ENODEV.  EVERY argument check comes before a device is
 *     asked for, so a call that would be refused for its arguments is refused the same way on a machine without a device.
 *   - device pointers must be aligned to their element (terms and out 4 bytes, weights 2).  A misaligned pointer is KP_EINVAL naming it.
 *   - the call selects `device` for its own work and puts the caller's current device back before it returns; so does kp_release_scratch.
 *   - the host arrays (row_off, the query CSR, the pairs) are read by the library alone: it turns each pair into a checked record (row start, row length,
 *     query index) in its own pinned staging buffer and copies the query CSR there; the kernel reads the device copies of those, never the caller's host
 *     arrays, and there is no row_off on the device.  Of the caller's row_off only row_off[pair_row[p]] and the entry after it are read.
 *   - the call waits for the work it enqueued on `stream` before it returns: results are ready and the caller's host arrays may be reused at once.  Calls for
 *     one device from several threads are serialised.
 *
 * FORWARD FORM.  Row r holds the entries row_off[r] .. row_off[r + 1] - 1 of `terms` (int32, strictly ascending within a row, 0 <= term < V) and `weights`
 * (IEEE binary16, finite and > 0): what SparseIndexer keeps as its host truth, mirrored on the device.
 *
 * RESULT DEFINITION (exact).  out[p] is the score that kirag_sparse.h's RESULT DEFINITION gives row pair_row[p] for query pair_q[p]: with the query's terms
 * t_1 < ... < t_m and fp32 weights q_1 .. q_m,
 *     s = 0;  for i = 1 .. m: if the row holds t_i with weight d: s = fl32(s + fl32(q_i * float(d)))
 * - one fp32 multiply and one fp32 add per shared term, NOT fused, in ascending term order.  A pair that shares no term (an empty row, a query without terms)
 * gives +0.0, sign bit clear.  A pair's result is a function of its row and its query alone: not of the other pairs of the call, their order or number, of
 * duplicates of the pair, or of how the call was sliced.  Consequence: wherever ks_search returns a row, kp_sparse_dot gives that row the same score bits.
 *
 * ROBUSTNESS.  The kernel clamps every record's row segment to nnz and every query segment to the staged query length, and bounds every loop by those
 * clamped values or a constant, so no content of the device arrays can make it read or write outside what it was given; it uses no atomics and no workgroup
 * waits for another.
 */
#ifndef KIRAG_PAIRS_H
#define KIRAG_PAIRS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef KP_API
#define KP_API
#endif

#define KP_OK 0
#define KP_EINVAL (-22)   /* bad argument; the message names the field */
#define KP_ENOMEM (-12)   /* hipMalloc failed */
#define KP_ENODEV (-19)   /* no usable HIP device */
#define KP_EHIP (-5)      /* a HIP runtime call failed; see kp_last_error() */

#define KP_ABI_VERSION 1

#define KP_MAX_QUERIES 65535       /* nq <= KP_MAX_QUERIES per call */
#define KP_MAX_PAIRS (1 << 24)     /* npairs <= KP_MAX_PAIRS per call */
/* Pair records (16 bytes each) are staged and launched in slices of at most this many.  The environment variable KIRAG_PAIRS_MAX_STAGED, read at every
 * call, lowers it (tests); the slicing does not change a result. */
#define KP_MAX_STAGED_PAIRS (1 << 20)

KP_API int kp_abi_version(void);
KP_API const char* kp_last_error(void);
/* frees the per-device workspaces; synchronises the devices that have one */
KP_API void kp_release_scratch(void);

/* The exact sparse score of npairs (query, row) pairs (see RESULT DEFINITION).
 *   terms, weights  DEVICE int32[nnz], binary16[nnz]: the forward form described above
 *   nnz             >= 0
 *   row_off         HOST int64[N + 1]; only the entries of referenced rows are read.  For a referenced row r: 0 <= row_off[r] <= row_off[r + 1] <= nnz and
 *                   row_off[r + 1] - row_off[r] <= V
 *   N, V            0 <= N <= 2^31, 1 <= V <= 2^24
 *   q_off           HOST int64[nq + 1]: starts at 0, non-decreasing.  A query without terms is allowed: its pairs score +0.0
 *   q_term          HOST int32[q_off[nq]]: strictly ascending within a query, 0 <= term < V
 *   q_w             HOST fp32[q_off[nq]]: finite and > 0
 *   pair_q          HOST int64[npairs], each in [0, nq);  pair_row  HOST int64[npairs], each in [0, N);  0 <= npairs <= KP_MAX_PAIRS
 *   out             DEVICE fp32[npairs]
 * npairs == 0 returns KP_OK (after the argument checks) without asking for a device. */
KP_API int kp_sparse_dot(const int32_t* terms, const uint16_t* weights, int64_t nnz, const int64_t* row_off, int64_t N, int V, const int64_t* q_off, int nq,
                         const int32_t* q_term, const float* q_w, const int64_t* pair_q, const int64_t* pair_row, int64_t npairs, float* out, int device,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
