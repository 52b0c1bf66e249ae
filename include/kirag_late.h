/* kirag_late.h - C ABI of libkirag_late.so: late interaction (MaxSim) over stored token vectors on the AMD Instinct MI355X (gfx950).
 *
 * A small library of its own next to libkirag_amd.so (include/kirag_amd.h), which it neither links nor shares an object file with: it links the HIP
 * runtime only.  Conventions as there:
 *   - every function returns KL_OK (0) or a negative error code; kl_last_error() gives a thread-local message.  The codes carry the values of the
 *     KR_E* codes they mirror.
 *   - there is NO CPU fallback: without a gfx950 device every compute call fails with KL_ENODEV.  Argument checks come first, so a call that would be
 *     refused for its arguments is refused the same way on a machine without a device.
 *   - device data pointers (`q`, `d`, `block`, and the `out` of kl_gather_rows_f16) must be aligned to 16 bytes, the fp32 `out` of kl_maxsim to 4: the kernels
 *     move rows in 16-byte pieces.  A misaligned pointer is KL_EINVAL naming it.
 *   - the compute calls select `device` for their own work and put the caller's current device back before they return; so does kl_release_scratch.
 *   - token vectors are rows of `P` IEEE binary16 values (uint16_t bit patterns), row-major, rows of one query / document adjacent: sequence s owns the
 *     rows off[s] .. off[s + 1] - 1.
 */
#ifndef KIRAG_LATE_H
#define KIRAG_LATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef KL_API
#define KL_API
#endif

#define KL_OK 0
#define KL_EINVAL (-22)   /* bad argument; the message names the field */
#define KL_ENOMEM (-12)   /* hipMalloc failed */
#define KL_ENODEV (-19)   /* no usable HIP device */
#define KL_EHIP (-5)      /* a HIP runtime call failed; see kl_last_error() */
#define KL_ERANGE (-34)   /* kl_gather_rows_f16 met a source element that is not finite, or not finite once rounded to binary16 */

#define KL_ABI_VERSION 1

#define KL_REDUCE_SUM 0
#define KL_REDUCE_MEAN 1

#define KL_MIN_DIM 32     /* P % 32 == 0 and KL_MIN_DIM <= P <= KL_MAX_DIM */
#define KL_MAX_DIM 2048

KL_API int kl_abi_version(void);
KL_API const char* kl_last_error(void);
/* frees the per-device workspaces (the copies of the caller's index arrays); synchronises the devices that have one */
KL_API void kl_release_scratch(void);

/* out[t][:] = binary16(block[src_row[t]][:]), rounded to nearest even, t < T.
 *   block    DEVICE, fp32 rows of width P (the colbert block of a flagged forward seen as [B * S, P])
 *   src_row  HOST, T row numbers into block, each >= 0 (the caller vouches for the upper end: the library does not know the block's height)
 *   out      DEVICE, T * P binary16
 * A source element that is NaN or +-Inf, or that rounds to +-Inf, returns KL_ERANGE (out is then written but unusable).  The call synchronises with
 * `stream`: it is the ingest path. */
KL_API int kl_gather_rows_f16(const float* block, const int64_t* src_row, int64_t T, int P, uint16_t* out, int device, void* stream);

/* out[p] = sum over the rows i of query pair_q[p] of ( max over the rows j of document pair_d[p] of q_i . d_j ), p < npairs; reduce = KL_REDUCE_MEAN
 * divides the sum by the query's row count (one correctly rounded fp32 division).  The products of the binary16 operands are exact and summed in fp32
 * (v_mfma_f32_32x32x16_f16).  A query or a document without rows gives +0.0.
 *   q, d     DEVICE, binary16 rows of width P
 *   q_off    HOST [nq + 1], d_off HOST [nd + 1]: start at 0, non-decreasing
 *   pair_q, pair_d  HOST [npairs]: 0 <= pair_q < nq, 0 <= pair_d < nd
 *   out      DEVICE [npairs] fp32
 * Everything above is checked before anything is launched (KL_EINVAL naming the offender); the kernel reads the library's own copy of the checked
 * values, never the caller's arrays.  A pair's result is a function of its own rows alone: not of the other pairs of the call, their order or number.
 * The call enqueues on `stream` and does not wait for the work it enqueued; the caller's host arrays may be reused at once.  The
 * pair records are staged in two pinned buffers used in turns: before it overwrites one, a call waits on the host until the upload of the call BEFORE the previous
 * one has executed (normally long done; it can block when two earlier calls still sit behind other work queued on their streams).  Calls for one device from several threads are
 * serialised; a call on another stream than the device's previous call is ordered behind that call's kernel on the device (an event, no host wait). */
KL_API int kl_maxsim(const uint16_t* q, const int64_t* q_off, int nq, const uint16_t* d, const int64_t* d_off, int64_t nd, const int64_t* pair_q,
                     const int64_t* pair_d, int64_t npairs, int P, int reduce, float* out, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif
