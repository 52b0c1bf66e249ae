// libkirag_late.so (include/kirag_late.h): late interaction over stored token vectors.  A translation unit of its own: it includes none of the product's
// headers and shares no object file with libkirag_amd.so.
//
// k_maxsim, one workgroup of four waves per (query, document) pair:
//   * orientation: the DOCUMENT's tokens are the rows of v_mfma_f32_32x32x16_f16 (operand A), the QUERY's tokens its columns (operand B, column = lane & 31).
//     Lane (r, h) = (lane & 31, lane >> 5) then holds, of one 32 x 32 score tile, the query token r against the document tokens 8 (i >> 2) + 4 h + (i & 3) in
//     accumulator register i: the max over document tokens is a max over the 16 registers of a lane, over the tiles a wave walks, one exchange between the
//     two halves and one between the waves; the sum over query tokens is a reduction over 32 lanes.  No score reaches memory.
//   * operands: both are K-contiguous, so a fragment is 16 consecutive bytes of one row.  The contraction index is permuted the same way in both: of every
//     64 elements of a row, half h takes the 32 consecutive ones 64 kb + 32 h .. + 31 as its four fragments, so a lane reads 64 consecutive bytes of its
//     document row in four loads and the two halves cover one 128-byte line (a remaining block of 32: 16 consecutive each).  The document goes from global
//     memory straight to registers, up to RING blocks ahead within a tile; the query tile (32 rows) sits in LDS with rows 16 bytes apart from a multiple of 256, which makes
//     the ds_read_b128 of a fragment conflict-free (row stride / 16 bytes = P / 8 + 1, odd).
//   * padding: lanes past the document's end hold zero fragments and their accumulator rows are left out of the max BY INDEX - a zero row would
//     win whenever every real score is negative.  Query rows past the query's end are zero in LDS and left out of the sum by index.
//   * determinism: max is order-free; the 32 columns of a query tile are summed by one fixed butterfly, the tiles of a query in ascending order by one
//     thread.  Nothing depends on the grid, on the other pairs or on which wave met which document tile.
#define KL_API __attribute__((visibility("default")))
#include "../../include/kirag_late.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

namespace {

std::string& last_error_ref() {
    static thread_local std::string e;
    return e;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return code;
}

#define KL_HIP(expr)                                                                                                              \
    do {                                                                                                                          \
        hipError_t _e = (expr);                                                                                                   \
        if (_e != hipSuccess)                                                                                                     \
            return fail(_e == hipErrorOutOfMemory ? KL_ENOMEM : KL_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                                                      \
    } while (0)

#define KL_TRY(expr)              \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)

using half8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int TILE = 32;        // rows of an MFMA tile
constexpr int KBLOCK = 64;      // elements of a row per pipelined step: 32 consecutive per lane half
constexpr int RING = 4;         // steps of document fragments in flight per lane (RING * 64 bytes)
constexpr int LDS_PAD = 8;      // elements between the end of a query row and the next one in LDS

// one checked pair: first row and row count of its query and of its document
struct Pair {
    long long q0, nq, d0, nd;
};

size_t maxsim_lds_bytes(int P) { return (size_t)TILE * (P + LDS_PAD) * 2 + (size_t)WAVES * TILE * sizeof(float); }

// Loads sit in no branch: every lane reads an address that is always readable (the caller clamps the row) and lanes without a row turn what they read
// into zeros by a select where the fragment is USED.  A load under a lane mask, or a select right behind the load, makes the compiler drain the queue
// (s_waitcnt vmcnt(0)) instead of counting the loads that may stay in flight.
__device__ __forceinline__ half8 load8(const _Float16* p) { return *reinterpret_cast<const half8*>(p); }
__device__ __forceinline__ half8 keep(half8 v, bool valid) {
    const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return valid ? v : z;
}

// Four waves per SIMD (128 registers): at narrow rows the LDS tile is small and the registers set the occupancy; measured at P = 128 it is a tenth faster than
// the 180 registers the compiler takes unasked, and as fast at P = 1024, where the LDS tile allows two workgroups either way (profiles/late/measurements.txt).
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_maxsim(const _Float16* __restrict__ q, const _Float16* __restrict__ d, const Pair* __restrict__ pairs, int P,
                                                    int reduce, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int ldq = P + LDS_PAD;
    _Float16* qs = reinterpret_cast<_Float16*>(smem);                              // [TILE][ldq]
    float* colmax = reinterpret_cast<float*>(smem + (size_t)TILE * ldq * 2);       // [WAVES][TILE]
    const Pair pr = pairs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    if (pr.nq == 0 || pr.nd == 0) {
        if (tid == 0) out[blockIdx.x] = 0.0f;
        return;
    }
    const int nkb = P / KBLOCK, chunks = P / 8;
    const _Float16* qrow_lds = qs + r * ldq;
    float total = 0.0f;
    for (long long qt = 0; qt * TILE < pr.nq; ++qt) {
        __syncthreads();      // the readers of the previous tile are done with qs and colmax
        for (int c = tid; c < TILE * chunks; c += THREADS) {
            const int row = c / chunks, col = c - row * chunks;
            const bool valid = qt * TILE + row < pr.nq;
            *reinterpret_cast<half8*>(qs + row * ldq + col * 8) = keep(load8(q + (pr.q0 + qt * TILE + (valid ? row : 0)) * P + col * 8), valid);
        }
        __syncthreads();
        float m = -INFINITY;
        for (long long dt = wave; dt * TILE < pr.nd; dt += WAVES) {
            const long long row = dt * TILE + r;
            const bool valid = row < pr.nd;
            const _Float16* drow = d + (pr.d0 + (valid ? row : 0)) * P;
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            half8 a[RING][4];
#pragma unroll
            for (int i = 0; i < RING; ++i)
                if (i < nkb) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) a[i][s] = load8(drow + i * KBLOCK + 32 * h + 8 * s);
                }
            for (int kb0 = 0; kb0 < nkb; kb0 += RING) {
#pragma unroll
                for (int i = 0; i < RING; ++i) {
                    const int kb = kb0 + i;
                    if (kb < nkb) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const half8 b = *reinterpret_cast<const half8*>(qrow_lds + kb * KBLOCK + 32 * h + 8 * s);
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(keep(a[i][s], valid), b, acc, 0, 0, 0);
                        }
                        if (kb + RING < nkb) {
#pragma unroll
                            for (int s = 0; s < 4; ++s) a[i][s] = load8(drow + (kb + RING) * KBLOCK + 32 * h + 8 * s);
                        }
                    }
                }
            }
            if (P & 32) {     // the last 32 elements: 16 consecutive per half
                const int k0 = nkb * KBLOCK + 16 * h;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const half8 b = *reinterpret_cast<const half8*>(qrow_lds + k0 + 8 * s);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(keep(load8(drow + k0 + 8 * s), valid), b, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (dt * TILE + 8 * (i >> 2) + 4 * h + (i & 3) < pr.nd) m = fmaxf(m, acc[i]);
        }
        m = fmaxf(m, __shfl_xor(m, 32));
        if (h == 0) colmax[wave * TILE + r] = m;
        __syncthreads();
        if (wave == 0) {
            float v = colmax[r];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) v = fmaxf(v, colmax[w * TILE + r]);
            if (!(qt * TILE + r < pr.nq)) v = 0.0f;
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            total += v;
        }
    }
    if (tid == 0) out[blockIdx.x] = reduce == KL_REDUCE_MEAN ? __fdiv_rn(total, (float)pr.nq) : total;
}

// eight elements per thread: two 16-byte loads, one 16-byte store
__global__ __launch_bounds__(256) void k_gather_f16(const float* __restrict__ block, const long long* __restrict__ rows, long long T, int P,
                                                    _Float16* __restrict__ out, int* __restrict__ flag) {
    const int chunks = P / 8;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * chunks) return;
    const long long t = idx / chunks;
    const int col = (int)(idx - t * chunks) * 8;
    const float4* src = reinterpret_cast<const float4*>(block + rows[t] * P + col);
    const float4 lo = src[0], hi = src[1];
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    half8 v;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = (_Float16)x[i];                           // round to nearest even
        bad |= !(fabsf((float)v[i]) <= 65504.0f);        // NaN or Inf, in the source or made by the rounding
    }
    *reinterpret_cast<half8*>(out + t * P + col) = v;
    if (bad) *flag = 1;
}

struct Workspace {
    void* dev = nullptr;          // the checked copies a kernel reads
    size_t cap = 0;
    void* host[2] = {nullptr, nullptr};          // two pinned staging buffers used in turns: a call waits for the upload of the call BEFORE the previous one
    size_t host_cap[2] = {0, 0};
    hipEvent_t copied[2] = {nullptr, nullptr};   // staging buffer i has been read by its upload
    bool staged[2] = {false, false};
    int slot = 0;                                // the staging buffer of the current call
    int* flag = nullptr;          // device flag of k_gather_f16
    int* flag_host = nullptr;     // pinned
    hipEvent_t done = nullptr;    // the last kernel that reads `dev` has finished
    hipStream_t last = nullptr;
    bool used = false;
    bool lds_raised = false;
};

std::mutex g_mutex;
std::map<int, Workspace> g_ws;

// the caller's current device, put back when an entry point returns (select_device and kl_release_scratch change it)
struct DeviceGuard {
    int saved = -1;
    DeviceGuard() {
        if (hipGetDevice(&saved) != hipSuccess) {
            (void)hipGetLastError();
            saved = -1;
        }
    }
    ~DeviceGuard() {
        int now = -1;
        if (saved >= 0 && hipGetDevice(&now) == hipSuccess && now != saved) (void)hipSetDevice(saved);
    }
};

int select_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(KL_ENODEV, "no HIP device available (%s); libkirag_late has no CPU fallback", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(KL_EINVAL, "device %d out of range [0,%d)", device, n);
    hipDeviceProp_t p;
    static thread_local int checked = -1;
    if (checked != device) {
        e = hipGetDeviceProperties(&p, device);
        if (e != hipSuccess) return fail(KL_EHIP, "hipGetDeviceProperties failed: %s", hipGetErrorString(e));
        if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
            return fail(KL_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device, p.gcnArchName);
        checked = device;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(KL_EHIP, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(e));
    return 0;
}

void free_workspace(Workspace& w) {
    if (w.dev) (void)hipFree(w.dev);
    for (int i = 0; i < 2; ++i) {
        if (w.host[i]) (void)hipHostFree(w.host[i]);
        if (w.copied[i]) (void)hipEventDestroy(w.copied[i]);
    }
    if (w.flag) (void)hipFree(w.flag);
    if (w.flag_host) (void)hipHostFree(w.flag_host);
    if (w.done) (void)hipEventDestroy(w.done);
    w = Workspace();
}

// the device's workspace with room for `bytes`, the staging buffer w.host[w.slot] free to be written, and `stream` ordered behind the last kernel that read
// the device copy
int acquire(int device, size_t bytes, hipStream_t stream, Workspace** out) {
    Workspace& w = g_ws[device];
    if (!w.done) {
        KL_HIP(hipEventCreateWithFlags(&w.copied[0], hipEventDisableTiming));
        KL_HIP(hipEventCreateWithFlags(&w.copied[1], hipEventDisableTiming));
        KL_HIP(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
        KL_HIP(hipMalloc(reinterpret_cast<void**>(&w.flag), sizeof(int)));
        KL_HIP(hipHostMalloc(reinterpret_cast<void**>(&w.flag_host), sizeof(int), hipHostMallocDefault));
    }
    w.slot ^= 1;
    const int k = w.slot;
    if (w.staged[k]) KL_HIP(hipEventSynchronize(w.copied[k]));     // the upload of two calls ago; the previous call's may still be queued
    if (w.used && w.last != stream) KL_HIP(hipStreamWaitEvent(stream, w.done, 0));
    size_t cap = 1 << 16;
    while (cap < bytes) cap *= 2;
    if (bytes > w.host_cap[k]) {
        if (w.host[k]) KL_HIP(hipHostFree(w.host[k]));
        w.host[k] = nullptr;
        w.host_cap[k] = 0;
        KL_HIP(hipHostMalloc(&w.host[k], cap, hipHostMallocDefault));
        w.host_cap[k] = cap;
    }
    if (bytes > w.cap) {
        if (w.used) KL_HIP(hipEventSynchronize(w.done));
        if (w.dev) KL_HIP(hipFree(w.dev));
        w.dev = nullptr;
        w.cap = 0;
        KL_HIP(hipMalloc(&w.dev, cap));
        w.cap = cap;
    }
    *out = &w;
    return 0;
}

int check_dim(const char* fn, int P) {
    if (P < KL_MIN_DIM || P > KL_MAX_DIM || P % 32 != 0)
        return fail(KL_EINVAL, "%s: P=%d: the row width must be a multiple of 32 in [%d, %d]", fn, P, KL_MIN_DIM, KL_MAX_DIM);
    return 0;
}

// the kernels read and write rows in 16-byte pieces (rows are a multiple of 64 bytes, so the first row's alignment is every row's)
int check_aligned(const char* fn, const char* name, const void* p, unsigned bytes) {
    if (reinterpret_cast<uintptr_t>(p) % bytes != 0) return fail(KL_EINVAL, "%s: %s=%p is not aligned to %u bytes", fn, name, p, bytes);
    return 0;
}

int check_offsets(const char* name, const int64_t* off, int64_t n) {
    if (n < 0) return fail(KL_EINVAL, "kl_maxsim: n%c=%lld is negative", name[0], (long long)n);
    if (!off) return fail(KL_EINVAL, "kl_maxsim: %s is null", name);
    if (off[0] != 0) return fail(KL_EINVAL, "kl_maxsim: %s[0]=%lld: offsets start at 0", name, (long long)off[0]);
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i])
            return fail(KL_EINVAL, "kl_maxsim: %s[%lld]=%lld is below %s[%lld]=%lld: offsets must not decrease", name, (long long)(i + 1), (long long)off[i + 1],
                        name, (long long)i, (long long)off[i]);
    return 0;
}

}  // namespace

extern "C" {

KL_API int kl_abi_version(void) { return KL_ABI_VERSION; }

KL_API const char* kl_last_error(void) { return last_error_ref().c_str(); }

KL_API void kl_release_scratch(void) {
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_ws.empty()) return;
    DeviceGuard guard;
    for (auto& kv : g_ws) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        if (kv.second.used) (void)hipEventSynchronize(kv.second.done);
        free_workspace(kv.second);
    }
    g_ws.clear();
}

KL_API int kl_gather_rows_f16(const float* block, const int64_t* src_row, int64_t T, int P, uint16_t* out, int device, void* stream) {
    KL_TRY(check_dim("kl_gather_rows_f16", P));
    if (T < 0) return fail(KL_EINVAL, "kl_gather_rows_f16: T=%lld is negative", (long long)T);
    if (T == 0) return 0;
    if (!src_row) return fail(KL_EINVAL, "kl_gather_rows_f16: src_row is null");
    for (int64_t t = 0; t < T; ++t)
        if (src_row[t] < 0) return fail(KL_EINVAL, "kl_gather_rows_f16: src_row[%lld]=%lld is negative", (long long)t, (long long)src_row[t]);
    if (!block || !out) return fail(KL_EINVAL, "kl_gather_rows_f16: block / out is null");
    KL_TRY(check_aligned("kl_gather_rows_f16", "block", block, 16));
    KL_TRY(check_aligned("kl_gather_rows_f16", "out", out, 16));
    const long long threads = (long long)T * (P / 8);
    if ((threads + 255) / 256 > 0x7fffffffLL) return fail(KL_EINVAL, "kl_gather_rows_f16: T=%lld rows of %d are more than one launch converts", (long long)T, P);
    std::lock_guard<std::mutex> lock(g_mutex);
    DeviceGuard guard;
    KL_TRY(select_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Workspace* w = nullptr;
    KL_TRY(acquire(device, (size_t)T * sizeof(long long), st, &w));
    std::memcpy(w->host[w->slot], src_row, (size_t)T * sizeof(long long));
    KL_HIP(hipMemcpyAsync(w->dev, w->host[w->slot], (size_t)T * sizeof(long long), hipMemcpyHostToDevice, st));
    KL_HIP(hipEventRecord(w->copied[w->slot], st));
    w->staged[w->slot] = true;
    KL_HIP(hipMemsetAsync(w->flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_gather_f16, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, block, static_cast<const long long*>(w->dev), (long long)T, P,
                       reinterpret_cast<_Float16*>(out), w->flag);
    KL_HIP(hipGetLastError());
    KL_HIP(hipEventRecord(w->done, st));
    w->used = true;
    w->last = st;
    KL_HIP(hipMemcpyAsync(w->flag_host, w->flag, sizeof(int), hipMemcpyDeviceToHost, st));
    KL_HIP(hipStreamSynchronize(st));
    if (*w->flag_host) return fail(KL_ERANGE, "kl_gather_rows_f16: a source element is not finite, or not finite once rounded to binary16");
    return 0;
}

KL_API int kl_maxsim(const uint16_t* q, const int64_t* q_off, int nq, const uint16_t* d, const int64_t* d_off, int64_t nd, const int64_t* pair_q,
                     const int64_t* pair_d, int64_t npairs, int P, int reduce, float* out, int device, void* stream) {
    KL_TRY(check_dim("kl_maxsim", P));
    if (reduce != KL_REDUCE_SUM && reduce != KL_REDUCE_MEAN) return fail(KL_EINVAL, "kl_maxsim: reduce=%d: 0 (sum) or 1 (mean)", reduce);
    KL_TRY(check_offsets("q_off", q_off, nq));
    KL_TRY(check_offsets("d_off", d_off, nd));
    if (npairs < 0 || npairs > 0x7fffffffLL) return fail(KL_EINVAL, "kl_maxsim: npairs=%lld outside [0, 2^31)", (long long)npairs);
    if (npairs > 0 && (!pair_q || !pair_d)) return fail(KL_EINVAL, "kl_maxsim: pair_q / pair_d is null");
    for (int64_t p = 0; p < npairs; ++p) {
        if (pair_q[p] < 0 || pair_q[p] >= nq) return fail(KL_EINVAL, "kl_maxsim: pair_q[%lld]=%lld outside [0, nq=%d)", (long long)p, (long long)pair_q[p], nq);
        if (pair_d[p] < 0 || pair_d[p] >= nd)
            return fail(KL_EINVAL, "kl_maxsim: pair_d[%lld]=%lld outside [0, nd=%lld)", (long long)p, (long long)pair_d[p], (long long)nd);
    }
    if (npairs == 0) return 0;
    if (!out || (q_off[nq] > 0 && !q) || (d_off[nd] > 0 && !d)) return fail(KL_EINVAL, "kl_maxsim: q / d / out is null");
    KL_TRY(check_aligned("kl_maxsim", "q", q, 16));
    KL_TRY(check_aligned("kl_maxsim", "d", d, 16));
    KL_TRY(check_aligned("kl_maxsim", "out", out, 4));
    std::lock_guard<std::mutex> lock(g_mutex);
    DeviceGuard guard;
    KL_TRY(select_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Workspace* w = nullptr;
    const size_t bytes = (size_t)npairs * sizeof(Pair);
    KL_TRY(acquire(device, bytes, st, &w));
    Pair* pairs = static_cast<Pair*>(w->host[w->slot]);
    for (int64_t p = 0; p < npairs; ++p) {
        const int64_t a = pair_q[p], b = pair_d[p];
        pairs[p] = Pair{q_off[a], q_off[a + 1] - q_off[a], d_off[b], d_off[b + 1] - d_off[b]};
    }
    const size_t lds = maxsim_lds_bytes(P);
    if (lds > 48 * 1024 && !w->lds_raised) {
        KL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_maxsim), hipFuncAttributeMaxDynamicSharedMemorySize, (int)maxsim_lds_bytes(KL_MAX_DIM)));
        w->lds_raised = true;
    }
    KL_HIP(hipMemcpyAsync(w->dev, w->host[w->slot], bytes, hipMemcpyHostToDevice, st));
    KL_HIP(hipEventRecord(w->copied[w->slot], st));
    w->staged[w->slot] = true;
    hipLaunchKernelGGL(k_maxsim, dim3((unsigned)npairs), dim3(THREADS), lds, st, reinterpret_cast<const _Float16*>(q), reinterpret_cast<const _Float16*>(d),
                       static_cast<const Pair*>(w->dev), P, reduce, out);
    KL_HIP(hipGetLastError());
    KL_HIP(hipEventRecord(w->done, st));
    w->used = true;
    w->last = st;
    return 0;
}

}  // extern "C"
