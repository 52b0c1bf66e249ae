// libkirag_sparse.so (include/kirag_sparse.h): exact top-k of sparse queries over a doc-range-blocked inverted index, and the ingest path that compacts the
// [B, V] block of a SPLADE forward into (term, binary16 weight) lists.  A translation unit of its own: it includes none of the product's headers and shares
// no object file with libkirag_amd.so or libkirag_late.so.  The few host helpers (error text, device guard, device selection) are restated from late.hip on
// purpose: the three libraries stay independent builds.
//
// k_sparse_scan, one workgroup of 1024 threads per (block, query):
//   * the block's R fp32 accumulators live in LDS (R = 16384: 64 KiB, two workgroups per CU; R = 32768: 128 KiB, one).  The query's terms are walked in ASCENDING order; the threads take the postings of one
//     term's segment and do a plain read-add-write on acc[local row]; a workgroup barrier separates the terms.  Within a term every posting names another
//     row, so no two threads touch one address and no atomic is needed; across terms the barrier fixes the order of the additions.  That IS the summation
//     order of the result definition, so the scores are the reference's bit for bit.
//   * the segments of up to 1024 terms are fetched at once (one dependent pointer-table read per 1024 terms, not per term) and the first 2048 postings of
//     the NEXT term are already in registers when a term's barrier is reached.
//   * select: positive fp32 values order like their bit patterns.  The key of a row is (score bits, R - 1 - row): all keys differ, larger is better, so the
//     k-th largest key is a threshold without ties.  It is found by a most-significant-digit-first radix select, 11 bits a pass (a 2048-bin histogram in LDS,
//     one suffix scan), which stops as soon as the digit's bin holds exactly what is still needed.  The rows at or above the threshold are appended to the
//     workgroup's candidate slots in any order: k_sparse_merge orders them.
//   * safety: the local row is masked to R - 1, the segment bounds are clamped to the block's posting count, candidate slots are clamped to k, and every
//     loop's trip count is bounded by those clamped values or by launch arguments.
// k_sparse_merge, one workgroup per query: the same radix select over the query's blocks * k candidate keys (score bits, ~global row), then a bitonic sort of
// the k survivors in LDS.
#define KS_API __attribute__((visibility("default")))
#include "../../include/kirag_sparse.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
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

#define KS_HIP(expr)                                                                                                              \
    do {                                                                                                                          \
        hipError_t _e = (expr);                                                                                                   \
        if (_e != hipSuccess)                                                                                                     \
            return fail(_e == hipErrorOutOfMemory ? KS_ENOMEM : KS_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                                                      \
    } while (0)

#define KS_TRY(expr)              \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)

using u32 = unsigned int;
using u64 = unsigned long long;

constexpr int R = KS_BLOCK_ROWS;
static_assert(R == 16384 || R == 32768, "KS_BLOCK_ROWS is 16384 or 32768: the local row is the high 16 bits of a posting and R fp32 accumulators fit LDS");
constexpr int ROW_BITS = R == 32768 ? 15 : 14;
constexpr int THREADS = 1024;
constexpr int WAVES = THREADS / 64;
constexpr int DIGIT = 11;                 // bits per select pass
constexpr int BINS = 1 << DIGIT;          // two bins per thread
constexpr int CHUNK = 1024;               // query terms whose segments are fetched at once
constexpr int CTHREADS = 256;             // the compaction kernels

// ---- the radix select both kernels use ----
// All THREADS threads call it.  key_at(i), i < n, gives a key > 0 or 0 for "no element"; the keys of one call differ from each other.  Returns the smallest
// key to keep so that min(k, number of elements) are kept, and that count in `kept` (0: keep nothing).  hist: BINS words, wsum: WAVES, res: 4.
template <int TOTAL_BITS, class KeyAt>
__device__ __forceinline__ u64 select_threshold(KeyAt key_at, long long n, u32 k, u32* hist, u32* wsum, u32* res, u32& kept) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 prefix = 0;
    u32 need = 0;
    int top = TOTAL_BITS;
    kept = 0;
    while (top > 0) {
        const int w = top < DIGIT ? top : DIGIT, shift = top - w;
        hist[2 * tid] = 0;
        hist[2 * tid + 1] = 0;
        __syncthreads();
        for (long long i = tid; i < n; i += THREADS) {
            const u64 key = key_at(i);
            if (key != 0 && (key >> top) == prefix) atomicAdd(&hist[(u32)(key >> shift) & ((1u << w) - 1)], 1u);
        }
        __syncthreads();
        // suffix sums from the largest digit down: thread t owns the bins BINS - 1 - 2t and BINS - 2 - 2t
        const u32 a = hist[BINS - 1 - 2 * tid], b = hist[BINS - 2 - 2 * tid], c = a + b;
        u32 incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u32 v = __shfl_up(incl, off);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        u32 before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < WAVES; ++i) {
            const u32 v = wsum[i];
            if (i < wave) before += v;
            total += v;
        }
        if (top == TOTAL_BITS) {
            need = total < k ? total : k;
            kept = need;
            if (need == 0) return ~0ull;
        }
        incl += before;
        const u32 excl = incl - c;
        if (excl < need && need <= incl) {
            const bool first = need <= excl + a;
            res[0] = first ? BINS - 1 - 2 * tid : BINS - 2 - 2 * tid;
            res[1] = first ? a : b;
            res[2] = first ? need - excl : need - excl - a;
        }
        __syncthreads();
        const u32 d = res[0], cnt = res[1];
        need = res[2];
        prefix = (prefix << w) | d;
        if (cnt == need) return prefix << shift;      // the whole bin is kept: nothing below it is
        top = shift;
    }
    return prefix;
}

__device__ __forceinline__ u64 local_key(float a, int row) {
    return a > 0.0f ? ((u64)__float_as_uint(a) << ROW_BITS) | (u32)(R - 1 - row) : 0ull;
}

__global__ __launch_bounds__(THREADS) void k_sparse_scan(const u32* __restrict__ post, const u32* __restrict__ ptr, const long long* __restrict__ post_off,
                                                         int V, int nblocks, const long long* __restrict__ q_off, const int* __restrict__ q_term,
                                                         const float* __restrict__ q_w, int nqs, int k, u64* __restrict__ cand, int* __restrict__ cand_cnt) {
    __shared__ __align__(16) float acc[R];
    __shared__ u32 aux[3 * CHUNK];          // the segments of a chunk of terms while scanning, the histogram while selecting
    __shared__ u32 wsum[WAVES];
    __shared__ u32 res[4];
    __shared__ u32 nsel;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nqs, q = blockIdx.x - b * nqs;      // neighbouring workgroups: neighbouring queries, the same block
    const long long t0 = q_off[q], t1 = q_off[q + 1];
    const long long base = post_off[b];
    const long long span = post_off[b + 1] - base;
    const long long cnt = span < 0 ? 0 : (span > 0xffffffffLL ? 0xffffffffLL : span);
    const long long slot0 = (long long)q * nblocks + b;
    if (t1 <= t0 || cnt == 0) {
        if (tid == 0) cand_cnt[slot0] = 0;
        return;
    }
    const u32* bp = post + base;
    const u32* pt = ptr + (long long)b * (V + 1);
    u32* seg_s = aux;
    u32* seg_e = aux + CHUNK;
    float* seg_w = reinterpret_cast<float*>(aux + 2 * CHUNK);
    if (tid == 0) nsel = 0;
    {
        const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        float4* a4 = reinterpret_cast<float4*>(acc);
#pragma unroll
        for (int i = 0; i < R / 4 / THREADS; ++i) a4[i * THREADS + tid] = z;
    }
    auto add = [&](u32 p, float w) {
        const int row = (int)(p >> 16) & (R - 1);
        const float d = (float)__builtin_bit_cast(_Float16, (unsigned short)(p & 0xffffu));
        acc[row] = __fadd_rn(acc[row], __fmul_rn(w, d));      // one multiply, one add, never fused
    };
    for (long long c0 = t0; c0 < t1; c0 += CHUNK) {
        const int mc = (int)(t1 - c0 < CHUNK ? t1 - c0 : CHUNK);
        __syncthreads();       // the zero fill; the readers of the previous chunk's segments
        if (tid < mc) {
            int t = q_term[c0 + tid];
            t = t < 0 ? 0 : (t >= V ? V - 1 : t);
            long long s = pt[t], e = pt[t + 1];
            s = s < cnt ? s : cnt;
            e = e < cnt ? e : cnt;
            if (e < s) e = s;
            seg_s[tid] = (u32)s;
            seg_e[tid] = (u32)e;
            seg_w[tid] = q_w[c0 + tid];
        }
        __syncthreads();
        long long s = seg_s[0], e = seg_e[0];
        u32 n0 = s + tid < e ? bp[s + tid] : 0u, n1 = s + tid + THREADS < e ? bp[s + tid + THREADS] : 0u;
        for (int j = 0; j < mc; ++j) {
            const long long cs = s, ce = e;
            const u32 p0 = n0, p1 = n1;
            const float w = seg_w[j];
            if (j + 1 < mc) {
                s = seg_s[j + 1];
                e = seg_e[j + 1];
                n0 = s + tid < e ? bp[s + tid] : 0u;
                n1 = s + tid + THREADS < e ? bp[s + tid + THREADS] : 0u;
            }
            if (cs + tid < ce) add(p0, w);
            if (cs + tid + THREADS < ce) add(p1, w);
            for (long long i = cs + tid + 2 * THREADS; i < ce; i += THREADS) add(bp[i], w);
            __syncthreads();
        }
    }
    u32 kept;
    const u64 T = select_threshold<31 + ROW_BITS>([&](long long i) { return local_key(acc[i], (int)i); }, R, (u32)k, aux, wsum, res, kept);
    if (tid == 0) cand_cnt[slot0] = (int)kept;
    if (kept == 0) return;
    u64* out = cand + slot0 * k;
#pragma unroll 4
    for (int i = tid; i < R; i += THREADS) {
        const float a = acc[i];
        const u64 key = local_key(a, i);
        if (key != 0 && key >= T) {
            const u32 slot = atomicAdd(&nsel, 1u);
            if (slot < (u32)k) out[slot] = ((u64)__float_as_uint(a) << 32) | (u32)~(u32)(b * R + i);
        }
    }
}

__global__ __launch_bounds__(THREADS) void k_sparse_merge(const u64* __restrict__ cand, const int* __restrict__ cand_cnt, int nblocks, int k, int sort_n,
                                                          float* __restrict__ out_score, long long* __restrict__ out_row) {
    __shared__ u32 hist[BINS];
    __shared__ u64 best[KS_MAX_K];
    __shared__ u32 wsum[WAVES];
    __shared__ u32 res[4];
    __shared__ u32 nsel;
    const int tid = threadIdx.x, q = blockIdx.x;
    const u64* cq = cand + (long long)q * nblocks * k;
    const int* cc = cand_cnt + (long long)q * nblocks;
    const long long n = (long long)nblocks * k;
    auto key_at = [&](long long i) -> u64 {
        const int b = (int)(i / k), s = (int)(i - (long long)b * k);
        return s < cc[b] ? cq[i] : 0ull;
    };
    best[tid] = 0;
    if (tid == 0) nsel = 0;
    u32 kept;
    const u64 T = select_threshold<63>(key_at, n, (u32)k, hist, wsum, res, kept);      // its barriers also publish best[] and nsel
    if (kept != 0) {
        for (long long i = tid; i < n; i += THREADS) {
            const u64 key = key_at(i);
            if (key != 0 && key >= T) {
                const u32 slot = atomicAdd(&nsel, 1u);
                if (slot < (u32)sort_n) best[slot] = key;
            }
        }
        // bitonic sort of best[0 .. sort_n), descending: (score descending, row ascending)
        for (int size = 2; size <= sort_n; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                __syncthreads();
                const int p = tid ^ stride;
                if (tid < sort_n && p > tid) {
                    const u64 a = best[tid], c = best[p];
                    if ((tid & size) == 0 ? a < c : a > c) {
                        best[tid] = c;
                        best[p] = a;
                    }
                }
            }
    }
    __syncthreads();
    if (tid < k) {
        const u64 key = best[tid];
        out_score[(long long)q * k + tid] = key ? __uint_as_float((u32)(key >> 32)) : 0.0f;
        out_row[(long long)q * k + tid] = key ? (long long)(u32)~(u32)key : -1LL;
    }
}

// ---- ingest: [B, V] fp32 -> per-row (term, binary16 weight) lists ----
struct Kept {
    bool keep, bad;
    unsigned short bits;
};

__device__ __forceinline__ Kept classify(float v, int c, const int* __restrict__ skip, int ns) {
    const _Float16 h = (_Float16)v;                       // round to nearest even
    const float hf = (float)h;
    Kept r;
    r.bad = !(fabsf(hf) <= 65504.0f);                     // NaN or Inf, in the source or made by the rounding
    r.keep = hf > 0.0f;
    for (int s = 0; s < ns; ++s) r.keep = r.keep && skip[s] != c;
    r.bits = __builtin_bit_cast(unsigned short, h);
    return r;
}

__global__ __launch_bounds__(CTHREADS) void k_sparse_count(const float* __restrict__ block, int V, const int* __restrict__ skip, int ns,
                                                           int* __restrict__ counts, int* __restrict__ flags) {
    __shared__ int wcnt[CTHREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* src = block + (long long)blockIdx.x * V;
    int n = 0;
    bool bad = false;
    for (int c = tid; c < V; c += CTHREADS) {
        const Kept r = classify(src[c], c, skip, ns);
        n += r.keep ? 1 : 0;
        bad |= r.bad;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off);
    if (lane == 0) wcnt[wave] = n;
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (bad) flags[0] = 1;
}

// one workgroup per row; tiles of CTHREADS terms in ascending order, a ballot per wave and a prefix over the waves keep the order
__global__ __launch_bounds__(CTHREADS) void k_sparse_compact(const float* __restrict__ block, int V, const int* __restrict__ skip, int ns,
                                                             const long long* __restrict__ row_off, int* __restrict__ terms,
                                                             unsigned short* __restrict__ weights, int* __restrict__ flags) {
    __shared__ int wcnt[2][CTHREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* src = block + (long long)blockIdx.x * V;
    const long long o = row_off[blockIdx.x], len = row_off[blockIdx.x + 1] - o;
    long long done = 0;
    bool bad = false;
    int buf = 0;
    for (int c0 = 0; c0 < V; c0 += CTHREADS, buf ^= 1) {
        const int c = c0 + tid;
        Kept r = {false, false, 0};
        if (c < V) r = classify(src[c], c, skip, ns);
        bad |= r.bad;
        const u64 mask = __ballot(r.keep);
        if (lane == 0) wcnt[buf][wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < CTHREADS / 64; ++i) {
            const int v = wcnt[buf][i];
            if (i < wave) before += v;
            total += v;
        }
        const long long pos = done + before + __popcll(mask & ((1ull << lane) - 1));
        if (r.keep && pos < len) {
            terms[o + pos] = c;
            weights[o + pos] = r.bits;
        }
        done += total;
    }
    if (bad) flags[0] = 1;
    if (tid == 0 && done != len) flags[1] = 1;
}

// ---- host side ----
struct Workspace {
    void* host = nullptr;        // pinned staging buffer: the checked copies of the caller's host arrays
    size_t host_cap = 0;
    void* dev = nullptr;         // their device copy
    size_t dev_cap = 0;
    void* cand = nullptr;        // candidate keys, then the per-(query, block) counts
    size_t cand_cap = 0;
    int* flags = nullptr;        // device int[2]: not finite, count mismatch
    int* flags_host = nullptr;   // pinned
};

std::mutex g_mutex;
std::map<int, Workspace> g_ws;

// the caller's current device, put back when an entry point returns (select_device and ks_release_scratch change it)
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
    if (e != hipSuccess || n <= 0) return fail(KS_ENODEV, "no HIP device available (%s); libkirag_sparse has no CPU fallback", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(KS_EINVAL, "device %d out of range [0,%d)", device, n);
    hipDeviceProp_t p;
    static thread_local int checked = -1;
    if (checked != device) {
        e = hipGetDeviceProperties(&p, device);
        if (e != hipSuccess) return fail(KS_EHIP, "hipGetDeviceProperties failed: %s", hipGetErrorString(e));
        if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
            return fail(KS_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device, p.gcnArchName);
        checked = device;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(KS_EHIP, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(e));
    return 0;
}

void free_workspace(Workspace& w) {
    if (w.host) (void)hipHostFree(w.host);
    if (w.dev) (void)hipFree(w.dev);
    if (w.cand) (void)hipFree(w.cand);
    if (w.flags) (void)hipFree(w.flags);
    if (w.flags_host) (void)hipHostFree(w.flags_host);
    w = Workspace();
}

size_t grown(size_t bytes) {
    size_t cap = 1 << 16;
    while (cap < bytes) cap *= 2;
    return cap;
}

// the device's workspace with `bytes` of staging room on both sides.  Every compute call ends with a stream synchronisation, so nothing is in flight here.
int acquire(int device, size_t bytes, Workspace** out) {
    Workspace& w = g_ws[device];
    if (!w.flags) {
        KS_HIP(hipMalloc(reinterpret_cast<void**>(&w.flags), 2 * sizeof(int)));
        KS_HIP(hipHostMalloc(reinterpret_cast<void**>(&w.flags_host), 2 * sizeof(int), hipHostMallocDefault));
    }
    if (bytes > w.host_cap) {
        if (w.host) KS_HIP(hipHostFree(w.host));
        w.host = nullptr;
        w.host_cap = 0;
        KS_HIP(hipHostMalloc(&w.host, grown(bytes), hipHostMallocDefault));
        w.host_cap = grown(bytes);
    }
    if (bytes > w.dev_cap) {
        if (w.dev) KS_HIP(hipFree(w.dev));
        w.dev = nullptr;
        w.dev_cap = 0;
        KS_HIP(hipMalloc(&w.dev, grown(bytes)));
        w.dev_cap = grown(bytes);
    }
    *out = &w;
    return 0;
}

int reserve_candidates(Workspace& w, size_t bytes) {
    if (bytes > w.cand_cap) {
        if (w.cand) KS_HIP(hipFree(w.cand));
        w.cand = nullptr;
        w.cand_cap = 0;
        KS_HIP(hipMalloc(&w.cand, grown(bytes)));
        w.cand_cap = grown(bytes);
    }
    return 0;
}

int check_aligned(const char* fn, const char* name, const void* p, unsigned bytes) {
    if (reinterpret_cast<uintptr_t>(p) % bytes != 0) return fail(KS_EINVAL, "%s: %s=%p is not aligned to %u bytes", fn, name, p, bytes);
    return 0;
}

int check_offsets(const char* fn, const char* name, const int64_t* off, int64_t n) {
    if (!off) return fail(KS_EINVAL, "%s: %s is null", fn, name);
    if (off[0] != 0) return fail(KS_EINVAL, "%s: %s[0]=%lld: offsets start at 0", fn, name, (long long)off[0]);
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i])
            return fail(KS_EINVAL, "%s: %s[%lld]=%lld is below %s[%lld]=%lld: offsets must not decrease", fn, name, (long long)(i + 1), (long long)off[i + 1],
                        name, (long long)i, (long long)off[i]);
    return 0;
}

long long candidate_bound() {
    const char* s = std::getenv("KIRAG_SPARSE_MAX_CANDIDATES");
    if (s && *s) {
        char* end = nullptr;
        const long long v = std::strtoll(s, &end, 10);
        if (end && *end == 0 && v >= 1 && v <= KS_MAX_CANDIDATES) return v;
    }
    return KS_MAX_CANDIDATES;
}

int check_block_args(const char* fn, const float* block, int B, int V, const int32_t* skip_terms, int ns) {
    if (B < 0) return fail(KS_EINVAL, "%s: B=%d is negative", fn, B);
    if (V < 1 || V > (1 << 24)) return fail(KS_EINVAL, "%s: V=%d outside [1, 2^24]", fn, V);
    if (ns < 0 || ns > KS_MAX_SKIP) return fail(KS_EINVAL, "%s: ns=%d outside [0, %d]", fn, ns, KS_MAX_SKIP);
    if (ns > 0 && !skip_terms) return fail(KS_EINVAL, "%s: skip_terms is null", fn);
    for (int s = 0; s < ns; ++s)
        if (skip_terms[s] < 0 || skip_terms[s] >= V) return fail(KS_EINVAL, "%s: skip_terms[%d]=%d outside [0, V=%d)", fn, s, skip_terms[s], V);
    if (B > 0 && !block) return fail(KS_EINVAL, "%s: block is null", fn);
    return check_aligned(fn, "block", block, 4);
}

constexpr size_t SKIP_BYTES = KS_MAX_SKIP * sizeof(int);      // the skip list leads the staging buffer of the ingest calls

int read_flags(Workspace* w, hipStream_t st) {
    KS_HIP(hipMemcpyAsync(w->flags_host, w->flags, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    KS_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

KS_API int ks_abi_version(void) { return KS_ABI_VERSION; }

KS_API const char* ks_last_error(void) { return last_error_ref().c_str(); }

KS_API int ks_block_rows(void) { return R; }

KS_API void ks_release_scratch(void) {
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_ws.empty()) return;
    DeviceGuard guard;
    for (auto& kv : g_ws) {
        if (hipSetDevice(kv.first) != hipSuccess) continue;
        (void)hipDeviceSynchronize();
        free_workspace(kv.second);
    }
    g_ws.clear();
}

KS_API int ks_search(const uint32_t* post, const uint32_t* ptr, const int64_t* post_off, int64_t N, int V, const int64_t* q_off, int nq,
                     const int32_t* q_term, const float* q_w, int k, float* out_score, int64_t* out_row, int device, void* stream) {
    const char* fn = "ks_search";
    if (N < 0 || N > (1LL << 31)) return fail(KS_EINVAL, "%s: N=%lld outside [0, 2^31]", fn, (long long)N);
    if (V < 1 || V > (1 << 24)) return fail(KS_EINVAL, "%s: V=%d outside [1, 2^24]", fn, V);
    if (k < 1 || k > KS_MAX_K) return fail(KS_EINVAL, "%s: k=%d outside [1, %d]", fn, k, KS_MAX_K);
    if (nq < 0 || nq > KS_MAX_QUERIES) return fail(KS_EINVAL, "%s: nq=%d outside [0, %d]", fn, nq, KS_MAX_QUERIES);
    const int64_t nblocks = (N + R - 1) / R;
    KS_TRY(check_offsets(fn, "post_off", post_off, nblocks));
    for (int64_t b = 0; b < nblocks; ++b)
        if (post_off[b + 1] - post_off[b] > 0xffffffffLL)
            return fail(KS_EINVAL, "%s: post_off[%lld]: block %lld holds %lld postings, more than 2^32 - 1", fn, (long long)(b + 1), (long long)b,
                        (long long)(post_off[b + 1] - post_off[b]));
    KS_TRY(check_offsets(fn, "q_off", q_off, nq));
    const int64_t nnz = q_off[nq];
    if (nnz > 0 && (!q_term || !q_w)) return fail(KS_EINVAL, "%s: q_term / q_w is null", fn);
    for (int i = 0; i < nq; ++i)
        for (int64_t j = q_off[i]; j < q_off[i + 1]; ++j) {
            if (q_term[j] < 0 || q_term[j] >= V) return fail(KS_EINVAL, "%s: q_term[%lld]=%d outside [0, V=%d)", fn, (long long)j, q_term[j], V);
            if (j > q_off[i] && q_term[j] <= q_term[j - 1])
                return fail(KS_EINVAL, "%s: q_term[%lld]=%d does not ascend after %d: the terms of a query are strictly ascending", fn, (long long)j,
                            q_term[j], q_term[j - 1]);
            if (!(q_w[j] > 0.0f) || !std::isfinite(q_w[j])) return fail(KS_EINVAL, "%s: q_w[%lld]=%g: query weights are finite and > 0", fn, (long long)j, (double)q_w[j]);
        }
    const long long bound = candidate_bound();
    const long long per_query = (long long)nblocks * k;
    if (per_query > bound)
        return fail(KS_EINVAL, "%s: N=%lld, k=%d: one query's %lld candidates exceed the workspace bound of %lld", fn, (long long)N, k, per_query, bound);
    if (nq == 0) return 0;
    if (!out_score || !out_row) return fail(KS_EINVAL, "%s: out_score / out_row is null", fn);
    if (nblocks > 0 && post_off[nblocks] > 0 && !post) return fail(KS_EINVAL, "%s: post is null", fn);
    if (nblocks > 0 && !ptr) return fail(KS_EINVAL, "%s: ptr is null", fn);
    KS_TRY(check_aligned(fn, "post", post, 4));
    KS_TRY(check_aligned(fn, "ptr", ptr, 4));
    KS_TRY(check_aligned(fn, "out_score", out_score, 4));
    KS_TRY(check_aligned(fn, "out_row", out_row, 8));

    std::lock_guard<std::mutex> lock(g_mutex);
    DeviceGuard guard;
    KS_TRY(select_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // staging: post_off | q_off | q_term (padded to 8 bytes) | q_w
    const size_t b_post = (size_t)(nblocks + 1) * 8, b_qoff = (size_t)(nq + 1) * 8, b_term = ((size_t)nnz * 4 + 7) / 8 * 8, b_w = (size_t)nnz * 4;
    const size_t bytes = b_post + b_qoff + b_term + b_w;
    Workspace* w = nullptr;
    KS_TRY(acquire(device, bytes, &w));
    char* h = static_cast<char*>(w->host);
    std::memcpy(h, post_off, b_post);
    std::memcpy(h + b_post, q_off, b_qoff);
    if (nnz) {
        std::memcpy(h + b_post + b_qoff, q_term, (size_t)nnz * 4);
        std::memcpy(h + b_post + b_qoff + b_term, q_w, b_w);
    }
    KS_HIP(hipMemcpyAsync(w->dev, w->host, bytes, hipMemcpyHostToDevice, st));
    const char* d = static_cast<const char*>(w->dev);
    const long long* d_post_off = reinterpret_cast<const long long*>(d);
    const long long* d_q_off = reinterpret_cast<const long long*>(d + b_post);
    const int* d_term = reinterpret_cast<const int*>(d + b_post + b_qoff);
    const float* d_w = reinterpret_cast<const float*>(d + b_post + b_qoff + b_term);

    const long long slice = per_query == 0 ? nq : (bound / per_query < nq ? bound / per_query : nq);       // >= 1: per_query <= bound
    const size_t key_bytes = (size_t)slice * per_query * sizeof(u64), cnt_bytes = (size_t)slice * nblocks * sizeof(int);
    KS_TRY(reserve_candidates(*w, key_bytes + cnt_bytes + 8));
    u64* cand = static_cast<u64*>(w->cand);
    int* cand_cnt = reinterpret_cast<int*>(static_cast<char*>(w->cand) + key_bytes);
    int sort_n = 2;
    while (sort_n < k) sort_n *= 2;
    for (long long q0 = 0; q0 < nq; q0 += slice) {
        const int nqs = (int)(nq - q0 < slice ? nq - q0 : slice);
        if (nblocks > 0) {
            hipLaunchKernelGGL(k_sparse_scan, dim3((unsigned)(nblocks * nqs)), dim3(THREADS), 0, st, post, ptr, d_post_off, V, (int)nblocks, d_q_off + q0,
                               d_term, d_w, nqs, k, cand, cand_cnt);
            KS_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(k_sparse_merge, dim3((unsigned)nqs), dim3(THREADS), 0, st, cand, cand_cnt, (int)nblocks, k, sort_n, out_score + q0 * k,
                           reinterpret_cast<long long*>(out_row) + q0 * k);
        KS_HIP(hipGetLastError());
    }
    KS_HIP(hipStreamSynchronize(st));
    return 0;
}

KS_API int ks_count_positive(const float* block, int B, int V, const int32_t* skip_terms, int ns, int64_t* counts, int device, void* stream) {
    const char* fn = "ks_count_positive";
    KS_TRY(check_block_args(fn, block, B, V, skip_terms, ns));
    if (B == 0) return 0;
    if (!counts) return fail(KS_EINVAL, "%s: counts is null", fn);
    std::lock_guard<std::mutex> lock(g_mutex);
    DeviceGuard guard;
    KS_TRY(select_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Workspace* w = nullptr;
    const size_t bytes = SKIP_BYTES + (size_t)B * sizeof(int);
    KS_TRY(acquire(device, bytes, &w));
    if (ns) std::memcpy(w->host, skip_terms, (size_t)ns * sizeof(int));
    KS_HIP(hipMemcpyAsync(w->dev, w->host, SKIP_BYTES, hipMemcpyHostToDevice, st));
    KS_HIP(hipMemsetAsync(w->flags, 0, 2 * sizeof(int), st));
    int* d_counts = reinterpret_cast<int*>(static_cast<char*>(w->dev) + SKIP_BYTES);
    hipLaunchKernelGGL(k_sparse_count, dim3((unsigned)B), dim3(CTHREADS), 0, st, block, V, static_cast<const int*>(w->dev), ns, d_counts, w->flags);
    KS_HIP(hipGetLastError());
    int* h_counts = reinterpret_cast<int*>(static_cast<char*>(w->host) + SKIP_BYTES);
    KS_HIP(hipMemcpyAsync(h_counts, d_counts, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    KS_TRY(read_flags(w, st));
    if (w->flags_host[0]) return fail(KS_ERANGE, "%s: an element of the block is not finite, or not finite once rounded to binary16", fn);
    for (int r = 0; r < B; ++r) counts[r] = h_counts[r];
    return 0;
}

KS_API int ks_compact_rows(const float* block, int B, int V, const int32_t* skip_terms, int ns, const int64_t* row_off, int32_t* terms,
                           uint16_t* weights, int device, void* stream) {
    const char* fn = "ks_compact_rows";
    KS_TRY(check_block_args(fn, block, B, V, skip_terms, ns));
    KS_TRY(check_offsets(fn, "row_off", row_off, B));
    for (int r = 0; r < B; ++r)
        if (row_off[r + 1] - row_off[r] > V)
            return fail(KS_EINVAL, "%s: row_off[%d]: row %d is given %lld entries, more than V=%d", fn, r + 1, r, (long long)(row_off[r + 1] - row_off[r]), V);
    if (B == 0) return 0;
    if (row_off[B] > 0 && (!terms || !weights)) return fail(KS_EINVAL, "%s: terms / weights is null", fn);
    KS_TRY(check_aligned(fn, "terms", terms, 4));
    KS_TRY(check_aligned(fn, "weights", weights, 2));
    std::lock_guard<std::mutex> lock(g_mutex);
    DeviceGuard guard;
    KS_TRY(select_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    Workspace* w = nullptr;
    const size_t bytes = SKIP_BYTES + (size_t)(B + 1) * sizeof(long long);
    KS_TRY(acquire(device, bytes, &w));
    if (ns) std::memcpy(w->host, skip_terms, (size_t)ns * sizeof(int));
    std::memcpy(static_cast<char*>(w->host) + SKIP_BYTES, row_off, (size_t)(B + 1) * sizeof(long long));
    KS_HIP(hipMemcpyAsync(w->dev, w->host, bytes, hipMemcpyHostToDevice, st));
    KS_HIP(hipMemsetAsync(w->flags, 0, 2 * sizeof(int), st));
    hipLaunchKernelGGL(k_sparse_compact, dim3((unsigned)B), dim3(CTHREADS), 0, st, block, V, static_cast<const int*>(w->dev), ns,
                       reinterpret_cast<const long long*>(static_cast<char*>(w->dev) + SKIP_BYTES), terms, weights, w->flags);
    KS_HIP(hipGetLastError());
    KS_TRY(read_flags(w, st));
    if (w->flags_host[0]) return fail(KS_ERANGE, "%s: an element of the block is not finite, or not finite once rounded to binary16", fn);
    if (w->flags_host[1]) return fail(KS_EINVAL, "%s: row_off disagrees with the number of kept elements of a row", fn);
    return 0;
}

}  // extern "C"
