// libkirag_pairs.so (include/kirag_pairs.h): the exact sparse score of given (query, row) pairs over the forward form of a sparse index.  A translation unit
// of its own: it includes none of the product's headers and shares no object file with libkirag_amd.so, libkirag_late.so or libkirag_sparse.so.  The few host
// helpers (error text, device guard, device selection, the pinned staging workspace) are restated from sparse.hip on purpose: the four
// libraries stay independent builds.
//
// k_pair_dot, one wave per pair, four waves per workgroup of 256 threads, no LDS:
//   * the wave walks the row's entries in chunks of 64, one entry per lane: 256 B of terms and 128 B of weights per chunk, coalesced.
//   * each lane looks its term up in the query's strictly ascending term list by a lower-bound binary search (at most 25 steps: a query holds at most
//     2^24 terms); the staged query CSR is small and shared by the pairs of a query, so it is served from L2.
//   * a hit computes p = q_w * float(d), one fp32 multiply (the build has -ffp-contract=off and the intrinsics say so again).
//   * the ordered sum walks the 64-bit ballot mask of the hits from the lowest lane up: s = s + readlane(p, lane).  Lanes within a chunk and chunks within a
//     row ascend by term, so this IS the summation order of the result definition and the bits are the reference's; s starts as +0.0.
//   * lane 0 writes out[p] with a plain store.
//   * safety: the record's row segment is clamped to [0, nnz], the query index to [0, nq), the query segment to the staged query length; every loop's trip
//     count is bounded by those clamped values or by the constant 25.  No atomics; no workgroup waits for another.
#define KP_API __attribute__((visibility("default")))
#include "../../include/kirag_pairs.h"

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

#define KP_HIP(expr)                                                                                                              \
    do {                                                                                                                          \
        hipError_t _e = (expr);                                                                                                   \
        if (_e != hipSuccess)                                                                                                     \
            return fail(_e == hipErrorOutOfMemory ? KP_ENOMEM : KP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                                                      \
    } while (0)

#define KP_TRY(expr)              \
    do {                          \
        int _rc = (expr);         \
        if (_rc != 0) return _rc; \
    } while (0)

using u64 = unsigned long long;

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;       // pairs per workgroup
constexpr int MAX_V = 1 << 24;
constexpr int SEARCH_STEPS = 25;          // a lower bound over at most 2^24 ascending terms

// what the host makes of a pair after checking it: the kernel reads these, never the caller's arrays
struct PairRec {
    long long start;      // row_off[row]
    int len;              // row_off[row + 1] - row_off[row], <= V
    int q;                // the query index
};
static_assert(sizeof(PairRec) == 16, "a pair record is 16 bytes");

__global__ __launch_bounds__(THREADS) void k_pair_dot(const int* __restrict__ terms, const unsigned short* __restrict__ weights, long long nnz,
                                                      const long long* __restrict__ q_off, int nq, long long qnnz, const int* __restrict__ q_term,
                                                      const float* __restrict__ q_w, const PairRec* __restrict__ rec, int n, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int p = (int)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (p >= n) return;
    const PairRec r = rec[p];
    int q = r.q;
    q = q < 0 ? 0 : (q >= nq ? nq - 1 : q);
    long long qs = q_off[q], qe = q_off[q + 1];
    qs = qs < 0 ? 0 : (qs > qnnz ? qnnz : qs);
    qe = qe < qs ? qs : (qe > qnnz ? qnnz : qe);
    const int m = (int)(qe - qs > MAX_V ? MAX_V : qe - qs);
    long long start = r.start;
    start = start < 0 ? 0 : (start > nnz ? nnz : start);
    long long room = nnz - start;
    room = room > MAX_V ? MAX_V : room;
    const int len = r.len < 0 ? 0 : (r.len > room ? (int)room : r.len);
    const int* qt = q_term + qs;
    const float* qw = q_w + qs;
    const int* rt = terms + start;
    const unsigned short* rw = weights + start;
    float s = 0.0f;
    if (m > 0)
        for (int c = 0; c < len; c += 64) {
            const int i = c + lane;
            const bool in = i < len;
            const int t = in ? rt[i] : -1;
            const unsigned short wb = in ? rw[i] : (unsigned short)0;
            int lo = 0, hi = m;
#pragma unroll 1
            for (int step = 0; step < SEARCH_STEPS && lo < hi; ++step) {
                const int mid = (lo + hi) >> 1;
                if (qt[mid] < t)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            const bool hit = in && lo < m && qt[lo] == t;
            float prod = 0.0f;
            if (hit) prod = __fmul_rn(qw[lo], (float)__builtin_bit_cast(_Float16, wb));      // one multiply, never fused with the add
            u64 mask = __ballot(hit);
            while (mask) {                                                                    // wave-uniform: the mask is the same in every lane
                const int l = __builtin_ctzll(mask);
                s = __fadd_rn(s, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(prod), l)));
                mask &= mask - 1;
            }
        }
    if (lane == 0) out[p] = s;
}

// ---- host side ----
struct Workspace {
    void* host = nullptr;        // pinned staging buffer: the query CSR and a slice of pair records
    size_t host_cap = 0;
    void* dev = nullptr;         // their device copy
    size_t dev_cap = 0;
};

std::mutex g_mutex;
std::map<int, Workspace> g_ws;

// the caller's current device, put back when an entry point returns (select_device and kp_release_scratch change it)
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
    if (e != hipSuccess || n <= 0) return fail(KP_ENODEV, "no HIP device available (%s); libkirag_pairs has no CPU fallback", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(KP_EINVAL, "device %d out of range [0,%d)", device, n);
    hipDeviceProp_t p;
    static thread_local int checked = -1;
    if (checked != device) {
        e = hipGetDeviceProperties(&p, device);
        if (e != hipSuccess) return fail(KP_EHIP, "hipGetDeviceProperties failed: %s", hipGetErrorString(e));
        if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
            return fail(KP_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device, p.gcnArchName);
        checked = device;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(KP_EHIP, "hipSetDevice(%d) failed: %s", device, hipGetErrorString(e));
    return 0;
}

void free_workspace(Workspace& w) {
    if (w.host) (void)hipHostFree(w.host);
    if (w.dev) (void)hipFree(w.dev);
    w = Workspace();
}

size_t grown(size_t bytes) {
    size_t cap = 1 << 16;
    while (cap < bytes) cap *= 2;
    return cap;
}

// the device's workspace with `bytes` of staging room on both sides.  Every call ends with a stream synchronisation, so nothing is in flight here.
int acquire(int device, size_t bytes, Workspace** out) {
    Workspace& w = g_ws[device];
    if (bytes > w.host_cap) {
        if (w.host) KP_HIP(hipHostFree(w.host));
        w.host = nullptr;
        w.host_cap = 0;
        KP_HIP(hipHostMalloc(&w.host, grown(bytes), hipHostMallocDefault));
        w.host_cap = grown(bytes);
    }
    if (bytes > w.dev_cap) {
        if (w.dev) KP_HIP(hipFree(w.dev));
        w.dev = nullptr;
        w.dev_cap = 0;
        KP_HIP(hipMalloc(&w.dev, grown(bytes)));
        w.dev_cap = grown(bytes);
    }
    *out = &w;
    return 0;
}

int check_aligned(const char* fn, const char* name, const void* p, unsigned bytes) {
    if (reinterpret_cast<uintptr_t>(p) % bytes != 0) return fail(KP_EINVAL, "%s: %s=%p is not aligned to %u bytes", fn, name, p, bytes);
    return 0;
}

int check_offsets(const char* fn, const char* name, const int64_t* off, int64_t n) {
    if (!off) return fail(KP_EINVAL, "%s: %s is null", fn, name);
    if (off[0] != 0) return fail(KP_EINVAL, "%s: %s[0]=%lld: offsets start at 0", fn, name, (long long)off[0]);
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i])
            return fail(KP_EINVAL, "%s: %s[%lld]=%lld is below %s[%lld]=%lld: offsets must not decrease", fn, name, (long long)(i + 1), (long long)off[i + 1],
                        name, (long long)i, (long long)off[i]);
    return 0;
}

long long staged_bound() {
    const char* s = std::getenv("KIRAG_PAIRS_MAX_STAGED");
    if (s && *s) {
        char* end = nullptr;
        const long long v = std::strtoll(s, &end, 10);
        if (end && *end == 0 && v >= 1 && v <= KP_MAX_STAGED_PAIRS) return v;
    }
    return KP_MAX_STAGED_PAIRS;
}

}  // namespace

extern "C" {

KP_API int kp_abi_version(void) { return KP_ABI_VERSION; }

KP_API const char* kp_last_error(void) { return last_error_ref().c_str(); }

KP_API void kp_release_scratch(void) {
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

KP_API int kp_sparse_dot(const int32_t* terms, const uint16_t* weights, int64_t nnz, const int64_t* row_off, int64_t N, int V, const int64_t* q_off, int nq,
                         const int32_t* q_term, const float* q_w, const int64_t* pair_q, const int64_t* pair_row, int64_t npairs, float* out, int device,
                         void* stream) {
    const char* fn = "kp_sparse_dot";
    if (V < 1 || V > MAX_V) return fail(KP_EINVAL, "%s: V=%d outside [1, 2^24]", fn, V);
    if (N < 0 || N > (1LL << 31)) return fail(KP_EINVAL, "%s: N=%lld outside [0, 2^31]", fn, (long long)N);
    if (nnz < 0) return fail(KP_EINVAL, "%s: nnz=%lld is negative", fn, (long long)nnz);
    if (npairs < 0 || npairs > KP_MAX_PAIRS) return fail(KP_EINVAL, "%s: npairs=%lld outside [0, %d]", fn, (long long)npairs, KP_MAX_PAIRS);
    if (nq < 0 || nq > KP_MAX_QUERIES) return fail(KP_EINVAL, "%s: nq=%d outside [0, %d]", fn, nq, KP_MAX_QUERIES);
    KP_TRY(check_offsets(fn, "q_off", q_off, nq));
    const int64_t qnnz = q_off[nq];
    if (qnnz > 0 && (!q_term || !q_w)) return fail(KP_EINVAL, "%s: q_term / q_w is null", fn);
    for (int i = 0; i < nq; ++i)
        for (int64_t j = q_off[i]; j < q_off[i + 1]; ++j) {
            if (q_term[j] < 0 || q_term[j] >= V) return fail(KP_EINVAL, "%s: q_term[%lld]=%d outside [0, V=%d)", fn, (long long)j, q_term[j], V);
            if (j > q_off[i] && q_term[j] <= q_term[j - 1])
                return fail(KP_EINVAL, "%s: q_term[%lld]=%d does not ascend after %d: the terms of a query are strictly ascending", fn, (long long)j,
                            q_term[j], q_term[j - 1]);
            if (!(q_w[j] > 0.0f) || !std::isfinite(q_w[j])) return fail(KP_EINVAL, "%s: q_w[%lld]=%g: query weights are finite and > 0", fn, (long long)j, (double)q_w[j]);
        }
    if (npairs > 0 && (!pair_q || !pair_row)) return fail(KP_EINVAL, "%s: pair_q / pair_row is null", fn);
    if (npairs > 0 && !row_off) return fail(KP_EINVAL, "%s: row_off is null", fn);
    bool any_entry = false;
    for (int64_t p = 0; p < npairs; ++p) {
        const int64_t q = pair_q[p], r = pair_row[p];
        if (q < 0 || q >= nq) return fail(KP_EINVAL, "%s: pair_q[%lld]=%lld outside [0, nq=%d)", fn, (long long)p, (long long)q, nq);
        if (r < 0 || r >= N) return fail(KP_EINVAL, "%s: pair_row[%lld]=%lld outside [0, N=%lld)", fn, (long long)p, (long long)r, (long long)N);
        const int64_t a = row_off[r], b = row_off[r + 1];
        if (a < 0) return fail(KP_EINVAL, "%s: row_off[%lld]=%lld is negative", fn, (long long)r, (long long)a);
        if (b < a) return fail(KP_EINVAL, "%s: row_off[%lld]=%lld is below row_off[%lld]=%lld: offsets must not decrease", fn, (long long)(r + 1), (long long)b,
                               (long long)r, (long long)a);
        if (b > nnz) return fail(KP_EINVAL, "%s: row_off[%lld]=%lld is above nnz=%lld", fn, (long long)(r + 1), (long long)b, (long long)nnz);
        if (b - a > V) return fail(KP_EINVAL, "%s: row_off[%lld]: row %lld holds %lld entries, more than V=%d", fn, (long long)(r + 1), (long long)r, (long long)(b - a), V);
        any_entry |= b > a;
    }
    if (any_entry && (!terms || !weights)) return fail(KP_EINVAL, "%s: terms / weights is null", fn);
    if (npairs > 0 && !out) return fail(KP_EINVAL, "%s: out is null", fn);
    KP_TRY(check_aligned(fn, "terms", terms, 4));
    KP_TRY(check_aligned(fn, "weights", weights, 2));
    KP_TRY(check_aligned(fn, "out", out, 4));
    if (npairs == 0) return 0;

    std::lock_guard<std::mutex> lock(g_mutex);
    DeviceGuard guard;
    KP_TRY(select_device(device));
    hipStream_t st = static_cast<hipStream_t>(stream);
    // staging: q_off | q_term (padded to 8 bytes) | q_w (padded to 8 bytes) | one slice of pair records
    const long long bound = staged_bound();
    const long long slice = npairs < bound ? npairs : bound;
    const size_t b_qoff = (size_t)(nq + 1) * 8, b_term = ((size_t)qnnz * 4 + 7) / 8 * 8, b_w = b_term;
    const size_t b_query = b_qoff + b_term + b_w, bytes = b_query + (size_t)slice * sizeof(PairRec);
    Workspace* w = nullptr;
    KP_TRY(acquire(device, bytes, &w));
    char* h = static_cast<char*>(w->host);
    std::memcpy(h, q_off, b_qoff);
    if (qnnz) {
        std::memcpy(h + b_qoff, q_term, (size_t)qnnz * 4);
        std::memcpy(h + b_qoff + b_term, q_w, (size_t)qnnz * 4);
    }
    char* d = static_cast<char*>(w->dev);
    const long long* d_q_off = reinterpret_cast<const long long*>(d);
    const int* d_term = reinterpret_cast<const int*>(d + b_qoff);
    const float* d_w = reinterpret_cast<const float*>(d + b_qoff + b_term);
    const PairRec* d_rec = reinterpret_cast<const PairRec*>(d + b_query);
    PairRec* h_rec = reinterpret_cast<PairRec*>(h + b_query);
    for (long long p0 = 0; p0 < npairs; p0 += slice) {
        const long long n = npairs - p0 < slice ? npairs - p0 : slice;
        for (long long i = 0; i < n; ++i) {
            const int64_t r = pair_row[p0 + i];
            h_rec[i].start = row_off[r];
            h_rec[i].len = (int)(row_off[r + 1] - row_off[r]);
            h_rec[i].q = (int)pair_q[p0 + i];
        }
        // the first slice carries the query CSR with it; the later ones only their records
        const size_t from = p0 == 0 ? 0 : b_query;
        KP_HIP(hipMemcpyAsync(d + from, h + from, b_query - from + (size_t)n * sizeof(PairRec), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pair_dot, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, reinterpret_cast<const int*>(terms),
                           reinterpret_cast<const unsigned short*>(weights), (long long)nnz, d_q_off, nq, (long long)qnnz, d_term, d_w, d_rec, (int)n, out + p0);
        KP_HIP(hipGetLastError());
        KP_HIP(hipStreamSynchronize(st));      // the pinned records are rewritten by the next slice
    }
    return 0;
}

}  // extern "C"
