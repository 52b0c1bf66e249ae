// Test-only probe of the 128-wide attention kernel (kirag_amd/csrc/encoder_attn.hpp: k_attn_wide) on operands the test controls, in the manner of attn_probe.hip
// next to it: no model, no weights, every key decisive at any length (tests/attn_probe_util.py builds the data, tests/test_gpu_attn_wide.py runs it).  Not part
// of libkirag_amd.so: kirag_amd/csrc/Makefile builds this file once per operand type into tests/capi/libattn_probe_wide_{bf16,f16}.so.
//
// One C entry point per type, kr_attn_probe_wide_bf16 / _f16(const AttnProbeArgs*), with attn_probe.hip's argument structure and array layout: q / ctx
// [capT, H], k [capT + 64, ldk], vT [ldk, capT + 64], col [capT + 64], H = heads x 128, ldk = kv_heads x 128.  `kernel` is the heads per block (1 / 2 / 4),
// `mode` 0 plain, 2 window, 3 causal (the bias table, mode 1, is not built at this width).  The launch is the library's launch_attn_wide.  Every argument set
// under which the kernel could read or write outside the caller's arrays, or ask for more LDS than a CU has, is refused (return value < 0, message through
// kr_attn_probe_wide_error), so a wrong test cannot fault the GPU.
#include "../../kirag_amd/csrc/encoder_attn.hpp"

#include <cstring>
#include <vector>

namespace kr {
std::string& last_error_ref() { static thread_local std::string e; return e; }
int fail(int code, const char*, ...) { return code; }
int select_device(int) { return 0; }
bool is_device_pointer(const void*) { return true; }
std::atomic<int> g_force_exact{0};
}
using namespace kr::KR_ENC_NS;

extern "C" {
struct AttnProbeArgs {        // attn_probe.hip's
    const uint16_t* q; const uint16_t* k; const uint16_t* vT; uint16_t* ctx;
    const int* seq_off; const int* seq_nk; const int* seq_nq; const int* col; const float* tab;
    int64_t capT;
    int nseq, H, ldk, heads, kv_heads, dh;
    int mode;                 // 0 plain, 2 window (wl, wr), 3 causal = window (wl = max_pos, 0)
    int width, wl, wr, gather;
    int kernel;               // 1 / 2 / 4: heads per block
    int cap;                  // the batch width rounded up to 32 (kchunk = min(cap, 128))
};
}

static thread_local char g_err[256];
static int refuse(const char* fmt, long long a = 0, long long b = 0, long long c = 0) { snprintf(g_err, sizeof g_err, fmt, a, b, c); return -1; }
#define PR_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(g_err, sizeof g_err, "HIP error %s at line %d", hipGetErrorString(e_), __LINE__); rc = -2; goto done; } } while (0)

template <class T>
static hipError_t upload(std::vector<void*>& bufs, T** d, const T* h, size_t n) {
    *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), n ? n * sizeof(T) : 1);
    if (e != hipSuccess) return e;
    bufs.push_back(*d);
    return n ? hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
}

// every read and write of the kernel stays inside the caller's arrays
static int check_args(const AttnProbeArgs& a) {
    if (a.dh != 128) return refuse("head width %lld: this probe launches the 128-wide kernel", a.dh);
    if (a.heads < 1 || a.heads >= 1024 || a.H != a.heads * a.dh) return refuse("H %lld != heads %lld x dh", a.H, a.heads);
    if (a.kv_heads < 1 || a.heads % a.kv_heads != 0 || a.heads / a.kv_heads > 64 || a.ldk != a.kv_heads * a.dh) return refuse("kv_heads %lld / ldk %lld", a.kv_heads, a.ldk);
    if (a.capT < 1 || a.capT + 64 > ((int64_t)1 << 24) || a.nseq < 1 || a.nseq > 65535) return refuse("capT %lld, nseq %lld", a.capT, a.nseq);
    if (a.mode != 0 && a.mode != 2 && a.mode != 3) return refuse("mode %lld: plain (0), window (2) and causal (3) are built at this width", a.mode);
    if (a.kernel != 1 && a.kernel != 2 && a.kernel != 4) return refuse("kernel %lld: 1, 2 or 4 heads per block", a.kernel);
    if (a.cap < 32 || a.cap % 32 != 0) return refuse("cap %lld", a.cap);
    if (attn_wide_lds(a.kernel, a.cap < 128 ? a.cap : 128) > 160 * 1024) return refuse("%lld heads per block at cap %lld: more LDS than a CU has", a.kernel, a.cap);
    if (a.mode >= 2 && (a.wl < 0 || a.wr < 0 || (int64_t)a.wl + a.wr < 1)) return refuse("window (%lld, %lld)", a.wl, a.wr);
    if (a.mode != 0 && !a.col) return refuse("mode %lld needs col", a.mode);
    for (int b = 0; b < a.nseq; ++b) {
        const int64_t off = a.seq_off[b], nk = a.seq_nk[b], nq = a.seq_nq[b];
        if (off < 0 || off % 4 != 0 || nk < 0 || (nq != nk && nq != nk + 1) || off + nq > a.capT) return refuse("sequence %lld: off %lld, nk %lld", b, off, nk);
        if (a.mode == 3 && nq != nk) return refuse("sequence %lld: a causal handle packs no query-only row", b);
        if (a.mode != 0)
            for (int64_t i = 0; i < nq; ++i) {
                const int c = a.col[off + i];
                if (c < 0 || c > (1 << 20)) return refuse("col[%lld] = %lld", off + i, c);
                if (i > 0 && i < nk && c <= a.col[off + i - 1]) return refuse("col[%lld]: the attended columns increase", off + i);
            }
    }
    return 0;
}

template <class BA>
static hipError_t run_kernel(const AttnProbeArgs& a, const AttnOperands& ops, int nqt, int device, const BA& ba) {
    int rc = 0;
    switch (a.kernel) {
        case 1: rc = launch_attn_wide<1>(ops, a.cap, nqt, ba, device, 0); break;
        case 2: rc = launch_attn_wide<2>(ops, a.cap, nqt, ba, device, 0); break;
        default: rc = launch_attn_wide<4>(ops, a.cap, nqt, ba, device, 0); break;
    }
    const hipError_t e = hipGetLastError();
    return e != hipSuccess || rc == 0 ? e : hipErrorInvalidValue;
}

#ifdef KR_ENC_BUILD_F16
#define KR_ATTN_PROBE kr_attn_probe_wide_f16
#else
#define KR_ATTN_PROBE kr_attn_probe_wide_bf16
#endif

extern "C" __attribute__((visibility("default"))) const char* kr_attn_probe_wide_error() { return g_err; }

extern "C" __attribute__((visibility("default"))) int KR_ATTN_PROBE(const AttnProbeArgs* pa) {
    const AttnProbeArgs& a = *pa;
    g_err[0] = 0;
    if (check_args(a) != 0) return -1;
    const int64_t capT = a.capT, ldv = capT + 64;      // ensure_ws: 64 rows behind K, 64 columns behind V^T, 64 entries behind col
    int nq_max = 0;
    for (int b = 0; b < a.nseq; ++b) nq_max = a.seq_nq[b] > nq_max ? a.seq_nq[b] : nq_max;
    const int nqt = (nq_max + 31) / 32;
    std::vector<void*> bufs;
    uint16_t *q = nullptr, *k = nullptr, *vT = nullptr, *ctx = nullptr; int *off = nullptr, *nk = nullptr, *nq = nullptr, *col = nullptr;
    int rc = 0;
    PR_HIP(upload(bufs, &q, a.q, (size_t)capT * a.H));
    PR_HIP(upload(bufs, &k, a.k, (size_t)(capT + 64) * a.ldk));
    PR_HIP(upload(bufs, &vT, a.vT, (size_t)a.ldk * ldv));
    PR_HIP(upload(bufs, &ctx, a.ctx, (size_t)capT * a.H));
    PR_HIP(upload(bufs, &off, a.seq_off, (size_t)a.nseq)); PR_HIP(upload(bufs, &nk, a.seq_nk, (size_t)a.nseq)); PR_HIP(upload(bufs, &nq, a.seq_nq, (size_t)a.nseq));
    if (a.mode != 0) PR_HIP(upload(bufs, &col, a.col, (size_t)(capT + 64)));
    if (nqt > 0) {
        int device = 0;
        PR_HIP(hipGetDevice(&device));
        const AttnOperands ops{q, k, vT, ldv, off, nk, nq, ctx, a.H, a.heads, a.ldk, capT, a.nseq};
        if (a.mode == 0) PR_HIP(run_kernel(a, ops, nqt, device, AttnNoBiasArgs{}));
        else PR_HIP(run_kernel(a, ops, nqt, device, AttnWinArgs{col, a.wl, a.wr, a.gather ? 1 : 0}));
    }
    PR_HIP(hipDeviceSynchronize());
    PR_HIP(hipMemcpy(a.ctx, ctx, (size_t)capT * a.H * 2, hipMemcpyDeviceToHost));
done:
    for (void* p : bufs) (void)hipFree(p);
    return rc;
}
