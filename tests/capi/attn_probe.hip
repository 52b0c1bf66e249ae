// Test-only probe of the attention kernels (kirag_amd/csrc/encoder_attn.hpp: k_attn_lds, k_attn_dma) on operands the test controls: no model, no weights, so
// every key can be made decisive at any length (tests/attn_probe_util.py, tests/test_gpu_attn_probe.py).  Not part of libkirag_amd.so: kirag_amd/csrc/Makefile
// builds this file once per operand type (bf16: as is; f16: -DKR_ENC_BUILD_F16) into tests/capi/libattn_probe_{bf16,f16}.so, the way tools/attn_bench.hip
// includes the header from outside the library.
//
// One C entry point per type, kr_attn_probe_bf16 / kr_attn_probe_f16(const AttnProbeArgs*): host arrays in, one kernel launch, ctx copied back.
// The host arrays already carry the library's slack (ensure_ws in encoder.hip): q / ctx [capT, H], k [capT + 64, ldk], vT [ldk, capT + 64], col [capT + 64];
// the caller fills slack, alignment rows and ctx (a sentinel) as it likes.  The entry point refuses every argument set under which a kernel could read or write
// outside these arrays (return value < 0, message through kr_attn_probe_error), so a wrong test cannot fault the GPU.
//
// The launch itself (grid, kchunk, LDS bytes and attribute, attn_kv_mul) is the library's: launch_attn_lds / launch_attn_dma of encoder_attn.hpp, the ones the
// forward goes through, called with the caller's `kernel` and `cap`.  Sequence offsets are aligned to 4 tokens for k_attn_lds and to 8 for k_attn_dma.
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
struct AttnProbeArgs {
    const uint16_t* q;        // [capT, H]
    const uint16_t* k;        // [capT + 64, ldk]
    const uint16_t* vT;       // [ldk, capT + 64]
    uint16_t* ctx;            // [capT, H]: in = the sentinel, out = what the kernel left
    const int* seq_off;       // [nseq]
    const int* seq_nk;
    const int* seq_nq;
    const int* col;           // [capT + 64] (modes 1 - 3)
    const float* tab;         // [heads, width] (mode 1)
    int64_t capT;
    int nseq, H, ldk, heads, kv_heads, dh;
    int mode;                 // 0 plain, 1 bias table, 2 window (wl, wr), 3 causal = window (wl = max_pos, 0) as causal_args sets it
    int width, wl, wr, gather;
    int kernel;               // 0: k_attn_dma; 1 / 2 / 4: k_attn_lds with that many heads per block
    int cap;                  // k_attn_lds: the batch width rounded up to 32 (kchunk = min(cap, 128))
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

// every read and write of both kernels stays inside the caller's arrays
static int check_args(const AttnProbeArgs& a) {
    if (a.dh != 32 && a.dh != 64) return refuse("head width %lld", a.dh);
    if (a.heads < 1 || a.heads >= 1024 || a.H != a.heads * a.dh) return refuse("H %lld != heads %lld x dh", a.H, a.heads);
    if (a.kv_heads < 1 || a.heads % a.kv_heads != 0 || a.heads / a.kv_heads > 64 || a.ldk != a.kv_heads * a.dh) return refuse("kv_heads %lld / ldk %lld", a.kv_heads, a.ldk);
    if (a.capT < 1 || a.capT + 64 > ((int64_t)1 << 24) || a.nseq < 1 || a.nseq > 65535) return refuse("capT %lld, nseq %lld", a.capT, a.nseq);
    if (a.mode < 0 || a.mode > 3) return refuse("mode %lld", a.mode);
    if (a.kernel != 0 && a.kernel != 1 && a.kernel != 2 && a.kernel != 4) return refuse("kernel %lld", a.kernel);
    if (a.kernel != 0 && (a.cap < 32 || a.cap % 32 != 0)) return refuse("cap %lld", a.cap);
    if (a.mode >= 2 && (a.wl < 0 || a.wr < 0 || (int64_t)a.wl + a.wr < 1)) return refuse("window (%lld, %lld)", a.wl, a.wr);
    if (a.mode != 0 && !a.col) return refuse("mode %lld needs col", a.mode);
    const int align = a.kernel == 0 ? 8 : 4;
    int64_t maxcol = 0;
    for (int b = 0; b < a.nseq; ++b) {
        const int64_t off = a.seq_off[b], nk = a.seq_nk[b], nq = a.seq_nq[b];
        if (off < 0 || off % align != 0 || nk < 0 || (nq != nk && nq != nk + 1) || off + nq > a.capT) return refuse("sequence %lld: off %lld, nk %lld", b, off, nk);
        if (a.kernel == 0 && nq < 1) return refuse("sequence %lld: k_attn_dma needs a query", b);
        if (a.mode == 3 && nq != nk) return refuse("sequence %lld: a causal handle packs no query-only row", b);
        if (a.mode != 0)
            for (int64_t i = 0; i < nq; ++i) {
                const int c = a.col[off + i];
                if (c < 0 || c > (1 << 20)) return refuse("col[%lld] = %lld", off + i, c);
                if (c > maxcol) maxcol = c;
                if (i > 0 && i < nk && c <= a.col[off + i - 1]) return refuse("col[%lld]: the attended columns increase", off + i);
            }
    }
    if (a.mode == 1) {
        // entries width / 2 + d for every column difference, plus the 64 keys a masked tile reads past its sequence (build_bias_table)
        if (!a.tab || a.width < 2 || a.width % 2 != 0 || a.width / 2 < maxcol + 65) return refuse("bias table of width %lld for columns up to %lld", a.width, maxcol);
    }
    return 0;
}

// the library's launchers (encoder_attn.hpp) with the caller's kernel, heads per block and cap.  A launcher that fails without a HIP error has refused its
// arguments
template <int DH, class BA>
static hipError_t run_kernel(const AttnProbeArgs& a, const AttnOperands& ops, int nqt, int device, const BA& ba) {
    int rc = 0;
    switch (a.kernel) {
        case 0: rc = launch_attn_dma<DH>(ops, nqt, ba, 0); break;
        case 1: rc = launch_attn_lds<DH, 1>(ops, a.cap, nqt, ba, device, 0); break;
        case 2: rc = launch_attn_lds<DH, 2>(ops, a.cap, nqt, ba, device, 0); break;
        default: rc = launch_attn_lds<DH, 4>(ops, a.cap, nqt, ba, device, 0); break;
    }
    const hipError_t e = hipGetLastError();
    return e != hipSuccess || rc == 0 ? e : hipErrorInvalidValue;
}

template <int DH>
static hipError_t run_mode(const AttnProbeArgs& a, const AttnOperands& ops, int nqt, int device, const int* col, const float* tab) {
    if (a.mode == 0) return run_kernel<DH>(a, ops, nqt, device, AttnNoBiasArgs{});
    if (a.mode == 1) return run_kernel<DH>(a, ops, nqt, device, AttnBiasArgs{tab, col, a.width, a.gather ? 1 : 0});
    return run_kernel<DH>(a, ops, nqt, device, AttnWinArgs{col, a.wl, a.wr, a.gather ? 1 : 0});
}

#ifdef KR_ENC_BUILD_F16
#define KR_ATTN_PROBE kr_attn_probe_f16
#else
#define KR_ATTN_PROBE kr_attn_probe_bf16
#endif

extern "C" __attribute__((visibility("default"))) const char* kr_attn_probe_error() { return g_err; }

extern "C" __attribute__((visibility("default"))) int KR_ATTN_PROBE(const AttnProbeArgs* pa) {
    const AttnProbeArgs& a = *pa;
    g_err[0] = 0;
    if (check_args(a) != 0) return -1;
    const int64_t capT = a.capT, ldv = capT + 64;      // ensure_ws: 64 rows behind K, 64 columns behind V^T, 64 entries behind col
    int nq_max = 0;
    for (int b = 0; b < a.nseq; ++b) nq_max = a.seq_nq[b] > nq_max ? a.seq_nq[b] : nq_max;
    const int nqt = (nq_max + 31) / 32;                  // q-tiles of the longest sequence
    std::vector<void*> bufs;
    uint16_t *q = nullptr, *k = nullptr, *vT = nullptr, *ctx = nullptr; int *off = nullptr, *nk = nullptr, *nq = nullptr, *col = nullptr; float* tab = nullptr;
    int rc = 0;
    PR_HIP(upload(bufs, &q, a.q, (size_t)capT * a.H));
    PR_HIP(upload(bufs, &k, a.k, (size_t)(capT + 64) * a.ldk));
    PR_HIP(upload(bufs, &vT, a.vT, (size_t)a.ldk * ldv));
    PR_HIP(upload(bufs, &ctx, a.ctx, (size_t)capT * a.H));
    PR_HIP(upload(bufs, &off, a.seq_off, (size_t)a.nseq)); PR_HIP(upload(bufs, &nk, a.seq_nk, (size_t)a.nseq)); PR_HIP(upload(bufs, &nq, a.seq_nq, (size_t)a.nseq));
    if (a.mode != 0) PR_HIP(upload(bufs, &col, a.col, (size_t)(capT + 64)));
    if (a.mode == 1) PR_HIP(upload(bufs, &tab, a.tab, (size_t)a.heads * a.width));
    if (nqt > 0) {
        int device = 0;
        PR_HIP(hipGetDevice(&device));
        const AttnOperands ops{q, k, vT, ldv, off, nk, nq, ctx, a.H, a.heads, a.ldk, capT, a.nseq};
        if (a.dh == 64) PR_HIP(run_mode<64>(a, ops, nqt, device, col, tab));
        else PR_HIP(run_mode<32>(a, ops, nqt, device, col, tab));
    }
    PR_HIP(hipDeviceSynchronize());
    PR_HIP(hipMemcpy(a.ctx, ctx, (size_t)capT * a.H * 2, hipMemcpyDeviceToHost));
done:
    for (void* p : bufs) (void)hipFree(p);
    return rc;
}
