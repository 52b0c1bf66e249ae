// Test-only probe of the projection kernels (kirag_amd/csrc/encoder_proj.hpp: k_proj<ShapeBig>, k_proj<ShapeSmall>, k_proj_split, k_proj_skinny over the main loops
// of gemm_nt.hpp) on operands the test controls: no model, no loader, so every epilogue runs on every main loop, on any grid, at any K (tests/proj_probe_util.py,
// tests/test_gpu_proj_probe.py).  Not part of libkirag_amd.so: kirag_amd/csrc/Makefile builds this file once per operand type (bf16: as is; f16:
// -DKR_ENC_BUILD_F16) into tests/capi/libproj_probe_{bf16,f16}.so, a sibling of attn_probe.hip.
//
// One C entry point per type, kr_proj_probe_bf16 / kr_proj_probe_f16(const ProjProbeArgs*): host arrays in, ONE kernel launch, outputs copied back.  W and bias
// arrive in the packed row order the loader gives them (tile_pair_row).  The probe allocates every output with guards around it, fills ALL of it with the
// caller's sentinel and copies ALL of it back:
//   out0 [256 + capT + 256, w0]   w0 = F (dense / GELU / ReLU), F / 2 (gated), H (the QKV epilogues)
//   out1 [256 + capT + 256, A]    k of the QKV epilogues
//   outT [32 + A + 32, 256 + ldT + 256]   V^T; the kernel's pitch is ldT + 512
//   smax [1 + nseq + 1, V]        EPI_SPLADE: the guard rows hold the 32-bit sentinel (sentinel << 16 | sentinel), the nseq rows start at zero
// The entry point refuses every argument set under which a kernel could read or write outside these arrays (return value -1, message through
// kr_proj_probe_error), so a wrong test cannot fault the GPU.  A HIP error returns -2.
//
// The launch itself (grid, block size, LDS bytes and attribute, the skinny rings, the instantiation an epilogue has on a loop) is the library's:
// launch_proj_loop of encoder_proj.hpp, the one every projection of a forward goes through, called with the caller's `loop`, `blocks`, `nt` and `ant`, ldx = K
// and ldo = F or F / 2.  `loop` means what KIRAG_AMD_PROJ_TILE means: 256 ping-pong, 128 streaming, 130 producer / consumer, 64 / 32 skinny.
#include "../../kirag_amd/csrc/encoder_proj.hpp"

#include <cstring>
#include <vector>

namespace kr {
std::string& last_error_ref() { static thread_local std::string e; return e; }
int fail(int code, const char*, ...) { return code; }
int select_device(int) { return 0; }
bool is_device_pointer(const void*) { return true; }
std::atomic<int> g_force_exact{0};
}
using namespace kr;
using namespace kr::KR_ENC_NS;

extern "C" {
struct ProjProbeArgs {
    const uint16_t* X;        // [capT, K]
    const uint16_t* W;        // [F, K], packed row order
    const float* bias;        // [F], packed row order (read by EPI_QKV, EPI_GELU, EPI_GEGLU, EPI_QKV_ROTB, EPI_SPLADE)
    uint16_t* out0;           // out: [capT + 512, w0]
    uint16_t* out1;           // out: [capT + 512, A] (QKV epilogues)
    uint16_t* outT;           // out: [A + 64, ldT + 512] (QKV epilogues)
    const float* rot_cos;     // [max_pos, dh / 2] (rotating epilogues)
    const float* rot_sin;
    const int* tpos;          // [capT] (rotating epilogues); any value: the kernel maps what is out of range to row 0
    const int* row_seq;       // [capT] (EPI_SPLADE): < nseq, negative = no sequence
    uint32_t* smax;           // out: [nseq + 2, V] (EPI_SPLADE)
    int64_t capT, ldT;
    int T, F, K, H, A, max_pos, dh, nseq, V;
    int epi, loop, blocks, nt, ant, epi_prio, pw;
    int sentinel;             // 16-bit pattern
};
}

constexpr int GUARD_ROWS = 256, GUARD_T_ROWS = 32, GUARD_T_COLS = 256;

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
// n 16-bit elements, all the sentinel
static hipError_t guarded(std::vector<void*>& bufs, uint16_t** d, size_t n, int sentinel) {
    *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), n * 2);
    if (e != hipSuccess) return e;
    bufs.push_back(*d);
    return hipMemsetD16(reinterpret_cast<hipDeviceptr_t>(*d), (unsigned short)sentinel, n);
}

static bool is_qkv(int epi) { return epi == EPI_QKV || epi_rotates(epi); }
static int out0_width(const ProjProbeArgs& a) { return is_qkv(a.epi) ? a.H : epi_gated(a.epi) ? a.F / 2 : a.F; }

// every read and write of every kernel stays inside the arrays above:
//   X rows are read below T (T >= 1) and W rows below F, K columns in whole 64-column tiles: the streaming, producer / consumer and skinny loops clamp a row
//   past the end to the last one, the ping-pong loop reads through a buffer resource that ends with the operand (rows past it arrive as zeros)
//   rows are written up to round_up(T, tile) <= capT (capT % 256 == 0), only for 64-feature groups below F (F % 64 == 0)
//   q | k | V^T regions are whole multiples of 64 features; V^T columns reach round_up(T, tile) <= capT <= ldT
//   the rotary tables are read at row p (dh / 2) for 0 <= p < max_pos, entries 0 .. dh / 2 - 1; tpos at rows < capT
//   row_seq at rows < capT, smax at (row_seq, f < V), bias at f < F
static int check_args(const ProjProbeArgs& a) {
    if (a.epi < 0 || a.epi > EPI_SPLADE) return refuse("epilogue %lld", a.epi);
    if (a.loop != 256 && a.loop != 128 && a.loop != 130 && a.loop != 64 && a.loop != 32) return refuse("loop %lld", a.loop);
    if (a.capT < 256 || a.capT % 256 != 0 || a.capT > (1 << 20) || a.T < 1 || a.T > a.capT) return refuse("T %lld, capT %lld", a.T, a.capT);
    if (a.K < 64 || a.K % 64 != 0 || a.K > (1 << 16)) return refuse("K %lld", a.K);
    if (a.F < 64 || a.F % 64 != 0 || a.F > (1 << 16)) return refuse("F %lld", a.F);
    if (!a.X || !a.W || !a.bias || !a.out0) return refuse("X, W, bias and out0 are needed");
    if ((a.sentinel & ~0xffff) != 0) return refuse("sentinel %lld", a.sentinel);
    if (is_qkv(a.epi)) {
        if (a.H < 64 || a.H % 64 != 0 || a.A < 64 || a.A % 64 != 0 || (int64_t)a.H + 2 * (int64_t)a.A != a.F) return refuse("F %lld != H %lld + 2 A %lld", a.F, a.H, a.A);
        if (a.epi == EPI_QKV && a.A != a.H) return refuse("EPI_QKV splits F into thirds: A %lld != H %lld", a.A, a.H);
        if (a.ldT < a.capT || a.ldT % 8 != 0 || a.ldT > (1 << 21)) return refuse("ldT %lld for capT %lld", a.ldT, a.capT);
        if (!a.out1 || !a.outT) return refuse("out1 and outT are needed");
    }
    if (epi_rotates(a.epi)) {
        if (a.dh != 32 && a.dh != 64) return refuse("head width %lld", a.dh);
        if (a.max_pos < 1 || a.max_pos > (1 << 20) || !a.rot_cos || !a.rot_sin || !a.tpos) return refuse("rotary tables of %lld rows", a.max_pos);
    }
    if (a.epi == EPI_SPLADE) {
        if (a.nseq < 1 || a.nseq > 65535 || a.V < 1 || a.V > a.F || !a.row_seq || !a.smax) return refuse("nseq %lld, V %lld, F %lld", a.nseq, a.V, a.F);
        for (int64_t t = 0; t < a.capT; ++t)
            if (a.row_seq[t] >= a.nseq) return refuse("row_seq[%lld] = %lld", t, a.row_seq[t]);
        if (a.nt) return refuse("EPI_SPLADE has no non-temporal stores");
    }
    if (a.epi == EPI_QKV_ROTB && a.loop == 256) return refuse("EPI_QKV_ROTB is not built for the 256 x 256 tile");
    const bool persistent = a.loop == 256 || a.loop == 128 || a.loop == 130;
    if (a.blocks != 0 && (!persistent || a.blocks < 8 || a.blocks % 8 != 0 || a.blocks > 4096)) return refuse("blocks %lld on loop %lld", a.blocks, a.loop);
    if ((a.nt != 0 && a.nt != 1) || (a.nt && a.loop != 256 && a.loop != 128)) return refuse("nt %lld on loop %lld", a.nt, a.loop);
    if ((a.ant != 0 && a.ant != 1) || (a.ant && (a.loop != 256 || a.epi != EPI_DENSE))) return refuse("ant %lld on loop %lld, epilogue %lld", a.ant, a.loop, a.epi);
    if (a.epi_prio < 0 || a.epi_prio > 2) return refuse("epi_prio %lld", a.epi_prio);
    if (a.pw < 1 || a.pw > 64) return refuse("pw %lld", a.pw);
    if (!persistent) {
        const int tile = a.loop;      // the token-tile limit of the skinny grid (gridDim.y)
        if ((a.T + tile - 1) / tile > 65535) return refuse("%lld token tiles of %lld", (a.T + tile - 1) / tile, tile);
    }
    return 0;
}

#ifdef KR_ENC_BUILD_F16
#define KR_PROJ_PROBE kr_proj_probe_f16
#else
#define KR_PROJ_PROBE kr_proj_probe_bf16
#endif

extern "C" __attribute__((visibility("default"))) const char* kr_proj_probe_error() { return g_err; }

extern "C" __attribute__((visibility("default"))) int KR_PROJ_PROBE(const ProjProbeArgs* pa) {
    const ProjProbeArgs& a = *pa;
    g_err[0] = 0;
    if (check_args(a) != 0) return -1;
    const bool qkv = is_qkv(a.epi), rot = epi_rotates(a.epi), splade = a.epi == EPI_SPLADE;
    const size_t capT = (size_t)a.capT, rows = capT + 2 * GUARD_ROWS, w0 = (size_t)out0_width(a);
    const size_t pitchT = (size_t)a.ldT + 2 * GUARD_T_COLS, rowsT = (size_t)a.A + 2 * GUARD_T_ROWS;
    const uint32_t sent32 = ((uint32_t)a.sentinel << 16) | (uint32_t)a.sentinel;
    std::vector<void*> bufs;
    uint16_t *X = nullptr, *W = nullptr, *out0 = nullptr, *out1 = nullptr, *outT = nullptr;
    float *bias = nullptr, *rc_ = nullptr, *rs_ = nullptr;
    int *tpos = nullptr, *row_seq = nullptr, *Tp = nullptr;
    uint32_t* smax = nullptr;
    int rc = 0, dev = 0, num_cu = 0;
    ProjArgs p{};
    PR_HIP(hipGetDevice(&dev));
    PR_HIP(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    if (num_cu < 8 || num_cu % 8 != 0) return refuse("%lld compute units: the tile walk takes grids in multiples of 8", num_cu);
    PR_HIP(upload(bufs, &X, a.X, capT * a.K));
    PR_HIP(upload(bufs, &W, a.W, (size_t)a.F * a.K));
    PR_HIP(upload(bufs, &bias, a.bias, (size_t)a.F));
    PR_HIP(upload(bufs, &Tp, &a.T, (size_t)1));
    if (!splade) PR_HIP(guarded(bufs, &out0, rows * w0, a.sentinel));
    if (qkv) {
        PR_HIP(guarded(bufs, &out1, rows * a.A, a.sentinel));
        PR_HIP(guarded(bufs, &outT, rowsT * pitchT, a.sentinel));
    }
    if (rot) {
        PR_HIP(upload(bufs, &rc_, a.rot_cos, (size_t)a.max_pos * (a.dh / 2)));
        PR_HIP(upload(bufs, &rs_, a.rot_sin, (size_t)a.max_pos * (a.dh / 2)));
        PR_HIP(upload(bufs, &tpos, a.tpos, capT));
    }
    if (splade) {
        std::vector<uint32_t> init((size_t)(a.nseq + 2) * a.V, 0u);
        for (int v = 0; v < a.V; ++v) init[(size_t)v] = init[(size_t)(a.nseq + 1) * a.V + v] = sent32;
        PR_HIP(upload(bufs, &smax, init.data(), init.size()));
        PR_HIP(upload(bufs, &row_seq, a.row_seq, capT));
    }
    // ProjArgs as launch_proj completes them (encoder_proj.hpp): ldx = K, ldo = the width of out0
    p.W = W; p.X = X; p.Tp = Tp; p.F = a.F; p.K = a.K; p.H = a.H; p.A = a.A; p.bias = bias;
    p.out0 = splade ? nullptr : out0 + GUARD_ROWS * w0;
    p.out1 = qkv ? out1 + (size_t)GUARD_ROWS * a.A : nullptr;
    p.outT = qkv ? outT + GUARD_T_ROWS * pitchT + GUARD_T_COLS : nullptr;
    p.ldT = (int64_t)pitchT; p.ldx = a.K; p.ldo = (int64_t)w0;
    p.pw = a.pw; p.epi_prio = a.epi_prio; p.ant = a.ant; p.nt = a.nt;
    p.rot_cos = rc_; p.rot_sin = rs_; p.tpos = tpos; p.max_pos = a.max_pos; p.dh = a.dh;
    p.row_seq = row_seq; p.smax = splade ? smax + a.V : nullptr; p.V = a.V;
    {   // the library's launcher on the caller's loop.  blocks = 0: the persistent grid of a forward, one block per CU, two on the streaming loop.  A launcher
        // that fails without a HIP error has refused its arguments (check_args refuses them first)
        const int blocks = a.blocks ? a.blocks : a.loop == 128 ? 2 * num_cu : num_cu;
        const int lrc = launch_proj_loop(a.epi, p, a.loop, blocks, a.T, dev, 0);
        const hipError_t le = hipGetLastError();
        PR_HIP(le != hipSuccess || lrc == 0 ? le : hipErrorInvalidValue);
    }
    PR_HIP(hipDeviceSynchronize());
    if (!splade) PR_HIP(hipMemcpy(a.out0, out0, rows * w0 * 2, hipMemcpyDeviceToHost));
    if (qkv) {
        PR_HIP(hipMemcpy(a.out1, out1, rows * a.A * 2, hipMemcpyDeviceToHost));
        PR_HIP(hipMemcpy(a.outT, outT, rowsT * pitchT * 2, hipMemcpyDeviceToHost));
    }
    if (splade) PR_HIP(hipMemcpy(a.smax, smax, (size_t)(a.nseq + 2) * a.V * 4, hipMemcpyDeviceToHost));
done:
    for (void* q : bufs) (void)hipFree(q);
    return rc;
}
