// Test-only probe of the row kernels (kirag_amd/csrc/encoder_rows.hpp: k_embed_ln, k_embed_rms, k_ln16, k_ln16_pre, k_ln16_head, k_qk_norm_rope, k_rot_pos,
// k_gather_cls and with them the device side of the residual low-byte codec) on operands the test controls: no model, no loader, a handful of rows
// (tests/rows_probe_util.py, tests/test_gpu_rows_probe.py).  Not part of libkirag_amd.so: kirag_amd/csrc/Makefile builds this file once per operand type
// (bf16: as is; f16: -DKR_ENC_BUILD_F16) into tests/capi/librows_probe_{bf16,f16}.so, a sibling of proj_probe.hip.
//
// One C entry point per type, kr_rows_probe_bf16 / kr_rows_probe_f16(const RowsProbeArgs*): host arrays in, ONE kernel launch through the library's own
// launchers (launch_ln_post, launch_ln_pre, launch_ln_head, launch_embed_ln, launch_embed_rms, launch_qk_norm_rope, launch_rot_pos, launch_gather_cls),
// outputs copied back.  Every output array is allocated with GUARD rows in front and behind and capT rows between them, filled ENTIRELY with the sentinel
// (16-bit arrays: `sentinel`; byte arrays: its low byte; int arrays: sentinel << 16 | sentinel) and copied back entirely:
//   xb, rb_out [G + capT + G, H] 16-bit;  xlo, rlo_out the same shape in bytes;  q [G + capT + G, qw], k [G + capT + G, kw];  i0, i1, i2 [G + capT + G] ints;
//   err [3] ints: guard, the word (starts at 0), guard
// A kernel that works in place finds its T input rows inside the guarded array (the rows behind them stay the sentinel).
// The entry point refuses every argument set under which a kernel could read or write outside these arrays (return value -1, message through
// kr_rows_probe_error), so a wrong test cannot fault the GPU.  A HIP error returns -2.
#include "../../kirag_amd/csrc/encoder_rows.hpp"

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

enum { OP_LN_POST = 0, OP_LN_PRE = 1, OP_LN_HEAD = 2, OP_EMBED_LN = 3, OP_EMBED_RMS = 4, OP_QK_NORM_ROPE = 5, OP_ROT_POS = 6, OP_GATHER_CLS = 7 };
enum { ALIAS_RB_XB = 1, ALIAS_RB = 2, ALIAS_LO = 4 };      // k_ln16_pre: rb_in == xb, rb_in == rb_out, rlo_in == rlo_out; k_ln16: ALIAS_LO = xlo_in == xlo

extern "C" {
struct RowsProbeArgs {
    // inputs (host)
    const uint16_t* y;        // [capT, H]  the projection's rows (norms)
    const float* ybias;       // [H]        the projection's bias (k_ln16, k_ln16_pre)
    const float* g;           // [H] gamma; k_qk_norm_rope: gq [dh]
    const float* beta;        // [H]
    const uint16_t* rb_in;    // [capT, H]  the residual's 16-bit half (k_ln16: the rows xb holds before the launch; k_gather_cls: the source rows)
    const uint8_t* rlo_in;    // [capT, H]  its low bytes, or null
    const float* word;        // [n_word, H]
    const float* pos;         // [n_pos, H]
    const float* type;        // [n_type, H]
    const int* tok_id;        // [capT]
    const int* tok_pos;       // [capT]  k_embed_ln: position ids; k_qk_norm_rope: rotary positions (any value); k_rot_pos: columns
    const int* tok_type;      // [capT]
    const int* row_seq;       // [capT]  k_ln16_head
    const uint16_t* q_in;     // [capT, qw]  k_qk_norm_rope: q; k_gather_cls: ctx
    const uint16_t* k_in;     // [capT, kw]
    const float* gk;          // [dh]
    const float* rot_cos;     // [max_pos, dh / 2]
    const float* rot_sin;
    const int* seq_off;       // [nseq]
    const int* seq_a;         // [nseq]  k_rot_pos: seq_nq; k_gather_cls: seq_cls
    const int* seq_nk;        // [nseq]  k_gather_cls
    // outputs (host, guarded); null = the kernel gets a null pointer
    uint16_t* xb;             // norms, embeddings: xb; k_gather_cls: c_xb
    uint8_t* xlo;             // xlo; c_xlo
    uint16_t* rb_out;
    uint8_t* rlo_out;
    uint16_t* q;              // q in place; c_ctx
    uint16_t* k;
    int* i0;                  // k_rot_pos: rpos; k_gather_cls: c_off
    int* i1;                  // c_nk
    int* i2;                  // c_cls
    int* err;                 // [3]: k_ln16_head: the error word; k_gather_cls: *d_B
    float eps, eps_k;         // eps_k: k_qk_norm_rope's second eps (eps = eps_q)
    int op, H, T, capT, grid, alias, rms, sentinel;
    int n_word, n_pos, n_type;
    int heads, kv_heads, dh, qw, kw, max_pos;
    int nseq, align, last_row;
};
}

constexpr int GUARD = 8;

static thread_local char g_err[256];
static int refuse(const char* fmt, long long a = 0, long long b = 0, long long c = 0) { snprintf(g_err, sizeof g_err, fmt, a, b, c); return -1; }
#define PR_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(g_err, sizeof g_err, "HIP error %s at line %d", hipGetErrorString(e_), __LINE__); rc = -2; goto done; } } while (0)

template <class T>
static hipError_t upload(std::vector<void*>& bufs, T** d, const T* h, size_t n) {
    *d = nullptr;
    if (!h) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), n ? n * sizeof(T) : 1);
    if (e != hipSuccess) return e;
    bufs.push_back(*d);
    return n ? hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
}
// n elements of 1, 2 or 4 bytes, all the sentinel; with `in`, `live` of them behind the front guard hold the caller's rows.  host == nullptr: no array
template <class T>
static hipError_t guarded(std::vector<void*>& bufs, T** d, const T* host, size_t n, int sentinel, const T* in = nullptr, size_t front = 0, size_t live = 0) {
    *d = nullptr;
    if (!host) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), n * sizeof(T));
    if (e != hipSuccess) return e;
    bufs.push_back(*d);
    if (sizeof(T) == 1) e = hipMemset(*d, sentinel & 0xff, n);
    else if (sizeof(T) == 2) e = hipMemsetD16(reinterpret_cast<hipDeviceptr_t>(*d), (unsigned short)sentinel, n);
    else e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(*d), (int)(((unsigned)sentinel << 16) | (unsigned)sentinel), n);
    if (e != hipSuccess || !in || !live) return e;
    return hipMemcpy(*d + front, in, live * sizeof(T), hipMemcpyHostToDevice);
}

static bool is_norm(int op) { return op == OP_LN_POST || op == OP_LN_PRE || op == OP_LN_HEAD; }

// every read and write of every kernel stays inside the arrays above:
//   the norms and the embeddings read and write rows below T <= capT, H columns in 8- or 4-element accesses (H % 128 == 0, H <= 2048: NS <= 4 steps of 512);
//     a grid-stride norm prefetches row t + step only where that is below T; table rows are read at the ids, which are checked against the tables
//   k_qk_norm_rope: (row, head) units below T (heads + kv_heads), dh columns each: q is qw = heads dh wide, k kw = kv_heads dh; the lane groups past the last
//     unit read unit 0 and store nothing; tpos at rows below T (and row 0), the tables at row p for 0 <= p < max_pos, else row 0
//   k_rot_pos: rows seq_off[b] .. seq_off[b] + round_up(seq_nq[b], align) of tok_pos and rpos
//   k_gather_cls: source row seq_off[b] + seq_cls[b] (last_row: + max(seq_nk[b] - 1, 0)) of ctx / xb / xlo, destination row b < nseq <= capT
static int check_args(const RowsProbeArgs& a) {
    if (a.op < 0 || a.op > OP_GATHER_CLS) return refuse("op %lld", a.op);
    if (a.capT < 1 || a.capT > (1 << 16) || a.T < 1 || a.T > a.capT) return refuse("T %lld, capT %lld", a.T, a.capT);
    if ((a.sentinel & ~0xffff) != 0) return refuse("sentinel %lld", a.sentinel);
    if (a.grid < 0) return refuse("grid %lld", a.grid);
    if (a.op != OP_QK_NORM_ROPE && a.op != OP_ROT_POS && (a.H < 128 || a.H % 128 != 0 || a.H > 2048)) return refuse("H %lld", a.H);
    if ((a.alias & ~7) != 0 || (a.alias && a.op != OP_LN_PRE && a.op != OP_LN_POST)) return refuse("alias %lld on op %lld", a.alias, a.op);
    if (is_norm(a.op)) {
        if (!a.y || !a.g || !a.beta || !a.xb) return refuse("y, g, beta and xb are needed");
        if (a.grid > a.T) return refuse("grid %lld above the %lld rows", a.grid, a.T);
        if (a.op != OP_LN_HEAD && (!a.ybias || !a.rb_in)) return refuse("ybias and rb_in are needed");
        if (a.op == OP_LN_HEAD && (!a.row_seq || !a.err)) return refuse("row_seq and err are needed");
        if (a.op == OP_LN_POST && (a.alias & ~ALIAS_LO)) return refuse("alias %lld: k_ln16 always reads its residual in xb", a.alias);
        if (a.op == OP_LN_POST && (a.alias & ALIAS_LO) && (!a.rlo_in || !a.xlo)) return refuse("xlo_in == xlo needs both");
        if (a.op == OP_LN_PRE) {
            if ((a.alias & ALIAS_RB_XB) && (a.alias & ALIAS_RB)) return refuse("rb_in cannot be xb and rb_out");
            if ((a.alias & ALIAS_RB) && !a.rb_out) return refuse("rb_in == rb_out needs rb_out");
            if ((a.alias & ALIAS_LO) && (!a.rlo_in || !a.rlo_out)) return refuse("rlo_in == rlo_out needs both");
            if (a.rlo_out && !a.rb_out) return refuse("rlo_out without rb_out is never written");
        }
    } else if (a.op == OP_EMBED_LN || a.op == OP_EMBED_RMS) {
        const bool ln = a.op == OP_EMBED_LN;
        if (!a.tok_id || !a.word || !a.g || !a.xb || a.n_word < 1) return refuse("tok_id, word, g and xb are needed");
        if (ln && (!a.tok_pos || !a.tok_type || !a.pos || !a.type || !a.beta || a.n_pos < 1 || a.n_type < 1)) return refuse("positions, types and beta are needed");
        if (!ln && !a.rb_out) return refuse("k_embed_rms stores the residual: rb_out is needed");
        for (int t = 0; t < a.T; ++t) {
            if (a.tok_id[t] < 0 || a.tok_id[t] >= a.n_word) return refuse("tok_id[%lld] = %lld of %lld", t, a.tok_id[t], a.n_word);
            if (ln && (a.tok_pos[t] < 0 || a.tok_pos[t] >= a.n_pos)) return refuse("tok_pos[%lld] = %lld of %lld", t, a.tok_pos[t], a.n_pos);
            if (ln && (a.tok_type[t] < 0 || a.tok_type[t] >= a.n_type)) return refuse("tok_type[%lld] = %lld of %lld", t, a.tok_type[t], a.n_type);
        }
        if (a.grid && (a.grid < (int)row_grid(a.T) || a.grid > (int)row_grid(a.capT))) return refuse("grid %lld for %lld rows", a.grid, a.T);
    } else if (a.op == OP_QK_NORM_ROPE) {
        if (a.dh != 32 && a.dh != 64 && a.dh != 128) return refuse("head width %lld", a.dh);
        if (a.heads < 1 || a.heads > 128 || a.kv_heads < 1 || a.heads % a.kv_heads != 0) return refuse("heads %lld, kv_heads %lld", a.heads, a.kv_heads);
        if (a.qw != a.heads * a.dh || a.kw != a.kv_heads * a.dh) return refuse("q / k width %lld / %lld for head width %lld", a.qw, a.kw, a.dh);
        if (a.max_pos < 1 || a.max_pos > (1 << 20) || !a.rot_cos || !a.rot_sin || !a.tok_pos) return refuse("rotary tables of %lld rows", a.max_pos);
        if (!a.q_in || !a.k_in || !a.q || !a.k || !a.g || !a.gk) return refuse("q, k and their norm weights are needed");
        const int lo = (int)qk_norm_grid(a.T, a.heads, a.kv_heads, a.dh), hi = (int)qk_norm_grid(a.capT, a.heads, a.kv_heads, a.dh);
        if (a.grid && (a.grid < lo || a.grid > hi)) return refuse("grid %lld for %lld rows", a.grid, a.T);
    } else if (a.op == OP_ROT_POS) {
        if (a.align != 4 && a.align != 8) return refuse("align %lld", a.align);
        if (a.nseq < 1 || a.nseq > 4096 || !a.seq_off || !a.seq_a || !a.tok_pos || !a.i0 || a.grid) return refuse("%lld sequences, their tables and rpos are needed", a.nseq);
        for (int b = 0; b < a.nseq; ++b) {
            const int64_t n = a.seq_a[b], padded = (n + a.align - 1) & ~(int64_t)(a.align - 1);
            if (a.seq_off[b] < 0 || n < 0 || n > a.capT || a.seq_off[b] + padded > a.capT) return refuse("sequence %lld: offset %lld, %lld rows", b, a.seq_off[b], n);
        }
    } else {
        if (a.nseq < 1 || a.nseq != a.T || a.grid) return refuse("%lld sequences for %lld gathered rows", a.nseq, a.T);
        if (a.qw < 8 || a.qw % 8 != 0 || a.qw > 8192) return refuse("Dq %lld", a.qw);
        if (!a.q_in || !a.rb_in || !a.seq_off || !a.seq_a || !a.seq_nk || !a.q || !a.xb || !a.i0 || !a.i1 || !a.i2 || !a.err) return refuse("ctx, xb, the tables and every output");
        if ((a.rlo_in != nullptr) != (a.xlo != nullptr)) return refuse("xlo and c_xlo go together");
        for (int b = 0; b < a.nseq; ++b) {
            const int64_t src = (int64_t)a.seq_off[b] + (a.last_row ? (a.seq_nk[b] > 0 ? a.seq_nk[b] - 1 : 0) : a.seq_a[b]);
            if (a.seq_off[b] < 0 || src < 0 || src >= a.capT) return refuse("sequence %lld gathers row %lld of %lld", b, src, a.capT);
        }
    }
    return 0;
}

#ifdef KR_ENC_BUILD_F16
#define KR_ROWS_PROBE kr_rows_probe_f16
#else
#define KR_ROWS_PROBE kr_rows_probe_bf16
#endif

extern "C" __attribute__((visibility("default"))) const char* kr_rows_probe_error() { return g_err; }

extern "C" __attribute__((visibility("default"))) int KR_ROWS_PROBE(const RowsProbeArgs* pa) {
    const RowsProbeArgs& a = *pa;
    g_err[0] = 0;
    if (check_args(a) != 0) return -1;
    const size_t capT = (size_t)a.capT, T = (size_t)a.T, H = (size_t)a.H, rows = capT + 2 * GUARD, front = (size_t)GUARD;
    const int S = a.sentinel;
    std::vector<void*> bufs;
    uint16_t *y = nullptr, *rb_in = nullptr, *q_in = nullptr, *xb = nullptr, *rb_out = nullptr, *q = nullptr, *k = nullptr;
    uint8_t *rlo_in = nullptr, *xlo = nullptr, *rlo_out = nullptr;
    float *ybias = nullptr, *g = nullptr, *beta = nullptr, *word = nullptr, *pos = nullptr, *type = nullptr, *gk = nullptr, *rc_ = nullptr, *rs_ = nullptr, *zero = nullptr;
    int *tok_id = nullptr, *tok_pos = nullptr, *tok_type = nullptr, *row_seq = nullptr, *seq_off = nullptr, *seq_a = nullptr, *seq_nk = nullptr, *Tp = nullptr;
    int *i0 = nullptr, *i1 = nullptr, *i2 = nullptr, *err = nullptr;
    int rc = 0, dev = 0, num_cu = 0;
    const int err_init[3] = {(int)(((unsigned)S << 16) | (unsigned)S), 0, (int)(((unsigned)S << 16) | (unsigned)S)};
    const std::vector<float> zeros(H, 0.f);
    PR_HIP(hipGetDevice(&dev));
    PR_HIP(hipDeviceGetAttribute(&num_cu, hipDeviceAttributeMultiprocessorCount, dev));
    PR_HIP(upload(bufs, &Tp, &a.T, (size_t)1));
    PR_HIP(upload(bufs, &err, a.err ? err_init : nullptr, (size_t)3));
    if (is_norm(a.op)) {
        const bool post = a.op == OP_LN_POST, pre = a.op == OP_LN_PRE;
        const bool in_xb = post || (pre && (a.alias & ALIAS_RB_XB));      // the residual's 16-bit half arrives inside xb
        const bool in_rb = pre && (a.alias & ALIAS_RB), lo_alias = (a.alias & ALIAS_LO) != 0;
        PR_HIP(upload(bufs, &y, a.y, capT * H));
        PR_HIP(upload(bufs, &ybias, a.ybias, H));
        PR_HIP(upload(bufs, &g, a.g, H));
        PR_HIP(upload(bufs, &beta, a.beta, H));
        PR_HIP(guarded(bufs, &xb, a.xb, rows * H, S, in_xb ? a.rb_in : nullptr, front * H, T * H));
        PR_HIP(guarded(bufs, &rb_out, a.rb_out, rows * H, S, in_rb ? a.rb_in : nullptr, front * H, T * H));
        PR_HIP(guarded(bufs, &xlo, a.xlo, rows * H, S, post && lo_alias ? a.rlo_in : nullptr, front * H, T * H));
        PR_HIP(guarded(bufs, &rlo_out, a.rlo_out, rows * H, S, pre && lo_alias ? a.rlo_in : nullptr, front * H, T * H));
        if (!in_xb && !in_rb) PR_HIP(upload(bufs, &rb_in, a.rb_in, capT * H));
        if (!lo_alias) PR_HIP(upload(bufs, &rlo_in, a.rlo_in, capT * H));
        uint16_t* xb0 = xb + front * H;
        uint8_t* xlo0 = xlo ? xlo + front * H : nullptr;
        uint16_t* rbo0 = rb_out ? rb_out + front * H : nullptr;
        uint8_t* rlo0 = rlo_out ? rlo_out + front * H : nullptr;
        const unsigned grid = a.grid ? (unsigned)a.grid : ln_grid(a.T, num_cu);
        if (post) launch_ln_post(y, ybias, Tp, g, beta, a.eps, a.H, lo_alias ? xlo0 : rlo_in, xlo0, xb0, grid, 0);
        else if (pre) launch_ln_pre(a.rms != 0, y, ybias, Tp, g, beta, a.eps, a.H, in_xb ? xb0 : in_rb ? rbo0 : rb_in, lo_alias ? rlo0 : rlo_in, rbo0, rlo0, xlo0, xb0, grid, 0);
        else {
            PR_HIP(upload(bufs, &zero, zeros.data(), H));
            PR_HIP(upload(bufs, &row_seq, a.row_seq, capT));
            launch_ln_head(y, zero, Tp, g, beta, a.eps, a.H, row_seq, xb0, err + 1, grid, 0);
        }
    } else if (a.op == OP_EMBED_LN || a.op == OP_EMBED_RMS) {
        const unsigned grid = a.grid ? (unsigned)a.grid : row_grid(a.T);
        PR_HIP(upload(bufs, &tok_id, a.tok_id, capT));
        PR_HIP(upload(bufs, &word, a.word, (size_t)a.n_word * H));
        PR_HIP(upload(bufs, &g, a.g, H));
        PR_HIP(guarded(bufs, &xb, a.xb, rows * H, S));
        if (a.op == OP_EMBED_LN) {
            PR_HIP(upload(bufs, &tok_pos, a.tok_pos, capT));
            PR_HIP(upload(bufs, &tok_type, a.tok_type, capT));
            PR_HIP(upload(bufs, &pos, a.pos, (size_t)a.n_pos * H));
            PR_HIP(upload(bufs, &type, a.type, (size_t)a.n_type * H));
            PR_HIP(upload(bufs, &beta, a.beta, H));
            PR_HIP(guarded(bufs, &xlo, a.xlo, rows * H, S));
            launch_embed_ln(tok_id, tok_pos, tok_type, Tp, word, pos, type, g, beta, a.eps, a.H, xlo ? xlo + front * H : nullptr, xb + front * H, grid, 0);
        } else {
            PR_HIP(guarded(bufs, &rb_out, a.rb_out, rows * H, S));
            PR_HIP(guarded(bufs, &rlo_out, a.rlo_out, rows * H, S));
            launch_embed_rms(tok_id, Tp, word, g, a.eps, a.H, rb_out + front * H, rlo_out ? rlo_out + front * H : nullptr, xb + front * H, grid, 0);
        }
    } else if (a.op == OP_QK_NORM_ROPE) {
        const size_t qw = (size_t)a.qw, kw = (size_t)a.kw, half = (size_t)a.dh / 2;
        PR_HIP(guarded(bufs, &q, a.q, rows * qw, S, a.q_in, front * qw, T * qw));
        PR_HIP(guarded(bufs, &k, a.k, rows * kw, S, a.k_in, front * kw, T * kw));
        PR_HIP(upload(bufs, &g, a.g, (size_t)a.dh));
        PR_HIP(upload(bufs, &gk, a.gk, (size_t)a.dh));
        PR_HIP(upload(bufs, &rc_, a.rot_cos, (size_t)a.max_pos * half));
        PR_HIP(upload(bufs, &rs_, a.rot_sin, (size_t)a.max_pos * half));
        PR_HIP(upload(bufs, &tok_pos, a.tok_pos, capT));
        const unsigned grid = a.grid ? (unsigned)a.grid : qk_norm_grid(a.T, a.heads, a.kv_heads, a.dh);
        launch_qk_norm_rope(a.dh, q + front * qw, k + front * kw, Tp, a.heads, a.kv_heads, g, gk, a.eps, a.eps_k, rc_, rs_, tok_pos, a.max_pos, grid, 0);
    } else if (a.op == OP_ROT_POS) {
        PR_HIP(upload(bufs, &seq_off, a.seq_off, (size_t)a.nseq));
        PR_HIP(upload(bufs, &seq_a, a.seq_a, (size_t)a.nseq));
        PR_HIP(upload(bufs, &tok_pos, a.tok_pos, capT));
        PR_HIP(guarded(bufs, &i0, a.i0, rows, S));
        launch_rot_pos(seq_off, seq_a, a.align, tok_pos, i0 + front, (unsigned)a.nseq, 0);
    } else {
        const size_t qw = (size_t)a.qw;
        PR_HIP(upload(bufs, &q_in, a.q_in, capT * qw));
        PR_HIP(upload(bufs, &rb_in, a.rb_in, capT * H));
        PR_HIP(upload(bufs, &rlo_in, a.rlo_in, capT * H));
        PR_HIP(upload(bufs, &seq_off, a.seq_off, (size_t)a.nseq));
        PR_HIP(upload(bufs, &seq_a, a.seq_a, (size_t)a.nseq));
        PR_HIP(upload(bufs, &seq_nk, a.seq_nk, (size_t)a.nseq));
        PR_HIP(guarded(bufs, &q, a.q, rows * qw, S));
        PR_HIP(guarded(bufs, &xb, a.xb, rows * H, S));
        PR_HIP(guarded(bufs, &xlo, a.xlo, rows * H, S));
        PR_HIP(guarded(bufs, &i0, a.i0, rows, S));
        PR_HIP(guarded(bufs, &i1, a.i1, rows, S));
        PR_HIP(guarded(bufs, &i2, a.i2, rows, S));
        launch_gather_cls(q_in, rb_in, rlo_in, seq_off, seq_a, seq_nk, a.H, q + front * qw, xb + front * H, xlo ? xlo + front * H : nullptr, i0 + front, i1 + front, i2 + front,
                          err + 1, a.last_row, a.qw, (unsigned)a.nseq, 0);
    }
    PR_HIP(hipGetLastError());
    PR_HIP(hipDeviceSynchronize());
    if (xb) PR_HIP(hipMemcpy(a.xb, xb, rows * H * 2, hipMemcpyDeviceToHost));
    if (xlo) PR_HIP(hipMemcpy(a.xlo, xlo, rows * H, hipMemcpyDeviceToHost));
    if (rb_out) PR_HIP(hipMemcpy(a.rb_out, rb_out, rows * H * 2, hipMemcpyDeviceToHost));
    if (rlo_out) PR_HIP(hipMemcpy(a.rlo_out, rlo_out, rows * H, hipMemcpyDeviceToHost));
    if (q) PR_HIP(hipMemcpy(a.q, q, rows * (size_t)a.qw * 2, hipMemcpyDeviceToHost));
    if (k) PR_HIP(hipMemcpy(a.k, k, rows * (size_t)a.kw * 2, hipMemcpyDeviceToHost));
    if (i0) PR_HIP(hipMemcpy(a.i0, i0, rows * 4, hipMemcpyDeviceToHost));
    if (i1) PR_HIP(hipMemcpy(a.i1, i1, rows * 4, hipMemcpyDeviceToHost));
    if (i2) PR_HIP(hipMemcpy(a.i2, i2, rows * 4, hipMemcpyDeviceToHost));
    if (err) PR_HIP(hipMemcpy(a.err, err, 3 * 4, hipMemcpyDeviceToHost));
done:
    for (void* p : bufs) (void)hipFree(p);
    return rc;
}
