// Sentence-encoder forward on MI355X — replaces HF's <Model>.forward + pooling + F.normalize behind retriever/encoders.py.
//
// Layout.  The [B,S] batch is PACKED on the device: only positions with attention_mask != 0 become token rows (sequence b owns rows [off_b, off_b + nq_b),
// off_b % 4 == 0; absolute position ids are kept per token), so the projections run on sum(len) rows instead of B*S.  No host round trip: grids are sized for
// B*(S+4) rows and blocks beyond the device-side total exit.  Residual stream = xb, 16-bit (it is also the MFMA operand) + by default xlo, ONE byte per element
// holding the remainder in units of ulp(hi) / 256 (lo_encode).  Operand type (f16 default, bf16) and the low half are fixed per handle at creation
// (encoder_api.hip: kr_encoder_create_ex; why the defaults are what they are: DESIGN.md sections 2 and 4.2a).  MFMA operands 16-bit (xb, q, k, vT, ctx, h), fp32
// accumulation everywhere.
//
// Per layer (post-LN):  ONE GEMM [Wq/8|Wk|Wv] x -> q, k (row-major) and v TRANSPOSED [H, T] (so that attention reads V^T fragments contiguously); attention =
// one block per (sequence, head group) with K and V^T staged once in LDS, swapped QK^T so the softmax reductions are in-lane, P^T fed from the accumulator
// straight into the V^T.P^T MFMA;  Wo ctx + b + residual -> LayerNorm;  W1 x + b -> activation;  W2 h + b + residual -> LayerNorm.  Pre-LN families run the
// same five launches with k_ln16_pre: r += y + bias, store r, xb = the NEXT norm of r.  Pooling (masked mean or CLS) + L2 normalisation produce out[B,H] fp32;
// a head runs behind it.  Which epilogues, norms and heads a handle runs is its ModelPlan, fixed by what the loader saw before the first finalize (a setting
// such as "config.t5_feed_forward", a head tensor such as "dense.weight"): the families, heads and settings are described next to the tables that implement
// them (encoder_model.hpp).
//
// Files.  This one: the Encoder handle, the workspace, the forward as a sequence of steps, the entry points.  encoder_model.hpp: what a handle is and what a
// pool runs on it (host-only).  encoder_weights.hpp: creation, the loader, finalize.  Per operand type, device code and the launchers of its kernels, which know
// nothing of the handle (the test-only probes under tests/capi launch through the same ones): encoder_rows.hpp (residual-stream codec, embedding, LayerNorm,
// pooling; set_lds_once), encoder_proj.hpp (projections: launch_proj picks the main loop, launch_proj_loop launches on one), encoder_attn.hpp (attention:
// launch_attention), encoder_pos.hpp (DeBERTa's position scores).  encoder_pack.hip: the token-packing front end.
#include "encoder_rows.hpp"
#include "encoder_proj.hpp"
#include "encoder_attn.hpp"
#include "encoder_pos.hpp"
#include "encoder_pack.hpp"
#include "encoder_model.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace kr {
namespace KR_ENC_NS {

struct LayerW {
    uint16_t *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr;   // bf16 [out, in]
    float *bqkv = nullptr, *bo = nullptr, *bo_eff = nullptr, *b1 = nullptr, *b2 = nullptr;   // bo_eff = bo + Wo.bv
    float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr;
    // w1 is allocated by its first tensor: [FF, H] (intermediate.dense) or, gated, [2 FF, H] (NomicBert's gate_proj | up_proj, ModernBert's mlp.Wi: interleaved
    // per 32-row tile)
    bool gated = false;
    float* b1p = nullptr;   // ModernBert handles: the bias of the [2 FF, H] projection in its rows' order (zero unless mlp.Wi.bias was loaded)
    // DeBERTa handles: query_proj / key_proj as loaded (fp32 [H, H]); PQ / PK = their projections of the position table, [heads][TP][d_h] 16-bit (build_disent_tables)
    float *wq32 = nullptr, *wk32 = nullptr;
    uint16_t *pq16 = nullptr, *pk16 = nullptr;
    // handles with q / k norms (Qwen3): the norm weights [d_h] fp32, q's with the score scale log2(e) / sqrt(d_h); the scale the loader folded into W_q (k_qk_norm_rope)
    float *qng = nullptr, *kng = nullptr;
    float qfold = 1.f;
};

// A/B switches of the projection / attention launches, read from the environment ONCE per forward (enqueue_forward), not per launch: a forward is 96
// projection launches and a small batch is bound by the host's launch rate (tests change KIRAG_AMD_PROJ_TILE between forwards of one handle, so
// reading them at kr_encoder_create would be too early)
struct Knobs {
    int pw = 8;            // KIRAG_AMD_PATCH_W: feature tiles per XCD patch of the tile walk (profiles/r03)
    int epi_prio = 0;      // KIRAG_AMD_EPI_PRIO (proj_epilogue)
    int force_tile = 0;    // KIRAG_AMD_PROJ_TILE: 32 / 128 / 130 / 256 force a projection path (tests run every parity case through all of them)
    bool attn_lds = false; // KIRAG_AMD_ATTN_LDS: the register-staged attention kernel for long sequences too
    void read() {
        auto geti = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        pw = geti("KIRAG_AMD_PATCH_W", 8); if (pw < 1) pw = 8;
        epi_prio = geti("KIRAG_AMD_EPI_PRIO", 0);
        force_tile = geti("KIRAG_AMD_PROJ_TILE", 0);
        attn_lds = getenv("KIRAG_AMD_ATTN_LDS") != nullptr;
    }
};

using model::AM_PLAIN;
using model::AM_BIAS;
using model::AM_WIN;
using model::AM_DISENT;
using model::AM_CAUSAL;

struct Encoder {
    kr_bert_cfg cfg{};
    Knobs kn;
    int device = 0;
    // what the handle is (encoder_model.hpp): the settings and what was loaded, as the loader recorded them; the plan enc_finalize derived from both — the one
    // thing the workspace and the forward consult (valid while `ready`)
    model::Settings set;
    model::Loaded ld;
    model::ModelPlan plan;
    bool ready = false, finalized_once = false;
    float *word = nullptr, *pos = nullptr, *type = nullptr, *elng = nullptr, *elnb = nullptr;
    std::vector<LayerW> L;
    // every hipMalloc of the handle is recorded where it is made (dmalloc) and freed by walking its list: ws_bufs = the workspace (free_ws), own_bufs = what
    // lives as long as the handle (enc_destroy)
    std::vector<void**> ws_bufs, own_bufs;
    float* stage = nullptr; size_t stage_elems = 0;   // fp32 upload staging for enc_load_weight
    // the tensors of the heads, HEADS[head].t[i] at head_p[head][i]: fp32, or the 16-bit operand where the row says HALF
    void* head_p[model::HEAD_ALL][model::HEAD_MAX_TENSORS] = {};
    float* hf(int head, int i) const { return static_cast<float*>(head_p[head][i]); }
    uint16_t* hh(int head, int i) const { return static_cast<uint16_t*>(head_p[head][i]); }
    // the relative attention bias as loaded (host) and the table the attention kernels read (AttnBiasArgs), built by finalize
    std::vector<float> rel_w;
    float* bias_tab = nullptr; int bias_width = 0;
    // DeBERTa handles: the position table and its norm as loaded (host); the bucket of every column difference (device, [2 max_pos - 1]); the workspace of
    // k_pos_scores, [capT][heads][2][capW] fp32 (ensure_ws)
    std::vector<float> rel_emb, rel_lng, rel_lnb;
    int* deb_bucket = nullptr;
    float* pos_sc = nullptr; int capW = 0;
    bool bias_gather = false;  // KIRAG_AMD_ATTN_BIAS_GATHER=1 at kr_encoder_create: key columns always from tok_pos (the path of masks with holes), for tests
    // rotary handles: cos / sin [max_pos][d_h / 2] of the global and the local frequencies; zero_row: H zeros (the embedding's position row; k_ln16_head's bias)
    float *rot_cos = nullptr, *rot_sin = nullptr, *rot_cos_l = nullptr, *rot_sin_l = nullptr, *zero_row = nullptr;
    // workspace
    int64_t capT = 0; int capB = 0; int64_t capBS = 0; int64_t ldv = 0;
    int64_t *d_ids = nullptr, *d_mask = nullptr, *d_tt = nullptr;   // d_tt: token_type_ids of the batch (only written when the caller passes them)
    // ragged input (kr_encoder_forward_packed) lives in the same three buffers: the int32 token list, the int32 lengths, scratch for the input offsets
    int* rag_ids() const { return reinterpret_cast<int*>(d_ids); }
    int* rag_lens() const { return reinterpret_cast<int*>(d_mask); }
    int* rag_in_off() const { return reinterpret_cast<int*>(d_tt); }
    int *seq_off = nullptr, *seq_nk = nullptr, *seq_nq = nullptr, *seq_cls = nullptr, *seq_has0 = nullptr, *d_T = nullptr, *d_err = nullptr;
    // per token: id, column (k_embed_ln under BERT's position rule, the un-packer), type; tok_epos: the embedding position under fairseq's rule; tok_zero: zeros
    // (a rotary handle's embedding adds zero_row); tok_rpos: the position each token is rotated by (k_rot_pos)
    int *tok_id = nullptr, *tok_pos = nullptr, *tok_type = nullptr, *tok_epos = nullptr, *tok_zero = nullptr, *tok_rpos = nullptr;
    // with a head (ModelPlan::ws): pooled = k_pool's [B, H] rows, the head's input; cy = the colbert product of the packed rows [capT, P]; slot_row = packed row
    // of every [b, s] column or -1; row_seq = the sequence of every packed row or -1.  tok_stage: the token-level blocks / the SPLADE result of a forward whose
    // `out` is host memory (grown on demand, freed with the handle)
    float* pooled = nullptr; uint16_t* cy = nullptr; int *slot_row = nullptr, *row_seq = nullptr;
    float* tok_stage = nullptr; size_t tok_stage_elems = 0;
    uint16_t *rb = nullptr, *c_rb = nullptr;   // the pre-LN residual stream (and its CLS-row copy): 16-bit high half
    uint8_t *rlo = nullptr, *c_rlo = nullptr;  // ... and the low-half bytes (use_lo)
    float *out = nullptr;
    uint8_t *xlo = nullptr;    // low half of the residual stream, one byte per element (lo_encode): written by every LayerNorm with use_lo, else by the last one only
    bool use_lo = false;       // KIRAG_AMD_RESIDUAL_LO=1 at kr_encoder_create
    uint16_t *y = nullptr, *xb = nullptr, *q = nullptr, *k = nullptr, *vT = nullptr, *ctx = nullptr, *h = nullptr;
    int lastB = 0, lastS = 0;
    int* h_err = nullptr;            // pinned: copy of d_err taken at the end of the last asynchronous forward
    hipEvent_t ev_done = nullptr;    // recorded after that copy
    bool pending = false;            // an asynchronous forward's error word has not been looked at yet
    hipStream_t last_stream = nullptr;
    int num_cu = 256;         // CUs the persistent projection grids are sized for
    int num_cu_all = 256;     // CUs of the device (grids of the memory-bound kernels)
    struct GraphEntryT { uint64_t key; int calls; hipGraphExec_t exec; };
    std::vector<GraphEntryT> graphs;   // captured forwards of small batch shapes (run_forward)
    hipStream_t gstream = nullptr; hipEvent_t ev_in = nullptr, ev_out = nullptr;
    bool graphs_off = false;
    // CLS pooling: the LAST layer's attention output / FFN only matter for one row per sequence.  Those rows are gathered into compact [B, ...] buffers
    // after the last attention and the rest of the layer runs on B rows instead of T (KIRAG_AMD_CLS_FULL=1 at kr_encoder_create: all rows, A/B and tests)
    bool cls_shortcut = true, last_shortcut = false;
    uint16_t *c_ctx = nullptr, *c_xb = nullptr, *c_y = nullptr, *c_h = nullptr; uint8_t* c_xlo = nullptr;
    int *c_off = nullptr, *c_nk = nullptr, *c_cls = nullptr, *d_B = nullptr;
};

typedef Encoder::GraphEntryT GraphEntry;
static void drop_graphs(Encoder* e) {
    for (auto& g : e->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    e->graphs.clear();
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// a buffer that `owner` (Encoder::ws_bufs / own_bufs) frees
template <class P>
static int dmalloc(std::vector<void**>& owner, P** p, size_t bytes) {
    KR_HIP(hipMalloc(reinterpret_cast<void**>(p), bytes));
    owner.push_back(reinterpret_cast<void**>(p));
    return 0;
}
static void free_bufs(std::vector<void**>& owner) {
    for (void** p : owner) { (void)hipFree(*p); *p = nullptr; }
    owner.clear();
}

static void free_ws(Encoder* e) {
    if (!e->graphs.empty()) { (void)hipDeviceSynchronize(); drop_graphs(e); }   // captured kernels hold workspace pointers
    free_bufs(e->ws_bufs);
    e->capT = 0; e->capB = 0; e->capBS = 0; e->capW = 0;
}

// DeBERTa handles: the buckets a batch of width S can reach, [p0, p0 + W) with p0 and W multiples of 32 inside the table's TP = round_up(2 Bk, 32) rows: column
// differences lie in [-(S - 1), S - 1], the bucket rule is odd and monotonic
static void pos_span(const Encoder* e, int S, int& p0, int& W) {
    const int Bk = e->plan.deb_buckets;
    const int lo = model::deberta_bucket(-(S - 1), Bk, e->plan.deb_max_rel), hi = model::deberta_bucket(S - 1, Bk, e->plan.deb_max_rel);
    p0 = lo & ~31;
    W = (int)round_up(hi + 1 - p0, 32);
}

static int ensure_ws(Encoder* e, int B, int S) {
    const int64_t maxT = (int64_t)B * (S + 8);
    const int H = e->cfg.hidden, FF = e->cfg.intermediate;
    const int64_t Dq = e->plan.q_dim;     // q and ctx rows: heads d_h wide, H unless the handle has a head width of its own
    int span_p0 = 0, span_W = 0;
    if (e->plan.family == model::DEBERTA) pos_span(e, S, span_p0, span_W);
    if (!e->d_T) {
        KR_TRY(dmalloc(e->own_bufs, &e->d_T, sizeof(int))); KR_TRY(dmalloc(e->own_bufs, &e->d_err, sizeof(int)));
        KR_HIP(hipMemset(e->d_err, 0, sizeof(int)));
        KR_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->h_err), sizeof(int), hipHostMallocDefault));
        *e->h_err = 0;
        KR_HIP(hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming));
    }
    if (maxT <= e->capT && B <= e->capB && (int64_t)B * S <= e->capBS && span_W <= e->capW) return 0;
    if (maxT > (int64_t)1 << 24) return fail(KR_EINVAL, "batch of %lld tokens: at most 2^24 per forward (32-bit offsets inside the attention kernels)", (long long)maxT);
    free_ws(e);
    const int64_t capT = round_up(maxT, 256), capB = B, capBS = (int64_t)B * S;   // multiple of the 256-token tile: see k_proj
    KR_TRY(dmalloc(e->ws_bufs, &e->d_ids, capBS * 8)); KR_TRY(dmalloc(e->ws_bufs, &e->d_mask, capBS * 8)); KR_TRY(dmalloc(e->ws_bufs, &e->d_tt, capBS * 8));
    KR_TRY(dmalloc(e->ws_bufs, &e->seq_off, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_nk, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_nq, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_cls, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_has0, capB * 4));
    KR_TRY(dmalloc(e->ws_bufs, &e->tok_id, capT * 4));
    KR_TRY(dmalloc(e->ws_bufs, &e->tok_pos, (capT + 64) * 4));    // 64 entries of slack: the window's gathered key columns are read in whole 64-key steps (attn_window_tile)
    KR_HIP(hipMemset(e->tok_pos, 0, (size_t)(capT + 64) * 4));
    KR_TRY(dmalloc(e->ws_bufs, &e->tok_type, capT * 4));
    const model::ModelPlan& p = e->plan;
    if (p.pos == model::POS_FAIRSEQ) KR_TRY(dmalloc(e->ws_bufs, &e->tok_epos, capT * 4));
    if (p.rotary) {
        KR_TRY(dmalloc(e->ws_bufs, &e->tok_zero, capT * 4)); KR_HIP(hipMemset(e->tok_zero, 0, (size_t)capT * 4));
        KR_TRY(dmalloc(e->ws_bufs, &e->tok_rpos, capT * 4)); KR_HIP(hipMemset(e->tok_rpos, 0, (size_t)capT * 4));
    }
    if (p.pos == model::POS_DISENT) {      // no position row either (a zero row), and the position scores of every packed row: heads x 2 x W floats per token
        KR_TRY(dmalloc(e->ws_bufs, &e->tok_zero, capT * 4)); KR_HIP(hipMemset(e->tok_zero, 0, (size_t)capT * 4));
        KR_TRY(dmalloc(e->ws_bufs, &e->pos_sc, (size_t)capT * e->cfg.heads * 2 * span_W * 4));
    }
    KR_TRY(dmalloc(e->ws_bufs, &e->xlo, capT * H)); KR_TRY(dmalloc(e->ws_bufs, &e->y, capT * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->out, (size_t)capB * p.out_width * 4));
    if (p.ws & model::WS_POOLED) KR_TRY(dmalloc(e->ws_bufs, &e->pooled, (size_t)capB * H * 4));
    if (p.ws & model::WS_SLOT_ROW) KR_TRY(dmalloc(e->ws_bufs, &e->slot_row, capBS * 4));
    if (p.ws & model::WS_ROW_SEQ) KR_TRY(dmalloc(e->ws_bufs, &e->row_seq, capT * 4));
    if (p.ws & model::WS_CY) KR_TRY(dmalloc(e->ws_bufs, &e->cy, capT * p.head_dim[model::HEAD_COLBERT] * 2));      // capT rows: the projection's tiles are whole (see k_proj)
    KR_TRY(dmalloc(e->ws_bufs, &e->xb, capT * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->q, capT * Dq * 2));
    const int64_t A = p.kv_dim;   // k [T, A] and V^T [A, ldv] exist once per KV head: A = H unless the handle is a grouped-query decoder's
    KR_TRY(dmalloc(e->ws_bufs, &e->k, (capT + 64) * A * 2));    // 64 rows of slack: k_attn_dma reads whole 64-key chunks (the rows past a sequence are masked)
    KR_HIP(hipMemset(e->k, 0, (size_t)(capT + 64) * A * 2));
    e->ldv = capT + 64;   // slack: the last key tile of the last sequence may read up to 43 columns past T
    KR_TRY(dmalloc(e->ws_bufs, &e->vT, (size_t)A * e->ldv * 2));
    KR_HIP(hipMemset(e->vT, 0, (size_t)A * e->ldv * 2));
    KR_TRY(dmalloc(e->ws_bufs, &e->ctx, capT * Dq * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->h, capT * FF * 2));
    if (p.pre_ln) {
        KR_TRY(dmalloc(e->ws_bufs, &e->rb, capT * H * 2));
        if (e->use_lo) KR_TRY(dmalloc(e->ws_bufs, &e->rlo, capT * H));
    }
    if (e->cls_shortcut) {
        const int64_t capC = round_up(capB, 256);                 // token-indexed buffers come in multiples of the 256-row tile (see k_proj)
        KR_TRY(dmalloc(e->ws_bufs, &e->c_ctx, capC * Dq * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->c_xb, capC * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->c_y, capC * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->c_xlo, capC * H));
        KR_TRY(dmalloc(e->ws_bufs, &e->c_h, capC * FF * 2));
        if (p.pre_ln) {
            KR_TRY(dmalloc(e->ws_bufs, &e->c_rb, capC * H * 2)); KR_HIP(hipMemset(e->c_rb, 0, (size_t)capC * H * 2));
            if (e->use_lo) { KR_TRY(dmalloc(e->ws_bufs, &e->c_rlo, capC * H)); KR_HIP(hipMemset(e->c_rlo, 0x80, (size_t)capC * H)); }
        }
        KR_HIP(hipMemset(e->c_ctx, 0, (size_t)capC * Dq * 2)); KR_HIP(hipMemset(e->c_xb, 0, (size_t)capC * H * 2)); KR_HIP(hipMemset(e->c_xlo, 0x80, (size_t)capC * H));
        KR_TRY(dmalloc(e->ws_bufs, &e->c_off, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->c_nk, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->c_cls, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->d_B, sizeof(int)));
    }
    e->capT = capT; e->capB = (int)capB; e->capBS = capBS; e->capW = span_W;
    return 0;
}

}  // namespace KR_ENC_NS
}  // namespace kr

#include "encoder_weights.hpp"

namespace kr {
namespace KR_ENC_NS {

// The attention of a layer (model::AttnMode) as a compile-time constant: f(std::integral_constant<int, AM>{}), in the manner of with_epilogue
template <class F>
static int with_attn_mode(int am, F&& f) {
    switch (am) {
        case AM_PLAIN: return f(std::integral_constant<int, AM_PLAIN>{});
        case AM_BIAS: return f(std::integral_constant<int, AM_BIAS>{});
        case AM_WIN: return f(std::integral_constant<int, AM_WIN>{});
        case AM_DISENT: return f(std::integral_constant<int, AM_DISENT>{});
        case AM_CAUSAL: return f(std::integral_constant<int, AM_CAUSAL>{});
        default: return fail(KR_ESTATE, "attention mode %d is not built into this library", am);
    }
}
// causal: the window's kernels with a one-sided window — every column to the left (no column difference reaches max_pos), none to the right
static AttnWinArgs causal_args(const Encoder* e) { return AttnWinArgs{e->tok_pos, e->cfg.max_pos, 0, e->bias_gather ? 1 : 0}; }
// what the attention kernels of mode AM read beside q, k and V^T: the one place that takes it from the handle (p0, W: pos_span of the forward's S — the
// layout k_pos_scores wrote a DeBERTa layer's scores in)
template <int AM>
static auto attn_mode_args(const Encoder* e, int p0, int W) {
    if constexpr (AM == AM_DISENT) return AttnDisentArgs{e->pos_sc, e->tok_pos, e->deb_bucket, e->cfg.max_pos - 1, p0, W, e->cfg.heads};
    else if constexpr (AM == AM_BIAS) return AttnBiasArgs{e->bias_tab, e->tok_pos, e->bias_width, e->bias_gather ? 1 : 0};
    else if constexpr (AM == AM_WIN) return AttnWinArgs{e->tok_pos, e->plan.half_window, e->plan.half_window, e->bias_gather ? 1 : 0};
    else if constexpr (AM == AM_CAUSAL) return causal_args(e);
    else return AttnNoBiasArgs{};
}

// The input of a forward as it lies in the workspace.  Padded: [B,S] ids / mask in d_ids / d_mask, with has_tt the caller's token types in d_tt (else all
// zero).  Ragged (kr_encoder_forward_packed): Encoder::rag_ids / rag_lens, `total` = length of the token list.
struct Input { bool ragged, has_tt; int total; };

// The rows the tail of a layer (Wo -> LayerNorm -> W1 + GELU -> W2 -> LayerNorm) and the pooling run on: every token row, or, for the last layer under CLS
// pooling, the gathered CLS rows (k_gather_cls)
struct RowSet {
    uint16_t *ctx, *xb, *y, *h;
    uint8_t *lo, *lo_last;       // low half the inner LayerNorms read / write (nullptr without use_lo); the one the LAST LayerNorm of the encoder always writes
    const int *off, *nk, *cls;   // sequence tables over these rows (k_pool)
    int* rows;                   // device word: how many rows are live
    int64_t max_rows;
    unsigned ln_grid;
    uint16_t* rb; uint8_t* rlo;  // ModernBert handles: the pre-LN residual stream of these rows (rlo: nullptr without use_lo)
};

// Row width as a compile-time constant (width_c, with_ln_width: encoder_rows.hpp): the pool and head family of kernels covers a row in NJ steps of 256
template <class F> static auto with_pool_width(int H, F&& f) { return H <= 256 ? f(width_c<1>{}) : H <= 512 ? f(width_c<2>{}) : H <= 1024 ? f(width_c<4>{}) : f(width_c<8>{}); }

// What the steps of one forward share (enqueue_forward fills it in)
struct Forward {
    Encoder* e; hipStream_t st;
    int B, S, H, FF; float eps;
    model::ForwardPool pool;     // what the requested pool packs like, selects and runs behind the last layer
    int flags; float* tok_out;   // enqueue_forward
    bool disent;                 // a DeBERTa handle: every sequence through k_attn_lds (the mode is not built into k_attn_dma)
    bool long_seq;               // > 128 tokens: the LDS-DMA attention kernel (KIRAG_AMD_ATTN_LDS=1: never)
    bool shortcut;               // the last layer finishes on one gathered row per sequence (cls_rows)
    int align;                   // sequence offsets: multiple of 8 tokens under long_seq so that V^T chunks start 16-B aligned, else of 4
    int nqt_max;                 // q-tiles of the longest possible sequence
    int span_p0, span_W;         // pos_span of S (DeBERTa handles)
    int64_t maxT;                // upper bound of the packed token count (each sequence is padded to `align`)
    unsigned row_grid, ln_grid;  // one wave per row; k_ln is grid-stride (its parameters stay in registers across rows)
    ProjLaunch pl;
    AttnOperands attn;
    RowSet all_rows, cls_rows;
};

// T5 and decoder handles: the embedding row is the residual stream itself, xb = block 0's attention norm of it
static bool embed_is_residual(const model::ModelPlan& p) { return p.pos == model::POS_BIAS_ONLY || p.family == model::DECODER; }

// the fields every projection site assigns (ldx / ldo = 0: K / F)
static void proj(ProjArgs& a, const uint16_t* W, const uint16_t* X, int F, int K, const float* bias, uint16_t* out0, int64_t ldx = 0, int64_t ldo = 0) {
    a.W = W; a.X = X; a.F = F; a.K = K; a.bias = bias; a.out0 = out0; a.ldx = ldx; a.ldo = ldo;
}

static void enqueue_embed(const Forward& f) {
    using namespace model;
    Encoder* e = f.e;
    const ModelPlan& p = e->plan;
    const int H = f.H;
    if (p.rotary) launch_rot_pos(e->seq_off, e->seq_nq, f.align, e->tok_pos, e->tok_rpos, (unsigned)f.B, f.st);
    if (embed_is_residual(p)) {
        launch_embed_rms(e->tok_id, e->d_T, e->word, e->elng, f.eps, H, e->rb, e->use_lo ? e->rlo : nullptr, e->xb, f.row_grid, f.st);
    } else {
        const bool no_pos = p.pos == POS_ROTARY || f.disent;      // a zero row in place of a position row
        launch_embed_ln(e->tok_id, no_pos ? e->tok_zero : p.pos == POS_FAIRSEQ ? e->tok_epos : e->tok_pos, e->tok_type, e->d_T, e->word, no_pos ? e->zero_row : e->pos, e->type,
                        e->elng, e->elnb, f.eps, H, e->use_lo ? e->xlo : nullptr, e->xb, f.row_grid, f.st);
    }
}

// The norm behind a residual projection of a layer's tail, on the rows of r.  Post-LN: xb = LayerNorm(y + bias + xb), the low half read at r.lo and written to
// lo_out.  Pre-LN (k_ln16_pre; RMS on T5 handles): (rin, rin_lo) + y + bias is the residual stream, stored to (rb_out, r.rlo) unless rb_out is nullptr; xb =
// the NEXT norm of it, its low half to lo_out unless that is nullptr.  (The kernels and their cache policies: launch_ln_pre / launch_ln_post, encoder_rows.hpp)
static void launch_norm(const Forward& f, const RowSet& r, const float* bias, const float* g, const float* b, const uint16_t* rin, const uint8_t* rin_lo, uint16_t* rb_out,
                        uint8_t* lo_out) {
    const model::ModelPlan& p = f.e->plan;
    if (p.pre_ln) launch_ln_pre(p.rms, r.y, bias, r.rows, g, b, f.eps, f.H, rin, rin_lo, rb_out, r.rlo, lo_out, r.xb, r.ln_grid, f.st);
    else launch_ln_post(r.y, bias, r.rows, g, b, f.eps, f.H, r.lo, lo_out, r.xb, r.ln_grid, f.st);
}
// The tail of a layer on the rows of r: Wo + residual -> norm, W1 + activation, W2 + residual -> norm.  Post-LN: the norms are LayerNorms of the sum.  Pre-LN
// (ModernBert, T5 and decoder handles) on the same five launches: r += y + b, xb = the next norm of r.  (rin, rin_lo): the residual stream as a pre-LN layer
// finds it — r.rb / r.rlo, or for layer 0 on all rows the embedding LayerNorm's output itself (xb / xlo: attn_norm of layer 0 is the identity)
static int enqueue_tail(const Forward& f, ProjArgs a, const LayerW& l, const RowSet& r, bool last, const uint16_t* rin, const uint8_t* rin_lo) {
    static constexpr int FF_EPI[] = {EPI_GELU, EPI_SWIGLU, EPI_GEGLU, EPI_RELU, EPI_GEGLU_TANH};   // by FfKind
    const model::ModelPlan& p = f.e->plan;
    const int H = f.H, FF = f.FF;
    const bool pre = p.pre_ln;
    a.Tp = r.rows; a.H = H;
    // attention.output.dense / attn.Wo (K = the width of the context), then the norm: xb = LayerNorm(y + b + xb), or r += y + b; xb = mlp_norm(r)
    proj(a, l.wo, r.ctx, H, p.q_dim, l.bo_eff, r.y);
    KR_TRY(launch_proj(EPI_DENSE, a, r.max_rows, f.pl, f.st));
    launch_norm(f, r, l.bo_eff, l.ln1g, l.ln1b, rin, rin_lo, r.rb, pre ? nullptr : r.lo);
    // intermediate.dense + GELU, or gate_proj | up_proj / mlp.Wi (input | gate) as one GEMM of 2 FF columns + SwiGLU / GEGLU: h [rows, FF] either way.  A T5
    // handle: wi + relu, or wi_0 | wi_1 the same way + gelu_new, no bias
    proj(a, l.w1, r.xb, p.ff_gated ? 2 * FF : FF, H, pre ? l.b1p : l.b1, r.h, 0, FF);
    KR_TRY(launch_proj(FF_EPI[p.ff], a, r.max_rows, f.pl, f.st));
    // output.dense / mlp.Wo, then the norm.  The LAST one always writes the low half: pooling and kr_encoder_last_hidden read the final hidden state with 16
    // mantissa bits.  Pre-LN: xb = the next layer's attn_norm(r), or final_norm(r), behind which nothing reads r
    proj(a, l.w2, r.h, H, FF, l.b2, r.y, FF, 0);
    KR_TRY(launch_proj(EPI_DENSE, a, r.max_rows, f.pl, f.st));
    launch_norm(f, r, l.b2, l.ln2g, l.ln2b, r.rb, r.rlo, last ? nullptr : r.rb, last ? r.lo_last : pre ? nullptr : r.lo);
    return 0;
}

// one layer: q | k | v^T, attention, for the last layer of a shortcut forward the gather, the tail
static int enqueue_layer(const Forward& f, size_t li) {
    using namespace model;
    static constexpr int QKV_EPI[] = {EPI_QKV, EPI_QKV_ROT, EPI_QKV_ROTB, EPI_QKV_SPLIT};   // by QkvKind
    Encoder* e = f.e;
    const ModelPlan& p = e->plan;
    const LayerW& l = e->L[li];
    const LayerPlan& lp = p.layers[li];
    const bool first = li == 0, last = li + 1 == e->L.size(), pre = p.pre_ln;
    const int H = f.H, Dq = p.q_dim;           // Dq = heads d_h: the width of q and ctx (H unless the handle has a head width of its own)
    const bool local = lp.attn == AM_WIN;      // a ModernBert handle's sliding-window layer: its own rotary table, windowed attention
    ProjArgs a{};
    a.Tp = e->d_T; a.H = Dq;
    a.rot_cos = local ? e->rot_cos_l : e->rot_cos; a.rot_sin = local ? e->rot_sin_l : e->rot_sin; a.tpos = e->tok_rpos; a.max_pos = e->cfg.max_pos; a.dh = p.head_w;
    // q | k | v^T in one GEMM (F = Dq + 2A: 3H unless k and v are a grouped-query decoder's or the head width is the handle's own)
    a.A = p.kv_dim;
    proj(a, l.wqkv, e->xb, Dq + 2 * p.kv_dim, H, l.bqkv, e->q);
    a.out1 = e->k; a.outT = e->vT; a.ldT = e->ldv;
    KR_TRY(launch_proj(QKV_EPI[lp.qkv], a, f.maxT, f.pl, f.st));
    if (lp.qkv == QKV_SPLIT) {
        // the q / k norms of the layer and the rotation behind them, in place on q and k: one more read and write of both
        const int kv_heads = p.kv_dim / p.head_w;
        launch_qk_norm_rope(p.head_w, e->q, e->k, e->d_T, e->cfg.heads, kv_heads, l.qng, l.kng, f.eps * l.qfold * l.qfold, f.eps, a.rot_cos, a.rot_sin, e->tok_rpos, e->cfg.max_pos,
                            qk_norm_grid(f.maxT, e->cfg.heads, kv_heads, p.head_w), f.st);
    }
    auto attend = [&](auto dh) -> int {
        constexpr int DH = decltype(dh)::value;
        if (lp.attn == AM_DISENT) {      // q . PK and k . PQ of every packed row, for the bias tiles of this layer's attention
            // (k_pos_scores reads k with q's pitch H and head h of both: a DeBERTa handle has one KV head per query head, describe() refuses any other)
            if (p.kv_dim != H) return fail(KR_ESTATE, "a DeBERTa handle with k / v width %d != hidden", p.kv_dim);
            const dim3 grid((unsigned)((f.maxT + POS_ROWS - 1) / POS_ROWS), (unsigned)e->cfg.heads);
            hipLaunchKernelGGL(k_pos_scores<DH>, grid, dim3(256), 0, f.st, e->q, e->k, e->d_T, H, e->cfg.heads, l.pk16, l.pq16, (int)round_up(2 * p.deb_buckets, 32), f.span_p0, f.span_W,
                               e->pos_sc);
        }
        return with_attn_mode(lp.attn, [&](auto am) -> int {
            return launch_attention<DH>(f.attn, (int)round_up(f.S, 32), f.nqt_max, f.long_seq, attn_mode_args<decltype(am)::value>(e, f.span_p0, f.span_W), e->device, f.st);
        });
    };
    if (p.head_w == 128) {
        // (its own lambda: the 128-wide kernels are built for the plain and the window / causal modes, and no k_pos_scores<128> exists)
        if (lp.attn == AM_CAUSAL) KR_TRY(launch_attention<128>(f.attn, (int)round_up(f.S, 32), f.nqt_max, false, causal_args(e), e->device, f.st));
        else if (lp.attn == AM_PLAIN) KR_TRY(launch_attention<128>(f.attn, (int)round_up(f.S, 32), f.nqt_max, false, AttnNoBiasArgs{}, e->device, f.st));
        else return fail(KR_ESTATE, "attention mode %d is not built for 128-wide heads", (int)lp.attn);
    } else if (p.head_w == 32) KR_TRY(attend(std::integral_constant<int, 32>{})); else KR_TRY(attend(std::integral_constant<int, 64>{}));
    // CLS shortcut: only the CLS row of every sequence is read after the last layer: gather those rows and finish the layer on B rows (same kernels, same
    // arithmetic per row: the projection loops are bit-identical for every tiling and LayerNorm is per row, so the embedding does not change by one bit)
    // (a pre-LN handle: the residual stream travels in the place of xb — the operand is rewritten by the first norm of the tail)
    // (a T5 or decoder handle: the embedding launch has stored the residual stream itself, layer 0 finds it like every layer)
    const bool in_rb = pre && (!first || embed_is_residual(p));
    const uint16_t* rin = in_rb ? e->rb : e->xb;
    const uint8_t* rin_lo = in_rb ? f.all_rows.rlo : f.all_rows.lo;
    if (!(last && f.shortcut)) return enqueue_tail(f, a, l, f.all_rows, last, rin, rin_lo);
    launch_gather_cls(e->ctx, rin, rin_lo, e->seq_off, e->seq_cls, e->seq_nk, H, e->c_ctx, pre ? e->c_rb : e->c_xb, pre ? e->c_rlo : e->c_xlo, e->c_off, e->c_nk, e->c_cls, e->d_B,
                      f.pool.score ? 1 : 0, Dq, (unsigned)f.B, f.st);
    return enqueue_tail(f, a, l, f.cls_rows, last, e->c_rb, f.cls_rows.rlo);
}
// KR_POOL_SPLADE behind the last layer: the MLM head on every packed row, max over each sequence's rows, log1p — into f.tok_out [B, vocab]
static int enqueue_splade_head(const Forward& f) {
    using namespace model;
    Encoder* e = f.e;
    const int H = f.H, V = e->cfg.vocab;
    // t = LayerNorm(gelu(Wt x + bt)) of the packed rows: y <- EPI_GELU, q <- k_ln16_head (both buffers are free behind the last layer; xb / xlo keep the
    // final hidden state for kr_encoder_last_hidden)
    ProjArgs a{};
    a.Tp = e->d_T; a.H = H;
    proj(a, e->hh(HEAD_MLM, 0), e->xb, H, H, e->hf(HEAD_MLM, 1), e->y);
    KR_TRY(launch_proj(EPI_GELU, a, f.maxT, f.pl, f.st));
    KR_HIP(hipMemsetAsync(e->row_seq, 0xff, (size_t)e->capT * 4, f.st));
    hipLaunchKernelGGL(k_splade_rowseq, dim3(f.B), dim3(64), 0, f.st, e->seq_off, e->seq_nk, e->row_seq);
    launch_ln_head(e->y, e->zero_row, e->d_T, e->hf(HEAD_MLM, 2), e->hf(HEAD_MLM, 3), f.eps, H, e->row_seq, e->q, e->d_err, f.ln_grid, f.st);
    // the decoder: [rows] x [Vpad, H]^T reduced over each sequence's rows inside the launch (EPI_SPLADE), then log1p in place
    KR_HIP(hipMemsetAsync(f.tok_out, 0, (size_t)f.B * V * 4, f.st));
    proj(a, e->hh(HEAD_MLM, 4), e->q, (int)extent(e->cfg, XVPAD), H, e->hf(HEAD_MLM, 5), nullptr);
    a.row_seq = e->row_seq; a.smax = reinterpret_cast<unsigned int*>(f.tok_out); a.V = V;
    KR_TRY(launch_proj(EPI_SPLADE, a, f.maxT, f.pl, f.st));
    const int64_t n = (int64_t)f.B * V;
    hipLaunchKernelGGL(k_splade_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, f.st, f.tok_out, n, e->d_err);
    return 0;
}

// pooling (masked mean, CLS or last row, L2-normalised; raw rows for a classifier) and the head behind it, into e->out
static int enqueue_pool_and_head(const Forward& f) {
    using namespace model;
    Encoder* e = f.e;
    const ModelPlan& p = e->plan;
    const int B = f.B, H = f.H;
    const RowSet& r = f.shortcut ? f.cls_rows : f.all_rows;
    const int NJ = with_pool_width(H, [](auto nj) { return (int)decltype(nj)::value; });
    // the rows stay as pooled (RAW) for a classifier, for the sentence-transformers Dense head (which normalises its own output) and under
    // config.normalize_output = 0; config.pool_tokens selects what a KR_POOL_MEAN forward pools (k_pool_tok: the max, sum / sqrt(n))
    const bool st_dense = p.head[HEAD_ST_DENSE] && !f.pool.classify;
    const bool raw = f.pool.classify || st_dense || !p.normalize;
    const int tok = f.pool.select == KR_POOL_MEAN && !f.pool.classify ? p.pool_tokens : POOL_TOK_MEAN;
    float* pool_out = p.head[HEAD_DENSE] || f.pool.classify || st_dense ? e->pooled : e->out;
    const int pool_lds = POOL_WAVES * NJ * 256 * 4 + POOL_WAVES * 4;
    if (tok != POOL_TOK_MEAN) {
        const auto tok_kernel = with_pool_width(H, [&](auto nj) {
            constexpr int N = decltype(nj)::value;
            return tok == POOL_TOK_MAX ? (raw ? &k_pool_tok<N, true, 1> : &k_pool_tok<N, false, 1>) : (raw ? &k_pool_tok<N, true, 2> : &k_pool_tok<N, false, 2>);
        });
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(tok_kernel), pool_lds, e->device));
        hipLaunchKernelGGL(tok_kernel, dim3(B), dim3(POOL_WAVES * 64), pool_lds, f.st, r.xb, r.lo_last, r.off, r.nk, H, pool_out, e->d_err);
    } else {
        const auto pool_kernel = raw ? with_pool_width(H, [](auto nj) { return &k_pool<decltype(nj)::value, true>; })
                                     : with_pool_width(H, [](auto nj) { return &k_pool<decltype(nj)::value>; });
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(pool_kernel), pool_lds, e->device));
        hipLaunchKernelGGL(pool_kernel, dim3(B), dim3(POOL_WAVES * 64), pool_lds, f.st, r.xb, r.lo_last, r.off, r.nk, r.cls, H, f.pool.select, pool_out, e->d_err);
    }
    if (st_dense) {              // out [B, P] = act(st_dense.weight . pooled + st_dense.bias), normalised unless config.normalize_output = 0
        const int P = p.head_dim[HEAD_ST_DENSE], dense_lds = PD_SEQ * (H + P) * 4 + PD_SEQ * 4;
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(&k_st_dense), PD_SEQ * (2048 + 2048) * 4 + PD_SEQ * 4, e->device));
        hipLaunchKernelGGL(k_st_dense, dim3((B + PD_SEQ - 1) / PD_SEQ), dim3(256), dense_lds, f.st, e->pooled, e->hf(HEAD_ST_DENSE, 0), e->hf(HEAD_ST_DENSE, 1), B, H, P,
                           p.st_tanh ? 1 : 0, p.normalize ? 1 : 0, r.nk, e->out, e->d_err);
        return 0;
    }
    if (f.pool.score) {          // a decoder handle's score head: out [B, L] = score.weight . pooled, one launch without LDS
        const int L = p.head_dim[HEAD_SCORE];
        const int64_t waves = (int64_t)B * ((L + SH_LABELS - 1) / SH_LABELS);
        hipLaunchKernelGGL(k_score_head, dim3((unsigned)((waves + SH_WAVES - 1) / SH_WAVES)), dim3(SH_WAVES * 64), 0, f.st, e->pooled, e->hf(HEAD_SCORE, 0), B, H, L, e->out, r.nk, e->d_err);
    } else if (f.pool.classify) {
        // the classification head: out [B, L] = Wo . act(Wd . pooled + bd) + bo, one kernel per (width, act).  HEAD_CLS {Wd, bd, Wo, bo}: tanh, or DeBERTa's
        // erf-GELU (cls_gelu).  HEAD_MODERN_CLS {Wd, bd, norm g, norm b, Wo, bo}: Wo . LayerNorm(erf_gelu(Wd . pooled + bd)) + bo.  The GELU variants guard
        // their result (r.nk, the error word); the tanh head takes neither
        const int hd = p.classifier;
        const bool gln = hd == HEAD_MODERN_CLS, gelu = gln || p.cls_gelu;
        const auto head_kernel = with_pool_width(H, [&](auto nj) {
            constexpr int N = decltype(nj)::value;
            return gln ? &k_cls_head<N, true> : gelu ? &k_cls_head<N, false, true> : &k_cls_head<N>;
        });
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(head_kernel), CH_SEQ * 2 * NJ * 256 * 4, e->device));      // the widest H of the instantiation (64 KiB at 2048)
        hipLaunchKernelGGL(head_kernel, dim3((B + CH_SEQ - 1) / CH_SEQ), dim3(CH_WAVES * 64), CH_SEQ * 2 * H * 4, f.st, e->pooled, e->hf(hd, 0), e->hf(hd, 1), e->hf(hd, gln ? 4 : 2),
                           e->hf(hd, gln ? 5 : 3), B, H, p.head_dim[hd], e->out, gln ? e->hf(hd, 2) : nullptr, gln ? e->hf(hd, 3) : nullptr, gln ? f.eps : 0.f,
                           gelu ? r.nk : nullptr, gelu ? e->d_err : nullptr);
    } else if (p.head[HEAD_DENSE]) {     // the Dense head: out [B, P] = normalize(W . pooled)
        const int P = p.head_dim[HEAD_DENSE], dense_lds = PD_SEQ * (H + P) * 4 + PD_SEQ * 4;
        // one kernel, an LDS size per handle: the attribute is set once per device (set_lds_once) to what the largest handle needs, H = P = 2048 (64 KiB + 16 B)
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(&k_pool_dense), PD_SEQ * (2048 + 2048) * 4 + PD_SEQ * 4, e->device));
        hipLaunchKernelGGL(k_pool_dense, dim3((B + PD_SEQ - 1) / PD_SEQ), dim3(256), dense_lds, f.st, e->pooled, e->hf(HEAD_DENSE, 0), B, H, P, e->out);
    }
    return 0;
}

// bge-m3's token-level blocks, straight into f.tok_out: sparse [B, S], then colbert [B, S, P]
static int enqueue_m3_blocks(const Forward& f) {
    using namespace model;
    Encoder* e = f.e;
    const int H = f.H, P = e->plan.head_dim[HEAD_COLBERT];
    const int64_t slots = (int64_t)f.B * f.S;
    const unsigned slot_grid = (unsigned)((slots + 3) / 4);
    hipLaunchKernelGGL(k_m3_slots, dim3(f.B), dim3(64), 0, f.st, e->d_mask, e->seq_off, f.S, e->slot_row);
    float* o = f.tok_out;
    if (f.flags & KR_POOL_WITH_SPARSE) {
        hipLaunchKernelGGL(k_m3_sparse, dim3(slot_grid), dim3(256), 0, f.st, e->xb, e->xlo, e->hf(HEAD_SPARSE, 0), e->hf(HEAD_SPARSE, 1), e->slot_row, slots, H, o, e->d_err);
        o += slots;
    }
    if (f.flags & KR_POOL_WITH_COLBERT) {      // one more projection of the packed rows on the loops every layer uses, then bias + norm + scatter
        ProjArgs a{};
        a.Tp = e->d_T; a.H = H;
        proj(a, e->hh(HEAD_COLBERT, 0), e->xb, P, H, e->hf(HEAD_COLBERT, 1), e->cy);
        KR_TRY(launch_proj(EPI_DENSE, a, f.maxT, f.pl, f.st));
        hipLaunchKernelGGL(k_m3_rows, dim3(slot_grid), dim3(256), 0, f.st, e->cy, e->hf(HEAD_COLBERT, 1), e->slot_row, slots, P, o, e->d_err);
    }
    return 0;
}

// every kernel of one forward, enqueued on `st` (input already in the workspace, result left in e->out): resolve the pool, pack, embed, the layers, the head
// flags: KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT (pool is the base pool); tok_out: device memory for the token-level blocks, [B, S] then [B, S, P]
// pool = KR_POOL_SPLADE: tok_out is the [B, vocab] result, used as the reduction buffer of the decoder launch; nothing is left in e->out
static int enqueue_forward(Encoder* e, int B, int S, int pool, hipStream_t st, const Input& in, int flags = 0, float* tok_out = nullptr) {
    using namespace model;
    const ModelPlan& p = e->plan;
    e->kn.read();
    Forward f{};
    f.e = e; f.st = st; f.B = B; f.S = S; f.H = e->cfg.hidden; f.FF = e->cfg.intermediate; f.eps = e->cfg.ln_eps; f.flags = flags; f.tok_out = tok_out;
    f.pool = resolve_pool(p, pool);
    f.pl = ProjLaunch{e->num_cu, e->device, e->kn.pw, e->kn.epi_prio, e->kn.force_tile};
    const int cls_row = f.pool.pack == KR_POOL_CLS ? 1 : 0;      // the query-only row of a masked column 0
    f.nqt_max = (S + cls_row + 31) / 32;
    f.disent = p.pos == POS_DISENT;
    f.long_seq = f.nqt_max > 4 && !e->kn.attn_lds && !f.disent && p.head_w != 128;      // (128-wide heads: k_attn_wide at every length)
    if (f.disent) pos_span(e, S, f.span_p0, f.span_W);
    f.align = f.long_seq ? 8 : 4;
    const PackRules rules{e->cfg.vocab, e->cfg.type_vocab, f.pool.pack, f.align, p.pad_idx};
    const SeqTables seq{e->seq_nk, e->seq_has0, e->seq_nq, e->seq_off, e->seq_cls, e->d_T};
    const TokTables tok{e->tok_id, e->tok_pos, e->tok_type, e->tok_epos, e->d_err};
    if (in.ragged) pack_ragged(e->rag_ids(), e->rag_lens(), e->rag_in_off(), B, S, in.total, rules, seq, tok, st);
    else pack_padded(e->d_ids, e->d_mask, in.has_tt ? e->d_tt : nullptr, B, S, rules, seq, tok, st);
    f.maxT = (int64_t)B * ((S + cls_row + f.align - 1) & ~(f.align - 1));
    f.row_grid = row_grid(f.maxT);
    f.ln_grid = ln_grid(f.maxT, e->num_cu_all);      // 8 LayerNorm blocks per CU (encoder_rows.hpp)
    // one row per sequence behind the last layer (the CLS row; the score head's last packed row — the embedding pools of a decoder handle keep every row): the
    // last layer finishes on the gathered rows.  The token-level heads read every row of the last layer
    f.shortcut = f.pool.one_row && e->cls_shortcut && e->c_ctx != nullptr && !flags;
    e->last_shortcut = f.shortcut;
    f.attn = AttnOperands{e->q, e->k, e->vT, e->ldv, e->seq_off, e->seq_nk, e->seq_nq, e->ctx, p.q_dim, e->cfg.heads, p.kv_dim, e->capT, B};
    f.all_rows = RowSet{e->ctx, e->xb, e->y, e->h, e->use_lo ? e->xlo : nullptr, e->xlo, e->seq_off, e->seq_nk, e->seq_cls, e->d_T, f.maxT, f.ln_grid,
                        e->rb, e->use_lo ? e->rlo : nullptr};
    f.cls_rows = RowSet{e->c_ctx, e->c_xb, e->c_y, e->c_h, e->use_lo ? e->c_xlo : nullptr, e->c_xlo, e->c_off, e->c_nk, e->c_cls, e->d_B, B,
                        ln_grid(B, e->num_cu_all), e->c_rb, e->use_lo ? e->c_rlo : nullptr};
    enqueue_embed(f);
    for (size_t li = 0; li < e->L.size(); ++li) KR_TRY(enqueue_layer(f, li));
    if (f.pool.splade) KR_TRY(enqueue_splade_head(f));
    else {
        KR_TRY(enqueue_pool_and_head(f));
        if (flags) KR_TRY(enqueue_m3_blocks(f));
    }
    KR_HIP(hipGetLastError());
    return 0;
}

// Small batches are launch-bound (a 1 x 32-token forward is ~175 launches of 6-13 us).  With KIRAG_AMD_GRAPH=1 (read at kr_encoder_create; OFF by
// default) the kernel sequence of a (B, S, pool) shape is replayed as ONE hipGraph from its second forward on.  Measured on MI355X / ROCm 7.2
// (tools/graph_bench.py, two encoders interleaved in one process, outputs bit-identical): replay is SLOWER than the eager launches, both back to back
// and with a synchronisation after every forward — 1 x 32 tokens 1.40 vs 1.20 ms, 2 x 256 2.14 vs 1.95, 8 x 128 2.31 vs 2.12, 100 x 32 3.42 vs 3.29 —
// about 1.1 us per graph node more than the launch it replaces, so the default stays eager (the asynchronous boundary already lets the host run ahead).  The first forward of a shape runs eagerly (it also sets the function
// attributes, which must not happen during capture); capture and replay use an internal stream (the caller's may be the legacy default stream,
// which cannot be captured), ordered against the caller's stream by events.  Any failure falls back to eager launches for good.
constexpr int64_t GRAPH_MAX_TOKENS = 4096;
static int run_forward(Encoder* e, int B, int S, int pool, hipStream_t st, bool has_tt) {
    const Input in{false, has_tt, 0};
    const int64_t maxT = (int64_t)B * (S + 8);
    if (e->graphs_off || maxT > GRAPH_MAX_TOKENS || has_tt) return enqueue_forward(e, B, S, pool, st, in);
    const uint64_t key = ((uint64_t)B << 32) | ((uint64_t)S << 8) | (uint64_t)pool;
    GraphEntry* ent = nullptr;
    for (auto& g : e->graphs) if (g.key == key) { ent = &g; break; }
    if (!ent) {
        if (e->graphs.size() >= 32) drop_graphs(e);
        e->graphs.push_back(GraphEntry{key, 0, nullptr});
        ent = &e->graphs.back();
    }
    ent->calls++;
    if (ent->calls == 1) return enqueue_forward(e, B, S, pool, st, in);
    if (!e->gstream) {
        if (hipStreamCreateWithFlags(&e->gstream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e->ev_out, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e->graphs_off = true; return enqueue_forward(e, B, S, pool, st, in); }
    }
    if (!ent->exec) {
        hipGraph_t graph = nullptr;
        bool ok = hipStreamBeginCapture(e->gstream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            const int rc = enqueue_forward(e, B, S, pool, e->gstream, in);
            const hipError_t ce = hipStreamEndCapture(e->gstream, &graph);
            ok = rc == 0 && ce == hipSuccess && graph != nullptr && hipGraphInstantiate(&ent->exec, graph, nullptr, nullptr, 0) == hipSuccess;
            if (graph) (void)hipGraphDestroy(graph);
        }
        if (!ok) { (void)hipGetLastError(); ent->exec = nullptr; e->graphs_off = true; return enqueue_forward(e, B, S, pool, st, in); }
    }
    KR_HIP(hipEventRecord(e->ev_in, st));
    KR_HIP(hipStreamWaitEvent(e->gstream, e->ev_in, 0));
    KR_HIP(hipGraphLaunch(ent->exec, e->gstream));
    KR_HIP(hipEventRecord(e->ev_out, e->gstream));
    KR_HIP(hipStreamWaitEvent(st, e->ev_out, 0));
    return 0;
}

// the sticky device error word has been copied to e->h_err and that copy has completed
static int report_token_error(Encoder* e, hipStream_t st) {
    const int w = *e->h_err;
    if (w == 0) return 0;
    *e->h_err = 0;
    KR_HIP(hipMemsetAsync(e->d_err, 0, sizeof(int), st));
    if (w & 1) return fail(KR_EINVAL, "input_ids contain a token id outside [0, %d)", e->cfg.vocab);
    if (w & 4) return fail(KR_EINVAL, "token_type_ids contain a value outside [0, %d)", e->cfg.type_vocab);
    if (w & 8) return fail(KR_EINVAL, "seq_lens hold a length outside [0, S] or do not add up to total_tokens (kr_encoder_forward_packed)");
#ifdef KR_ENC_BUILD_F16
    return fail(KR_ERANGE, "non-finite activations in the forward: a value left the f16 operand range (|x| > 65504) or the weights hold NaN / Inf; "
                           "the embeddings of this batch are not usable (KIRAG_AMD_ENCODER_DTYPE=bf16 has the fp32 exponent range)");
#else
    return fail(KR_ERANGE, "non-finite activations in the forward: the weights (or an overflowing accumulation) hold NaN / Inf; the embeddings of this batch are not usable");
#endif
}

// What both forward entry points check before anything else.  bad_shape: the caller's own pointer / shape test; total_tokens < 0: padded input.
constexpr int M3_FLAGS = KR_POOL_WITH_SPARSE | KR_POOL_WITH_COLBERT;
static int check_forward_args(const Encoder* e, bool bad_shape, int B, int S, int64_t total_tokens, int pool) {
    if (!e) return fail(KR_EINVAL, "encoder is NULL");
    if (!e->ready) return fail(KR_ESTATE, "encoder weights incomplete: call kr_encoder_finalize after loading every tensor");
    if (bad_shape) return fail(KR_EINVAL, "bad input pointers / shape");
    if (S > e->cfg.max_pos) return fail(KR_EINVAL, "sequence length %d exceeds max_position_embeddings %d", S, e->cfg.max_pos);
    const model::ModelPlan& p = e->plan;
    if (p.pad_idx >= 0 && S + p.pad_idx + 1 > e->cfg.max_pos)
        return fail(KR_EINVAL, "sequence length %d + padding index %d + 1 exceeds max_position_embeddings %d (fairseq position rule: at most %d tokens)", S, p.pad_idx,
                    e->cfg.max_pos, e->cfg.max_pos - p.pad_idx - 1);
    if (total_tokens > (int64_t)B * S) return fail(KR_EINVAL, "total_tokens %lld exceeds B * S = %lld", (long long)total_tokens, (long long)B * S);
    const int flags = pool & M3_FLAGS;
    pool &= ~M3_FLAGS;
    const bool decoder = p.family == model::DECODER;
    if (pool == KR_POOL_LAST && !decoder)
        return fail(KR_EINVAL, "pool = 5 (last token) on a %s handle: last-token pooling is accepted on decoder handles (config.decoder_attention) only; elsewhere "
                               "pool must be 0 (mean), 1 (cls), 2 (classify) or 4 (splade), 0 and 1 optionally with KR_POOL_WITH_SPARSE (0x10) / KR_POOL_WITH_COLBERT (0x20)",
                    model::family_name(p.family));
    if (pool != KR_POOL_MEAN && pool != KR_POOL_CLS && pool != KR_POOL_CLASSIFY && pool != KR_POOL_SPLADE && pool != KR_POOL_LAST)
        return fail(KR_EINVAL, "pool must be 0 (mean), 1 (cls), 2 (classify) or 4 (splade), 0 and 1 optionally with KR_POOL_WITH_SPARSE (0x10) / KR_POOL_WITH_COLBERT (0x20)");
    if (flags && pool == KR_POOL_LAST) return fail(KR_EINVAL, "KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT go with pool 0 (mean) or 1 (cls), not with 5 (last token)");
    // (KR_POOL_CLASSIFY on a decoder handle that holds the score head passes: the flags' refusal and the forward below)
    if (decoder && pool != KR_POOL_MEAN && pool != KR_POOL_LAST && !(pool == KR_POOL_CLASSIFY && p.classifier >= 0))
        return fail(KR_EINVAL, "pool = %d (%s) on a decoder handle: it takes KR_POOL_MEAN (0) and KR_POOL_LAST (5) — under a causal mask the first token sees itself alone, "
                               "and the handle has no head", pool, pool == KR_POOL_CLS ? "KR_POOL_CLS" : pool == KR_POOL_CLASSIFY ? "KR_POOL_CLASSIFY" : "KR_POOL_SPLADE");
    if (flags && pool == KR_POOL_CLASSIFY) return fail(KR_EINVAL, "KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT go with pool 0 (mean) or 1 (cls), not with 2 (classify)");
    if (flags && pool == KR_POOL_SPLADE) return fail(KR_EINVAL, "KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT go with pool 0 (mean) or 1 (cls), not with 4 (splade)");
    if (pool == KR_POOL_SPLADE && !p.head[model::HEAD_MLM])
        return fail(KR_ESTATE, "pool = 4 (splade) on a handle without an MLM head: cls.predictions.transform.dense.{weight,bias}, cls.predictions.transform.LayerNorm.{weight,bias} "
                               "and cls.predictions.decoder.{weight,bias} were never loaded");
    if (flags && total_tokens >= 0)
        return fail(KR_EINVAL, "kr_encoder_forward_packed takes no KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT: the token-level blocks are laid out by the columns of a padded batch");
    if ((flags & KR_POOL_WITH_SPARSE) && !p.head[model::HEAD_SPARSE])
        return fail(KR_ESTATE, "KR_POOL_WITH_SPARSE on a handle without a sparse head: sparse_linear.weight and sparse_linear.bias were never loaded");
    if ((flags & KR_POOL_WITH_COLBERT) && !p.head[model::HEAD_COLBERT])
        return fail(KR_ESTATE, "KR_POOL_WITH_COLBERT on a handle without a colbert head: colbert_linear.weight and colbert_linear.bias were never loaded");
    if (pool == KR_POOL_CLASSIFY && p.classifier < 0)
        return fail(KR_ESTATE, p.family == model::MODERN ? "pool = 2 (classify) on a ModernBert handle without a classification head: head.dense.weight, head.norm.weight, "
                                             "classifier.weight and classifier.bias were never loaded"
                                           : "pool = 2 (classify) on a handle without a classification head: classifier.dense.{weight,bias} and "
                                             "classifier.out_proj.{weight,bias} were never loaded");
    if (B > 65535) return fail(KR_EINVAL, "at most 65535 sequences per call");
    return 0;
}

// before the uploads of a forward of B > 0 sequences: the previous asynchronous forward's error word, the workspace
static int begin_forward(Encoder* e, int B, int S, hipStream_t st) {
    KR_TRY(select_device(e->device));
    if (e->pending) {
        if (st != e->last_stream) KR_HIP(hipEventSynchronize(e->ev_done));      // the workspace is shared: a forward on another stream waits for the previous one
        if (hipEventQuery(e->ev_done) == hipSuccess) {                          // finished: report its token-id error now (never blocks)
            e->pending = false;
            KR_TRY(report_token_error(e, st));
        }
    }
    return ensure_ws(e, B, S);
}

// behind the kernels of a forward: the result and the error word travel to the caller
// (tok_elems > 0: the token-level blocks of a flagged forward with a host `out` wait in e->tok_stage and follow the dense block)
static int finish_forward(Encoder* e, int B, int S, int pool, float* out, hipStream_t st, size_t tok_elems = 0) {
    // (KR_POOL_SPLADE has no dense block: its [B, vocab] result is written to a device `out` by the kernels, or waits in e->tok_stage like a token-level block)
    const model::ForwardPool fp = model::resolve_pool(e->plan, pool);
    const size_t dense_elems = fp.splade ? 0 : (size_t)B * (fp.classify ? e->plan.head_dim[e->plan.classifier] : e->plan.out_dim);
    if (dense_elems) KR_HIP(hipMemcpyAsync(out, e->out, dense_elems * 4, hipMemcpyDefault, st));
    if (tok_elems) KR_HIP(hipMemcpyAsync(out + dense_elems, e->tok_stage, tok_elems * 4, hipMemcpyDefault, st));
    e->lastB = B; e->lastS = S; e->last_stream = st;
    KR_HIP(hipMemcpyAsync(e->h_err, e->d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    if (is_device_pointer(out)) {
        // device output: nothing here waits for the GPU.  The token-id error word (the only thing the host would need) travels to pinned memory
        // behind the forward; it is looked at by the next call on this handle or by kr_encoder_check().
        KR_HIP(hipEventRecord(e->ev_done, st));
        e->pending = true;
        return 0;
    }
    KR_HIP(hipStreamSynchronize(st));   // a host pointer is returned: the caller reads it as soon as we return
    e->pending = false;
    return report_token_error(e, st);
}

// host-staging buffer of the token-level blocks / the SPLADE result: at least `elems` floats
static int grow_tok_stage(Encoder* e, size_t elems) {
    if (elems <= e->tok_stage_elems) return 0;
    KR_HIP(hipStreamSynchronize(e->last_stream));      // an earlier staged copy may still read the old buffer
    if (e->tok_stage) (void)hipFree(e->tok_stage);
    e->tok_stage = nullptr; e->tok_stage_elems = 0;
    KR_HIP(hipMalloc(reinterpret_cast<void**>(&e->tok_stage), elems * 4));
    e->tok_stage_elems = elems;
    return 0;
}
// Where the kernels write what a forward returns beside the dense block — bge-m3's token-level blocks (flags), the [B, vocab] result of KR_POOL_SPLADE (also
// the reduction buffer of its decoder launch) — and how many floats of it wait in e->tok_stage for finish_forward.  A device `out` takes them straight from the
// kernels (0.5 GB at 1024 x 128 x 1024: no second trip through the workspace), a host `out` is staged.  The kernels hold the caller's pointer, so such a forward
// is never replayed from a captured graph.  *target = nullptr: the forward has no such block
static int token_target(Encoder* e, int B, int S, int pool, int flags, float* out, float** target, size_t* staged) {
    const size_t slots = (size_t)B * S;
    const size_t elems = pool == KR_POOL_SPLADE ? (size_t)B * e->cfg.vocab
                                                : ((flags & KR_POOL_WITH_SPARSE) ? slots : 0) + ((flags & KR_POOL_WITH_COLBERT) ? slots * e->plan.head_dim[model::HEAD_COLBERT] : 0);
    *target = nullptr; *staged = 0;
    if (!elems) return 0;
    if (is_device_pointer(out)) { *target = pool == KR_POOL_SPLADE ? out : out + (size_t)B * e->plan.out_dim; return 0; }
    KR_TRY(grow_tok_stage(e, elems));
    *target = e->tok_stage; *staged = elems;
    return 0;
}

int enc_forward(void* h, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* token_type_ids, int B, int S, int pool, float* out, void* stream) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    KR_TRY(check_forward_args(e, B < 0 || S <= 0 || (B > 0 && (!input_ids || !attention_mask || !out)), B, S, -1, pool));
    if (B == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    KR_TRY(begin_forward(e, B, S, st));
    KR_HIP(hipMemcpyAsync(e->d_ids, input_ids, (size_t)B * S * 8, hipMemcpyDefault, st));
    KR_HIP(hipMemcpyAsync(e->d_mask, attention_mask, (size_t)B * S * 8, hipMemcpyDefault, st));
    if (token_type_ids) KR_HIP(hipMemcpyAsync(e->d_tt, token_type_ids, (size_t)B * S * 8, hipMemcpyDefault, st));
    const int flags = pool & M3_FLAGS;
    pool &= ~M3_FLAGS;
    float* target = nullptr; size_t staged = 0;
    KR_TRY(token_target(e, B, S, pool, flags, out, &target, &staged));
    if (target) KR_TRY(enqueue_forward(e, B, S, pool, st, Input{false, token_type_ids != nullptr, 0}, flags, target));
    else KR_TRY(run_forward(e, B, S, pool, st, token_type_ids != nullptr));
    return finish_forward(e, B, S, pool, out, st, staged);
}

// kr_encoder_forward_packed: the same forward from the ragged token list (int32 ids of the attended positions + int32 length per sequence)
int enc_forward_packed(void* h, const int32_t* token_ids, const int32_t* seq_lens, int B, int S, int64_t total_tokens, int pool, float* out, void* stream) {
    Encoder* e = reinterpret_cast<Encoder*>(h);
    KR_TRY(check_forward_args(e, B < 0 || S <= 0 || total_tokens < 0 || (B > 0 && (!seq_lens || !out)) || (total_tokens > 0 && !token_ids), B, S, total_tokens, pool));
    if (B == 0) return 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    KR_TRY(begin_forward(e, B, S, st));
    if (total_tokens > 0) KR_HIP(hipMemcpyAsync(e->rag_ids(), token_ids, (size_t)total_tokens * 4, hipMemcpyDefault, st));
    KR_HIP(hipMemcpyAsync(e->rag_lens(), seq_lens, (size_t)B * 4, hipMemcpyDefault, st));
    float* target = nullptr; size_t staged = 0;      // (check_forward_args: a ragged forward takes no flags)
    KR_TRY(token_target(e, B, S, pool, 0, out, &target, &staged));
    KR_TRY(enqueue_forward(e, B, S, pool, st, Input{true, false, (int)total_tokens}, 0, target));
    return finish_forward(e, B, S, pool, out, st, staged);
}

int enc_check(void* h) {
    if (!h) return fail(KR_EINVAL, "encoder is NULL");
    Encoder* e = reinterpret_cast<Encoder*>(h);
    if (!e->pending) return 0;
    KR_TRY(select_device(e->device));
    KR_HIP(hipEventSynchronize(e->ev_done));
    e->pending = false;
    return report_token_error(e, e->last_stream);
}

// last_hidden_state of the previous forward, un-packed to [B,S,H]; rows of non-attended positions are zero
int enc_last_hidden(void* h, float* out, int B, int S) {
    if (!h || !out) return fail(KR_EINVAL, "NULL argument");
    Encoder* e = reinterpret_cast<Encoder*>(h);
    if (B != e->lastB || S != e->lastS || B == 0) return fail(KR_ESTATE, "no forward of shape [%d,%d] to read back", B, S);
    if (e->last_shortcut)
        return fail(KR_ESTATE, e->plan.family == model::DECODER
                                   ? "the last forward ran the score head: its last layer ran on the last rows only (create the encoder with KIRAG_AMD_CLS_FULL=1 to keep every row)"
                                   : "the last forward pooled the CLS token: its last layer ran on the CLS rows only (create the encoder with KIRAG_AMD_CLS_FULL=1 to keep every row)");
    KR_TRY(select_device(e->device));
    KR_HIP(hipStreamSynchronize(e->last_stream));
    const int H = e->cfg.hidden;
    std::vector<int> off(B), nq(B);
    int T = 0;
    KR_HIP(hipMemcpy(off.data(), e->seq_off, B * 4, hipMemcpyDeviceToHost));
    KR_HIP(hipMemcpy(nq.data(), e->seq_nq, B * 4, hipMemcpyDeviceToHost));
    KR_HIP(hipMemcpy(&T, e->d_T, 4, hipMemcpyDeviceToHost));
    std::vector<int> pos(T);
    std::vector<float> x((size_t)T * H);
    KR_HIP(hipMemcpy(pos.data(), e->tok_pos, (size_t)T * 4, hipMemcpyDeviceToHost));
    {   // the final hidden state is stored as (16-bit hi, 8-bit lo in units of ulp(hi) / 256): see lo_encode
        std::vector<uint16_t> hi((size_t)T * H); std::vector<uint8_t> lo((size_t)T * H);
        KR_HIP(hipMemcpy(hi.data(), e->xb, hi.size() * 2, hipMemcpyDeviceToHost));
        KR_HIP(hipMemcpy(lo.data(), e->xlo, lo.size(), hipMemcpyDeviceToHost));
#ifdef KR_ENC_BUILD_F16
        auto f = [](uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); };
#else
        auto f = [](uint16_t b) { uint32_t u = (uint32_t)b << 16; float v; std::memcpy(&v, &u, 4); return v; };
#endif
        for (size_t i = 0; i < x.size(); ++i) {      // the host twin of lo_decode_final
            const float hf = f(hi[i]);
            uint32_t bits; std::memcpy(&bits, &hf, 4);
            if ((bits & 0x7f800000u) != 0x7f800000u) bits += ((uint32_t)lo[i] << LO_SH) - (128u << LO_SH);
            std::memcpy(&x[i], &bits, 4);
        }
    }
    std::vector<float> full((size_t)B * S * H, 0.f);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < nq[b]; ++i)
            std::memcpy(&full[((size_t)b * S + pos[off[b] + i]) * H], &x[(size_t)(off[b] + i) * H], (size_t)H * 4);
    KR_HIP(hipMemcpy(out, full.data(), full.size() * 4, hipMemcpyDefault));
    return 0;
}

}  // namespace KR_ENC_NS
}  // namespace kr
