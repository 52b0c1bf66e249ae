// BERT-family sentence encoder forward on MI355X — replaces HF BertModel.forward + pooling + F.normalize behind
// retriever/encoders.py (E5Encoder.forward :67-77, BGEEncoder.forward :106-118; retriever/e5.py:51-61).
//
// Layout.  The [B,S] batch is PACKED on the device: only positions with attention_mask != 0 become token rows
// (sequence b owns rows [off_b, off_b + nq_b), off_b % 4 == 0; absolute position ids are kept per token), so the
// projections run on sum(len) rows instead of B*S.  No host round trip: grids are sized for B*(S+4) rows and blocks
// beyond the device-side total exit.  Residual stream = xb, 16-bit (it is also the MFMA operand) + by default xlo, ONE byte per element holding the
// remainder in units of ulp(hi) / 256 (lo_encode: 19 significand bits with f16 operands).  Operand type (f16 default, bf16) and the low half are fixed
// per handle at creation (encoder_api.hip: kr_encoder_create_ex); why the defaults are what they are: DESIGN.md sections 2 and 4.2a (golden set G10:
// with outlier hidden channels two orders above the median (out3) only f16 + low half stays inside the 1e-3 score tolerance with margin: 1.4e-4; on the 5 x harsher
// out16 set it measures 1.0e-3 and its test bar is 1.5e-3).  MFMA operands
// 16-bit (xb, q, k, vT, ctx, h), fp32 accumulation everywhere.
//
// Per layer (post-LN BERT):  ONE GEMM [Wq/8|Wk|Wv] x -> q, k (row-major) and v TRANSPOSED [H, T] (so that attention reads
// V^T fragments contiguously); attention = one block per (sequence, head group) with K and V^T staged once in LDS, swapped QK^T so
// the softmax reductions are in-lane, P^T fed from the accumulator straight into the V^T.P^T MFMA;  Wo ctx + b +
// residual -> LayerNorm;  W1 x + b -> erf-GELU;  W2 h + b + residual -> LayerNorm.  Pooling (masked mean or CLS)
// + L2 normalisation produce out[B,H] fp32.
//
// NomicBert handles (config.rotary_inv_freq, see Encoder::inv_freq): no position table, q and k rotated by the token's column in the QKV epilogue (EPI_QKV_ROT),
// [gate | up] x as one GEMM whose epilogue writes silu(gate) * up (EPI_SWIGLU) in place of W1 x + b -> erf-GELU; everything else as above.
//
// ModernBert handles (config.local_attention_layers, see Encoder::local_layers): a PRE-LN stack on the same launches.  The residual stream r (rb + rlo) is kept
// apart from the normalised operand xb; each of the two LayerNorm launches of a layer is k_ln16_pre: r += y + bias, store r, xb = LN_next(r), LN_next = this
// layer's mlp_norm, then the next layer's attn_norm (final_norm behind the last layer).  Rotary q / k as above with one table per layer type, the MLP
// Wo (erf_gelu(input) * gate) as one [2 FF, H] projection (EPI_GEGLU), and in the layers flagged local a sliding window over the key columns (k_attn_*<.., WIN>).
//
// T5 handles (config.t5_feed_forward, see Encoder::t5_ff): ModernBert's pre-LN schedule with T5LayerNorm (RMS: k_ln16_pre<.., true>), the embedding row straight
// into the residual stream (k_embed_rms), MPNet's relative attention bias in every layer with scores q.k + bias (no 1 / sqrt(d_h): log2(e) alone is folded into
// Wq), no linear bias, the FF wo(relu(wi x)) (EPI_RELU) or wo(gelu_new(wi_0 x) * wi_1 x) (EPI_GEGLU_TANH), and optionally the sentence-transformers Dense head
// behind the pooling ("dense.weight", k_pool_dense: out [B, P]).
//
// Sequence classification (cross-encoder rerankers, KR_POOL_CLASSIFY): BERT / RoBERTa handles with the four "classifier.*" tensors run CLS pooling's forward up
// to the last LayerNorm, then k_pool<.., RAW> (the un-normalised CLS row) and k_cls_head: out [B, L] = Wo . tanh(Wd . x + bd) + bo, raw logits.
// ModernBert handles with "head.dense.*" / "head.norm.*" / "classifier.{weight,bias}" (ModernBertForSequenceClassification): x = the raw CLS row or, with
// config.classifier_pooling = 1, the raw masked mean (the forward of KR_POOL_MEAN), and k_cls_head<.., true>: Wo . LayerNorm(erf_gelu(Wd . x + bd)) + bo.
//
// bge-m3's token-level heads (KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT on BERT / RoBERTa handles with "sparse_linear.*" / "colbert_linear.*"): a flagged forward
// runs its last layer on every row; behind the pooling k_m3_slots maps the [B, S] columns to packed rows, k_m3_sparse writes max(0, w . x + b) per column, and
// the colbert vectors are one more EPI_DENSE projection of the packed rows followed by k_m3_rows (bias, norm, scatter to [b, s], zeros for masked columns).
//
// SPLADE (KR_POOL_SPLADE on BERT handles with the six "cls.predictions.*" tensors of BertForMaskedLM): the stack runs as for mean pooling, then one EPI_GELU
// projection H -> H and k_ln16_head give the transform's rows, and the decoder [Vpad, H] runs on the projection loops with the EPI_SPLADE epilogue
// (encoder_proj.hpp): the max over each sequence's rows lands in the [B, V] output itself by atomicMax, no [T, V] logits exist; k_splade_finish applies log1p.
//
// Files.  This one: the Encoder handle, launch selection, the entry points.  Device code per operand type, included here: encoder_rows.hpp (residual-stream
// codec, embedding, LayerNorm, pooling), encoder_proj.hpp (projections), encoder_attn.hpp (attention).  encoder_pack.hip: the token-packing front end.
#include "encoder_rows.hpp"
#include "encoder_proj.hpp"
#include "encoder_attn.hpp"
#include "encoder_pack.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
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

enum { MH_DW = 1, MH_DB = 2, MH_NW = 4, MH_NB = 8, MH_CW = 16, MH_CB = 32, MH_REQUIRED = MH_DW | MH_NW | MH_CW | MH_CB };

struct Encoder {
    kr_bert_cfg cfg{};
    Knobs kn;
    int device = 0;
    float *word = nullptr, *pos = nullptr, *type = nullptr, *elng = nullptr, *elnb = nullptr;
    std::vector<LayerW> L;
    // every hipMalloc of the handle is recorded where it is made (dmalloc) and freed by walking its list: ws_bufs = the workspace (free_ws), own_bufs = what
    // lives as long as the handle (enc_destroy)
    std::vector<void**> ws_bufs, own_bufs;
    std::vector<uint8_t> got;     // 5 + L_COUNT * layers flags: 0 = never loaded, else the family of the name it was loaded under (FAM_*; enc_finalize: names and handle kind agree)
    bool ready = false;
    float* stage = nullptr; size_t stage_elems = 0;   // fp32 upload staging for load_weight
    // workspace
    int64_t capT = 0; int capB = 0; int64_t capBS = 0; int64_t ldv = 0;
    int64_t *d_ids = nullptr, *d_mask = nullptr, *d_tt = nullptr;   // d_tt: token_type_ids of the batch (only written when the caller passes them)
    // ragged input (kr_encoder_forward_packed) lives in the same three buffers: the int32 token list, the int32 lengths, scratch for the input offsets
    int* rag_ids() const { return reinterpret_cast<int*>(d_ids); }
    int* rag_lens() const { return reinterpret_cast<int*>(d_mask); }
    int* rag_in_off() const { return reinterpret_cast<int*>(d_tt); }
    int *seq_off = nullptr, *seq_nk = nullptr, *seq_nq = nullptr, *seq_cls = nullptr, *seq_has0 = nullptr, *d_T = nullptr, *d_err = nullptr;
    int *tok_id = nullptr, *tok_pos = nullptr, *tok_type = nullptr;
    // position rule of the handle.  pad_idx < 0: BERT's (embedding position = column, tok_pos serves k_embed_ln and the un-packer).  pad_idx = P >= 0: fairseq's
    // (RoBERTa / XLM-R: P + number of ids != P up to and including the column, P itself where the id is P): the packers write that into tok_epos for k_embed_ln
    // and tok_pos keeps the column for the un-packer.  Set through the reserved name "config.position_padding_idx" before the first finalize.
    int pad_idx = -1;
    bool finalized_once = false;
    int *tok_epos = nullptr;
    // relative attention bias (MPNet): loading "encoder.relative_attention_bias.weight" [32 buckets, heads] makes the handle an MPNet handle; like the position
    // rule that is fixed at the first finalize.  rel_w: the tensor as loaded (host); bias_tab: what the attention kernels read (AttnBiasArgs), built by finalize
    std::vector<float> rel_w;
    float* bias_tab = nullptr; int bias_width = 0;
    bool bias_gather = false;  // KIRAG_AMD_ATTN_BIAS_GATHER=1 at kr_encoder_create: key columns always from tok_pos (the path of masks with holes), for tests
    // rotary positions (NomicBert): loading "config.rotary_inv_freq" (d_h / 2 values, HF's rotary_emb.inv_freq) before the first finalize makes the handle a
    // NomicBert handle for life: no position table (the embedding adds pos_zero through tok_zero), q and k rotated in the QKV epilogue by rot_cos / rot_sin
    // [max_pos][d_h / 2] (built by finalize), gate | up as ONE projection with the SwiGLU epilogue, linear biases zero unless loaded
    std::vector<float> inv_freq;
    float *rot_cos = nullptr, *rot_sin = nullptr, *pos_zero = nullptr;
    int *tok_zero = nullptr, *tok_rpos = nullptr;   // tok_rpos: the position each token is rotated by (k_rot_pos)
    bool rotary() const { return !inv_freq.empty(); }
    // ModernBert: loading "config.local_attention_layers" (one 0 / 1 flag per layer: 1 = sliding-window attention) before the first finalize makes the handle a
    // ModernBert handle for life (needs config.rotary_inv_freq too): pre-LN stack, ModernBert's state-dict names, GEGLU.  Local layers rotate by
    // "config.rotary_inv_freq_local" (rot_cos_l / rot_sin_l) and admit key columns within "config.attention_half_window" of the query's.
    std::vector<float> local_layers, inv_freq_local;
    int half_window = 0;
    float *rot_cos_l = nullptr, *rot_sin_l = nullptr;
    bool modern() const { return !local_layers.empty(); }
    bool local_layer(int li) const { return (size_t)li < local_layers.size() && local_layers[li] != 0.f; }
    // T5 (transformers.T5EncoderModel: gtr-t5, sentence-t5, instructor): loading "config.t5_feed_forward" (0 = relu, 1 = gated gelu_new) before the first finalize
    // makes the handle a T5 handle for life.  rel_fam: the family of the name the bias table came under (MPNet's or T5's; enc_finalize: name and kind agree).
    int t5_ff = -1;
    int rel_fam = 0;
    bool t5() const { return t5_ff >= 0; }
    bool pre_ln() const { return modern() || t5(); }
    // "dense.weight" [P, H] fp32 (T5 handles only): the Dense head behind the pooling.  dense_rows = P (0: none); pooled: k_pool's [B, H] rows, the head's input
    float* dense_w = nullptr; int dense_rows = 0;
    float* pooled = nullptr;
    int out_dim() const { return dense_rows > 0 ? dense_rows : cfg.hidden; }
    // "classifier.{dense,out_proj}.{weight,bias}" fp32: the sequence-classification head behind the raw CLS row (KR_POOL_CLASSIFY, k_cls_head).  cls_labels = L,
    // the rows of out_proj (0: none yet); cls_got: one bit per tensor (CLS_*), all four or none at finalize; with it `pooled` holds the head's input
    float *cls_wd = nullptr, *cls_bd = nullptr, *cls_wo = nullptr, *cls_bo = nullptr;
    int cls_labels = 0; unsigned cls_got = 0;
    // ModernBert's head (MH_NAMES, one bit of mh_got each): "head.dense.{weight,bias}" [H, H] / [H], "head.norm.{weight,bias}" [H], "classifier.{weight,bias}"
    // [L, H] / [L]; the two head.*.bias are optional (zero unless loaded), the other four come together or not at all.  mh_labels = L (0: none yet).
    // cls_pooling: "config.classifier_pooling", -1 = never set (the [CLS] row), 0 = the [CLS] row, 1 = the masked mean
    float *mh_wd = nullptr, *mh_bd = nullptr, *mh_g = nullptr, *mh_b = nullptr, *mh_wo = nullptr, *mh_bo = nullptr;
    int mh_labels = 0; unsigned mh_got = 0; int cls_pooling = -1;
    bool has_tanh_head() const { return cls_got == 15u; }
    bool has_modern_head() const { return (mh_got & MH_REQUIRED) == MH_REQUIRED; }
    bool has_head() const { return has_tanh_head() || has_modern_head(); }
    int head_labels() const { return std::max(cls_labels, mh_labels); }    // a finalized handle holds one of the two heads
    int out_width() const { return std::max(out_dim(), head_labels()); }   // what a row of `out` must hold, whatever the pool
    // bge-m3's heads.  "colbert_linear.{weight,bias}": col_w = the 16-bit copy [P, H] the projection loops read, col_b fp32 [P], col_rows = P (0: none yet).
    // "sparse_linear.{weight,bias}": sp_w fp32 [H], sp_b fp32 [1].  *_got: bit 1 = weight, bit 2 = bias; a head is both or nothing at finalize.
    // cy: the colbert product of the packed rows [capT, P] (16-bit, EPI_DENSE); slot_row: packed row of every [b, s] column or -1 (k_m3_slots);
    // tok_stage: the token-level blocks of a forward whose `out` is host memory (grown on demand, freed with the handle)
    uint16_t* col_w = nullptr; float* col_b = nullptr; int col_rows = 0; unsigned col_got = 0;
    float *sp_w = nullptr, *sp_b = nullptr; unsigned sp_got = 0;
    bool has_colbert() const { return col_got == 3u; }
    bool has_sparse() const { return sp_got == 3u; }
    uint16_t* cy = nullptr; int* slot_row = nullptr;
    // SPLADE's MLM head, "cls.predictions.{transform.dense,transform.LayerNorm,decoder}.{weight,bias}" (MLM_NAMES, one bit of mlm_got each; all six or none at
    // finalize).  mlm_wt: the 16-bit copy [H, H]; mlm_wd: the 16-bit copy [Vpad, H] of the decoder, Vpad = vocab rounded up to MLM_COLS by zero rows; mlm_bd fp32
    // [Vpad] (zero behind V); mlm_zero: H zeros (k_ln16_head).  row_seq: the sequence of every packed row or -1 (workspace, k_splade_rowseq)
    uint16_t *mlm_wt = nullptr, *mlm_wd = nullptr; float *mlm_bt = nullptr, *mlm_g = nullptr, *mlm_b = nullptr, *mlm_bd = nullptr, *mlm_zero = nullptr;
    unsigned mlm_got = 0;
    bool has_mlm() const { return mlm_got == 63u; }
    int* row_seq = nullptr;
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
    e->capT = 0; e->capB = 0; e->capBS = 0;
}

static int ensure_ws(Encoder* e, int B, int S) {
    const int64_t maxT = (int64_t)B * (S + 8);
    const int H = e->cfg.hidden, FF = e->cfg.intermediate;
    if (!e->d_T) {
        KR_TRY(dmalloc(e->own_bufs, &e->d_T, sizeof(int))); KR_TRY(dmalloc(e->own_bufs, &e->d_err, sizeof(int)));
        KR_HIP(hipMemset(e->d_err, 0, sizeof(int)));
        KR_HIP(hipHostMalloc(reinterpret_cast<void**>(&e->h_err), sizeof(int), hipHostMallocDefault));
        *e->h_err = 0;
        KR_HIP(hipEventCreateWithFlags(&e->ev_done, hipEventDisableTiming));
    }
    if (maxT <= e->capT && B <= e->capB && (int64_t)B * S <= e->capBS) return 0;
    if (maxT > (int64_t)1 << 24) return fail(KR_EINVAL, "batch of %lld tokens: at most 2^24 per forward (32-bit offsets inside the attention kernels)", (long long)maxT);
    free_ws(e);
    const int64_t capT = round_up(maxT, 256), capB = B, capBS = (int64_t)B * S;   // multiple of the 256-token tile: see k_proj
    KR_TRY(dmalloc(e->ws_bufs, &e->d_ids, capBS * 8)); KR_TRY(dmalloc(e->ws_bufs, &e->d_mask, capBS * 8)); KR_TRY(dmalloc(e->ws_bufs, &e->d_tt, capBS * 8));
    KR_TRY(dmalloc(e->ws_bufs, &e->seq_off, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_nk, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_nq, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_cls, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->seq_has0, capB * 4));
    KR_TRY(dmalloc(e->ws_bufs, &e->tok_id, capT * 4));
    KR_TRY(dmalloc(e->ws_bufs, &e->tok_pos, (capT + 64) * 4));    // 64 entries of slack: the window's gathered key columns are read in whole 64-key steps (attn_window_tile)
    KR_HIP(hipMemset(e->tok_pos, 0, (size_t)(capT + 64) * 4));
    KR_TRY(dmalloc(e->ws_bufs, &e->tok_type, capT * 4));
    if (e->pad_idx >= 0) KR_TRY(dmalloc(e->ws_bufs, &e->tok_epos, capT * 4));
    if (e->rotary()) {
        KR_TRY(dmalloc(e->ws_bufs, &e->tok_zero, capT * 4)); KR_HIP(hipMemset(e->tok_zero, 0, (size_t)capT * 4));
        KR_TRY(dmalloc(e->ws_bufs, &e->tok_rpos, capT * 4)); KR_HIP(hipMemset(e->tok_rpos, 0, (size_t)capT * 4));
    }
    KR_TRY(dmalloc(e->ws_bufs, &e->xlo, capT * H)); KR_TRY(dmalloc(e->ws_bufs, &e->y, capT * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->out, (size_t)capB * e->out_width() * 4));
    if (e->dense_rows > 0 || e->cls_got || e->mh_got) KR_TRY(dmalloc(e->ws_bufs, &e->pooled, (size_t)capB * H * 4));
    if (e->col_got || e->sp_got) KR_TRY(dmalloc(e->ws_bufs, &e->slot_row, capBS * 4));
    if (e->mlm_got) KR_TRY(dmalloc(e->ws_bufs, &e->row_seq, capT * 4));
    if (e->col_rows > 0) KR_TRY(dmalloc(e->ws_bufs, &e->cy, capT * e->col_rows * 2));      // capT rows: the projection's tiles are whole (see k_proj)
    KR_TRY(dmalloc(e->ws_bufs, &e->xb, capT * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->q, capT * H * 2));
    KR_TRY(dmalloc(e->ws_bufs, &e->k, (capT + 64) * H * 2));    // 64 rows of slack: k_attn_dma reads whole 64-key chunks (the rows past a sequence are masked)
    KR_HIP(hipMemset(e->k, 0, (size_t)(capT + 64) * H * 2));
    e->ldv = capT + 64;   // slack: the last key tile of the last sequence may read up to 43 columns past T
    KR_TRY(dmalloc(e->ws_bufs, &e->vT, (size_t)H * e->ldv * 2));
    KR_HIP(hipMemset(e->vT, 0, (size_t)H * e->ldv * 2));
    KR_TRY(dmalloc(e->ws_bufs, &e->ctx, capT * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->h, capT * FF * 2));
    if (e->pre_ln()) {
        KR_TRY(dmalloc(e->ws_bufs, &e->rb, capT * H * 2));
        if (e->use_lo) KR_TRY(dmalloc(e->ws_bufs, &e->rlo, capT * H));
    }
    if (e->cls_shortcut) {
        const int64_t capC = round_up(capB, 256);                 // token-indexed buffers come in multiples of the 256-row tile (see k_proj)
        KR_TRY(dmalloc(e->ws_bufs, &e->c_ctx, capC * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->c_xb, capC * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->c_y, capC * H * 2)); KR_TRY(dmalloc(e->ws_bufs, &e->c_xlo, capC * H));
        KR_TRY(dmalloc(e->ws_bufs, &e->c_h, capC * FF * 2));
        if (e->pre_ln()) {
            KR_TRY(dmalloc(e->ws_bufs, &e->c_rb, capC * H * 2)); KR_HIP(hipMemset(e->c_rb, 0, (size_t)capC * H * 2));
            if (e->use_lo) { KR_TRY(dmalloc(e->ws_bufs, &e->c_rlo, capC * H)); KR_HIP(hipMemset(e->c_rlo, 0x80, (size_t)capC * H)); }
        }
        KR_HIP(hipMemset(e->c_ctx, 0, (size_t)capC * H * 2)); KR_HIP(hipMemset(e->c_xb, 0, (size_t)capC * H * 2)); KR_HIP(hipMemset(e->c_xlo, 0x80, (size_t)capC * H));
        KR_TRY(dmalloc(e->ws_bufs, &e->c_off, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->c_nk, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->c_cls, capB * 4)); KR_TRY(dmalloc(e->ws_bufs, &e->d_B, sizeof(int)));
    }
    e->capT = capT; e->capB = (int)capB; e->capBS = capBS;
    return 0;
}

// tensor slot ids: 0..4 embeddings, then L_COUNT per layer (L_UW: NomicBert's up_proj, the second half of a gated intermediate projection)
enum { T_WORD = 0, T_POS, T_TYPE, T_ELNG, T_ELNB, T_LAYER0 };
constexpr int T_RELBIAS = -2;          // not a slot of `got`: an optional tensor (parse_name)
constexpr int T_WQKV = -3, T_WI = -4, T_WIB = -5, T_WQKVB = -6;   // ModernBert's fused tensors of layer `layer` (parse_name): attn.Wqkv.weight, mlp.Wi.weight, mlp.Wi.bias, attn.Wqkv.bias
enum { FAM_BERT = 1, FAM_NOMIC = 2, FAM_MODERN = 3, FAM_T5 = 4, FAM_T5G = 5 };   // whose state-dict name a tensor came under (FAM_T5G: T5's gated FF, wi_0 / wi_1)
static bool fam_t5(int fam) { return fam == FAM_T5 || fam == FAM_T5G; }
constexpr int REL_BUCKETS = 32;        // HF's MPNetEncoder uses 32 buckets and max_distance 128 whatever the config says
enum { L_QW = 0, L_QB, L_KW, L_KB, L_VW, L_VB, L_OW, L_OB, L_LN1G, L_LN1B, L_IW, L_IB, L_FW, L_FB, L_LN2G, L_LN2B, L_UW, L_COUNT };

// fam: FAM_NOMIC = the name is NomicBertModel's ("layers.N.self_attn.q_proj.weight", ...), FAM_MODERN = ModernBertModel's ("layers.N.attn.Wqkv.weight", ...);
// layer: the layer of a fused ModernBert tensor (slot T_WQKV / T_WI / T_WIB)
static int parse_name(const Encoder* e, const char* name, int& slot, int64_t& numel, int& fam, int& layer) {
    std::string s(name);
    bool nomic = false;
    fam = FAM_BERT; layer = -1;
    size_t p = s.find("embeddings.");
    size_t pl = s.find("encoder.layer.");
    size_t skip = strlen("encoder.layer.");
    if (pl == std::string::npos && (s.compare(0, 7, "layers.") == 0 || s.find(".layers.") != std::string::npos)) {
        pl = s.compare(0, 7, "layers.") == 0 ? 0 : s.find(".layers.") + 1;
        skip = strlen("layers.");
        nomic = true;
    }
    const int64_t H = e->cfg.hidden, FF = e->cfg.intermediate;
    if (s.find("position_ids") != std::string::npos || s.find("pooler.") != std::string::npos) { slot = -1; return 0; }
    auto ends_with = [&](const char* t) { const size_t n = strlen(t); return s.size() >= n && s.compare(s.size() - n, n, t) == 0 && (s.size() == n || s[s.size() - n - 1] == '.'); };
    // T5EncoderModel's names.  The norms sit in ModernBert's places: layer_norm of block N's attention is the norm behind the FF of block N - 1 (the launch that
    // applies it; block 0's: the embedding launch), layer.1.layer_norm the one behind the attention output, final_layer_norm the last one
    // (matched as T5EncoderModel spells them, with or without its "encoder." prefix: another family's tensor that merely contains "block." or ends in
    // "embed_tokens.weight" stays an unknown tensor name at load time)
    if (s == "shared.weight" || s == "encoder.embed_tokens.weight" || s == "embed_tokens.weight") { fam = FAM_T5; slot = T_WORD; numel = (int64_t)e->cfg.vocab * H; return 0; }
    if (s == "encoder.final_layer_norm.weight" || s == "final_layer_norm.weight") { fam = FAM_T5; slot = T_LAYER0 + (e->cfg.layers - 1) * L_COUNT + L_LN2G; numel = H; return 0; }
    if (const size_t pb = s.compare(0, 14, "encoder.block.") == 0 ? 8 : s.compare(0, 6, "block.") == 0 ? 0 : std::string::npos; pb != std::string::npos) {
        const char* c = s.c_str() + pb + strlen("block.");
        char* end = nullptr;
        const long l = strtol(c, &end, 10);
        if (end == c || *end != '.' || l < 0 || l >= e->cfg.layers) return fail(KR_EINVAL, "bad layer index in '%s'", name);
        const std::string r(end + 1);
        struct T5Name { const char* n; int id; };
        static const T5Name t5_tbl[] = {{"layer.0.SelfAttention.q.weight", L_QW}, {"layer.0.SelfAttention.k.weight", L_KW}, {"layer.0.SelfAttention.v.weight", L_VW},
                                        {"layer.0.SelfAttention.o.weight", L_OW}, {"layer.0.layer_norm.weight", L_LN2G}, {"layer.1.layer_norm.weight", L_LN1G},
                                        {"layer.1.DenseReluDense.wi.weight", L_IW}, {"layer.1.DenseReluDense.wi_0.weight", L_IW},
                                        {"layer.1.DenseReluDense.wi_1.weight", L_UW}, {"layer.1.DenseReluDense.wo.weight", L_FW}};
        if (r == "layer.0.SelfAttention.relative_attention_bias.weight") {
            if (l != 0) return fail(KR_EINVAL, "'%s': block 0 holds a T5 encoder's one relative attention bias", name);
            fam = FAM_T5; slot = T_RELBIAS; numel = (int64_t)REL_BUCKETS * e->cfg.heads;
            return 0;
        }
        for (const T5Name& t : t5_tbl)
            if (r == t.n) {
                fam = (t.id == L_UW || r == "layer.1.DenseReluDense.wi_0.weight") ? FAM_T5G : FAM_T5;
                const bool attn_norm = t.id == L_LN2G;
                slot = attn_norm && l == 0 ? (int)T_ELNG : T_LAYER0 + (int)(attn_norm ? l - 1 : l) * L_COUNT + t.id;
                numel = t.id == L_IW || t.id == L_UW || t.id == L_FW ? H * FF : t.id == L_LN1G || t.id == L_LN2G ? H : H * H;
                return 0;
            }
        return fail(KR_EINVAL, "unknown layer tensor '%s'", name);
    }
    // ModernBert: final_norm is the LayerNorm behind the last layer's MLP
    if (ends_with("final_norm.weight") || ends_with("final_norm.bias")) {
        fam = FAM_MODERN; numel = H;
        slot = T_LAYER0 + (e->cfg.layers - 1) * L_COUNT + (ends_with("final_norm.weight") ? L_LN2G : L_LN2B);
        return 0;
    }
    {
        static const char rel[] = "encoder.relative_attention_bias.weight";
        if (s.size() >= sizeof(rel) - 1 && s.compare(s.size() - (sizeof(rel) - 1), sizeof(rel) - 1, rel) == 0) { slot = T_RELBIAS; numel = (int64_t)REL_BUCKETS * e->cfg.heads; return 0; }
    }
    if (pl != std::string::npos) {
        const char* c = s.c_str() + pl + skip;
        char* end = nullptr;
        const long l = strtol(c, &end, 10);
        if (end == c || *end != '.' || l < 0 || l >= e->cfg.layers) return fail(KR_EINVAL, "bad layer index in '%s'", name);
        const std::string r(end + 1);
        // BERT's names (BertModel, RobertaModel, XLMRobertaModel) and MPNet's (MPNetModel: attention.attn.{q,k,v,o}, attention.LayerNorm) for the same slots
        struct NameId { const char* n; int id; };
        static const NameId nomic_tbl[] = {
            {"self_attn.q_proj.weight", L_QW}, {"self_attn.k_proj.weight", L_KW}, {"self_attn.v_proj.weight", L_VW}, {"self_attn.o_proj.weight", L_OW},
            {"post_attention_layernorm.weight", L_LN1G}, {"post_attention_layernorm.bias", L_LN1B}, {"mlp.gate_proj.weight", L_IW}, {"mlp.up_proj.weight", L_UW},
            {"mlp.down_proj.weight", L_FW}, {"post_mlp_layernorm.weight", L_LN2G}, {"post_mlp_layernorm.bias", L_LN2B}};
        static const NameId bert_tbl[] = {
            {"attention.attn.q.weight", L_QW}, {"attention.attn.q.bias", L_QB}, {"attention.attn.k.weight", L_KW}, {"attention.attn.k.bias", L_KB},
            {"attention.attn.v.weight", L_VW}, {"attention.attn.v.bias", L_VB}, {"attention.attn.o.weight", L_OW}, {"attention.attn.o.bias", L_OB},
            {"attention.LayerNorm.weight", L_LN1G}, {"attention.LayerNorm.bias", L_LN1B},
            {"attention.self.query.weight", L_QW}, {"attention.self.query.bias", L_QB}, {"attention.self.key.weight", L_KW},
            {"attention.self.key.bias", L_KB}, {"attention.self.value.weight", L_VW}, {"attention.self.value.bias", L_VB},
            {"attention.output.dense.weight", L_OW}, {"attention.output.dense.bias", L_OB},
            {"attention.output.LayerNorm.weight", L_LN1G}, {"attention.output.LayerNorm.bias", L_LN1B},
            {"intermediate.dense.weight", L_IW}, {"intermediate.dense.bias", L_IB}, {"output.dense.weight", L_FW}, {"output.dense.bias", L_FB},
            {"output.LayerNorm.weight", L_LN2G}, {"output.LayerNorm.bias", L_LN2B}};
        if (nomic) {
            // ModernBert's names first.  The fused tensors have slots of their own; attn_norm of layer N is the LayerNorm behind the MLP of layer N - 1 (the
            // launch that applies it), mlp_norm the one behind the attention output
            static const NameId modern_tbl[] = {{"attn.Wqkv.weight", T_WQKV}, {"attn.Wqkv.bias", T_WQKVB}, {"mlp.Wi.weight", T_WI}, {"mlp.Wi.bias", T_WIB},
                                                {"attn.Wo.weight", L_OW}, {"attn.Wo.bias", L_OB}, {"mlp_norm.weight", L_LN1G}, {"mlp_norm.bias", L_LN1B},
                                                {"mlp.Wo.weight", L_FW}, {"mlp.Wo.bias", L_FB}, {"attn_norm.weight", L_LN2G}, {"attn_norm.bias", L_LN2B}};
            for (const NameId& t : modern_tbl)
                if (r == t.n) {
                    fam = FAM_MODERN; layer = (int)l;
                    const bool attn_norm = t.id == L_LN2G || t.id == L_LN2B;
                    if (attn_norm && l == 0) return fail(KR_EINVAL, "'%s': attn_norm of layer 0 is the identity in ModernBert", name);
                    slot = t.id < 0 ? t.id : T_LAYER0 + (int)(attn_norm ? l - 1 : l) * L_COUNT + t.id;
                    numel = t.id == T_WQKV ? 3 * H * H : t.id == T_WQKVB ? 3 * H : t.id == T_WI ? 2 * H * FF : t.id == T_WIB ? 2 * FF : t.id == L_OW ? H * H
                          : t.id == L_FW ? H * FF : H;
                    return 0;
                }
            fam = FAM_NOMIC;
        }
        const NameId* tbl = nomic ? nomic_tbl : bert_tbl;
        const size_t tbl_n = nomic ? sizeof(nomic_tbl) / sizeof(nomic_tbl[0]) : sizeof(bert_tbl) / sizeof(bert_tbl[0]);
        for (size_t ti = 0; ti < tbl_n; ++ti)
            if (const NameId& t = tbl[ti]; r == t.n) {
                slot = T_LAYER0 + (int)l * L_COUNT + t.id;
                switch (t.id) {
                    case L_QW: case L_KW: case L_VW: case L_OW: numel = H * H; break;
                    case L_IW: case L_FW: case L_UW: numel = H * FF; break;
                    case L_IB: numel = FF; break;
                    default: numel = H;
                }
                return 0;
            }
        return fail(KR_EINVAL, "unknown layer tensor '%s'", name);
    }
    if (p != std::string::npos) {
        const std::string r = s.substr(p + strlen("embeddings."));
        if (r == "tok_embeddings.weight") { fam = FAM_MODERN; slot = T_WORD; numel = (int64_t)e->cfg.vocab * H; return 0; }
        if (r == "norm.weight") { fam = FAM_MODERN; slot = T_ELNG; numel = H; return 0; }
        if (r == "norm.bias") { fam = FAM_MODERN; slot = T_ELNB; numel = H; return 0; }
        if (r == "word_embeddings.weight") { slot = T_WORD; numel = (int64_t)e->cfg.vocab * H; return 0; }
        if (r == "position_embeddings.weight") { slot = T_POS; numel = (int64_t)e->cfg.max_pos * H; return 0; }
        if (r == "token_type_embeddings.weight") { slot = T_TYPE; numel = (int64_t)e->cfg.type_vocab * H; return 0; }
        if (r == "LayerNorm.weight") { slot = T_ELNG; numel = H; return 0; }
        if (r == "LayerNorm.bias") { slot = T_ELNB; numel = H; return 0; }
    }
    return fail(KR_EINVAL, "unknown tensor name '%s'", name);
}

static AttnBiasArgs bias_args(const Encoder* e) { return AttnBiasArgs{e->bias_tab, e->tok_pos, e->bias_width, e->bias_gather ? 1 : 0}; }
static AttnWinArgs win_args(const Encoder* e) { return AttnWinArgs{e->tok_pos, e->half_window, e->bias_gather ? 1 : 0}; }
// AM, the attention of a layer: 0 plain, 1 with the relative attention bias (MPNet handles), 2 under the sliding window (local layers of ModernBert handles)
enum { AM_PLAIN = 0, AM_BIAS = 1, AM_WIN = 2 };
template <int AM>
static AttnBiasArg<AM == AM_BIAS, AM == AM_WIN> attn_mode_args(const Encoder* e) {
    if constexpr (AM == AM_BIAS) return bias_args(e);
    else if constexpr (AM == AM_WIN) return win_args(e);
    else return AttnNoBiasArgs{};
}

template <int DH, int HPB, int AM>
static int launch_attn(const Encoder* e, int B, int cap, int nqt, hipStream_t st) {
    const int H = e->cfg.hidden, heads = e->cfg.heads;
    // keys staged at a time: K kchunk x 2 DH B + V^T DH x (2 kchunk + 8) B per head, plus 4 O tiles of 32 x 2 DH B.  DH = 64: 49-50 KiB per block for any
    // (S, HPB), 3 blocks per CU; DH = 32: 24-25 KiB, 4 blocks per CU (attn_lds_blocks: the registers, not the LDS, bound it)
    const int kchunk = cap < 128 ? cap : 128;
    const int lds = HPB * (kchunk * 2 * DH + DH * (kchunk * 2 + 8)) + 4 * 32 * 2 * DH;
    constexpr bool BIAS = AM == AM_BIAS, WIN = AM == AM_WIN;
    static int attr_lds_dev[64] = {};   // per device: function attributes belong to the device's code object instance (one per instantiation of this function)
    int& attr_lds = attr_lds_dev[e->device & 63];
    if (lds > attr_lds) {
        KR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_attn_lds<DH, HPB, BIAS, WIN>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        attr_lds = lds;
    }
    const int qgroups = (nqt + (4 / HPB) - 1) / (4 / HPB);   // blocks per (sequence, head group): 4 / HPB q-tiles each
    const auto ba = attn_mode_args<AM>(e);
    hipLaunchKernelGGL((k_attn_lds<DH, HPB, BIAS, WIN>), dim3((unsigned)((heads + HPB - 1) / HPB), (unsigned)B, (unsigned)qgroups), dim3(256), lds, st, e->q, e->k, e->vT,
                       e->ldv, e->seq_off, e->seq_nk, e->seq_nq, H, heads, kchunk, e->ctx, ba);
    return 0;
}

template <int DH, int AM>
static int launch_attn_dma(const Encoder* e, int B, int nqt, hipStream_t st) {
    const int qgroups = (nqt + ADMA_QT - 1) / ADMA_QT;       // blocks per (sequence, head): 8 q-tiles each
    const int64_t pairs = (int64_t)B * e->cfg.heads;
    const int64_t blocks = (pairs + 7) / 8 * 8 * qgroups;    // whole groups of 8 pairs (see k_attn_dma)
    const auto ba = attn_mode_args<AM>(e);
    hipLaunchKernelGGL((k_attn_dma<DH, AM == AM_BIAS, AM == AM_WIN>), dim3((unsigned)blocks), dim3(ADMA_THREADS), AdmaGeom<DH>::LDS, st, e->q, e->k, e->vT, e->ldv,
                       e->seq_off, e->seq_nk, e->seq_nq, e->cfg.hidden, e->capT, e->ctx, e->cfg.heads, B, qgroups, ba);
    return 0;
}

// the attention of one layer: the LDS-DMA ring for long sequences, else the register-staged kernel with 1 / 2 / 4 heads per block by q-tiles per sequence
template <int DH, int AM>
static int launch_attention(const Encoder* e, int B, int cap, int nqt, bool long_seq, hipStream_t st) {
    if (long_seq) return launch_attn_dma<DH, AM>(e, B, nqt, st);
    if (nqt >= 3) return launch_attn<DH, 1, AM>(e, B, cap, nqt, st);
    if (nqt == 2) return launch_attn<DH, 2, AM>(e, B, cap, nqt, st);
    return launch_attn<DH, 4, AM>(e, B, cap, nqt, st);
}

static int set_lds_once(const void* kern, int lds, int device);
template <class Shape, int STAGES, bool NT>
static int launch_proj_shape_nt(int epi, const ProjArgs& a, int blocks, int device, hipStream_t st) {
    constexpr int lds = STAGES * Shape::STAGE_BYTES + Shape::NWAVE * EPI_STAGE_BYTES;   // 160 KiB for the 256x256 tile: the whole LDS of a CU
    // function attributes belong to the device's code-object instance: once per (kernel, device)
    auto go = [&](auto kern) -> int {
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(kern), lds, device));
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(Shape::NTHREADS), lds, st, a);
        return 0;
    };
    const bool ant = a.ant && Shape::BM == 256;   // the non-temporal activation operand exists for the ping-pong loop only
    switch (epi) {
        case EPI_QKV: return go(&k_proj<EPI_QKV, Shape, STAGES, NT>);
        case EPI_DENSE: return ant ? go(&k_proj<EPI_DENSE, Shape, STAGES, NT, true>) : go(&k_proj<EPI_DENSE, Shape, STAGES, NT>);
        case EPI_GELU: return go(&k_proj<EPI_GELU, Shape, STAGES, NT>);
        case EPI_QKV_ROT: return go(&k_proj<EPI_QKV_ROT, Shape, STAGES, NT>);
        case EPI_QKV_ROTB:      // not on the 256 x 256 tile (launch_proj): the bias quads next to its 128 accumulators spill
            if constexpr (Shape::BM == 256) return fail(KR_EINVAL, "projection epilogue %d is not built for the 256 x 256 tile", epi);
            else return go(&k_proj<EPI_QKV_ROTB, Shape, STAGES, NT>);
        case EPI_SWIGLU: return go(&k_proj<EPI_SWIGLU, Shape, STAGES, NT>);
        case EPI_GEGLU: return go(&k_proj<EPI_GEGLU, Shape, STAGES, NT>);
        case EPI_RELU: return go(&k_proj<EPI_RELU, Shape, STAGES, NT>);
        case EPI_GEGLU_TANH: return go(&k_proj<EPI_GEGLU_TANH, Shape, STAGES, NT>);
        case EPI_SPLADE:        // stores no rows: one instantiation per shape (launch_proj clears nt)
            if constexpr (NT) return fail(KR_EINVAL, "projection epilogue %d has no non-temporal stores", epi);
            else return go(&k_proj<EPI_SPLADE, Shape, STAGES, false>);
        default: return fail(KR_EINVAL, "projection epilogue %d is not built into this library", epi);
    }
}
template <class Shape, int STAGES>
static int launch_proj_shape(int epi, const ProjArgs& a, int blocks, int device, hipStream_t st) {
    return a.nt ? launch_proj_shape_nt<Shape, STAGES, true>(epi, a, blocks, device, st) : launch_proj_shape_nt<Shape, STAGES, false>(epi, a, blocks, device, st);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel, device), safe against concurrent first launches from several host threads (a query
// encoder and a corpus encoder on one device: ADVICE r04) and with the outcome cached, so that a failing attribute is reported by every launch
static int set_lds_once(const void* kern, int lds, int device) {
    struct Ent { const void* k; int dev; hipError_t rc; };
    static std::mutex mu;
    static std::vector<Ent> done;
    std::lock_guard<std::mutex> lock(mu);
    for (const Ent& x : done)
        if (x.k == kern && x.dev == device) { if (x.rc != hipSuccess) return fail(KR_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(x.rc)); return 0; }
    const hipError_t rc = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    done.push_back({kern, device, rc});
    if (rc != hipSuccess) return fail(KR_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(rc));
    return 0;
}

// tile shape per launch: when the 256x256 tiling has fewer tiles than ~5/8 of the CUs (small batches: the reference's per_gpu_batch_size 4-8, the KiRAG
// loop's triple batches, a 1/8 slice of a query batch) the 128x128 tiling gives 4x the parallelism at a quarter of the per-tile latency
static int launch_proj(int epi, const ProjArgs& a_in, int64_t max_tokens, const Encoder* e, hipStream_t st) {
    const Knobs& kn = e->kn;
    const int num_cu = e->num_cu, device = e->device;
    ProjArgs a = a_in;
    if (a.ldx == 0) a.ldx = a.K;
    if (a.ldo == 0) a.ldo = a.F;
    a.pw = kn.pw;
    a.epi_prio = kn.epi_prio;
    // store policy by output size (see ProjArgs::nt)
    a.nt = epi != EPI_SPLADE && max_tokens * (int64_t)(epi_gated(epi) ? a.F / 2 : a.F) * 2 > ((int64_t)96 << 20) ? 1 : 0;
    // FF2 (K = FF > H): its activation operand h is a once-through stream four times the size of every other activation (256 MiB at 32 k tokens); loaded
    // non-temporally it leaves the L2 / Infinity Cache to the weights and to the residual stream the LayerNorm behind it reads: -0.7 % forward time at
    // 1000 x 32 tokens, neutral elsewhere (profiles/r04/tried_nt_activations.txt; outputs bit-identical).
    a.ant = a.K > a.H ? 1 : 0;
    const int64_t big_tiles = ((max_tokens + 255) / 256) * ((a.F + 255) / 256);
    const int64_t small_tiles = ((max_tokens + 127) / 128) * ((a.F + 127) / 128);
    const int force = kn.force_tile;
    const bool small = force == 128 || (force != 256 && big_tiles * 8 < (int64_t)num_cu * 5) || epi == EPI_QKV_ROTB;   // measured crossover: ~5/8 of the CUs busy with 256x256 tiles
    // a handful of token rows: the skinny loop, one tile per block (latency chain: the operand stream of the launch spread over as many CUs as it has
    // tiles).  32 x 32 tiles while there is at most one per CU, 64 x 64 (four multiplying waves share every staged K-tile: half the L2 -> LDS bytes per
    // output element) up to four 32 x 32 tiles' worth per CU — the crossover against the 128x128 producer / consumer loop measured in round 1.
    // KIRAG_AMD_PROJ_TILE = 32 / 64 forces one of the two.
    const int64_t skinny_tiles = ((max_tokens + 31) / 32) * (a.F / 32);
    if (force == 32 || force == 64 || (force == 0 && skinny_tiles <= 4 * (int64_t)num_cu && (max_tokens + 31) / 32 <= 65535)) {
        const bool one = force == 32 || (force == 0 && skinny_tiles <= num_cu);
        auto launch = [&](auto shape_tag, auto kern) -> int {
            constexpr int WM = decltype(shape_tag)::value, RING = WM == 1 ? 16 : 8;
            using G = SkinnyGeom<WM, WM>;
            constexpr int lds = RING * G::STAGE;
            const dim3 grid((unsigned)(a.F / (32 * WM)), (unsigned)((max_tokens + 32 * WM - 1) / (32 * WM)));
            KR_TRY(set_lds_once(reinterpret_cast<const void*>(kern), lds, device));
            hipLaunchKernelGGL(kern, grid, dim3(G::THREADS), lds, st, a);
            return 0;
        };
        auto pick = [&](auto shape_tag) -> int {
            constexpr int WM = decltype(shape_tag)::value, RING = WM == 1 ? 16 : 8;
            switch (epi) {
                case EPI_QKV: return launch(shape_tag, &k_proj_skinny<EPI_QKV, RING, WM, WM>);
                case EPI_DENSE: return launch(shape_tag, &k_proj_skinny<EPI_DENSE, RING, WM, WM>);
                case EPI_GELU: return launch(shape_tag, &k_proj_skinny<EPI_GELU, RING, WM, WM>);
                case EPI_QKV_ROT: return launch(shape_tag, &k_proj_skinny<EPI_QKV_ROT, RING, WM, WM>);
                case EPI_QKV_ROTB: return launch(shape_tag, &k_proj_skinny<EPI_QKV_ROTB, RING, WM, WM>);
                case EPI_SWIGLU: return launch(shape_tag, &k_proj_skinny<EPI_SWIGLU, RING, WM, WM>);
                case EPI_GEGLU: return launch(shape_tag, &k_proj_skinny<EPI_GEGLU, RING, WM, WM>);
                case EPI_RELU: return launch(shape_tag, &k_proj_skinny<EPI_RELU, RING, WM, WM>);
                case EPI_GEGLU_TANH: return launch(shape_tag, &k_proj_skinny<EPI_GEGLU_TANH, RING, WM, WM>);
                case EPI_SPLADE: return launch(shape_tag, &k_proj_skinny<EPI_SPLADE, RING, WM, WM>);
                default: return fail(KR_EINVAL, "projection epilogue %d is not built into this library", epi);
            }
        };
        return one ? pick(std::integral_constant<int, 1>{}) : pick(std::integral_constant<int, 2>{});
    }
    if (!small) return launch_proj_shape<ShapeBig, 2>(epi, a, num_cu, device, st);
    // producer/consumer loop (one persistent block per CU): at most one tile per CU, or more than two (measured: 600 tiles -7 % vs the streaming loop
    // with two blocks per CU; between one and two tiles per CU the two co-resident streaming blocks quantise better).  130 forces it, 128 the streaming loop
    if (((small_tiles <= num_cu || small_tiles > 2 * num_cu) && force != 128) || force == 130) {
        constexpr int lds = SPLIT_RING * ShapeSplit::STAGE_BYTES + 4 * EPI_STAGE_BYTES;
        auto go = [&](auto kern) -> int {
            KR_TRY(set_lds_once(reinterpret_cast<const void*>(kern), lds, device));
            hipLaunchKernelGGL(kern, dim3(num_cu), dim3(SPLIT_THREADS), lds, st, a);
            return 0;
        };
        switch (epi) {
            case EPI_QKV: return go(&k_proj_split<EPI_QKV>);
            case EPI_DENSE: return go(&k_proj_split<EPI_DENSE>);
            case EPI_GELU: return go(&k_proj_split<EPI_GELU>);
            case EPI_QKV_ROT: return go(&k_proj_split<EPI_QKV_ROT>);
            case EPI_QKV_ROTB: return go(&k_proj_split<EPI_QKV_ROTB>);
            case EPI_SWIGLU: return go(&k_proj_split<EPI_SWIGLU>);
            case EPI_GEGLU: return go(&k_proj_split<EPI_GEGLU>);
            case EPI_RELU: return go(&k_proj_split<EPI_RELU>);
            case EPI_GEGLU_TANH: return go(&k_proj_split<EPI_GEGLU_TANH>);
            case EPI_SPLADE: return go(&k_proj_split<EPI_SPLADE>);
            default: return fail(KR_EINVAL, "projection epilogue %d is not built into this library", epi);
        }
    }
    return launch_proj_shape<ShapeSmall, 2>(epi, a, 2 * num_cu, device, st);
}

// ---------------------------------------------------------------------------------------------------------
// entry points of this operand type (C linkage lives in encoder_api.hip, which dispatches on the handle's type)
// ---------------------------------------------------------------------------------------------------------
void enc_destroy(void* h);

int enc_create(const kr_bert_cfg* cfg, int device, int residual_lo, void** out) {
    if (!out || !cfg) return fail(KR_EINVAL, "NULL argument");
    *out = nullptr;
    if (cfg->hidden <= 0 || cfg->hidden % 128 != 0 || cfg->hidden > 2048) return fail(KR_EINVAL, "hidden=%d unsupported (multiple of 128, <= 2048)", cfg->hidden);
    if (cfg->heads <= 0 || (cfg->hidden != cfg->heads * 64 && cfg->hidden != cfg->heads * 32))
        return fail(KR_EINVAL, "hidden/heads must be 32 or 64 (got %d/%d)", cfg->hidden, cfg->heads);
    if (cfg->intermediate <= 0 || cfg->intermediate % 128 != 0) return fail(KR_EINVAL, "intermediate=%d must be a multiple of 128", cfg->intermediate);
    if (cfg->layers <= 0 || cfg->vocab <= 0 || cfg->max_pos <= 0 || cfg->type_vocab <= 0) return fail(KR_EINVAL, "bad BERT config");
    KR_TRY(select_device(device));
    Encoder* e = new Encoder();
    e->cfg = *cfg; e->device = device;
    e->use_lo = residual_lo != 0;
    { const char* v = getenv("KIRAG_AMD_CLS_FULL"); e->cls_shortcut = !(v && atoi(v) != 0); }
    { const char* v = getenv("KIRAG_AMD_ATTN_BIAS_GATHER"); e->bias_gather = v && atoi(v) != 0; }
    { const char* v = getenv("KIRAG_AMD_GRAPH"); e->graphs_off = !(v && atoi(v) != 0); }   // opt-in: measured SLOWER than eager launches on ROCm 7.2 (see run_forward)
    { hipDeviceProp_t p; if (hipGetDeviceProperties(&p, device) == hipSuccess && p.multiProcessorCount > 0) e->num_cu = (p.multiProcessorCount / 8) * 8; }
    e->num_cu_all = e->num_cu;
    e->L.resize(cfg->layers);
    e->got.assign(T_LAYER0 + (size_t)cfg->layers * L_COUNT, 0);
    const size_t H = cfg->hidden, FF = cfg->intermediate;
    int rc = 0;
    auto A = [&](auto** p, size_t bytes) { if (!rc) rc = dmalloc(e->own_bufs, p, bytes); };
    A(&e->word, (size_t)cfg->vocab * H * 4); A(&e->type, (size_t)cfg->type_vocab * H * 4);
    A(&e->elng, H * 4); A(&e->elnb, H * 4);
    // the position table and every layer's w1 are allocated by their first tensor (enc_load_weight): a NomicBert handle has no table, and its w1 is [2 FF, H]
    for (auto& l : e->L) {
        A(&l.wqkv, 3 * H * H * 2); A(&l.wo, H * H * 2); A(&l.w2, H * FF * 2);
        A(&l.bqkv, 3 * H * 4); A(&l.bo, H * 4); A(&l.bo_eff, H * 4); A(&l.b1, FF * 4); A(&l.b2, H * 4);
        A(&l.ln1g, H * 4); A(&l.ln1b, H * 4); A(&l.ln2g, H * 4); A(&l.ln2b, H * 4);
    }
    if (rc) { enc_destroy(e); return rc; }
    *out = e;
    return 0;
}

void enc_destroy(void* h) {
    if (!h) return;
    Encoder* e = reinterpret_cast<Encoder*>(h);
    (void)hipSetDevice(e->device);
    free_ws(e);
    if (e->h_err) (void)hipHostFree(e->h_err);
    if (e->ev_done) (void)hipEventDestroy(e->ev_done);
    if (e->ev_in) (void)hipEventDestroy(e->ev_in);
    if (e->ev_out) (void)hipEventDestroy(e->ev_out);
    if (e->gstream) (void)hipStreamDestroy(e->gstream);
    if (e->stage) (void)hipFree(e->stage);
    if (e->tok_stage) (void)hipFree(e->tok_stage);
    free_bufs(e->own_bufs);
    delete e;
}

// Settings of the handle travel through the name-addressed loader under the reserved prefix "config." (no tensor of an HF state dict starts with it).
// config.position_padding_idx = P (one float holding an integer, 0 <= P <= max_pos - 2): fairseq's position rule.  Accepted before the first finalize; later
// the same value is a no-op and any other is refused (the workspace and the meaning of every embedding depend on it).
// config.rotary_inv_freq = d_h / 2 values (HF's rotary_emb.inv_freq): rotary positions, a NomicBert handle (Encoder::inv_freq).  The same rule: before the first
// finalize; later the same values are a no-op, anything else is refused.
static int set_rotary(Encoder* e, const float* data, int64_t numel) {
    const int half = e->cfg.hidden / e->cfg.heads / 2;
    if (numel != half) return fail(KR_EINVAL, "config.rotary_inv_freq takes d_h / 2 = %d values, got %lld", half, (long long)numel);
    if (e->cfg.max_pos > 8192) return fail(KR_EINVAL, "config.rotary_inv_freq: max_position_embeddings = %d, rotary tables are built for at most 8192", e->cfg.max_pos);
    std::vector<float> v((size_t)half);
    KR_HIP(hipMemcpy(v.data(), data, (size_t)half * 4, hipMemcpyDefault));
    for (float x : v) if (!std::isfinite(x)) return fail(KR_EINVAL, "config.rotary_inv_freq holds a non-finite value");
    if (e->finalized_once) {
        if (!e->rotary())
            return fail(KR_EINVAL, "config.rotary_inv_freq after kr_encoder_finalize: the handle was finalized without rotary positions and stays a BERT / RoBERTa / MPNet handle");
        if (std::memcmp(v.data(), e->inv_freq.data(), (size_t)half * 4) != 0)
            return fail(KR_EINVAL, "config.rotary_inv_freq with other values after kr_encoder_finalize: the handle's rotary frequencies are fixed");
        return 0;
    }
    e->inv_freq.swap(v);
    e->ready = false;
    return 0;
}

// The settings of a ModernBert handle (kirag_amd.h).  They are only stored here — what they must add up to is enc_finalize's business — under the rule of the
// other two: before the first finalize; later the same values are a no-op and anything else is refused.
static int set_modern(Encoder* e, const char* name, std::vector<float>& dst, const float* data, int64_t numel) {
    if (numel < 1 || numel > 4096) return fail(KR_EINVAL, "'%s': %lld values", name, (long long)numel);
    std::vector<float> v((size_t)numel);
    KR_HIP(hipMemcpy(v.data(), data, (size_t)numel * 4, hipMemcpyDefault));
    for (float x : v) if (!std::isfinite(x)) return fail(KR_EINVAL, "'%s' holds a non-finite value", name);
    if (e->finalized_once) {
        if (v.size() == dst.size() && std::memcmp(v.data(), dst.data(), v.size() * 4) == 0) return 0;
        return fail(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle's kind and its attention settings are fixed at the first finalize", name);
    }
    dst.swap(v);
    e->ready = false;
    return 0;
}

static int set_config(Encoder* e, const char* name, const float* data, int64_t numel) {
    if (std::strcmp(name, "config.rotary_inv_freq") == 0) return set_rotary(e, data, numel);
    if (std::strcmp(name, "config.local_attention_layers") == 0) {
        std::vector<float> v = e->local_layers;
        KR_TRY(set_modern(e, name, v, data, numel));
        for (float x : v) if (x != 0.f && x != 1.f) return fail(KR_EINVAL, "'%s' takes one 0 / 1 flag per layer, got %g", name, (double)x);
        e->local_layers.swap(v);
        return 0;
    }
    if (std::strcmp(name, "config.rotary_inv_freq_local") == 0) {
        const int half = e->cfg.hidden / e->cfg.heads / 2;
        if (numel != half) return fail(KR_EINVAL, "%s takes d_h / 2 = %d values, got %lld", name, half, (long long)numel);
        return set_modern(e, name, e->inv_freq_local, data, numel);
    }
    if (std::strcmp(name, "config.attention_half_window") == 0) {
        if (numel != 1) return fail(KR_EINVAL, "'%s' takes one value, got %lld", name, (long long)numel);
        std::vector<float> v;
        if (e->half_window > 0) v.push_back((float)e->half_window);
        KR_TRY(set_modern(e, name, v, data, numel));
        if (!(v[0] >= 1.f && v[0] <= 65536.f) || v[0] != (float)(int)v[0]) return fail(KR_EINVAL, "%s = %g: expected an integer >= 1", name, (double)v[0]);
        e->half_window = (int)v[0];
        return 0;
    }
    if (std::strcmp(name, "config.t5_feed_forward") == 0) {
        // 0 = wo(relu(wi x)), 1 = wo(gelu_new(wi_0 x) * wi_1 x): makes the handle a T5 handle, under the rule of the other settings
        if (numel != 1) return fail(KR_EINVAL, "'%s' takes one value, got %lld", name, (long long)numel);
        float v = -1.f;
        KR_HIP(hipMemcpy(&v, data, sizeof(float), hipMemcpyDefault));
        if (v != 0.f && v != 1.f) return fail(KR_EINVAL, "%s = %g: expected 0 (relu) or 1 (gated gelu_new)", name, (double)v);
        if (e->finalized_once) {
            if ((int)v == e->t5_ff) return 0;
            return fail(KR_EINVAL, e->t5() ? "%s = %d after kr_encoder_finalize: the handle's feed-forward kind is fixed (it has %d)"
                                           : "%s = %d after kr_encoder_finalize: the handle was finalized without it and stays what it is (%d = not a T5 handle)",
                        name, (int)v, e->t5_ff);
        }
        e->t5_ff = (int)v;
        e->ready = false;
        return 0;
    }
    if (std::strcmp(name, "config.classifier_pooling") == 0) {
        // the row ModernBert's classification head reads: 0 = the [CLS] row (the default), 1 = the masked mean.  Under the rule of the other settings; that the
        // handle is a ModernBert handle with that head is enc_finalize's business
        if (numel != 1) return fail(KR_EINVAL, "'%s' takes one value, got %lld", name, (long long)numel);
        float v = -1.f;
        KR_HIP(hipMemcpy(&v, data, sizeof(float), hipMemcpyDefault));
        if (v != 0.f && v != 1.f) return fail(KR_EINVAL, "%s = %g: expected 0 ([CLS] row) or 1 (masked mean)", name, (double)v);
        if (e->finalized_once) {
            if (!e->has_modern_head())
                return fail(KR_EINVAL, "%s after kr_encoder_finalize: the handle was finalized without ModernBert's classification head (head.dense / head.norm / classifier)", name);
            if ((int)v == std::max(e->cls_pooling, 0)) return 0;
            return fail(KR_EINVAL, "%s = %d after kr_encoder_finalize: the row the classification head reads is fixed (it has %d)", name, (int)v, std::max(e->cls_pooling, 0));
        }
        e->cls_pooling = (int)v;
        e->ready = false;
        return 0;
    }
    if (std::strcmp(name, "config.position_padding_idx") != 0)
        return fail(KR_EINVAL, "unknown setting '%s' (known: config.position_padding_idx, config.rotary_inv_freq, config.rotary_inv_freq_local, "
                               "config.attention_half_window, config.local_attention_layers, config.t5_feed_forward, config.classifier_pooling)", name);
    if (numel != 1) return fail(KR_EINVAL, "'%s' takes one value, got %lld", name, (long long)numel);
    float v = 0.f;
    KR_HIP(hipMemcpy(&v, data, sizeof(float), hipMemcpyDefault));
    if (!(v >= 0.f && v <= (float)(e->cfg.max_pos - 2)) || v != (float)(int)v)
        return fail(KR_EINVAL, "config.position_padding_idx = %g: expected an integer in [0, max_position_embeddings - 2 = %d]", (double)v, e->cfg.max_pos - 2);
    if (e->finalized_once) {
        if ((int)v == e->pad_idx) return 0;
        return fail(KR_EINVAL, "config.position_padding_idx = %d after kr_encoder_finalize: the handle's position rule is fixed (it has %d; -1 = BERT's rule)", (int)v, e->pad_idx);
    }
    e->pad_idx = (int)v;
    return 0;
}

// MPNet's bucket of a column difference d = col_key - col_query (MPNetEncoder.relative_position_bucket with its fixed 32 buckets / max_distance 128, whose
// float32 log this integer rule reproduces for every |d| <= 8200): n = |d|; n < 8: n, else min(15, 8 + max{j >= 0 : 64 * 2^j <= n^2}); + 16 when d > 0
static int rel_bucket(int d) {
    const int64_t n = d < 0 ? -(int64_t)d : d;
    int b = (int)n;
    if (n >= 8) {
        b = 8;
        while (b < 15 && (int64_t)128 << (b - 8) <= n * n) ++b;
    }
    return b + (d > 0 ? 16 : 0);
}

// encoder.relative_attention_bias.weight [32, heads].  Before the first finalize it makes the handle an MPNet handle; afterwards a handle that has it takes
// new values (the weight sync reloads every parameter) and a handle finalized without it refuses it.
static int load_rel_bias(Encoder* e, const char* name, const float* data, int64_t numel, int64_t want, int fam) {
    if (numel != want)
        return fail(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld (%d buckets x %d heads: MPNet always uses %d buckets, and so do the T5 handles)", name,
                    (long long)numel, (long long)want, REL_BUCKETS, e->cfg.heads, REL_BUCKETS);
    if (e->finalized_once && e->rel_w.empty())
        return fail(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without a relative attention bias and stays a BERT / RoBERTa handle", name);
    std::vector<float> w((size_t)numel);
    KR_HIP(hipMemcpy(w.data(), data, (size_t)numel * 4, hipMemcpyDefault));
    e->rel_w.swap(w);
    e->rel_fam = fam;
    e->ready = false;
    return 0;
}

// the table the attention kernels read (AttnBiasArgs): per head, log2(e) * W[bucket(d)][head] at entry width / 2 + d, |d| < max_pos + 64 (every column
// difference the position table allows; the slack covers the keys a masked tile reads past the end of its sequence).  The scores are in log2 units
// (enc_load_weight folds log2(e) / sqrt(d_h) into W_q; a T5 handle, whose scores are q.k + bias, log2(e) alone): the same fp32 multiply here.
static int build_bias_table(Encoder* e) {
    const int heads = e->cfg.heads, half = e->cfg.max_pos + 64, width = 2 * half;
    std::vector<float> tab((size_t)heads * width);
    const float log2e = (float)1.4426950408889634;
    for (int h = 0; h < heads; ++h)
        for (int i = 0; i < width; ++i) tab[(size_t)h * width + i] = e->rel_w[(size_t)rel_bucket(i - half) * heads + h] * log2e;
    if (!e->bias_tab) KR_TRY(dmalloc(e->own_bufs, &e->bias_tab, tab.size() * 4));
    KR_HIP(hipMemcpy(e->bias_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    e->bias_width = width;
    return 0;
}

// cos / sin [max_pos][d_h / 2] with HF's arithmetic (NomicBertRotaryEmbedding.forward): the angle is the fp32 product float(pos) * inv_freq[j], the entry the
// cosine / sine of that fp32 angle (evaluated in double and rounded once).  Also the zero row the embedding adds in place of a position row.
// One pair of tables per frequency vector: the handle's (global) one, and for ModernBert handles with local layers the local one.
static int build_rotary_table(Encoder* e, const std::vector<float>& inv_freq, float** cos_tab, float** sin_tab) {
    const int half = (int)inv_freq.size(), P = e->cfg.max_pos;
    std::vector<float> cs((size_t)P * half), sn((size_t)P * half);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < half; ++j) {
            const float ang = (float)p * inv_freq[j];
            cs[(size_t)p * half + j] = (float)std::cos((double)ang);
            sn[(size_t)p * half + j] = (float)std::sin((double)ang);
        }
    if (!*cos_tab) { KR_TRY(dmalloc(e->own_bufs, cos_tab, cs.size() * 4)); KR_TRY(dmalloc(e->own_bufs, sin_tab, sn.size() * 4)); }
    KR_HIP(hipMemcpy(*cos_tab, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(*sin_tab, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
    return 0;
}
static int build_rotary_tables(Encoder* e) {
    const int H = e->cfg.hidden;
    if (!e->pos_zero) {
        KR_TRY(dmalloc(e->own_bufs, &e->pos_zero, (size_t)H * 4));
        KR_HIP(hipMemset(e->pos_zero, 0, (size_t)H * 4));
    }
    KR_TRY(build_rotary_table(e, e->inv_freq, &e->rot_cos, &e->rot_sin));
    if (!e->inv_freq_local.empty()) KR_TRY(build_rotary_table(e, e->inv_freq_local, &e->rot_cos_l, &e->rot_sin_l));
    return 0;
}

// "dense.weight" [P, H]: the Dense head behind the pooling of a T5 handle (that it IS one is enc_finalize's business).  The output width of every forward
// depends on it, so it follows the rule of the settings: before the first finalize; later the same P takes new values (the weight sync reloads every
// parameter), another P or a handle finalized without it is refused.
static int load_dense(Encoder* e, const float* data, int64_t numel) {
    const int64_t H = e->cfg.hidden, P = numel / H;
    if (numel <= 0 || numel % H != 0 || P < 4 || P > 2048 || P % 4 != 0)
        return fail(KR_EINVAL, "'dense.weight' has %lld elements: expected [P, %lld] with 4 <= P <= 2048 and P %% 4 == 0", (long long)numel, (long long)H);
    if (e->finalized_once && e->dense_rows != (int)P)
        return fail(KR_EINVAL, e->dense_rows ? "'dense.weight' with P = %d after kr_encoder_finalize: the handle's output width is fixed (it has P = %d)"
                                             : "'dense.weight' (P = %d) after kr_encoder_finalize: the handle was finalized without a Dense head (%d)", (int)P, e->dense_rows);
    if (e->dense_w && e->dense_rows != (int)P) return fail(KR_EINVAL, "'dense.weight' with P = %d: the handle already holds one with P = %d", (int)P, e->dense_rows);
    if (!e->dense_w) KR_TRY(dmalloc(e->own_bufs, &e->dense_w, (size_t)numel * 4));
    KR_HIP(hipMemcpy(e->dense_w, data, (size_t)numel * 4, hipMemcpyDefault));
    if (e->dense_rows != (int)P) free_ws(e);       // e->out is sized by the output width
    e->dense_rows = (int)P;
    e->ready = false;
    return 0;
}

// "classifier.dense.{weight,bias}" [H, H] / [H] and "classifier.out_proj.{weight,bias}" [L, H] / [L], 1 <= L <= 64: the sequence-classification head
// (RobertaClassificationHead's names).  L is fixed by the first of the two out_proj tensors; like "dense.weight" the head belongs to the handle from its
// first finalize on: later the same shapes take new values, another L — or any of the four on a handle finalized without the head — is refused.
enum { CLS_DW = 1, CLS_DB = 2, CLS_OW = 4, CLS_OB = 8, CLS_MAX_LABELS = 64 };
static const char* const CLS_NAMES[4] = {"classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias"};
static int load_cls_head(Encoder* e, int which, const float* data, int64_t numel) {
    const char* name = CLS_NAMES[which];
    const unsigned bit = 1u << which;
    const int64_t H = e->cfg.hidden;
    int64_t L = e->cls_labels;
    if (bit == CLS_DW || bit == CLS_DB) {
        const int64_t want = bit == CLS_DW ? H * H : H;
        if (numel != want) return fail(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)want);
    } else {
        L = bit == CLS_OW ? numel / H : numel;
        if (numel <= 0 || (bit == CLS_OW && numel % H != 0) || L < 1 || L > CLS_MAX_LABELS)
            return fail(KR_EINVAL, "'%s' has %lld elements: expected %s with 1 <= L <= %d", name, (long long)numel, bit == CLS_OW ? "[L, hidden]" : "[L]", (int)CLS_MAX_LABELS);
        if (e->finalized_once && e->has_tanh_head() && e->cls_labels != (int)L)
            return fail(KR_EINVAL, "'%s' with L = %d after kr_encoder_finalize: the handle's classification head is fixed (it has L = %d)", name, (int)L, e->cls_labels);
    }
    if (e->finalized_once && !e->has_tanh_head())
        return fail(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without a classification head", name);
    if (e->cls_labels && e->cls_labels != (int)L) return fail(KR_EINVAL, "'%s' with L = %d: the handle already holds an out_proj tensor with L = %d", name, (int)L, e->cls_labels);
    float** dst = bit == CLS_DW ? &e->cls_wd : bit == CLS_DB ? &e->cls_bd : bit == CLS_OW ? &e->cls_wo : &e->cls_bo;
    if (!*dst) KR_TRY(dmalloc(e->own_bufs, dst, (size_t)numel * 4));
    KR_HIP(hipMemcpy(*dst, data, (size_t)numel * 4, hipMemcpyDefault));
    if (e->cls_labels != (int)L || !e->cls_got) free_ws(e);      // e->out is sized by the widest row, `pooled` exists with the head
    e->cls_labels = (int)L;
    e->cls_got |= bit;
    e->ready = false;
    return 0;
}

// ModernBertForSequenceClassification's head under HF's own names: "head.dense.{weight,bias}" [H, H] / [H], "head.norm.{weight,bias}" [H] and
// "classifier.{weight,bias}" [L, H] / [L], 1 <= L <= 64.  The rule of "classifier.{dense,out_proj}.*": L is fixed by the first of the two classifier tensors,
// and the head belongs to the handle from its first finalize on — later the same shapes take new values, another L, or any of the six on a handle finalized
// without the head, is refused.  (That the handle is a ModernBert handle is enc_finalize's business.)
static const char* const MH_NAMES[6] = {"head.dense.weight", "head.dense.bias", "head.norm.weight", "head.norm.bias", "classifier.weight", "classifier.bias"};
static int load_modern_head(Encoder* e, int which, const float* data, int64_t numel) {
    const char* name = MH_NAMES[which];
    const unsigned bit = 1u << which;
    const int64_t H = e->cfg.hidden;
    int64_t L = e->mh_labels;
    if (bit != MH_CW && bit != MH_CB) {
        const int64_t want = bit == MH_DW ? H * H : H;
        if (numel != want) return fail(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)want);
    } else {
        L = bit == MH_CW ? numel / H : numel;
        if (numel <= 0 || (bit == MH_CW && numel % H != 0) || L < 1 || L > CLS_MAX_LABELS)
            return fail(KR_EINVAL, "'%s' has %lld elements: expected %s with 1 <= L <= %d", name, (long long)numel, bit == MH_CW ? "[L, hidden]" : "[L]", (int)CLS_MAX_LABELS);
        if (e->finalized_once && e->has_modern_head() && e->mh_labels != (int)L)
            return fail(KR_EINVAL, "'%s' with L = %d after kr_encoder_finalize: the handle's classification head is fixed (it has L = %d)", name, (int)L, e->mh_labels);
    }
    if (e->finalized_once && !e->has_modern_head())
        return fail(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without ModernBert's classification head", name);
    if (e->mh_labels && e->mh_labels != (int)L) return fail(KR_EINVAL, "'%s' with L = %d: the handle already holds a classifier tensor with L = %d", name, (int)L, e->mh_labels);
    float** dst = bit == MH_DW ? &e->mh_wd : bit == MH_DB ? &e->mh_bd : bit == MH_NW ? &e->mh_g : bit == MH_NB ? &e->mh_b : bit == MH_CW ? &e->mh_wo : &e->mh_bo;
    if (!*dst) KR_TRY(dmalloc(e->own_bufs, dst, (size_t)numel * 4));
    KR_HIP(hipMemcpy(*dst, data, (size_t)numel * 4, hipMemcpyDefault));
    if (e->mh_labels != (int)L || !e->mh_got) free_ws(e);        // e->out is sized by the widest row, `pooled` exists with the head
    e->mh_labels = (int)L;
    e->mh_got |= bit;
    e->ready = false;
    return 0;
}

// fp32 [numel] from the caller -> the handle's 16-bit operand type at dst
static int upload_16bit(const float* data, int64_t numel, uint16_t* dst) {
    float* tmp = nullptr;
    KR_HIP(hipMalloc(reinterpret_cast<void**>(&tmp), (size_t)numel * 4));
    hipError_t rc = hipMemcpy(tmp, data, (size_t)numel * 4, hipMemcpyDefault);
    if (rc == hipSuccess) {
        hipLaunchKernelGGL(k_f32_to_bf16, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, 0, tmp, dst, numel, 1.f);
        rc = hipGetLastError();
        if (rc == hipSuccess) rc = hipDeviceSynchronize();
    }
    (void)hipFree(tmp);
    KR_HIP(rc);
    return 0;
}
// "colbert_linear.{weight,bias}" [P, H] / [P] (P % 128 == 0, 128 <= P <= 2048) and "sparse_linear.{weight,bias}" [1, H] / [1]: bge-m3's token-level heads.
// Two independent heads under the rule of "classifier.*": a head belongs to the handle from its first finalize on — later the same P takes new values,
// another P, or a head on a handle finalized without it, is refused.
static const char* const M3_NAMES[4] = {"colbert_linear.weight", "colbert_linear.bias", "sparse_linear.weight", "sparse_linear.bias"};
constexpr int M3_FLAGS = KR_POOL_WITH_SPARSE | KR_POOL_WITH_COLBERT;
static int load_m3_head(Encoder* e, int which, const float* data, int64_t numel) {
    const char* name = M3_NAMES[which];
    const bool colbert = which < 2, weight = (which & 1) == 0;
    const unsigned bit = weight ? 1u : 2u;
    const int64_t H = e->cfg.hidden;
    if (!colbert) {
        const int64_t want = weight ? H : 1;
        if (numel != want) return fail(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)want);
        if (e->finalized_once && !e->has_sparse()) return fail(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without a sparse head", name);
        float** dst = weight ? &e->sp_w : &e->sp_b;
        if (!*dst) KR_TRY(dmalloc(e->own_bufs, dst, (size_t)numel * 4));
        KR_HIP(hipMemcpy(*dst, data, (size_t)numel * 4, hipMemcpyDefault));
        if (!e->sp_got) free_ws(e);           // slot_row exists with a head
        e->sp_got |= bit;
        e->ready = false;
        return 0;
    }
    const int64_t P = weight ? numel / H : numel;
    if (numel <= 0 || (weight && numel % H != 0) || P < 128 || P > 2048 || P % 128 != 0)
        return fail(KR_EINVAL, "'%s' has %lld elements: expected %s with P %% 128 == 0 and 128 <= P <= 2048", name, (long long)numel, weight ? "[P, hidden]" : "[P]");
    if (e->finalized_once && !e->has_colbert()) return fail(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without a colbert head", name);
    if (e->finalized_once && e->col_rows != (int)P)
        return fail(KR_EINVAL, "'%s' with P = %d after kr_encoder_finalize: the handle's colbert head is fixed (it has P = %d)", name, (int)P, e->col_rows);
    if (e->col_rows && e->col_rows != (int)P) return fail(KR_EINVAL, "'%s' with P = %d: the handle already holds a colbert_linear tensor with P = %d", name, (int)P, e->col_rows);
    if (weight) {
        if (!e->col_w) KR_TRY(dmalloc(e->own_bufs, &e->col_w, (size_t)numel * 2));
        KR_TRY(upload_16bit(data, numel, e->col_w));
    } else {
        if (!e->col_b) KR_TRY(dmalloc(e->own_bufs, &e->col_b, (size_t)numel * 4));
        KR_HIP(hipMemcpy(e->col_b, data, (size_t)numel * 4, hipMemcpyDefault));
    }
    if (!e->col_got) free_ws(e);              // cy is sized by P, slot_row exists with a head
    e->col_rows = (int)P;
    e->col_got |= bit;
    e->ready = false;
    return 0;
}

// SPLADE's MLM head: BertForMaskedLM's "cls.predictions.transform.dense.{weight,bias}" [H, H] / [H], "cls.predictions.transform.LayerNorm.{weight,bias}" [H] and
// "cls.predictions.decoder.{weight,bias}" [V, H] / [V] with V = cfg.vocab exactly (the decoder is loaded explicitly: tying it to the word table is the caller's
// business).  Under the rule of "classifier.*": the head belongs to the handle from its first finalize on — later the same shapes take new values, a head
// arriving on a handle finalized without it is refused.
static const char* const MLM_NAMES[6] = {"cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias", "cls.predictions.transform.LayerNorm.weight",
                                         "cls.predictions.transform.LayerNorm.bias", "cls.predictions.decoder.weight", "cls.predictions.decoder.bias"};
constexpr int MLM_COLS = 128;          // column granularity of the projection loops (a wave owns 64 columns, the 128 x 128 tiles are whole)
static int64_t mlm_vpad(const Encoder* e) { return round_up((int64_t)e->cfg.vocab, MLM_COLS); }
static int load_mlm_head(Encoder* e, int which, const float* data, int64_t numel) {
    const char* name = MLM_NAMES[which];
    const int64_t H = e->cfg.hidden, V = e->cfg.vocab, Vpad = mlm_vpad(e);
    const int64_t want = which == 0 ? H * H : which == 4 ? V * H : which == 5 ? V : H;
    if (numel != want)
        return fail(KR_EINVAL, which >= 4 ? "tensor '%s' has %lld elements, expected %lld (vocab_size = %d rows)" : "tensor '%s' has %lld elements, expected %lld", name,
                    (long long)numel, (long long)want, e->cfg.vocab);
    if (e->finalized_once && !e->has_mlm()) return fail(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without an MLM head", name);
    if (which == 0 || which == 4) {
        uint16_t** dst = which == 0 ? &e->mlm_wt : &e->mlm_wd;
        if (!*dst) {
            const size_t bytes = (size_t)(which == 0 ? H : Vpad) * H * 2;
            KR_TRY(dmalloc(e->own_bufs, dst, bytes));
            KR_HIP(hipMemset(*dst, 0, bytes));       // the decoder's rows V .. Vpad - 1 stay zero
        }
        KR_TRY(upload_16bit(data, numel, *dst));
    } else {
        float** dst = which == 1 ? &e->mlm_bt : which == 2 ? &e->mlm_g : which == 3 ? &e->mlm_b : &e->mlm_bd;
        if (!*dst) {
            const size_t bytes = (size_t)(which == 5 ? Vpad : H) * 4;
            KR_TRY(dmalloc(e->own_bufs, dst, bytes));
            KR_HIP(hipMemset(*dst, 0, bytes));
        }
        KR_HIP(hipMemcpy(*dst, data, (size_t)numel * 4, hipMemcpyDefault));
    }
    if (!e->mlm_zero) {
        KR_TRY(dmalloc(e->own_bufs, &e->mlm_zero, (size_t)H * 4));
        KR_HIP(hipMemset(e->mlm_zero, 0, (size_t)H * 4));
    }
    if (!e->mlm_got) free_ws(e);              // row_seq exists with the head
    e->mlm_got |= 1u << which;
    e->ready = false;
    return 0;
}

int enc_load_weight(void* h, const char* hf_name, const float* data, int64_t numel) {
    if (!h || !hf_name || !data) return fail(KR_EINVAL, "NULL argument");
    Encoder* e = reinterpret_cast<Encoder*>(h);
    KR_TRY(select_device(e->device));
    if (std::strncmp(hf_name, "config.", 7) == 0) return set_config(e, hf_name, data, numel);
    if (std::strcmp(hf_name, "dense.weight") == 0) return load_dense(e, data, numel);
    for (int i = 0; i < 4; ++i) if (std::strcmp(hf_name, CLS_NAMES[i]) == 0) return load_cls_head(e, i, data, numel);
    for (int i = 0; i < 6; ++i) if (std::strcmp(hf_name, MH_NAMES[i]) == 0) return load_modern_head(e, i, data, numel);
    for (int i = 0; i < 4; ++i) if (std::strcmp(hf_name, M3_NAMES[i]) == 0) return load_m3_head(e, i, data, numel);
    for (int i = 0; i < 6; ++i) if (std::strcmp(hf_name, MLM_NAMES[i]) == 0) return load_mlm_head(e, i, data, numel);
    int slot = -1, fam = FAM_BERT, layer = -1; int64_t want = 0;
    KR_TRY(parse_name(e, hf_name, slot, want, fam, layer));
    // NomicBert's and ModernBert's names: q / k (rotary partners) and the gated projection's rows go into tile-pair order; T5's: wi_0 | wi_1 only
    const bool paired = fam == FAM_NOMIC || fam == FAM_MODERN, gated = paired || fam == FAM_T5G;
    if (slot == T_RELBIAS) return load_rel_bias(e, hf_name, data, numel, want, fam);
    if (slot == -1) return 0;   // pooler.* / position_ids: not used by the encoders (encoders.py:74,115 take last_hidden_state)
    if (numel != want) return fail(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld", hf_name, (long long)numel, (long long)want);
    if ((size_t)numel > e->stage_elems) {
        if (e->stage) (void)hipFree(e->stage);
        e->stage = nullptr; e->stage_elems = 0;
        KR_HIP(hipMalloc(reinterpret_cast<void**>(&e->stage), (size_t)numel * 4));
        e->stage_elems = (size_t)numel;
    }
    KR_HIP(hipMemcpy(e->stage, data, (size_t)numel * 4, hipMemcpyDefault));
    const int64_t H = e->cfg.hidden;
    // (T5 scores are q.k + bias, no 1 / sqrt(d_h): under T5's names log2(e) alone is folded in)
    const float qscale = fam_t5(fam) ? (float)1.4426950408889634 : (float)(1.4426950408889634 / std::sqrt((double)(H / e->cfg.heads)));
    const unsigned grid = (unsigned)((numel + 255) / 256);
    auto to_bf16 = [&](uint16_t* dst, float scale) { hipLaunchKernelGGL(k_f32_to_bf16, dim3(grid), dim3(256), 0, 0, e->stage, dst, numel, scale); };
    // a row block [n / cols, cols] of a fused ModernBert tensor, from element `first` of the staged copy
    auto block_to_bf16 = [&](uint16_t* dst, int64_t first, int64_t n, int cols, float scale, int mode) {
        const unsigned g = (unsigned)((n + 255) / 256);
        if (mode < 0) hipLaunchKernelGGL(k_f32_to_bf16, dim3(g), dim3(256), 0, 0, e->stage + first, dst, n, scale);
        else hipLaunchKernelGGL(k_f32_to_bf16_rows, dim3(g), dim3(256), 0, 0, e->stage + first, dst, n, cols, scale, mode);
    };
    auto to_f32 = [&](float* dst, float scale) { hipLaunchKernelGGL(k_scale_copy, dim3(grid), dim3(256), 0, 0, e->stage, dst, numel, scale); };
    // the matrices whose rows go into tile-pair order (k_f32_to_bf16_rows)
    auto to_bf16_rows = [&](uint16_t* dst, float scale, int mode) {
        hipLaunchKernelGGL(k_f32_to_bf16_rows, dim3(grid), dim3(256), 0, 0, e->stage, dst, numel, (int)H, scale, mode);
    };
    const bool head64 = paired && H == 64 * e->cfg.heads;
    if (slot == T_WQKV || slot == T_WI || slot == T_WIB || slot == T_WQKVB) {
        // ModernBert's fused tensors.  Wqkv [3H, H] = q | k | v row blocks (heads contiguous inside each): the blocks the loader fills for the other families, q with
        // the log2(e) / sqrt(d_h) fold, q and k in the rotary row order.  mlp.Wi [2 FF, H] = input | gate: input (the half the GELU is applied to) takes the place
        // of NomicBert's gate_proj, gate that of up_proj.  mlp.Wi.bias in the same order.
        LayerW& l = e->L[layer];
        uint8_t* g = &e->got[T_LAYER0 + (size_t)layer * L_COUNT];
        const int64_t FF = e->cfg.intermediate;
        if (slot == T_WQKV) {
            block_to_bf16(l.wqkv, 0, H * H, (int)H, qscale, head64 ? ROWS_HEAD64 : -1);
            block_to_bf16(l.wqkv + H * H, H * H, H * H, (int)H, 1.f, head64 ? ROWS_HEAD64 : -1);
            block_to_bf16(l.wqkv + 2 * H * H, 2 * H * H, H * H, (int)H, 1.f, -1);
            g[L_QW] = g[L_KW] = g[L_VW] = FAM_MODERN;
        } else if (slot == T_WQKVB) {
            // q | k | v biases: q with the fold, q and k in their rows' order (added before the rotation: EPI_QKV_ROTB), v as always (folded into bo_eff)
            std::vector<float> b((size_t)numel), pb((size_t)numel);
            KR_HIP(hipMemcpy(b.data(), e->stage, (size_t)numel * 4, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < H; ++i) {
                const int64_t d = head64 ? tile_pair_row(i, ROWS_HEAD64) : i;
                pb[(size_t)d] = b[(size_t)i] * qscale; pb[(size_t)(H + d)] = b[(size_t)(H + i)]; pb[(size_t)(2 * H + i)] = b[(size_t)(2 * H + i)];
            }
            KR_HIP(hipMemcpy(l.bqkv, pb.data(), (size_t)numel * 4, hipMemcpyHostToDevice));
            g[L_QB] = g[L_KB] = g[L_VB] = FAM_MODERN;
        } else if (slot == T_WI) {
            if (l.w1 && !l.gated) return fail(KR_EINVAL, "'%s': layer %d already holds intermediate.dense", hf_name, layer);
            if (!l.w1) KR_TRY(dmalloc(e->own_bufs, &l.w1, (size_t)numel * 2));
            l.gated = true;
            block_to_bf16(l.w1, 0, H * FF, (int)H, 1.f, ROWS_GATE);
            block_to_bf16(l.w1, H * FF, H * FF, (int)H, 1.f, ROWS_UP);
            g[L_IW] = g[L_UW] = FAM_MODERN;
        } else {
            if (!l.b1p) KR_TRY(dmalloc(e->own_bufs, &l.b1p, (size_t)numel * 4));
            std::vector<float> b((size_t)numel), pb((size_t)numel);
            KR_HIP(hipMemcpy(b.data(), e->stage, (size_t)numel * 4, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < FF; ++i) { pb[(size_t)tile_pair_row(i, ROWS_GATE)] = b[(size_t)i]; pb[(size_t)tile_pair_row(i, ROWS_UP)] = b[(size_t)(FF + i)]; }
            KR_HIP(hipMemcpy(l.b1p, pb.data(), (size_t)numel * 4, hipMemcpyHostToDevice));
            g[L_IB] = FAM_MODERN;
        }
        KR_HIP(hipGetLastError());
        KR_HIP(hipDeviceSynchronize());
        e->ready = false;
        return 0;
    }
    if (slot < T_LAYER0) {
        if (slot == T_POS && !e->pos) KR_TRY(dmalloc(e->own_bufs, &e->pos, (size_t)numel * 4));
        float* dst[] = {e->word, e->pos, e->type, e->elng, e->elnb};
        to_f32(dst[slot], 1.f);
    } else {
        LayerW& l = e->L[(slot - T_LAYER0) / L_COUNT];
        const int id = (slot - T_LAYER0) % L_COUNT;
        if (id == L_IW || id == L_UW) {
            if (l.w1 && l.gated != gated)
                return fail(KR_EINVAL, "'%s': layer %d already holds %s", hf_name, (slot - T_LAYER0) / L_COUNT, gated ? "a plain intermediate projection" : "a gated projection (gate_proj / up_proj, wi_0 / wi_1)");
            if (!l.w1) KR_TRY(dmalloc(e->own_bufs, &l.w1, (size_t)numel * (gated ? 4 : 2)));
            l.gated = gated;
        }
        switch (id) {
            // log2(e) / sqrt(d_h) is folded into the query projection: the attention scores come out in log2 units and the softmax is a bare exp2.  The
            // multiply is fp32, before the 16-bit conversion (d_h = 32: the factor is not a power of two; d_h = 64: the same bits as log2(e) / 8)
            case L_QW: if (head64) to_bf16_rows(l.wqkv, qscale, ROWS_HEAD64); else to_bf16(l.wqkv, qscale); break;
            case L_QB: to_f32(l.bqkv, qscale); break;
            case L_KW: if (head64) to_bf16_rows(l.wqkv + H * H, 1.f, ROWS_HEAD64); else to_bf16(l.wqkv + H * H, 1.f); break;
            case L_KB: to_f32(l.bqkv + H, 1.f); break;
            case L_VW: to_bf16(l.wqkv + 2 * H * H, 1.f); break;
            case L_VB: to_f32(l.bqkv + 2 * H, 1.f); break;
            case L_OW: to_bf16(l.wo, 1.f); break;
            case L_OB: to_f32(l.bo, 1.f); break;
            case L_LN1G: to_f32(l.ln1g, 1.f); break;
            case L_LN1B: to_f32(l.ln1b, 1.f); break;
            case L_IW: if (gated) to_bf16_rows(l.w1, 1.f, ROWS_GATE); else to_bf16(l.w1, 1.f); break;
            case L_UW: to_bf16_rows(l.w1, 1.f, ROWS_UP); break;
            case L_IB: to_f32(l.b1, 1.f); break;
            case L_FW: to_bf16(l.w2, 1.f); break;
            case L_FB: to_f32(l.b2, 1.f); break;
            case L_LN2G: to_f32(l.ln2g, 1.f); break;
            case L_LN2B: to_f32(l.ln2b, 1.f); break;
        }
    }
    KR_HIP(hipGetLastError());
    KR_HIP(hipDeviceSynchronize());
    e->got[slot] = (uint8_t)fam;
    e->ready = false;
    return 0;
}

int enc_finalize(void* h) {
    if (!h) return fail(KR_EINVAL, "NULL argument");
    Encoder* e = reinterpret_cast<Encoder*>(h);
    const bool rot = e->rotary(), modern = e->modern(), t5 = e->t5();
    if (t5 && (e->pad_idx >= 0 || rot || modern || !e->inv_freq_local.empty() || e->half_window > 0))
        return fail(KR_EINVAL, "config.t5_feed_forward next to config.position_padding_idx / config.rotary_inv_freq* / config.local_attention_layers / "
                               "config.attention_half_window: a T5 handle's one position scheme is its relative attention bias");
    if (!modern && (!e->inv_freq_local.empty() || e->half_window > 0))
        return fail(KR_EINVAL, "config.rotary_inv_freq_local / config.attention_half_window without config.local_attention_layers: they are settings of a ModernBert handle");
    if (modern) {
        if (e->pad_idx >= 0 || !e->rel_w.empty())
            return fail(KR_EINVAL, "config.local_attention_layers next to config.position_padding_idx / a relative attention bias: a handle has one position scheme");
        if (!rot) return fail(KR_EINVAL, "config.local_attention_layers without config.rotary_inv_freq: a ModernBert handle rotates q and k");
        if ((int)e->local_layers.size() != e->cfg.layers)
            return fail(KR_EINVAL, "config.local_attention_layers holds %zu flags, the handle has %d layers", e->local_layers.size(), e->cfg.layers);
        bool any_local = false;
        for (int li = 0; li < e->cfg.layers; ++li) any_local = any_local || e->local_layer(li);
        if (any_local && (e->inv_freq_local.empty() || e->half_window < 1))
            return fail(KR_EINVAL, "config.local_attention_layers flags local layers, but %s was never loaded",
                        e->inv_freq_local.empty() ? "config.rotary_inv_freq_local" : "config.attention_half_window");
    }
    // names and handle kind agree: ModernBert's names on a ModernBert handle only, and nothing but them there (the token-type row has no ModernBert name)
    for (size_t i = 0; i < e->got.size(); ++i) {
        if (!e->got[i] || i == T_TYPE) continue;
        if ((e->got[i] == FAM_MODERN) != modern)
            return fail(KR_EINVAL, modern ? "weight slot %zu was loaded under a BERT / NomicBert name: a handle with config.local_attention_layers takes ModernBert's names"
                                          : "weight slot %zu was loaded under a ModernBert name but config.local_attention_layers was never loaded: load it before kr_encoder_finalize", i);
    }
    // ... and T5's names on a T5 handle only, and nothing but them there; the bias table under the family's own name; the Dense head on T5 handles only
    for (size_t i = 0; i < e->got.size(); ++i) {
        if (!e->got[i] || i == T_TYPE) continue;
        if (fam_t5(e->got[i]) != t5)
            return fail(KR_EINVAL, t5 ? "weight slot %zu was loaded under another family's name: a handle with config.t5_feed_forward takes T5EncoderModel's names"
                                      : "weight slot %zu was loaded under a T5 name but config.t5_feed_forward was never loaded: load it before kr_encoder_finalize", i);
    }
    if (!e->rel_w.empty() && fam_t5(e->rel_fam) != t5)
        return fail(KR_EINVAL, t5 ? "a handle with config.t5_feed_forward takes its bias table as encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
                                  : "a relative attention bias under T5's name but config.t5_feed_forward was never loaded: load it before kr_encoder_finalize");
    // SPLADE's MLM head: on BERT / RoBERTa handles only, never next to another head, whole
    if (e->mlm_got) {
        int fi = 0;
        while (!(e->mlm_got & (1u << fi))) ++fi;
        const char* first = MLM_NAMES[fi];
        const bool mpnet = !e->rel_w.empty() && !t5;
        if (rot || modern || t5 || mpnet)
            return fail(KR_EINVAL, "'%s' on a %s handle: the MLM head of SPLADE is BertForMaskedLM's and is accepted on BERT handles", first,
                        t5 ? "T5" : modern ? "ModernBert" : rot ? "NomicBert" : "MPNet");
        if (e->cls_got) return fail(KR_EINVAL, "'%s' next to 'classifier.*': a handle has the classification head or the MLM head", first);
        if (e->dense_rows > 0) return fail(KR_EINVAL, "'%s' next to 'dense.weight': a handle has the Dense head or the MLM head", first);
        if (e->col_got || e->sp_got)
            return fail(KR_EINVAL, "'%s' next to '%s': a handle has bge-m3's token-level heads or the MLM head", first, e->col_got ? "colbert_linear.*" : "sparse_linear.*");
        for (int i = 0; i < 6; ++i)
            if (!(e->mlm_got & (1u << i))) return fail(KR_ESTATE, "'%s' was never loaded: the MLM head takes all six cls.predictions.* tensors or none", MLM_NAMES[i]);
    }
    // bge-m3's heads: on BERT / RoBERTa handles only, never next to another head, each one whole (checked before the Dense head's own rule, so
    // that 'dense.weight' + a token-level head on a BERT handle is refused by both names)
    for (int hd = 0; hd < 2; ++hd) {
        const unsigned got = hd == 0 ? e->col_got : e->sp_got;
        if (!got) continue;
        const char* first = M3_NAMES[2 * hd + ((got & 1u) ? 0 : 1)];
        const bool mpnet = !e->rel_w.empty() && !t5;
        if (rot || modern || t5 || mpnet)
            return fail(KR_EINVAL, "'%s' on a %s handle: bge-m3's token-level heads are accepted on BERT and RoBERTa / XLM-R handles", first,
                        t5 ? "T5" : modern ? "ModernBert" : rot ? "NomicBert" : "MPNet");
        if (e->cls_got) return fail(KR_EINVAL, "'%s' next to 'classifier.*': a handle has the classification head or the token-level heads", first);
        if (e->dense_rows > 0) return fail(KR_EINVAL, "'%s' next to 'dense.weight': a handle has the Dense head or the token-level heads", first);
        for (int i = 0; i < 2; ++i)
            if (!(got & (1u << i))) return fail(KR_ESTATE, "'%s' was never loaded: a token-level head takes its weight and its bias or neither", M3_NAMES[2 * hd + i]);
    }
    if (e->dense_rows > 0 && !t5) return fail(KR_EINVAL, "'dense.weight' without config.t5_feed_forward: the Dense head is part of T5 handles only");
    // the classification head: on BERT / RoBERTa / MPNet-shaped handles only (the other families' heads are other functions), never next to the Dense head, whole
    if (e->cls_got) {
        if (rot || modern || t5)
            return fail(KR_EINVAL, "'classifier.*' on a %s handle: the classification head Wo . tanh(Wd . x + bd) + bo is BERT's and RoBERTa's; this family's is not implemented",
                        t5 ? "T5" : modern ? "ModernBert" : "NomicBert");
        if (e->dense_rows > 0) return fail(KR_EINVAL, "'classifier.*' next to 'dense.weight': a handle has one head");
        for (int i = 0; i < 4; ++i)
            if (!(e->cls_got & (1u << i))) return fail(KR_ESTATE, "'%s' was never loaded: the classification head takes all four classifier.* tensors or none", CLS_NAMES[i]);
    }
    // ModernBert's classification head: on ModernBert handles only (a refusal names the first of its tensors that was loaded), its four required tensors
    // together; the pooling setting goes with that head
    if (e->mh_got) {
        int fi = 0;
        while (!(e->mh_got & (1u << fi))) ++fi;
        if (!modern)
            return fail(KR_EINVAL, "'%s' on a handle without config.local_attention_layers: the head classifier . LayerNorm(gelu(head.dense . x)) is "
                                   "ModernBertForSequenceClassification's and is accepted on ModernBert handles", MH_NAMES[fi]);
        for (int i = 0; i < 6; ++i)
            if ((MH_REQUIRED & (1u << i)) && !(e->mh_got & (1u << i)))
                return fail(KR_ESTATE, "'%s' was never loaded: ModernBert's classification head takes head.dense.weight, head.norm.weight, classifier.weight and "
                                       "classifier.bias together or none of them", MH_NAMES[i]);
    }
    if (e->cls_pooling >= 0 && !(modern && e->mh_got))
        return fail(KR_EINVAL, "config.classifier_pooling on a %s: it selects the row ModernBert's classification head reads",
                    modern ? "ModernBert handle without head.dense / head.norm / classifier" : "handle that is no ModernBert handle");
    if (t5) {
        for (int li = 0; li < e->cfg.layers; ++li) {
            const uint8_t* g = &e->got[T_LAYER0 + (size_t)li * L_COUNT];
            if (g[L_IW] && (g[L_IW] == FAM_T5G) != (e->t5_ff == 1))
                return fail(KR_EINVAL, "layer %d: config.t5_feed_forward = %d takes DenseReluDense.%s", li, e->t5_ff, e->t5_ff ? "wi_0 / wi_1, not wi" : "wi, not wi_0 / wi_1");
            if (g[L_UW] && e->t5_ff == 0) return fail(KR_EINVAL, "layer %d: config.t5_feed_forward = 0 takes DenseReluDense.wi, not wi_0 / wi_1", li);
        }
        if (e->rel_w.empty())
            return fail(KR_ESTATE, "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight was never loaded");
    }
    if (rot && (e->pad_idx >= 0 || !e->rel_w.empty()))
        return fail(KR_EINVAL, "config.rotary_inv_freq next to config.position_padding_idx / a relative attention bias: a handle has one position scheme");
    // q / k and the intermediate projection are packed in another row order under NomicBert's names (enc_load_weight): names and handle kind must agree
    for (int li = 0; li < e->cfg.layers; ++li) {
        const uint8_t* g = &e->got[T_LAYER0 + (size_t)li * L_COUNT];
        if (modern || t5) continue;
        if (rot && (g[L_QW] == 1 || g[L_KW] == 1 || g[L_IW] == 1))
            return fail(KR_EINVAL, "layer %d: a handle with config.rotary_inv_freq takes self_attn.{q,k}_proj and mlp.{gate,up}_proj under NomicBert's names", li);
        if (rot && (g[L_QB] || g[L_KB] || g[L_IB]))
            return fail(KR_EINVAL, "layer %d: the q / k / gate / up projections of a NomicBert handle have no bias", li);
        if (!rot && (g[L_QW] == 2 || g[L_KW] == 2 || g[L_IW] == 2 || g[L_UW]))
            return fail(KR_EINVAL, "layer %d holds tensors under NomicBert's names but config.rotary_inv_freq was never loaded: load it before kr_encoder_finalize", li);
    }
    // a NomicBert handle has no position table and needs up_proj; its linear biases are zero unless loaded
    auto optional = [&](size_t i) {
        if (t5) {      // no position table, no token types, no beta, no linear bias; wi_1 with the gated FF only
            if (i < T_LAYER0) return i == T_POS || i == T_TYPE || i == T_ELNB;
            const int id = (int)((i - T_LAYER0) % L_COUNT);
            return id == L_UW ? e->t5_ff == 0 : !(id == L_QW || id == L_KW || id == L_VW || id == L_OW || id == L_LN1G || id == L_IW || id == L_FW || id == L_LN2G);
        }
        if (i < T_LAYER0) return (rot && i == T_POS) || (modern && i == T_ELNB);
        const int id = (int)((i - T_LAYER0) % L_COUNT);
        if (modern && (id == L_LN1B || id == L_LN2B)) return true;
        if (id == L_UW) return !rot;
        return rot && (id == L_QB || id == L_KB || id == L_VB || id == L_OB || id == L_IB || id == L_FB);
    };
    for (size_t i = 0; i < e->got.size(); ++i)
        if (!e->got[i] && !optional(i)) return fail(KR_ESTATE, "weight slot %zu (layer %d, tensor %d) was never loaded", i,
                                    i < T_LAYER0 ? -1 : (int)((i - T_LAYER0) / L_COUNT), i < T_LAYER0 ? (int)i : (int)((i - T_LAYER0) % L_COUNT));
    if (e->stage) { (void)hipFree(e->stage); e->stage = nullptr; e->stage_elems = 0; }
    KR_TRY(select_device(e->device));
    const int H = e->cfg.hidden;
    if (e->mh_got) {      // head.dense.bias / head.norm.bias are zero unless loaded (classifier_bias / norm_bias false)
        for (float** b : {&e->mh_bd, &e->mh_b})
            if (!*b) { KR_TRY(dmalloc(e->own_bufs, b, (size_t)H * 4)); KR_HIP(hipMemset(*b, 0, (size_t)H * 4)); }
    }
    if (rot) {
        if (modern && !e->got[T_ELNB]) KR_HIP(hipMemset(e->elnb, 0, (size_t)H * 4));
        for (int li = 0; li < e->cfg.layers; ++li) {
            const uint8_t* g = &e->got[T_LAYER0 + (size_t)li * L_COUNT];
            LayerW& l = e->L[li];
            if (modern) {      // LayerNorm betas and the gated projection's bias are zero unless loaded
                if (!g[L_LN1B]) KR_HIP(hipMemset(l.ln1b, 0, (size_t)H * 4));
                if (!g[L_LN2B]) KR_HIP(hipMemset(l.ln2b, 0, (size_t)H * 4));
                if (!l.b1p) {
                    KR_TRY(dmalloc(e->own_bufs, &l.b1p, (size_t)2 * e->cfg.intermediate * 4));
                    KR_HIP(hipMemset(l.b1p, 0, (size_t)2 * e->cfg.intermediate * 4));
                }
            }
            if (!(modern && g[L_QB])) KR_HIP(hipMemset(l.bqkv, 0, (size_t)2 * H * 4));     // (a ModernBert layer with attn.Wqkv.bias: EPI_QKV_ROTB adds it)
            if (!g[L_VB]) KR_HIP(hipMemset(l.bqkv + 2 * H, 0, (size_t)H * 4));
            if (!g[L_OB]) KR_HIP(hipMemset(l.bo, 0, (size_t)H * 4));
            if (!g[L_FB]) KR_HIP(hipMemset(l.b2, 0, (size_t)H * 4));
        }
        KR_TRY(build_rotary_tables(e));
    }
    if (t5)      // no linear bias anywhere: the QKV epilogue adds zeros, v's fold into bo_eff is zero (the RMS norms read no beta)
        for (auto& l : e->L) {
            KR_HIP(hipMemset(l.bqkv, 0, (size_t)3 * H * 4)); KR_HIP(hipMemset(l.bo, 0, (size_t)H * 4)); KR_HIP(hipMemset(l.b2, 0, (size_t)H * 4));
        }
    for (auto& l : e->L) hipLaunchKernelGGL(k_fold_vbias, dim3((H + 127) / 128), dim3(128), 0, 0, l.wo, l.bo, l.bqkv + 2 * H, l.bo_eff, H);
    if (!e->rel_w.empty()) KR_TRY(build_bias_table(e));
    KR_HIP(hipGetLastError());
    KR_HIP(hipDeviceSynchronize());
    e->ready = true;
    e->finalized_once = true;
    return 0;
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

// every kernel of one forward, enqueued on `st` (input already in the workspace, result left in e->out)
// flags: KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT (pool is the base pool); tok_out: device memory for the token-level blocks, [B, S] then [B, S, P]
// pool = KR_POOL_SPLADE: tok_out is the [B, vocab] result, used as the reduction buffer of the decoder launch; nothing is left in e->out
static int enqueue_forward(Encoder* e, int B, int S, int pool, hipStream_t st, const Input& in, int flags = 0, float* tok_out = nullptr) {
    const int H = e->cfg.hidden, FF = e->cfg.intermediate;
    const float eps = e->cfg.ln_eps;
    e->kn.read();
    // KR_POOL_CLASSIFY reads the CLS row like KR_POOL_CLS — the query row of a masked column 0, the packed token count, the CLS shortcut — and differs behind
    // the last LayerNorm only (k_pool's raw rows, then k_cls_head): everything up to there sees KR_POOL_CLS
    // (ModernBert's head with config.classifier_pooling = 1 reads the masked mean: everything up to the last LayerNorm sees KR_POOL_MEAN)
    const bool classify = pool == KR_POOL_CLASSIFY, modern_head = classify && e->has_modern_head();
    if (classify) pool = modern_head && e->cls_pooling == 1 ? KR_POOL_MEAN : KR_POOL_CLS;
    // KR_POOL_SPLADE packs and attends like KR_POOL_MEAN (no query-only rows) and differs behind the last LayerNorm only
    const bool splade = pool == KR_POOL_SPLADE;
    if (splade) pool = KR_POOL_MEAN;
    const int nqt_max = (S + (pool == KR_POOL_CLS ? 1 : 0) + 31) / 32;             // q-tiles of the longest possible sequence
    const bool long_seq = nqt_max > 4 && !e->kn.attn_lds;                          // > 128 tokens: the LDS-DMA attention kernel (KIRAG_AMD_ATTN_LDS=1: never)
    const int align = long_seq ? 8 : 4;                                            // sequence offsets: multiple of 8 tokens so that V^T chunks start 16-B aligned
    const PackRules rules{e->cfg.vocab, e->cfg.type_vocab, pool, align, e->pad_idx};
    const SeqTables seq{e->seq_nk, e->seq_has0, e->seq_nq, e->seq_off, e->seq_cls, e->d_T};
    const TokTables tok{e->tok_id, e->tok_pos, e->tok_type, e->tok_epos, e->d_err};
    if (in.ragged) pack_ragged(e->rag_ids(), e->rag_lens(), e->rag_in_off(), B, S, in.total, rules, seq, tok, st);
    else pack_padded(e->d_ids, e->d_mask, in.has_tt ? e->d_tt : nullptr, B, S, rules, seq, tok, st);
    const int64_t maxT = (int64_t)B * (((S + (pool == KR_POOL_CLS ? 1 : 0)) + align - 1) & ~(align - 1));   // upper bound of the packed token count (each sequence is padded to `align`)
    const unsigned row_grid = (unsigned)((maxT + 3) / 4);
    // LayerNorm streams: y (dead after the kernel) and the low half (next read by the next LayerNorm, ~600 MiB of traffic later) are loaded / stored
    // non-temporally — they do not displace the 16-bit stream the next GEMM reads: -1.3 % forward at 1024 x 128 tokens, -0.1...0.5 % at 1000 x 32; 8 blocks
    // per CU instead of 4: -0.25 % (profiles/r04/tried_ln_policies.txt; outputs bit-identical)
    auto ln_kernel = H <= 512 ? &k_ln16<1, 7> : H <= 1024 ? &k_ln16<2, 7> : &k_ln16<4, 7>;
    auto ln_pre_kernel = H <= 512 ? &k_ln16_pre<1, 1> : H <= 1024 ? &k_ln16_pre<2, 1> : &k_ln16_pre<4, 1>;      // ModernBert handles (y non-temporal as above)
    const bool modern = e->modern(), t5 = e->t5(), pre = modern || t5;
    auto ln_rms_kernel = H <= 512 ? &k_ln16_pre<1, 1, true> : H <= 1024 ? &k_ln16_pre<2, 1, true> : &k_ln16_pre<4, 1, true>;    // T5 handles
    const auto ln_tail_kernel = t5 ? ln_rms_kernel : ln_pre_kernel;
    auto pool_kernel = classify ? (H <= 256 ? &k_pool<1, true> : H <= 512 ? &k_pool<2, true> : H <= 1024 ? &k_pool<4, true> : &k_pool<8, true>)
                                : (H <= 256 ? &k_pool<1> : H <= 512 ? &k_pool<2> : H <= 1024 ? &k_pool<4> : &k_pool<8>);
    const int pool_lds = POOL_WAVES * (H <= 256 ? 1 : H <= 512 ? 2 : H <= 1024 ? 4 : 8) * 256 * 4 + POOL_WAVES * 4;
    unsigned ln_mult = 8u;
    const unsigned ln_grid = std::min(row_grid, (unsigned)e->num_cu_all * ln_mult);   // k_ln is grid-stride (its parameters stay in registers across rows)
    const bool rot = e->rotary();       // a NomicBert handle: no position row in the embedding (a zero row through tok_zero), rotary QKV and SwiGLU epilogues
    if (rot) hipLaunchKernelGGL(k_rot_pos, dim3(B), dim3(64), 0, st, e->seq_off, e->seq_nq, align, e->tok_pos, e->tok_rpos);
    if (t5) {     // the embedding row is the residual stream; xb = block 0's attention norm of it
        auto embed_kernel = H <= 512 ? &k_embed_rms<1> : H <= 1024 ? &k_embed_rms<2> : &k_embed_rms<4>;
        hipLaunchKernelGGL(embed_kernel, dim3(row_grid), dim3(256), 0, st, e->tok_id, e->d_T, e->word, e->elng, eps, H, e->rb, e->use_lo ? e->rlo : nullptr, e->xb);
    } else {
        hipLaunchKernelGGL(k_embed_ln, dim3(row_grid), dim3(256), 0, st, e->tok_id, rot ? e->tok_zero : e->pad_idx >= 0 ? e->tok_epos : e->tok_pos, e->tok_type, e->d_T, e->word,
                           rot ? e->pos_zero : e->pos, e->type, e->elng, e->elnb, eps, H,
                           e->use_lo ? e->xlo : nullptr, e->xb);
    }
    const bool shortcut = pool == KR_POOL_CLS && e->cls_shortcut && e->c_ctx != nullptr && !flags;      // the token-level heads read every row of the last layer
    e->last_shortcut = shortcut;
    const RowSet all_rows{e->ctx, e->xb, e->y, e->h, e->use_lo ? e->xlo : nullptr, e->xlo, e->seq_off, e->seq_nk, e->seq_cls, e->d_T, maxT, ln_grid,
                          e->rb, e->use_lo ? e->rlo : nullptr};
    const RowSet cls_rows{e->c_ctx, e->c_xb, e->c_y, e->c_h, e->use_lo ? e->c_xlo : nullptr, e->c_xlo, e->c_off, e->c_nk, e->c_cls, e->d_B, B,
                          std::min((unsigned)((B + 3) / 4), (unsigned)e->num_cu_all * ln_mult), e->c_rb, e->use_lo ? e->c_rlo : nullptr};
    // the pre-LN tail of a ModernBert layer on the same five launches.  (rin, rin_lo): the residual stream as this layer finds it — r.rb / r.rlo, or for layer
    // 0 on all rows the embedding LayerNorm's output itself (xb / xlo: attn_norm of layer 0 is the identity)
    auto tail_pre = [&](ProjArgs a, const LayerW& l, const RowSet& r, bool last, const uint16_t* rin, const uint8_t* rin_lo) {
        a.Tp = r.rows;
        // attn.Wo; r += y + b; xb = mlp_norm(r)
        a.W = l.wo; a.X = r.ctx; a.F = H; a.K = H; a.bias = l.bo_eff; a.out0 = r.y; a.ldx = 0; a.ldo = 0;
        KR_TRY(launch_proj(EPI_DENSE, a, r.max_rows, e, st));
        hipLaunchKernelGGL(ln_tail_kernel, dim3(r.ln_grid), dim3(256), 0, st, r.y, l.bo_eff, r.rows, l.ln1g, l.ln1b, eps, H, rin, rin_lo, r.rb, r.rlo, (uint8_t*)nullptr, r.xb);
        // mlp.Wi (input | gate as one GEMM of 2 FF columns) + GEGLU: h [rows, FF].  A T5 handle: wi + relu, or wi_0 | wi_1 the same way + gelu_new, no bias
        const bool plain = t5 && e->t5_ff == 0;
        a.W = l.w1; a.X = r.xb; a.F = plain ? FF : 2 * FF; a.K = H; a.bias = l.b1p; a.out0 = r.h; a.ldx = 0; a.ldo = FF;
        KR_TRY(launch_proj(plain ? EPI_RELU : t5 ? EPI_GEGLU_TANH : EPI_GEGLU, a, r.max_rows, e, st));
        // mlp.Wo; r += y + b; xb = the next layer's attn_norm(r), or final_norm(r) with its low half for the readers of the final hidden state
        a.W = l.w2; a.X = r.h; a.F = H; a.K = FF; a.bias = l.b2; a.out0 = r.y; a.ldx = FF; a.ldo = 0;
        KR_TRY(launch_proj(EPI_DENSE, a, r.max_rows, e, st));
        hipLaunchKernelGGL(ln_tail_kernel, dim3(r.ln_grid), dim3(256), 0, st, r.y, l.b2, r.rows, l.ln2g, l.ln2b, eps, H, (const uint16_t*)r.rb, (const uint8_t*)r.rlo,
                           last ? (uint16_t*)nullptr : r.rb, r.rlo, last ? r.lo_last : (uint8_t*)nullptr, r.xb);
        return 0;
    };
    auto tail = [&](ProjArgs a, const LayerW& l, const RowSet& r, bool last) {
        a.Tp = r.rows;
        // attention.output.dense + residual -> LayerNorm
        a.W = l.wo; a.X = r.ctx; a.F = H; a.K = H; a.bias = l.bo_eff; a.out0 = r.y; a.ldx = 0; a.ldo = 0;
        KR_TRY(launch_proj(EPI_DENSE, a, r.max_rows, e, st));
        hipLaunchKernelGGL(ln_kernel, dim3(r.ln_grid), dim3(256), 0, st, r.y, l.bo_eff, r.rows, l.ln1g, l.ln1b, eps, H, r.lo, r.lo, r.xb);
        // intermediate.dense + GELU, or gate_proj | up_proj (one GEMM of 2 FF columns) + SwiGLU: h [rows, FF] either way
        a.W = l.w1; a.X = r.xb; a.F = rot ? 2 * FF : FF; a.K = H; a.bias = l.b1; a.out0 = r.h; a.ldx = 0; a.ldo = FF;
        KR_TRY(launch_proj(rot ? EPI_SWIGLU : EPI_GELU, a, r.max_rows, e, st));
        // output.dense + residual -> LayerNorm
        a.W = l.w2; a.X = r.h; a.F = H; a.K = FF; a.bias = l.b2; a.out0 = r.y; a.ldx = FF; a.ldo = 0;
        KR_TRY(launch_proj(EPI_DENSE, a, r.max_rows, e, st));
        // the LAST LayerNorm always writes the low half: pooling and kr_encoder_last_hidden read the final hidden state with 16 mantissa bits
        hipLaunchKernelGGL(ln_kernel, dim3(r.ln_grid), dim3(256), 0, st, r.y, l.b2, r.rows, l.ln2g, l.ln2b, eps, H, r.lo, last ? r.lo_last : r.lo, r.xb);
        return 0;
    };
    for (const LayerW& l : e->L) {
        const bool last = (&l == &e->L.back());
        const bool first = (&l == &e->L.front());
        const bool local = e->local_layer((int)(&l - &e->L.front()));      // a ModernBert handle's sliding-window layer: its own rotary table, windowed attention
        ProjArgs a{};
        a.Tp = e->d_T; a.H = H;
        a.rot_cos = local ? e->rot_cos_l : e->rot_cos; a.rot_sin = local ? e->rot_sin_l : e->rot_sin; a.tpos = e->tok_rpos; a.max_pos = e->cfg.max_pos; a.dh = H / e->cfg.heads;
        // q | k | v^T in one GEMM (F = 3H)
        a.W = l.wqkv; a.X = e->xb; a.F = 3 * H; a.K = H; a.bias = l.bqkv; a.out0 = e->q; a.out1 = e->k; a.outT = e->vT; a.ldT = e->ldv; a.ldx = 0; a.ldo = 0;
        const bool qk_bias = modern && e->got[T_LAYER0 + (size_t)(&l - &e->L.front()) * L_COUNT + L_QB] != 0;      // attn.Wqkv.bias was loaded
        KR_TRY(launch_proj(!rot ? EPI_QKV : qk_bias ? EPI_QKV_ROTB : EPI_QKV_ROT, a, maxT, e, st));
        {
            const int cap = (int)round_up(S, 32);
            // an MPNet handle: the instantiations with the relative attention bias; a local layer of a ModernBert handle: those with the window
            const int am = e->bias_tab != nullptr ? AM_BIAS : local ? AM_WIN : AM_PLAIN;
            auto go = [&](auto dh) -> int {
                constexpr int DH = decltype(dh)::value;
                return am == AM_BIAS ? launch_attention<DH, AM_BIAS>(e, B, cap, nqt_max, long_seq, st)
                     : am == AM_WIN ? launch_attention<DH, AM_WIN>(e, B, cap, nqt_max, long_seq, st) : launch_attention<DH, AM_PLAIN>(e, B, cap, nqt_max, long_seq, st);
            };
            if (H == 32 * e->cfg.heads) KR_TRY(go(std::integral_constant<int, 32>{})); else KR_TRY(go(std::integral_constant<int, 64>{}));
        }
        // CLS shortcut: only the CLS row of every sequence is read after the last layer: gather those rows and finish the layer on B rows (same kernels, same
        // arithmetic per row: the projection loops are bit-identical for every tiling and LayerNorm is per row, so the embedding does not change by one bit)
        // (a ModernBert handle: the residual stream travels in the place of xb — the operand is rewritten by the first LayerNorm of the tail)
        // (a T5 handle: the embedding launch has stored the residual stream itself, layer 0 finds it like every layer)
        const uint16_t* rin = (modern && !first) || t5 ? e->rb : e->xb;
        const uint8_t* rin_lo = (modern && !first) || t5 ? all_rows.rlo : all_rows.lo;
        if (last && shortcut)
            hipLaunchKernelGGL(k_gather_cls, dim3(B), dim3(256), 0, st, e->ctx, rin, rin_lo, e->seq_off, e->seq_cls, e->seq_nk, H, e->c_ctx, pre ? e->c_rb : e->c_xb,
                               pre ? e->c_rlo : e->c_xlo, e->c_off, e->c_nk, e->c_cls, e->d_B);
        if (pre) {
            if (last && shortcut) KR_TRY(tail_pre(a, l, cls_rows, last, e->c_rb, cls_rows.rlo));
            else KR_TRY(tail_pre(a, l, all_rows, last, rin, rin_lo));
        } else {
            KR_TRY(tail(a, l, last && shortcut ? cls_rows : all_rows, last));
        }
    }
    if (splade) {
        // t = LayerNorm(gelu(Wt x + bt)) of the packed rows: y <- EPI_GELU, q <- k_ln16_head (both buffers are free behind the last layer; xb / xlo keep the
        // final hidden state for kr_encoder_last_hidden)
        ProjArgs a{};
        a.Tp = e->d_T; a.H = H; a.W = e->mlm_wt; a.X = e->xb; a.F = H; a.K = H; a.bias = e->mlm_bt; a.out0 = e->y;
        KR_TRY(launch_proj(EPI_GELU, a, maxT, e, st));
        KR_HIP(hipMemsetAsync(e->row_seq, 0xff, (size_t)e->capT * 4, st));
        hipLaunchKernelGGL(k_splade_rowseq, dim3(B), dim3(64), 0, st, e->seq_off, e->seq_nk, e->row_seq);
        auto head_ln = H <= 512 ? &k_ln16_head<1> : H <= 1024 ? &k_ln16_head<2> : &k_ln16_head<4>;
        hipLaunchKernelGGL(head_ln, dim3(ln_grid), dim3(256), 0, st, e->y, e->mlm_zero, e->d_T, e->mlm_g, e->mlm_b, eps, H, e->row_seq, e->q, e->d_err);
        // the decoder: [rows] x [Vpad, H]^T reduced over each sequence's rows inside the launch (EPI_SPLADE), then log1p in place
        const int V = e->cfg.vocab;
        KR_HIP(hipMemsetAsync(tok_out, 0, (size_t)B * V * 4, st));
        a.W = e->mlm_wd; a.X = e->q; a.F = (int)mlm_vpad(e); a.bias = e->mlm_bd; a.out0 = nullptr;
        a.row_seq = e->row_seq; a.smax = reinterpret_cast<unsigned int*>(tok_out); a.V = V;
        KR_TRY(launch_proj(EPI_SPLADE, a, maxT, e, st));
        const int64_t n = (int64_t)B * V;
        hipLaunchKernelGGL(k_splade_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tok_out, n, e->d_err);
        KR_HIP(hipGetLastError());
        return 0;
    }
    const RowSet& r = shortcut ? cls_rows : all_rows;
    KR_TRY(set_lds_once(reinterpret_cast<const void*>(pool_kernel), pool_lds, e->device));
    hipLaunchKernelGGL(pool_kernel, dim3(B), dim3(POOL_WAVES * 64), pool_lds, st, r.xb, r.lo_last, r.off, r.nk, r.cls, H, pool,
                       e->dense_rows > 0 || classify ? e->pooled : e->out, e->d_err);
    if (classify) {              // the classification head: out [B, L] = Wo . tanh(Wd . pooled + bd) + bo
        const int NJ = H <= 256 ? 1 : H <= 512 ? 2 : H <= 1024 ? 4 : 8, head_lds = CH_SEQ * 2 * H * 4;
        auto head_kernel = NJ == 1 ? &k_cls_head<1> : NJ == 2 ? &k_cls_head<2> : NJ == 4 ? &k_cls_head<4> : &k_cls_head<8>;
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(head_kernel), CH_SEQ * 2 * NJ * 256 * 4, e->device));      // the widest H of the instantiation (64 KiB at 2048)
        if (modern_head) {       // ModernBert's: Wo . LayerNorm(erf_gelu(Wd . pooled + bd)) + bo, same LDS
            auto gln_kernel = NJ == 1 ? &k_cls_head<1, true> : NJ == 2 ? &k_cls_head<2, true> : NJ == 4 ? &k_cls_head<4, true> : &k_cls_head<8, true>;
            KR_TRY(set_lds_once(reinterpret_cast<const void*>(gln_kernel), CH_SEQ * 2 * NJ * 256 * 4, e->device));
            hipLaunchKernelGGL(gln_kernel, dim3((B + CH_SEQ - 1) / CH_SEQ), dim3(CH_WAVES * 64), head_lds, st, e->pooled, e->mh_wd, e->mh_bd, e->mh_wo, e->mh_bo, B, H,
                               e->mh_labels, e->out, e->mh_g, e->mh_b, eps, r.nk, e->d_err);
        } else
        hipLaunchKernelGGL(head_kernel, dim3((B + CH_SEQ - 1) / CH_SEQ), dim3(CH_WAVES * 64), head_lds, st, e->pooled, e->cls_wd, e->cls_bd, e->cls_wo, e->cls_bo, B, H,
                           e->cls_labels, e->out, nullptr, nullptr, 0.f, nullptr, nullptr);
    } else
    if (e->dense_rows > 0) {     // the Dense head: out [B, P] = normalize(W . pooled)
        const int P = e->dense_rows, dense_lds = PD_SEQ * (H + P) * 4 + PD_SEQ * 4;
        // one kernel, an LDS size per handle: the attribute is set once per device (set_lds_once) to what the largest handle needs, H = P = 2048 (64 KiB + 16 B)
        KR_TRY(set_lds_once(reinterpret_cast<const void*>(&k_pool_dense), PD_SEQ * (2048 + 2048) * 4 + PD_SEQ * 4, e->device));
        hipLaunchKernelGGL(k_pool_dense, dim3((B + PD_SEQ - 1) / PD_SEQ), dim3(256), dense_lds, st, e->pooled, e->dense_w, B, H, P, e->out);
    }
    if (flags) {                 // bge-m3's token-level blocks, straight into tok_out: sparse [B, S], then colbert [B, S, P]
        const int64_t slots = (int64_t)B * S;
        const unsigned slot_grid = (unsigned)((slots + 3) / 4);
        hipLaunchKernelGGL(k_m3_slots, dim3(B), dim3(64), 0, st, e->d_mask, e->seq_off, S, e->slot_row);
        float* o = tok_out;
        if (flags & KR_POOL_WITH_SPARSE) {
            hipLaunchKernelGGL(k_m3_sparse, dim3(slot_grid), dim3(256), 0, st, e->xb, e->xlo, e->sp_w, e->sp_b, e->slot_row, slots, H, o, e->d_err);
            o += slots;
        }
        if (flags & KR_POOL_WITH_COLBERT) {      // one more projection of the packed rows on the loops every layer uses, then bias + norm + scatter
            ProjArgs a{};
            a.Tp = e->d_T; a.H = H; a.W = e->col_w; a.X = e->xb; a.F = e->col_rows; a.K = H; a.bias = e->col_b; a.out0 = e->cy;
            KR_TRY(launch_proj(EPI_DENSE, a, maxT, e, st));
            hipLaunchKernelGGL(k_m3_rows, dim3(slot_grid), dim3(256), 0, st, e->cy, e->col_b, e->slot_row, slots, e->col_rows, o, e->d_err);
        }
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
static int check_forward_args(const Encoder* e, bool bad_shape, int B, int S, int64_t total_tokens, int pool) {
    if (!e) return fail(KR_EINVAL, "encoder is NULL");
    if (!e->ready) return fail(KR_ESTATE, "encoder weights incomplete: call kr_encoder_finalize after loading every tensor");
    if (bad_shape) return fail(KR_EINVAL, "bad input pointers / shape");
    if (S > e->cfg.max_pos) return fail(KR_EINVAL, "sequence length %d exceeds max_position_embeddings %d", S, e->cfg.max_pos);
    if (e->pad_idx >= 0 && S + e->pad_idx + 1 > e->cfg.max_pos)
        return fail(KR_EINVAL, "sequence length %d + padding index %d + 1 exceeds max_position_embeddings %d (fairseq position rule: at most %d tokens)", S, e->pad_idx,
                    e->cfg.max_pos, e->cfg.max_pos - e->pad_idx - 1);
    if (total_tokens > (int64_t)B * S) return fail(KR_EINVAL, "total_tokens %lld exceeds B * S = %lld", (long long)total_tokens, (long long)B * S);
    const int flags = pool & M3_FLAGS;
    pool &= ~M3_FLAGS;
    if (pool != KR_POOL_MEAN && pool != KR_POOL_CLS && pool != KR_POOL_CLASSIFY && pool != KR_POOL_SPLADE)
        return fail(KR_EINVAL, "pool must be 0 (mean), 1 (cls), 2 (classify) or 4 (splade), 0 and 1 optionally with KR_POOL_WITH_SPARSE (0x10) / KR_POOL_WITH_COLBERT (0x20)");
    if (flags && pool == KR_POOL_CLASSIFY) return fail(KR_EINVAL, "KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT go with pool 0 (mean) or 1 (cls), not with 2 (classify)");
    if (flags && pool == KR_POOL_SPLADE) return fail(KR_EINVAL, "KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT go with pool 0 (mean) or 1 (cls), not with 4 (splade)");
    if (pool == KR_POOL_SPLADE && !e->has_mlm())
        return fail(KR_ESTATE, "pool = 4 (splade) on a handle without an MLM head: cls.predictions.transform.dense.{weight,bias}, cls.predictions.transform.LayerNorm.{weight,bias} "
                               "and cls.predictions.decoder.{weight,bias} were never loaded");
    if (flags && total_tokens >= 0)
        return fail(KR_EINVAL, "kr_encoder_forward_packed takes no KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT: the token-level blocks are laid out by the columns of a padded batch");
    if ((flags & KR_POOL_WITH_SPARSE) && !e->has_sparse())
        return fail(KR_ESTATE, "KR_POOL_WITH_SPARSE on a handle without a sparse head: sparse_linear.weight and sparse_linear.bias were never loaded");
    if ((flags & KR_POOL_WITH_COLBERT) && !e->has_colbert())
        return fail(KR_ESTATE, "KR_POOL_WITH_COLBERT on a handle without a colbert head: colbert_linear.weight and colbert_linear.bias were never loaded");
    if (pool == KR_POOL_CLASSIFY && !e->has_head())
        return fail(KR_ESTATE, e->modern() ? "pool = 2 (classify) on a ModernBert handle without a classification head: head.dense.weight, head.norm.weight, "
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
    const size_t dense_elems = pool == KR_POOL_SPLADE ? 0 : (size_t)B * (pool == KR_POOL_CLASSIFY ? e->head_labels() : e->out_dim());
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
// where a KR_POOL_SPLADE forward reduces into: a device `out` is the reduction buffer itself (the kernels hold the caller's pointer: never replayed from a
// captured graph), a host `out` is staged
static int splade_target(Encoder* e, int B, float* out, float** red) {
    if (is_device_pointer(out)) { *red = out; return 0; }
    KR_TRY(grow_tok_stage(e, (size_t)B * e->cfg.vocab));
    *red = e->tok_stage;
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
    if (pool == KR_POOL_SPLADE) {
        float* red = nullptr;
        KR_TRY(splade_target(e, B, out, &red));
        KR_TRY(enqueue_forward(e, B, S, pool, st, Input{false, token_type_ids != nullptr, 0}, 0, red));
        return finish_forward(e, B, S, pool, out, st, red == out ? 0 : (size_t)B * e->cfg.vocab);
    }
    if (!flags) {
        KR_TRY(run_forward(e, B, S, pool, st, token_type_ids != nullptr));
        return finish_forward(e, B, S, pool, out, st);
    }
    // bge-m3's token-level blocks: a device `out` takes them straight from the kernels (0.5 GB at 1024 x 128 x 1024: no second trip through the workspace), a
    // host `out` is staged.  The kernels hold the caller's pointer, so a flagged forward is never replayed from a captured graph.
    pool &= ~M3_FLAGS;
    const size_t slots = (size_t)B * S;
    const size_t tok_elems = ((flags & KR_POOL_WITH_SPARSE) ? slots : 0) + ((flags & KR_POOL_WITH_COLBERT) ? slots * e->col_rows : 0);
    const bool direct = is_device_pointer(out);
    if (!direct) KR_TRY(grow_tok_stage(e, tok_elems));
    KR_TRY(enqueue_forward(e, B, S, pool, st, Input{false, token_type_ids != nullptr, 0}, flags, direct ? out + (size_t)B * e->out_dim() : e->tok_stage));
    return finish_forward(e, B, S, pool, out, st, direct ? 0 : tok_elems);
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
    float* red = nullptr;
    if (pool == KR_POOL_SPLADE) KR_TRY(splade_target(e, B, out, &red));
    KR_TRY(enqueue_forward(e, B, S, pool, st, Input{true, false, (int)total_tokens}, 0, red));
    return finish_forward(e, B, S, pool, out, st, red && red != out ? (size_t)B * e->cfg.vocab : 0);
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
        return fail(KR_ESTATE, "the last forward pooled the CLS token: its last layer ran on the CLS rows only (create the encoder with KIRAG_AMD_CLS_FULL=1 to keep every row)");
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
