// What an encoder handle IS, decided in one place and without a device: the state-dict names of the eight model families, the heads, the settings, and
// describe(), which turns what was loaded into a ModelPlan (or the refusal kr_encoder_finalize returns).  Host-only: nothing here includes HIP, so the
// tables are tested by a stand-alone program (tests/capi/encoder_model_check.cpp).  The device side of every row lives in encoder_weights.hpp (where a
// slot is stored) and encoder.hip (enqueue_forward: which launches a plan selects).  Adding a family or a head: DESIGN.md, "Adding a family / a head".
#pragma once
#include "../../include/kirag_amd.h"

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace kr {
namespace model {

struct Error { int code = 0; std::string msg; };
inline Error err(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
inline Error err(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return Error{code, buf};
}

// ---------------------------------------------------------------------------------------------------------
// families
// ---------------------------------------------------------------------------------------------------------
// BERT: BertModel / RobertaModel / XLMRobertaModel, post-LN, position table (fairseq's position rule is the setting config.position_padding_idx of BERT and
//   MPNet handles, not a family).  MPNET: the same stack under MPNetModel's names with "encoder.relative_attention_bias.weight" [32, heads] added to the scores.
// NOMIC (config.rotary_inv_freq): no position table, q and k rotated in the QKV epilogue, [gate | up] x as one GEMM with the SwiGLU epilogue, no linear bias
//   unless loaded.  MODERN (config.local_attention_layers, needs config.rotary_inv_freq): a PRE-LN stack — the residual stream is kept apart from the normalised
//   operand, attn_norm of layer N runs in the launch behind the MLP of layer N - 1 — with GEGLU and, in the layers flagged local, a sliding window and the
//   local rotary table.  T5 (config.t5_feed_forward, T5EncoderModel): MODERN's schedule with RMS norms, the embedding row straight into the residual stream, a
//   relative attention bias in every layer with scores q.k + bias (no 1 / sqrt(d_h)), no linear bias, relu or gated gelu_new.  DEBERTA
//   (config.deberta_position_buckets + config.deberta_max_relative_positions, DebertaV2Model): BERT's post-LN layer under the projections' names query_proj /
//   key_proj / value_proj, no position table and no token types, and disentangled attention: every score carries q_i . PK[p] + k_j . PQ[p] with p the log bucket
//   of the column difference (deberta_bucket), PQ / PK the layer's own q / k projections of the (normalised) table encoder.rel_embeddings, scale 1 / sqrt(3 d_h).
//   DECODER (config.decoder_attention, needs config.rotary_inv_freq; Qwen2Model / LlamaModel / MistralModel used as embedders): T5's schedule — pre-LN, RMS
//   norms, the embedding row straight into the residual stream — with NOMIC's rotary q / k and SwiGLU under NOMIC's projection names, optional q / k / v biases
//   (Qwen2), and with the setting's value 1 a causal mask: key column <= query column (AM_CAUSAL).  Grouped-query attention is native: k_proj / v_proj (and their biases) come as
//   [A, H] (/ [A]), A = kv_heads d_h with kv_heads dividing heads and A % 64 == 0 (kv_dim_ok), or expanded to [H, H]; A is read off the element count, k and v
//   of every layer must agree (describe()), and query head h reads KV head h / (heads / kv_heads).
//   Qwen3 (config.head_dim + layers.N.self_attn.{q,k}_norm.weight): the head width d_h is a setting of its own, 32 / 64 / 128, and need not be hidden / heads:
//   q and the context are Dq = heads d_h wide (q_proj [Dq, H], o_proj [H, Dq]), k / V^T A = kv_heads d_h <= Dq.  With the two norm vectors [d_h] of every
//   layer, q and k leave the projection unrotated (QKV_SPLIT) and k_qk_norm_rope applies the RMS norm over each head and then the rotation (encoder_rows.hpp);
//   d_h = 128 exists with the norms only and runs k_attn_wide at every length.
//   ROTARY_BERT (config.rotary_feed_forward = 1, needs config.rotary_inv_freq; JinaEmbeddingsV3Model): NOMIC's post-LN stack and rotary q / k under NOMIC's
//   projection names, with BERT's feed-forward fc2(gelu(fc1 x + b1)) + b2 in place of SwiGLU (mlp.fc1 in PLAIN row order) and optional biases on q / k / v
//   (the decoders' rows: q's and k's in the packed rows' order, added before the rotation) and o.
enum Family : uint8_t { FAM_NONE = 0, BERT, MPNET, NOMIC, MODERN, T5, DEBERTA, DECODER, ROTARY_BERT };
constexpr uint8_t GATED_NAME = 0x80;   // or-ed into a slot's family: the tensor came as one half of a gated projection under T5's names (wi_0 / wi_1)
inline Family fam_of(uint8_t got) { return (Family)(got & 0x7f); }
inline const char* family_name(Family f) { static const char* const n[] = {"unknown", "BERT / RoBERTa", "MPNet", "NomicBert", "ModernBert", "T5", "DeBERTa-v2", "decoder", "rotary BERT (jina-embeddings-v3)"}; return n[f]; }

// tensor slots: 0..4 embeddings, then L_COUNT per layer (L_UW: the second half of a gated intermediate projection); below zero what is no slot of `got`
enum { T_WORD = 0, T_POS, T_TYPE, T_ELNG, T_ELNB, T_LAYER0 };
enum { T_IGNORED = -1, T_RELBIAS = -2, T_WQKV = -3, T_WI = -4, T_WIB = -5, T_WQKVB = -6 };   // ModernBert's fused tensors of one layer: attn.Wqkv.{weight,bias}, mlp.Wi.{weight,bias}
enum { T_QNORM = -10, T_KNORM = -11 };                      // a Qwen3 layer's self_attn.q_norm.weight / k_norm.weight [d_h] (no slot of `got`: Loaded::qk_norm)
enum { T_RELEMB = -7, T_RELLNG = -8, T_RELLNB = -9 };      // DeBERTa's position table encoder.rel_embeddings.weight [2 Bk, H] and the norm over its rows, encoder.LayerNorm.{weight,bias}
constexpr int DEB_MAX_BUCKETS = 256;   // position_buckets of every v3 checkpoint, and the most a handle takes: 512 table rows
enum { L_QW = 0, L_QB, L_KW, L_KB, L_VW, L_VB, L_OW, L_OB, L_LN1G, L_LN1B, L_IW, L_IB, L_FW, L_FB, L_LN2G, L_LN2B, L_UW, L_COUNT };
constexpr int REL_BUCKETS = 32;        // HF's MPNetEncoder uses 32 buckets and max_distance 128 whatever the config says, and so do the T5 handles
constexpr int MLM_COLS = 128;          // column granularity of the projection loops: the MLM decoder is stored with vocab rounded up to it by zero rows

// the extents every shape rule is written in
enum Ext : uint8_t { X1, XH, X3H, XFF, X2FF, XV, XVPAD, XPOS, XTYPE, XBUCKETS, XHEADS, XHALF_DH, XFREE, XANY };
inline int64_t extent(const kr_bert_cfg& c, Ext x, int64_t free_dim = 0) {
    switch (x) {
        case X1: return 1;
        case XH: return c.hidden;
        case X3H: return 3 * (int64_t)c.hidden;
        case XFF: return c.intermediate;
        case X2FF: return 2 * (int64_t)c.intermediate;
        case XV: return c.vocab;
        case XVPAD: return ((int64_t)c.vocab + MLM_COLS - 1) / MLM_COLS * MLM_COLS;
        case XPOS: return c.max_pos;
        case XTYPE: return c.type_vocab;
        case XBUCKETS: return REL_BUCKETS;
        case XHEADS: return c.heads;
        case XHALF_DH: return c.hidden / c.heads / 2;
        default: return free_dim;
    }
}

// ---------------------------------------------------------------------------------------------------------
// state-dict names
// ---------------------------------------------------------------------------------------------------------
// How a row's text is matched: the whole name; the name's tail behind a '.' (or the whole name); the name's tail; what follows "embeddings."; what follows
// the layer prefix of the row's family and the layer index.  The layer prefixes (layer_prefix): "encoder.layer." anywhere for BERT's and MPNet's rows,
// else "layers." at the start or behind a '.' for NomicBert's and ModernBert's, "encoder.block." / "block." at the start for T5's.
enum Match : uint8_t { WHOLE, TAIL, ENDS, EMB, LAYER };
// NORM_BEFORE: a pre-LN family's norm in front of the attention of layer N is applied by the launch behind the FF of layer N - 1 and stored there (L_LN2*);
//   layer 0's is the embedding norm's slot under T5's and the decoders' names and the identity (refused) under ModernBert's.  LAST_LAYER: the stack's final norm, the L_LN2* of
//   the last layer.  BLOCK0: T5's one bias table is spelled as a tensor of block 0.  GATED: see GATED_NAME.
enum : uint8_t { NORM_BEFORE = 1, LAST_LAYER = 2, BLOCK0 = 4, GATED = 8 };
struct NameRow { const char* text; Match match; Family fam; int id; Ext r, c; uint8_t flags; };
static const NameRow NAME_ROWS[] = {
    {"shared.weight", WHOLE, T5, T_WORD, XV, XH, 0}, {"encoder.embed_tokens.weight", WHOLE, T5, T_WORD, XV, XH, 0}, {"embed_tokens.weight", WHOLE, T5, T_WORD, XV, XH, 0},
    {"encoder.final_layer_norm.weight", WHOLE, T5, L_LN2G, XH, X1, LAST_LAYER}, {"final_layer_norm.weight", WHOLE, T5, L_LN2G, XH, X1, LAST_LAYER},
    {"layer.0.SelfAttention.q.weight", LAYER, T5, L_QW, XH, XH, 0}, {"layer.0.SelfAttention.k.weight", LAYER, T5, L_KW, XH, XH, 0},
    {"layer.0.SelfAttention.v.weight", LAYER, T5, L_VW, XH, XH, 0}, {"layer.0.SelfAttention.o.weight", LAYER, T5, L_OW, XH, XH, 0},
    {"layer.0.SelfAttention.relative_attention_bias.weight", LAYER, T5, T_RELBIAS, XBUCKETS, XHEADS, BLOCK0},
    {"layer.0.layer_norm.weight", LAYER, T5, L_LN2G, XH, X1, NORM_BEFORE}, {"layer.1.layer_norm.weight", LAYER, T5, L_LN1G, XH, X1, 0},
    {"layer.1.DenseReluDense.wi.weight", LAYER, T5, L_IW, XFF, XH, 0}, {"layer.1.DenseReluDense.wi_0.weight", LAYER, T5, L_IW, XFF, XH, GATED},
    {"layer.1.DenseReluDense.wi_1.weight", LAYER, T5, L_UW, XFF, XH, GATED}, {"layer.1.DenseReluDense.wo.weight", LAYER, T5, L_FW, XH, XFF, 0},
    // Qwen2Model / LlamaModel / MistralModel (with or without the "model." prefix of the ...ForCausalLM state dicts): the projections come under NomicBert's rows
    // below; the final norm by its WHOLE names (a tail "norm.weight" would be ModernBert's embeddings.norm.weight); embed_tokens.weight is T5's row above
    {"model.embed_tokens.weight", WHOLE, DECODER, T_WORD, XV, XH, 0}, {"norm.weight", WHOLE, DECODER, L_LN2G, XH, X1, LAST_LAYER}, {"model.norm.weight", WHOLE, DECODER, L_LN2G, XH, X1, LAST_LAYER},
    {"input_layernorm.weight", LAYER, DECODER, L_LN2G, XH, X1, NORM_BEFORE}, {"self_attn.q_proj.bias", LAYER, DECODER, L_QB, XH, X1, 0},
    {"self_attn.k_proj.bias", LAYER, DECODER, L_KB, XH, X1, 0}, {"self_attn.v_proj.bias", LAYER, DECODER, L_VB, XH, X1, 0},
    {"self_attn.q_norm.weight", LAYER, DECODER, T_QNORM, XHALF_DH, X1, 0}, {"self_attn.k_norm.weight", LAYER, DECODER, T_KNORM, XHALF_DH, X1, 0},      // (d_h elements: check_tensor)
    {"final_norm.weight", TAIL, MODERN, L_LN2G, XH, X1, LAST_LAYER}, {"final_norm.bias", TAIL, MODERN, L_LN2B, XH, X1, LAST_LAYER},
    {"encoder.relative_attention_bias.weight", ENDS, MPNET, T_RELBIAS, XBUCKETS, XHEADS, 0},
    // DebertaV2Model: the position table (its row count is 2 Bk: check_tensor) and its norm; the attention projections into BERT's slots, every other tensor
    // under BERT's own names
    {"encoder.rel_embeddings.weight", TAIL, DEBERTA, T_RELEMB, XANY, XH, 0}, {"encoder.LayerNorm.weight", TAIL, DEBERTA, T_RELLNG, XH, X1, 0},
    {"encoder.LayerNorm.bias", TAIL, DEBERTA, T_RELLNB, XH, X1, 0},
    {"attention.self.query_proj.weight", LAYER, DEBERTA, L_QW, XH, XH, 0}, {"attention.self.query_proj.bias", LAYER, DEBERTA, L_QB, XH, X1, 0},
    {"attention.self.key_proj.weight", LAYER, DEBERTA, L_KW, XH, XH, 0}, {"attention.self.key_proj.bias", LAYER, DEBERTA, L_KB, XH, X1, 0},
    {"attention.self.value_proj.weight", LAYER, DEBERTA, L_VW, XH, XH, 0}, {"attention.self.value_proj.bias", LAYER, DEBERTA, L_VB, XH, X1, 0},
    // ModernBertModel: Wqkv [3H, H] = q | k | v row blocks, mlp.Wi [2 FF, H] = input | gate (input, the half the GELU is applied to, in the place of NomicBert's
    // gate_proj, gate in that of up_proj); mlp_norm is the norm behind the attention output
    {"attn.Wqkv.weight", LAYER, MODERN, T_WQKV, X3H, XH, 0}, {"attn.Wqkv.bias", LAYER, MODERN, T_WQKVB, X3H, X1, 0}, {"mlp.Wi.weight", LAYER, MODERN, T_WI, X2FF, XH, 0},
    {"mlp.Wi.bias", LAYER, MODERN, T_WIB, X2FF, X1, 0}, {"attn.Wo.weight", LAYER, MODERN, L_OW, XH, XH, 0}, {"attn.Wo.bias", LAYER, MODERN, L_OB, XH, X1, 0},
    {"mlp_norm.weight", LAYER, MODERN, L_LN1G, XH, X1, 0}, {"mlp_norm.bias", LAYER, MODERN, L_LN1B, XH, X1, 0}, {"mlp.Wo.weight", LAYER, MODERN, L_FW, XH, XFF, 0},
    {"mlp.Wo.bias", LAYER, MODERN, L_FB, XH, X1, 0}, {"attn_norm.weight", LAYER, MODERN, L_LN2G, XH, X1, NORM_BEFORE}, {"attn_norm.bias", LAYER, MODERN, L_LN2B, XH, X1, NORM_BEFORE},
    // JinaEmbeddingsV3Model: the projections and norms under NomicBert's rows below, the q / k / v biases under the decoders' rows above; fc1 is stored in plain
    // row order (EPI_GELU), not in the gate / up pairing
    {"self_attn.o_proj.bias", LAYER, ROTARY_BERT, L_OB, XH, X1, 0}, {"mlp.fc1.weight", LAYER, ROTARY_BERT, L_IW, XFF, XH, 0}, {"mlp.fc1.bias", LAYER, ROTARY_BERT, L_IB, XFF, X1, 0},
    {"mlp.fc2.weight", LAYER, ROTARY_BERT, L_FW, XH, XFF, 0}, {"mlp.fc2.bias", LAYER, ROTARY_BERT, L_FB, XH, X1, 0},
    // NomicBertModel
    {"self_attn.q_proj.weight", LAYER, NOMIC, L_QW, XH, XH, 0}, {"self_attn.k_proj.weight", LAYER, NOMIC, L_KW, XH, XH, 0}, {"self_attn.v_proj.weight", LAYER, NOMIC, L_VW, XH, XH, 0},
    {"self_attn.o_proj.weight", LAYER, NOMIC, L_OW, XH, XH, 0}, {"post_attention_layernorm.weight", LAYER, NOMIC, L_LN1G, XH, X1, 0},
    {"post_attention_layernorm.bias", LAYER, NOMIC, L_LN1B, XH, X1, 0}, {"mlp.gate_proj.weight", LAYER, NOMIC, L_IW, XFF, XH, 0}, {"mlp.up_proj.weight", LAYER, NOMIC, L_UW, XFF, XH, 0},
    {"mlp.down_proj.weight", LAYER, NOMIC, L_FW, XH, XFF, 0}, {"post_mlp_layernorm.weight", LAYER, NOMIC, L_LN2G, XH, X1, 0}, {"post_mlp_layernorm.bias", LAYER, NOMIC, L_LN2B, XH, X1, 0},
    // MPNetModel's spelling of the attention block, then BertModel's / RobertaModel's / XLMRobertaModel's names (a handle takes either spelling per tensor)
    {"attention.attn.q.weight", LAYER, MPNET, L_QW, XH, XH, 0}, {"attention.attn.q.bias", LAYER, MPNET, L_QB, XH, X1, 0}, {"attention.attn.k.weight", LAYER, MPNET, L_KW, XH, XH, 0},
    {"attention.attn.k.bias", LAYER, MPNET, L_KB, XH, X1, 0}, {"attention.attn.v.weight", LAYER, MPNET, L_VW, XH, XH, 0}, {"attention.attn.v.bias", LAYER, MPNET, L_VB, XH, X1, 0},
    {"attention.attn.o.weight", LAYER, MPNET, L_OW, XH, XH, 0}, {"attention.attn.o.bias", LAYER, MPNET, L_OB, XH, X1, 0},
    {"attention.LayerNorm.weight", LAYER, MPNET, L_LN1G, XH, X1, 0}, {"attention.LayerNorm.bias", LAYER, MPNET, L_LN1B, XH, X1, 0},
    {"attention.self.query.weight", LAYER, BERT, L_QW, XH, XH, 0}, {"attention.self.query.bias", LAYER, BERT, L_QB, XH, X1, 0}, {"attention.self.key.weight", LAYER, BERT, L_KW, XH, XH, 0},
    {"attention.self.key.bias", LAYER, BERT, L_KB, XH, X1, 0}, {"attention.self.value.weight", LAYER, BERT, L_VW, XH, XH, 0}, {"attention.self.value.bias", LAYER, BERT, L_VB, XH, X1, 0},
    {"attention.output.dense.weight", LAYER, BERT, L_OW, XH, XH, 0}, {"attention.output.dense.bias", LAYER, BERT, L_OB, XH, X1, 0},
    {"attention.output.LayerNorm.weight", LAYER, BERT, L_LN1G, XH, X1, 0}, {"attention.output.LayerNorm.bias", LAYER, BERT, L_LN1B, XH, X1, 0},
    {"intermediate.dense.weight", LAYER, BERT, L_IW, XFF, XH, 0}, {"intermediate.dense.bias", LAYER, BERT, L_IB, XFF, X1, 0}, {"output.dense.weight", LAYER, BERT, L_FW, XH, XFF, 0},
    {"output.dense.bias", LAYER, BERT, L_FB, XH, X1, 0}, {"output.LayerNorm.weight", LAYER, BERT, L_LN2G, XH, X1, 0}, {"output.LayerNorm.bias", LAYER, BERT, L_LN2B, XH, X1, 0},
    // embeddings (NomicBert and MPNet spell theirs as BERT does)
    {"tok_embeddings.weight", EMB, MODERN, T_WORD, XV, XH, 0}, {"norm.weight", EMB, MODERN, T_ELNG, XH, X1, 0}, {"norm.bias", EMB, MODERN, T_ELNB, XH, X1, 0},
    {"word_embeddings.weight", EMB, BERT, T_WORD, XV, XH, 0}, {"position_embeddings.weight", EMB, BERT, T_POS, XPOS, XH, 0},
    {"token_type_embeddings.weight", EMB, BERT, T_TYPE, XTYPE, XH, 0}, {"LayerNorm.weight", EMB, BERT, T_ELNG, XH, X1, 0}, {"LayerNorm.bias", EMB, BERT, T_ELNB, XH, X1, 0},
};

// the rows a layer prefix leads to: 0 = BERT's and MPNet's, 1 = NomicBert's and ModernBert's, 2 = T5's
inline int prefix_group(Family f) { return f == T5 ? 2 : f == NOMIC || f == MODERN || f == DECODER || f == ROTARY_BERT ? 1 : 0; }      // (DeBERTa's layers are "encoder.layer.N.": group 0)
// the layer prefix of `s`, T5's only or the other two: its group and where the layer index starts, or -1
inline int layer_prefix(const std::string& s, bool t5, size_t& at) {
    if (t5) {
        if (s.compare(0, 14, "encoder.block.") == 0) { at = 14; return 2; }
        if (s.compare(0, 6, "block.") == 0) { at = 6; return 2; }
        return -1;
    }
    if (const size_t p = s.find("encoder.layer."); p != std::string::npos) { at = p + 14; return 0; }
    if (s.compare(0, 7, "layers.") == 0) { at = 7; return 1; }
    if (const size_t p = s.find(".layers."); p != std::string::npos) { at = p + 8; return 1; }
    return -1;
}

// slot >= 0: a slot of `got`; T_RELBIAS; T_RELEMB / T_RELLNG / T_RELLNB; a fused ModernBert tensor of layer `layer`; T_IGNORED ("pooler.*", "position_ids": the encoders read last_hidden_state)
struct Resolved { int slot = T_IGNORED; Family fam = BERT; int layer = -1; int64_t numel = 0; bool gated = false; };

inline Error resolve_name(const kr_bert_cfg& cfg, const char* name, Resolved& out) {
    const std::string s(name);
    out = Resolved{};
    if (s.find("position_ids") != std::string::npos || s.find("pooler.") != std::string::npos) return Error{};
    auto tail = [&](const char* t, bool dot) {
        const size_t n = strlen(t);
        return s.size() >= n && s.compare(s.size() - n, n, t) == 0 && (!dot || s.size() == n || s[s.size() - n - 1] == '.');
    };
    auto take = [&](const NameRow& r, long l) -> Error {
        out.fam = r.fam; out.gated = (r.flags & GATED) != 0; out.numel = extent(cfg, r.r) * extent(cfg, r.c); out.layer = (int)l;
        if ((r.flags & BLOCK0) && l != 0) return err(KR_EINVAL, "'%s': block 0 holds a T5 encoder's one relative attention bias", name);
        if ((r.flags & NORM_BEFORE) && l == 0 && r.fam == MODERN) return err(KR_EINVAL, "'%s': attn_norm of layer 0 is the identity in ModernBert", name);
        if (r.flags & LAST_LAYER) l = cfg.layers - 1;
        if ((r.flags & NORM_BEFORE) && l == 0) out.slot = T_ELNG;
        else out.slot = r.id < 0 || (r.match != LAYER && !(r.flags & LAST_LAYER)) ? r.id : T_LAYER0 + (int)((r.flags & NORM_BEFORE) ? l - 1 : l) * L_COUNT + r.id;
        return Error{};
    };
    // in this order: whole names, T5's blocks, tails, the other layer prefixes, embeddings
    for (int pass = 0; pass < 5; ++pass) {
        if (pass == 1 || pass == 3) {
            size_t at = 0;
            const int group = layer_prefix(s, pass == 1, at);
            if (group < 0) continue;
            char* end = nullptr;
            const long l = strtol(s.c_str() + at, &end, 10);
            if (end == s.c_str() + at || *end != '.' || l < 0 || l >= cfg.layers) return err(KR_EINVAL, "bad layer index in '%s'", name);
            for (const NameRow& r : NAME_ROWS)
                if (r.match == LAYER && prefix_group(r.fam) == group && strcmp(end + 1, r.text) == 0) return take(r, l);
            return err(KR_EINVAL, "unknown layer tensor '%s'", name);
        }
        const size_t emb = s.find("embeddings.");
        for (const NameRow& r : NAME_ROWS)
            if ((pass == 0 && r.match == WHOLE && s == r.text) || (pass == 2 && (r.match == TAIL || r.match == ENDS) && tail(r.text, r.match == TAIL)) ||
                (pass == 4 && r.match == EMB && emb != std::string::npos && s.compare(emb + 11, std::string::npos, r.text) == 0))
                return take(r, -1);
    }
    return err(KR_EINVAL, "unknown tensor name '%s'", name);
}

// ---------------------------------------------------------------------------------------------------------
// heads
// ---------------------------------------------------------------------------------------------------------
// The rule of every head.  It belongs to the handle from its first finalize on: later loads with the same shape take new values (the weight sync reloads
// every parameter); another free dimension, or a head arriving on a handle finalized without it, is KR_EINVAL.  At finalize a head is accepted on its
// families only, never next to the heads it excludes, and whole (every REQUIRED tensor) or absent; an optional tensor is zero unless loaded.
//   HEAD_MLM: SPLADE's BertForMaskedLM head (KR_POOL_SPLADE): one EPI_GELU projection H -> H, k_ln16_head, the decoder [Vpad, H] with the EPI_SPLADE epilogue.
//   HEAD_COLBERT / HEAD_SPARSE: bge-m3's token-level heads (KR_POOL_WITH_COLBERT / KR_POOL_WITH_SPARSE): a flagged forward runs its last layer on every row.
//   HEAD_DENSE: the sentence-transformers Dense head behind the pooling of a T5 handle (k_pool_dense: out [B, P]).
//   HEAD_CLS: RobertaClassificationHead (KR_POOL_CLASSIFY): out [B, L] = Wo . tanh(Wd . x + bd) + bo of the raw CLS row.  On a DeBERTa handle the same four
//   names are DebertaV2ForSequenceClassification's ContextPooler + classifier: erf-GELU where the tanh stands (ModelPlan::cls_gelu).
//   HEAD_MODERN_CLS: ModernBertForSequenceClassification's, Wo . LayerNorm(erf_gelu(Wd . x + bd)) + bo of the raw CLS row or (config.classifier_pooling = 1) mean.
//   HEAD_SCORE: the score head of Qwen2 / Llama / MistralForSequenceClassification (HF's GenericForSequenceClassification.score, a Linear without a bias;
//   KR_POOL_CLASSIFY on a decoder handle): out [B, L] = score.weight . x of the raw row of the highest attended column, behind the final norm.
//   HEAD_ST_DENSE: sentence-transformers' Dense module behind the pooling of ANY family (k_st_dense): out [B, P] = act(st_dense.weight . x + st_dense.bias) of the
//   RAW pooled row x, act = config.st_dense_activation (identity / tanh), then divided by its norm unless config.normalize_output = 0.  Never next to another head.
// HEAD_COUNT counts the heads of the encoder families — the ones the plan line of tests/capi/encoder_model_check.cpp prints, one digit each — and the decoders'
// head follows them: the tables and per-head arrays are HEAD_ALL long.
enum Head { HEAD_MLM = 0, HEAD_COLBERT, HEAD_SPARSE, HEAD_DENSE, HEAD_CLS, HEAD_MODERN_CLS, HEAD_COUNT, HEAD_SCORE = HEAD_COUNT, HEAD_ST_DENSE, HEAD_ALL };
enum : uint8_t { REQUIRED = 1, HALF = 2 };       // HALF: stored as the handle's 16-bit operand (a projection of the loops every layer uses), else fp32
// workspace buffers that exist because of a head: the head's input rows [B, H]; the packed row of every [b, s] column; the sequence of every packed row; the
// colbert product [T, P]
enum : unsigned { WS_POOLED = 1, WS_SLOT_ROW = 2, WS_ROW_SEQ = 4, WS_CY = 8 };
constexpr int HEAD_MAX_TENSORS = 6;
enum { POOL_TOK_MEAN = 0, POOL_TOK_MAX = 1, POOL_TOK_SQRT_LEN = 2 };      // config.pool_tokens
struct HeadTensor { const char* name; Ext r, c, store_r; uint8_t flags; };     // store_r: the rows it is stored with (zero rows behind r)
struct HeadDesc {
    const char* subject;         // what a refusal calls the head's tensors (nullptr: the first one that was loaded)
    const char* noun;            // "... finalized without <noun>"
    const char* accepted;        // why another family does not take it
    const char* whole;           // what "whole" means
    int n; HeadTensor t[HEAD_MAX_TENSORS];
    char dim; int dim_min, dim_max, dim_step;    // the free dimension XFREE (0: none)
    unsigned families;           // bit per Family
    int excludes[4];             // heads it is never next to, in the order they are reported; -1 ends the list
    unsigned ws;
};
static const HeadDesc HEADS[HEAD_ALL] = {
    {nullptr, "an MLM head", "the MLM head of SPLADE is BertForMaskedLM's and is accepted on BERT handles", "the MLM head takes all six cls.predictions.* tensors or none", 6,
     {{"cls.predictions.transform.dense.weight", XH, XH, XH, REQUIRED | HALF}, {"cls.predictions.transform.dense.bias", XH, X1, XH, REQUIRED},
      {"cls.predictions.transform.LayerNorm.weight", XH, X1, XH, REQUIRED}, {"cls.predictions.transform.LayerNorm.bias", XH, X1, XH, REQUIRED},
      {"cls.predictions.decoder.weight", XV, XH, XVPAD, REQUIRED | HALF}, {"cls.predictions.decoder.bias", XV, X1, XVPAD, REQUIRED}},
     0, 0, 0, 0, 1u << BERT, {HEAD_CLS, HEAD_DENSE, HEAD_COLBERT, HEAD_SPARSE}, WS_ROW_SEQ},
    {nullptr, "a colbert head", "bge-m3's token-level heads are accepted on BERT and RoBERTa / XLM-R handles", "a token-level head takes its weight and its bias or neither", 2,
     {{"colbert_linear.weight", XFREE, XH, XFREE, REQUIRED | HALF}, {"colbert_linear.bias", XFREE, X1, XFREE, REQUIRED}},
     'P', 128, 2048, 128, 1u << BERT, {HEAD_CLS, HEAD_DENSE, -1}, WS_SLOT_ROW | WS_CY},
    {nullptr, "a sparse head", "bge-m3's token-level heads are accepted on BERT and RoBERTa / XLM-R handles", "a token-level head takes its weight and its bias or neither", 2,
     {{"sparse_linear.weight", X1, XH, X1, REQUIRED}, {"sparse_linear.bias", X1, X1, X1, REQUIRED}},
     0, 0, 0, 0, 1u << BERT, {HEAD_CLS, HEAD_DENSE, -1}, WS_SLOT_ROW},
    {"dense.weight", "a Dense head", "the Dense head is part of T5 handles only (config.t5_feed_forward)", "", 1,
     {{"dense.weight", XFREE, XH, XFREE, REQUIRED}}, 'P', 4, 2048, 4, 1u << T5, {-1}, WS_POOLED},
    {"classifier.*", "a classification head", "the classification head Wo . act(Wd . x + bd) + bo is BERT's and RoBERTa's (tanh) and DeBERTa's (gelu); this family's is not implemented",
     "the classification head takes all four classifier.* tensors or none", 4,
     {{"classifier.dense.weight", XH, XH, XH, REQUIRED}, {"classifier.dense.bias", XH, X1, XH, REQUIRED}, {"classifier.out_proj.weight", XFREE, XH, XFREE, REQUIRED},
      {"classifier.out_proj.bias", XFREE, X1, XFREE, REQUIRED}},
     'L', 1, 64, 1, 1u << BERT | 1u << MPNET | 1u << DEBERTA, {HEAD_DENSE, -1}, WS_POOLED},
    {nullptr, "ModernBert's classification head (head.dense / head.norm / classifier)",
     "the head classifier . LayerNorm(gelu(head.dense . x)) is ModernBertForSequenceClassification's and is accepted on ModernBert handles (config.local_attention_layers)",
     "ModernBert's classification head takes head.dense.weight, head.norm.weight, classifier.weight and classifier.bias together or none of them", 6,
     {{"head.dense.weight", XH, XH, XH, REQUIRED}, {"head.dense.bias", XH, X1, XH, 0}, {"head.norm.weight", XH, X1, XH, REQUIRED}, {"head.norm.bias", XH, X1, XH, 0},
      {"classifier.weight", XFREE, XH, XFREE, REQUIRED}, {"classifier.bias", XFREE, X1, XFREE, REQUIRED}},
     'L', 1, 64, 1, 1u << MODERN, {-1}, WS_POOLED},
    {nullptr, "a score head (score.weight)",
     "the score head score.weight . x of the last attended token is Qwen2 / Llama / MistralForSequenceClassification's and is accepted on decoder handles (config.decoder_attention)",
     "", 1, {{"score.weight", XFREE, XH, XFREE, REQUIRED}}, 'L', 1, 64, 1, 1u << DECODER, {-1}, WS_POOLED},
    {"st_dense.*", "a sentence-transformers Dense head (st_dense.weight)", "the sentence-transformers Dense head is accepted on every family",
     "the sentence-transformers Dense head takes st_dense.weight, with or without st_dense.bias", 2,
     {{"st_dense.weight", XFREE, XH, XFREE, REQUIRED}, {"st_dense.bias", XFREE, X1, XFREE, 0}}, 'P', 4, 2048, 4, ~0u, {-1}, WS_POOLED},
};

struct HeadState { int dim = 0; unsigned got = 0; };      // the free dimension (0: not known yet), one bit per tensor that was loaded
inline bool head_whole(int head, const HeadState& s) {
    for (int i = 0; i < HEADS[head].n; ++i)
        if ((HEADS[head].t[i].flags & REQUIRED) && !(s.got & (1u << i))) return false;
    return true;
}
inline const char* head_first(int head, const HeadState& s) {
    if (HEADS[head].subject) return HEADS[head].subject;
    int i = 0;
    while (i < HEADS[head].n - 1 && !(s.got & (1u << i))) ++i;
    return HEADS[head].t[i].name;
}
inline bool find_head_tensor(const char* name, int& head, int& idx) {
    for (head = 0; head < HEAD_ALL; ++head)
        for (idx = 0; idx < HEADS[head].n; ++idx)
            if (strcmp(name, HEADS[head].t[idx].name) == 0) return true;
    return false;
}
// tensor `idx` of `head` arriving with `numel` elements: its shape, then the rule above.  dim: the head's free dimension after this load
inline Error check_head_tensor(const kr_bert_cfg& cfg, int head, int idx, int64_t numel, const HeadState& s, bool finalized_once, int& dim) {
    const HeadDesc& d = HEADS[head];
    const HeadTensor& t = d.t[idx];
    dim = s.dim;
    if (t.r != XFREE) {
        const int64_t want = extent(cfg, t.r) * extent(cfg, t.c);
        if (numel != want && t.r == XV) return err(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld (vocab_size = %d rows)", t.name, (long long)numel, (long long)want, cfg.vocab);
        if (numel != want) return err(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld", t.name, (long long)numel, (long long)want);
    } else {
        const int64_t cols = extent(cfg, t.c), n = numel / cols;
        if (numel <= 0 || numel % cols != 0 || n < d.dim_min || n > d.dim_max || n % d.dim_step != 0)
        {
            char step[32] = "";
            if (d.dim_step > 1) snprintf(step, sizeof(step), " and %c %% %d == 0", d.dim, d.dim_step);
            return err(KR_EINVAL, "'%s' has %lld elements: expected [%c%s] with %d <= %c <= %d%s", t.name, (long long)numel, d.dim, t.c == XH ? ", hidden" : "", d.dim_min,
                       d.dim, d.dim_max, step);
        }
        dim = (int)n;
    }
    if (finalized_once && !(s.got && head_whole(head, s))) return err(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without %s", t.name, d.noun);
    if (finalized_once && dim != s.dim)
        return err(KR_EINVAL, "'%s' with %c = %d after kr_encoder_finalize: the shape of the handle's head is fixed (it has %c = %d)", t.name, d.dim, dim, d.dim, s.dim);
    if (s.dim && dim != s.dim) return err(KR_EINVAL, "'%s' with %c = %d: the handle already holds a tensor of this head with %c = %d", t.name, d.dim, dim, d.dim, s.dim);
    return Error{};
}

// ---------------------------------------------------------------------------------------------------------
// settings
// ---------------------------------------------------------------------------------------------------------
// Settings travel through the name-addressed loader under the reserved prefix "config." (no tensor of an HF state dict starts with it), as floats.  One rule:
// accepted before the handle's first finalize; later the same values are a no-op and anything else is refused (the family, the workspace and the meaning of
// every tensor depend on them).  What the settings of a handle must add up to is describe()'s business.
//   config.position_padding_idx = P: fairseq's position rule (RoBERTa / XLM-R: P + number of ids != P up to and including the column, P where the id is P).
//   config.rotary_inv_freq: d_h / 2 values, HF's rotary_emb.inv_freq; config.rotary_inv_freq_local: the same for ModernBert's local layers.
//   config.attention_half_window: local layers admit key columns within it of the query's.  config.local_attention_layers: one 0 / 1 flag per layer.
//   config.t5_feed_forward: 0 = wo(relu(wi x)), 1 = wo(gelu_new(wi_0 x) * wi_1 x).
//   config.classifier_pooling: the row ModernBert's classification head reads, 0 = [CLS] (also when never set), 1 = the masked mean; after the first finalize it
//   is known to handles with that head only.
//   config.deberta_position_buckets = Bk (even, 2 .. 256) and config.deberta_max_relative_positions = M (M - 1 > Bk / 2): DebertaV2Config's position_buckets and
//   max_relative_positions (max_position_embeddings where that is < 1); the two together make the handle a DeBERTa handle.
//   config.decoder_attention: the handle is a decoder-LLM stack (needs config.rotary_inv_freq); 1 = causal attention, 0 = bidirectional on the same stack.
//   config.head_dim: the head width d_h of a decoder handle, 32 / 64 / 128, where it is not hidden / heads (Qwen3Config.head_dim).  Sent before
//   config.rotary_inv_freq (which then takes d_h / 2 values) and before the weights: q_proj is [heads d_h, hidden], o_proj [hidden, heads d_h], k_proj / v_proj
//   [kv_heads d_h, hidden].  128 needs the q / k norms of every layer.  Never set: hidden / heads, and the handle is what it was without the setting.
//   config.rotary_feed_forward: the feed-forward of a rotary post-LN handle (config.rotary_inv_freq), 0 = NomicBert's SwiGLU (also when never set),
//   1 = fc2(gelu(fc1 x + b1)) + b2 with linear biases: a rotary BERT handle (jina-embeddings-v3).
//   The tail of a sentence-transformers pipeline (modules.json: Pooling, Dense, Normalize), on every family and never next to a head other than HEAD_ST_DENSE:
//   config.normalize_output: 1 (also when never set) = the KR_POOL_MEAN / KR_POOL_CLS / KR_POOL_LAST row, or the Dense head's, is divided by its norm; 0 = it is
//   written as it is (checkpoints trained for the dot product).  The norm is formed either way: a non-finite row stays KR_ERANGE.
//   config.pool_tokens: what a KR_POOL_MEAN forward pools over the attended tokens, 0 = their mean (also when never set), 1 = the element-wise max,
//   2 = sum / sqrt(n) (mean_sqrt_len_tokens).  A sequence without attended tokens gives NaN under all three.
//   config.st_dense_activation: the activation of HEAD_ST_DENSE, 0 = identity (also when never set), 1 = tanh; after the first finalize it is known to handles
//   with that head only.
enum Setting { SET_PAD_IDX = 0, SET_ROTARY, SET_ROTARY_LOCAL, SET_HALF_WINDOW, SET_LOCAL_LAYERS, SET_T5_FF, SET_CLS_POOLING, SET_DEB_BUCKETS, SET_DEB_MAX_REL, SET_ROTARY_FF, SET_HEAD_DIM, SET_NORMALIZE_OUT, SET_POOL_TOKENS, SET_ST_ACT, SET_DECODER_ATTN, SET_COUNT };
enum ValueRule : uint8_t { V_FINITE, V_FLAGS, V_INT };
struct SettingRow {
    const char* name;
    Ext count;             // how many values it takes (XANY: 1 .. SETTING_MAX_VALUES)
    ValueRule rule;        // finite floats, 0 / 1 flags, or ONE integer in [lo, hi] (hi < 0: max_pos + hi), described by `expects`
    int lo, hi;
    const char* expects;
    const char* unset;     // what a handle finalized without the setting is
    int max_pos_limit;     // > 0: refused on a handle with more position rows (the rotary tables are built for at most 8192)
    int dflt;              // >= 0: the value a handle finalized without the setting runs with, so that loading it later is a no-op
    int needs_head;        // >= 0: after the first finalize the setting is known to handles with this head only
    int step;              // > 1: a V_INT setting takes multiples of it only
};
static const SettingRow SETTINGS[SET_COUNT] = {
    {"config.position_padding_idx", X1, V_INT, 0, -2, "an integer in [0, max_position_embeddings - 2]", "BERT's position rule", 0, -1, -1, 0},
    {"config.rotary_inv_freq", XHALF_DH, V_FINITE, 0, 0, "", "no rotary positions: a BERT / RoBERTa / MPNet handle", 8192, -1, -1, 0},
    {"config.rotary_inv_freq_local", XHALF_DH, V_FINITE, 0, 0, "", "no local rotary table", 0, -1, -1, 0},
    {"config.attention_half_window", X1, V_INT, 1, 65536, "an integer >= 1", "no attention window", 0, -1, -1, 0},
    {"config.local_attention_layers", XANY, V_FLAGS, 0, 1, "", "not a ModernBert handle", 0, -1, -1, 0},
    {"config.t5_feed_forward", X1, V_INT, 0, 1, "0 (relu) or 1 (gated gelu_new)", "not a T5 handle", 0, -1, -1, 0},
    {"config.classifier_pooling", X1, V_INT, 0, 1, "0 ([CLS] row) or 1 (masked mean)", "the [CLS] row", 0, 0, HEAD_MODERN_CLS, 0},
    {"config.deberta_position_buckets", X1, V_INT, 2, DEB_MAX_BUCKETS, "an even integer", "no disentangled attention: not a DeBERTa handle", 0, -1, -1, 2},
    {"config.deberta_max_relative_positions", X1, V_INT, 2, 65536, "an integer M with M - 1 > position_buckets / 2", "no disentangled attention: not a DeBERTa handle", 0, -1, -1, 0},
    {"config.rotary_feed_forward", X1, V_INT, 0, 1, "0 (SwiGLU) or 1 (gelu with biases)", "NomicBert's SwiGLU", 0, 0, -1, 0},
    {"config.head_dim", X1, V_INT, 32, 128, "32, 64 or 128", "heads of hidden / heads features", 0, -1, -1, 32},
    {"config.normalize_output", X1, V_INT, 0, 1, "0 (rows as pooled) or 1 (divided by their norm)", "normalised rows", 0, 1, -1, 0},
    {"config.pool_tokens", X1, V_INT, 0, 2, "0 (mean), 1 (max) or 2 (sum / sqrt(n))", "the masked mean", 0, 0, -1, 0},
    {"config.st_dense_activation", X1, V_INT, 0, 1, "0 (identity) or 1 (tanh)", "the identity", 0, 0, HEAD_ST_DENSE, 0},
    {"config.decoder_attention", X1, V_INT, 0, 1, "0 (bidirectional) or 1 (causal)", "not a decoder handle", 0, -1, -1, 0},
};
constexpr int64_t SETTING_MAX_VALUES = 4096;
struct Settings {
    std::vector<float> v[SET_COUNT];      // empty: never set
    bool has(Setting s) const { return !v[s].empty(); }
    int value(Setting s, int unset = -1) const { return v[s].empty() ? unset : (int)v[s][0]; }
};
inline int find_setting(const char* name) {
    for (int i = 0; i < SET_COUNT; ++i) if (strcmp(name, SETTINGS[i].name) == 0) return i;
    return -1;
}
// vals: `numel` host floats (not read when the count is wrong).  stored: whether `set` changed
inline Error set_setting(const kr_bert_cfg& cfg, Settings& set, const HeadState* heads, bool finalized_once, const char* name, const float* vals, int64_t numel, bool& stored) {
    stored = false;
    const int si = find_setting(name);
    if (si < 0) {
        std::string known;
        for (const SettingRow& r : SETTINGS) known += std::string(known.empty() ? "" : ", ") + r.name;
        return err(KR_EINVAL, "unknown setting '%s' (known: %s)", name, known.c_str());
    }
    const SettingRow& r = SETTINGS[si];
    // (the rotary frequencies of a handle with config.head_dim: half of THAT width)
    const int64_t count = r.count == XHALF_DH && set.has(SET_HEAD_DIM) ? set.value(SET_HEAD_DIM) / 2 : extent(cfg, r.count);
    if (r.count == XANY ? (numel < 1 || numel > SETTING_MAX_VALUES) : numel != count)
        return r.count == XHALF_DH ? err(KR_EINVAL, "%s takes d_h / 2 = %lld values, got %lld", name, (long long)count, (long long)numel)
             : r.count == X1 ? err(KR_EINVAL, "'%s' takes one value, got %lld", name, (long long)numel) : err(KR_EINVAL, "'%s': %lld values", name, (long long)numel);
    if (r.max_pos_limit && cfg.max_pos > r.max_pos_limit)
        return err(KR_EINVAL, "%s: max_position_embeddings = %d, rotary tables are built for at most %d", name, cfg.max_pos, r.max_pos_limit);
    const int hi = r.hi < 0 ? cfg.max_pos + r.hi : r.hi;
    for (int64_t i = 0; i < numel; ++i) {
        const float x = vals[i];
        if (r.rule != V_INT && !std::isfinite(x)) return err(KR_EINVAL, "'%s' holds a non-finite value", name);
        if (si == SET_HEAD_DIM && x == 96.f) return err(KR_EINVAL, "%s = 96: expected %s", name, r.expects);
        if (r.rule == V_INT && (!(x >= (float)r.lo && x <= (float)hi) || x != (float)(int)x || (r.step > 1 && (int)x % r.step != 0))) return err(KR_EINVAL, "%s = %g: expected %s (%d .. %d)", name, (double)x, r.expects, r.lo, hi);
    }
    const std::vector<float> v(vals, vals + numel);
    if (finalized_once) {
        if (r.needs_head >= 0 && !(heads[r.needs_head].got && head_whole(r.needs_head, heads[r.needs_head])))
            return err(KR_EINVAL, "%s after kr_encoder_finalize: the handle was finalized without %s", name, HEADS[r.needs_head].noun);
        const std::vector<float> now = set.v[si].empty() && r.dflt >= 0 ? std::vector<float>(1, (float)r.dflt) : set.v[si];
        if (v == now) return Error{};
        const char* more = numel > 1 ? ", ..." : "";
        if (now.empty())
            return err(KR_EINVAL, "%s = %g%s after kr_encoder_finalize: the handle was finalized without it (%s) and stays what it is", name, (double)v[0], more, r.unset);
        return err(KR_EINVAL, "%s = %g%s after kr_encoder_finalize: it is fixed at the handle's first finalize (it has %g%s)", name, (double)v[0], more, (double)now[0],
                   now.size() > 1 ? ", ..." : "");
    }
    if (r.rule == V_FLAGS)
        for (float x : v) if (x != 0.f && x != 1.f) return err(KR_EINVAL, "'%s' takes one 0 / 1 flag per layer, got %g", name, (double)x);
    set.v[si] = v;
    stored = true;
    return Error{};
}

// ---------------------------------------------------------------------------------------------------------
// DeBERTa's bucket rule
// ---------------------------------------------------------------------------------------------------------
// make_log_bucket_position of modeling_deberta_v2.py for the column difference r = col_query - col_key: the identity up to mid = Bk / 2, beyond it
// sign(r) (ceil(ln(|r| / mid) / ln((M - 1) / mid) (mid - 1)) + mid).  In float64 it equals HF's float32 tensor arithmetic for every |r| < M at
// (Bk, M) = (256, 512), (32, 128) and (64, 512) (tests/test_deberta_host.py).  Needs Bk >= 2 and M - 1 > mid (describe()).
inline int deberta_delta(int r, int Bk, int M) {
    const int mid = Bk / 2, a = r < 0 ? -r : r;
    if (a <= mid) return r;
    const double lp = std::ceil(std::log((double)a / mid) / std::log((double)(M - 1) / mid) * (mid - 1)) + mid;
    const double big = 1 << 20;      // far outside every table: the clamp of deberta_bucket decides
    const int d = (int)(lp < big ? lp : big);
    return r < 0 ? -d : d;
}
// the row of PQ / PK a pair reads (c2p_pos / p2c_pos of HF's disentangled_attention_bias, which agree because the rule is odd): clamped into the table
inline int deberta_bucket(int r, int Bk, int M) {
    const int p = deberta_delta(r, Bk, M) + Bk;
    return p < 0 ? 0 : p > 2 * Bk - 1 ? 2 * Bk - 1 : p;
}

// ---------------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------------
// what was loaded: per slot 0 = never, else the Family of the name it came under (| GATED_NAME); the family of the bias table's name; the heads
struct Loaded {
    std::vector<uint8_t> got;
    std::vector<int> kv;                   // per layer the rows A of k_proj.weight, v_proj.weight, k_proj.bias, v_proj.bias as loaded under the shared names (0: never)
    int kv_seen = 0;                       // ... of the tensor check_tensor saw last (mark_loaded takes it over)
    Family rel_fam = FAM_NONE;
    int rel_rows = 0, rel_rows_seen = 0;   // rows of DeBERTa's position table as loaded (0: never); of the tensor check_tensor saw last (mark_loaded takes it over)
    bool rel_ln[2] = {false, false};       // encoder.LayerNorm.weight / .bias were loaded
    HeadState heads[HEAD_ALL];
    std::vector<uint8_t> qk_norm;          // per layer: self_attn.q_norm.weight, self_attn.k_norm.weight were loaded
    int q_rows = 0, o_cols = 0;            // rows of the last q_proj.weight / columns of the last o_proj.weight loaded under the shared names (0: never), with
    int q_rows_seen = 0, o_cols_seen = 0;  // ... those of the tensor check_tensor saw last (mark_loaded takes them over)
    explicit Loaded(int layers = 0) : got(T_LAYER0 + (size_t)layers * L_COUNT, 0), kv((size_t)layers * 4, 0), qk_norm((size_t)layers * 2, 0) {}
    bool any_qk_norm() const { for (uint8_t x : qk_norm) if (x) return true; return false; }
};
// the q / o projections under the names a decoder handle shares with NomicBert: 0 = q_proj.weight, 1 = o_proj.weight, 2 = q_proj.bias (-1: none).  Their
// width is Dq = heads d_h, hidden unless the handle has config.head_dim
inline int qo_index(const Resolved& r) {
    if (r.slot < T_LAYER0 || (r.fam != NOMIC && r.fam != DECODER)) return -1;
    switch ((r.slot - T_LAYER0) % L_COUNT) { case L_QW: return 0; case L_OW: return 1; case L_QB: return 2; default: return -1; }
}
// The k / v projections under the names a decoder handle shares with NomicBert (self_attn.{k,v}_proj.weight) and their biases: which of the four a resolved
// tensor is (-1: none).  They alone come in a grouped-query form.
inline int kv_index(const Resolved& r) {
    if (r.slot < T_LAYER0 || (r.fam != NOMIC && r.fam != DECODER)) return -1;
    switch ((r.slot - T_LAYER0) % L_COUNT) { case L_KW: return 0; case L_VW: return 1; case L_KB: return 2; case L_VB: return 3; default: return -1; }
}
// A = kv_heads d_h rows: whole KV heads, their number a divisor of the query heads, and whole 64-column wave slices of the QKV epilogue (no wave straddles
// q | k | v); A = H is the plain (or expanded) form
// (head_dim: the value of config.head_dim, 0 = never set: d_h = hidden / heads; A <= Dq = heads d_h)
inline bool kv_dim_ok(const kr_bert_cfg& c, int64_t A, int head_dim = 0) {
    const int64_t dh = head_dim ? head_dim : c.hidden / c.heads;
    return A > 0 && A <= c.heads * dh && A % dh == 0 && c.heads % (A / dh) == 0 && A % 64 == 0;
}
// A resolved tensor arriving with `numel` elements: its count.  The bias table [32, heads] (MPNet's name or T5's) has the rule of the heads: before the first
// finalize it makes the handle an MPNet handle (a T5 handle needs it); afterwards a handle that has it takes new values (the weight sync reloads every
// parameter) and a handle finalized without it refuses it.
// DeBERTa's position table [2 Bk, H] and its norm have the same rule; the table's row count is fixed with it (describe() holds it against the setting).
// head_dim: the value of config.head_dim (0: never set).  With it the q / o projections are held against Dq = heads d_h, k / v against whole heads of d_h.
inline Error check_tensor(const kr_bert_cfg& cfg, const char* name, const Resolved& r, int64_t numel, Loaded& ld, bool finalized_once, int head_dim = 0) {
    if (r.slot == T_IGNORED) return Error{};
    const int64_t dh = head_dim ? head_dim : cfg.hidden / cfg.heads, Dq = cfg.heads * dh;
    if (r.slot == T_QNORM || r.slot == T_KNORM) {
        if (numel != dh) return err(KR_EINVAL, "tensor '%s' has %lld elements, expected head_dim = %lld", name, (long long)numel, (long long)dh);
        if (finalized_once && !ld.any_qk_norm())
            return err(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without q / k norms and stays what it is", name);
        return Error{};
    }
    if (const int qi = qo_index(r); qi >= 0 && head_dim) {
        const int64_t want = qi == 2 ? Dq : Dq * cfg.hidden;
        if (numel != want)
            return err(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld (config.head_dim = %d: %d heads x %d = %lld %s)", name, (long long)numel, (long long)want, head_dim,
                       cfg.heads, head_dim, (long long)Dq, qi == 1 ? "columns" : "rows");
        if (qi == 0) ld.q_rows_seen = (int)Dq; else if (qi == 1) ld.o_cols_seen = (int)Dq;
        return Error{};
    }
    if (const int qi = qo_index(r); qi == 0) ld.q_rows_seen = cfg.hidden; else if (qi == 1) ld.o_cols_seen = cfg.hidden;
    if (r.slot == T_RELEMB) {
        const int64_t rows = numel / cfg.hidden;
        if (numel <= 0 || numel % cfg.hidden != 0 || rows % 2 != 0 || rows < 4 || rows > 2 * DEB_MAX_BUCKETS)
            return err(KR_EINVAL, "tensor '%s' has %lld elements, expected [2 * position_buckets, hidden] with 2 <= position_buckets <= %d", name, (long long)numel, DEB_MAX_BUCKETS);
        if (finalized_once && ld.rel_rows && rows != ld.rel_rows)
            return err(KR_EINVAL, "'%s' with %lld rows after kr_encoder_finalize: the table of the handle is fixed (it has %d rows)", name, (long long)rows, ld.rel_rows);
        ld.rel_rows_seen = (int)rows;
    } else if (r.slot == T_RELLNG || r.slot == T_RELLNB) {
        if (numel != r.numel) return err(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)r.numel);
        if (finalized_once && ld.rel_rows && !ld.rel_ln[0])
            return err(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without encoder.LayerNorm (norm_rel_ebd none) and stays what it is", name);
    }
    if (r.slot <= T_RELEMB) {
        if (finalized_once && !ld.rel_rows)
            return err(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without config.deberta_position_buckets and is no DeBERTa handle", name);
        return Error{};
    }
    if (r.slot == T_RELBIAS && numel != r.numel)
        return err(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld (%d buckets x %d heads: MPNet always uses %d buckets, and so do the T5 handles)", name,
                   (long long)numel, (long long)r.numel, REL_BUCKETS, cfg.heads, REL_BUCKETS);
    if (const int kvi = kv_index(r); kvi >= 0) {
        // [A, H] / [A]: every valid A is taken here; whether the handle is one that takes A < H, and whether its tensors agree, is describe()'s business.
        // After the first finalize A is what the handle has (all four kinds and all layers agree by then)
        const int64_t cols = kvi < 2 ? cfg.hidden : 1, A = numel / cols;
        if (numel % cols != 0 || !kv_dim_ok(cfg, A, head_dim))
            return err(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld, or the grouped-query form %s with A = kv_heads * %d, kv_heads a divisor of %d and A %% 64 == 0", name,
                       (long long)numel, (long long)(head_dim ? Dq * cols : r.numel), kvi < 2 ? "[A, hidden]" : "[A]", (int)dh, cfg.heads);
        if (finalized_once && ld.kv[0] && A != ld.kv[0])
            return err(KR_EINVAL, "'%s' with A = %lld rows after kr_encoder_finalize: the k / v width of the handle is fixed (it has A = %d)", name, (long long)A, ld.kv[0]);
        ld.kv_seen = (int)A;
        return Error{};
    }
    if (numel != r.numel) return err(KR_EINVAL, "tensor '%s' has %lld elements, expected %lld", name, (long long)numel, (long long)r.numel);
    if (r.slot == T_RELBIAS && finalized_once && ld.rel_fam == FAM_NONE)
        return err(KR_EINVAL, "'%s' after kr_encoder_finalize: the handle was finalized without a relative attention bias and stays a BERT / RoBERTa handle", name);
    return Error{};
}
// a resolved tensor has been stored: its slot (a fused ModernBert tensor: the slots it fills) carries the family of its name
inline void mark_loaded(Loaded& ld, const Resolved& r) {
    const uint8_t tag = (uint8_t)(r.fam | (r.gated ? GATED_NAME : 0));
    uint8_t* g = r.layer >= 0 ? &ld.got[T_LAYER0 + (size_t)r.layer * L_COUNT] : nullptr;
    if (r.slot == T_RELBIAS) ld.rel_fam = r.fam;
    else if (r.slot == T_QNORM || r.slot == T_KNORM) ld.qk_norm[(size_t)r.layer * 2 + (r.slot == T_KNORM)] = 1;
    else if (r.slot == T_RELEMB) ld.rel_rows = ld.rel_rows_seen;
    else if (r.slot == T_RELLNG || r.slot == T_RELLNB) ld.rel_ln[r.slot == T_RELLNB] = true;
    else if (r.slot == T_WQKV) g[L_QW] = g[L_KW] = g[L_VW] = tag;
    else if (r.slot == T_WQKVB) g[L_QB] = g[L_KB] = g[L_VB] = tag;
    else if (r.slot == T_WI) g[L_IW] = g[L_UW] = tag;
    else if (r.slot == T_WIB) g[L_IB] = tag;
    else if (r.slot >= 0) ld.got[r.slot] = tag;
    if (const int qi = qo_index(r); qi == 0) ld.q_rows = ld.q_rows_seen; else if (qi == 1) ld.o_cols = ld.o_cols_seen;
    if (const int kvi = kv_index(r); kvi >= 0) {
        // k's rows start at H and v's behind k's A rows of the packed matrix: a matrix that comes back with another A has overwritten, or moved away from,
        // its partner, which therefore counts as never loaded
        int& have = ld.kv[(size_t)r.layer * 4 + kvi];
        if (kvi < 2 && have && have != ld.kv_seen) g[kvi == 0 ? L_VW : L_KW] = 0;
        have = ld.kv_seen;
    }
}
// the slots a family needs; every other one is optional and zero unless loaded (T5's wi_1: needed with the gated FF)
struct FamilyRow { Family fam; bool pre_ln, rms; unsigned embed, layer; };
constexpr unsigned bits() { return 0; }
template <class... T> constexpr unsigned bits(int b, T... rest) { return 1u << b | bits(rest...); }
constexpr unsigned LAYER_MATRICES = bits(L_QW, L_KW, L_VW, L_OW, L_IW, L_FW), LAYER_NORMS = bits(L_LN1G, L_LN1B, L_LN2G, L_LN2B);
static const FamilyRow FAMILIES[] = {
    {FAM_NONE, false, false, 0, 0},
    {BERT, false, false, bits(T_WORD, T_POS, T_TYPE, T_ELNG, T_ELNB), (1u << L_COUNT) - 1 - bits(L_UW)},
    {MPNET, false, false, bits(T_WORD, T_POS, T_TYPE, T_ELNG, T_ELNB), (1u << L_COUNT) - 1 - bits(L_UW)},
    {NOMIC, false, false, bits(T_WORD, T_TYPE, T_ELNG, T_ELNB), LAYER_MATRICES | LAYER_NORMS | bits(L_UW)},
    {MODERN, true, false, bits(T_WORD, T_TYPE, T_ELNG), LAYER_MATRICES | bits(L_LN1G, L_LN2G, L_UW)},
    {T5, true, true, bits(T_WORD, T_ELNG), LAYER_MATRICES | bits(L_LN1G, L_LN2G)},
    {DEBERTA, false, false, bits(T_WORD, T_ELNG, T_ELNB), (1u << L_COUNT) - 1 - bits(L_UW)},
    {DECODER, true, true, bits(T_WORD, T_ELNG), LAYER_MATRICES | bits(L_LN1G, L_LN2G, L_UW)},
    {ROTARY_BERT, false, false, bits(T_WORD, T_TYPE, T_ELNG, T_ELNB), LAYER_MATRICES | LAYER_NORMS},
};

enum PosSource : uint8_t { POS_COLUMN, POS_FAIRSEQ, POS_ROTARY, POS_BIAS_ONLY, POS_DISENT };   // the embedding's position row: by column, by fairseq's rule, none (a zero row; q / k rotated), none (T5: no table), none (DeBERTa: a zero row)
enum QkvKind : uint8_t { QKV_PLAIN, QKV_ROT, QKV_ROT_BIAS, QKV_SPLIT };            // EPI_QKV, EPI_QKV_ROT, EPI_QKV_ROTB (a ModernBert layer with attn.Wqkv.bias), EPI_QKV_SPLIT (q / k norms: rotated behind them)
enum AttnMode : uint8_t { AM_PLAIN = 0, AM_BIAS = 1, AM_WIN = 2, AM_DISENT = 3, AM_CAUSAL = 4 };  // plain, with the relative attention bias, under the sliding window (and the local rotary table), DeBERTa's disentangled position terms, key column <= query column (the window's kernels with a one-sided window)
enum FfKind : uint8_t { FF_GELU, FF_SWIGLU, FF_GEGLU, FF_RELU, FF_GEGLU_TANH };    // EPI_GELU, EPI_SWIGLU, EPI_GEGLU, EPI_RELU, EPI_GEGLU_TANH
struct LayerPlan { QkvKind qkv; AttnMode attn; };
struct ModelPlan {
    Family family = FAM_NONE;
    bool pre_ln = false, rms = false, rotary = false, rotary_local = false, rel_bias = false;
    PosSource pos = POS_COLUMN;
    int pad_idx = -1, half_window = 0;
    int deb_buckets = 0, deb_max_rel = 0;  // DeBERTa: Bk and M of deberta_bucket (0: no such handle)
    bool deb_norm = false;                 // ... and whether the table goes through encoder.LayerNorm
    bool cls_gelu = false;                 // HEAD_CLS computes erf-GELU where BERT's computes tanh (DeBERTa's ContextPooler)
    std::vector<LayerPlan> layers;
    FfKind ff = FF_GELU;
    bool ff_gated = false;                 // w1 is [2 FF, H]
    std::vector<int> zero_fill;            // optional slots that were not loaded
    bool head[HEAD_ALL] = {};
    int head_dim[HEAD_ALL] = {};
    int classifier = -1;                   // the head KR_POOL_CLASSIFY runs (HEAD_CLS / HEAD_MODERN_CLS / HEAD_SCORE), -1: none
    bool classify_mean = false;            // ... on the masked mean (config.classifier_pooling = 1)
    int kv_dim = 0;                        // A: columns of k and rows of V^T (hidden, or kv_heads d_h of a grouped-query decoder handle)
    int head_w = 0, q_dim = 0;             // d_h and Dq = heads d_h, the width of q and of the context: hidden / heads and hidden unless config.head_dim says otherwise
    bool qk_norm = false;                  // every layer has self_attn.{q,k}_norm.weight: QKV_SPLIT, then k_qk_norm_rope
    int out_dim = 0, out_width = 0;        // columns of a pooled row; of the widest row `out` must hold, whatever the pool
    bool normalize = true;                 // config.normalize_output
    int pool_tokens = 0;                   // config.pool_tokens: POOL_TOK_*
    bool st_tanh = false;                  // config.st_dense_activation = 1
    unsigned ws = 0;                       // WS_*
};

// the state-dict name a slot was loaded under, for refusals: the first row of `f` that fills it ("weight slot N" when the table has none)
inline std::string slot_tensor_name(size_t slot, Family f) {
    const int layer = slot < T_LAYER0 ? -1 : (int)((slot - T_LAYER0) / L_COUNT), id = slot < T_LAYER0 ? (int)slot : (int)((slot - T_LAYER0) % L_COUNT);
    static const char* const prefix[] = {"encoder.layer.", "layers.", "encoder.block."};
    for (const NameRow& r : NAME_ROWS) {
        if (r.fam != f || r.id != id || (r.match == LAYER) != (layer >= 0)) continue;
        if (layer >= 0) return std::string(prefix[prefix_group(f)]) + std::to_string(layer) + "." + r.text;
        return std::string(r.match == EMB ? "embeddings." : "") + r.text;
    }
    return "weight slot " + std::to_string(slot);
}

inline Error describe(const kr_bert_cfg& cfg, const Settings& set, const Loaded& ld, ModelPlan& plan) {
    const bool rot = set.has(SET_ROTARY), modern = set.has(SET_LOCAL_LAYERS), t5 = set.has(SET_T5_FF), rel = ld.rel_fam != FAM_NONE;
    const bool local_set = set.has(SET_ROTARY_LOCAL) || set.has(SET_HALF_WINDOW);
    const bool deb = set.has(SET_DEB_BUCKETS) || set.has(SET_DEB_MAX_REL), dec = set.has(SET_DECODER_ATTN);
    const int pad_idx = set.value(SET_PAD_IDX), t5_ff = set.value(SET_T5_FF), Bk = set.value(SET_DEB_BUCKETS, 0), max_rel = set.value(SET_DEB_MAX_REL, 0);
    const bool rbert = set.value(SET_ROTARY_FF, 0) == 1;
    const int head_w = set.value(SET_HEAD_DIM, cfg.hidden / cfg.heads), q_dim = cfg.heads * head_w;
    const bool qk_norm = ld.any_qk_norm();
    if (set.has(SET_HEAD_DIM) && !dec)
        return err(KR_EINVAL, "config.head_dim on a handle without config.decoder_attention: a head width of its own is accepted on decoder handles only");
    if (qk_norm && !dec)
        return err(KR_EINVAL, "'layers.N.self_attn.{q,k}_norm.weight' on a handle without config.decoder_attention: the q / k norms are accepted on decoder handles only");
    if (set.has(SET_HEAD_DIM)) {
        if (q_dim % 128 != 0 || q_dim > 4096)
            return err(KR_EINVAL, "config.head_dim = %d with %d heads: heads * head_dim = %d must be a multiple of 128 up to 4096", head_w, cfg.heads, q_dim);
        if (rot && (int)set.v[SET_ROTARY].size() != head_w / 2)
            return err(KR_EINVAL, "config.rotary_inv_freq holds %zu values, config.head_dim = %d needs %d: load config.head_dim first", set.v[SET_ROTARY].size(), head_w, head_w / 2);
        if (ld.q_rows && ld.q_rows != q_dim)
            return err(KR_EINVAL, "'layers.N.self_attn.q_proj.weight' has %d rows, config.head_dim = %d needs %d: load config.head_dim before the weights", ld.q_rows, head_w, q_dim);
        if (ld.o_cols && ld.o_cols != q_dim)
            return err(KR_EINVAL, "'layers.N.self_attn.o_proj.weight' has %d columns, config.head_dim = %d needs %d: load config.head_dim before the weights", ld.o_cols, head_w, q_dim);
    }
    if (qk_norm)
        for (int li = 0; li < cfg.layers; ++li) {
            for (int x = 0; x < 2; ++x)
                if (!ld.qk_norm[(size_t)li * 2 + x])
                    return err(KR_ESTATE, "'layers.%d.self_attn.%s_norm.weight' was never loaded: a handle takes the q / k norms of every layer or none", li, x ? "k" : "q");
            for (const int id : {L_QB, L_KB})
                if (ld.got[T_LAYER0 + (size_t)li * L_COUNT + id])
                    return err(KR_EINVAL, "'%s' next to the q / k norms: a handle with self_attn.{q,k}_norm.weight has no q / k bias",
                               slot_tensor_name(T_LAYER0 + (size_t)li * L_COUNT + id, DECODER).c_str());
        }
    if (head_w == 128 && !qk_norm)
        return err(KR_EINVAL, "config.head_dim = 128 without layers.N.self_attn.{q,k}_norm.weight: 128-wide heads run with the q / k norms only (Qwen3)");
    const Family fam = dec ? DECODER : deb ? DEBERTA : t5 ? T5 : modern ? MODERN : rbert ? ROTARY_BERT : rot ? NOMIC : rel ? MPNET : BERT;
    const std::vector<float>& flags = set.v[SET_LOCAL_LAYERS];
    if (rbert) {
        if (pad_idx >= 0 || modern || local_set || t5 || deb || dec || rel)
            return err(KR_EINVAL, "config.rotary_feed_forward = 1 next to config.position_padding_idx / config.local_attention_layers / config.rotary_inv_freq_local / "
                                  "config.attention_half_window / config.t5_feed_forward / config.deberta_* / config.decoder_attention / a relative attention bias: "
                                  "a handle has one position scheme");
        if (!rot) return err(KR_EINVAL, "config.rotary_feed_forward = 1 without config.rotary_inv_freq: a rotary BERT handle rotates q and k");
    }
    if (dec) {
        if (pad_idx >= 0 || modern || local_set || t5 || deb || rel)
            return err(KR_EINVAL, "config.decoder_attention next to config.position_padding_idx / config.local_attention_layers / config.rotary_inv_freq_local / "
                                  "config.attention_half_window / config.t5_feed_forward / config.deberta_* / a relative attention bias: a handle has one position scheme");
        if (!rot) return err(KR_EINVAL, "config.decoder_attention without config.rotary_inv_freq: a decoder handle rotates q and k");
        // names and family agree: the projections, post_attention_layernorm.weight under NomicBert's names (their packed row order), the norms in front of the
        // attention, the final norm and the q / k / v biases under the decoders' own, the embedding under either spelling — and nothing else
        for (size_t i = 0; i < ld.got.size(); ++i) {
            if (!ld.got[i]) continue;
            const Family g = fam_of(ld.got[i]);
            const int id = i < T_LAYER0 ? -1 : (int)((i - T_LAYER0) % L_COUNT);
            const bool nomic_slot = id == L_QW || id == L_KW || id == L_VW || id == L_OW || id == L_LN1G || id == L_IW || id == L_UW || id == L_FW;
            const bool own_slot = i == T_ELNG || id == L_QB || id == L_KB || id == L_VB || id == L_LN2G;
            if (i == T_WORD ? (g == DECODER || g == T5) : nomic_slot ? g == NOMIC : own_slot && g == DECODER) continue;
            return err(KR_EINVAL, "'%s' on a decoder handle (config.decoder_attention): it takes embed_tokens, layers.N.{input_layernorm,post_attention_layernorm}.weight, "
                                  "layers.N.self_attn.{q,k,v,o}_proj.weight, layers.N.self_attn.{q,k,v}_proj.bias, layers.N.mlp.{gate,up,down}_proj.weight and norm.weight",
                       slot_tensor_name(i, g).c_str());
        }
    } else {
        // (a rotary BERT handle takes its q / k / v biases under the decoders' rows, and nothing else of theirs)
        for (size_t i = 0; i < ld.got.size(); ++i) {
            if (fam_of(ld.got[i]) != DECODER) continue;
            const int id = i < T_LAYER0 ? -1 : (int)((i - T_LAYER0) % L_COUNT);
            if (!rbert) return err(KR_EINVAL, "'%s' but config.decoder_attention was never loaded: load it before kr_encoder_finalize", slot_tensor_name(i, DECODER).c_str());
            if (id != L_QB && id != L_KB && id != L_VB)
                return err(KR_EINVAL, "'%s' on a rotary BERT handle (config.rotary_feed_forward = 1): of the decoders' names it takes layers.N.self_attn.{q,k,v}_proj.bias only",
                           slot_tensor_name(i, DECODER).c_str());
        }
    }
    // the rotary BERT rows (self_attn.o_proj.bias, mlp.fc1, mlp.fc2) on their own handles only
    for (size_t i = 0; i < ld.got.size() && !rbert; ++i)
        if (fam_of(ld.got[i]) == ROTARY_BERT)
            return err(KR_EINVAL, "'%s' but config.rotary_feed_forward = 1 was never loaded: load it (and config.rotary_inv_freq) before kr_encoder_finalize",
                       slot_tensor_name(i, ROTARY_BERT).c_str());
    // the k / v width A: one per handle — k and v of a layer agree, the layers agree, the biases agree with the matrices; A < H on decoder handles only (the
    // attention kernels of every other family read K / V^T of head h, not of head h / group)
    int kv_dim = q_dim;
    {
        static const int ids[4] = {L_KW, L_VW, L_KB, L_VB};
        int first_l = -1, first_k = 0;
        for (int li = 0; li < cfg.layers; ++li)
            for (int x = 0; x < 4; ++x) {
                const size_t slot = T_LAYER0 + (size_t)li * L_COUNT + ids[x];
                const int A = ld.kv[(size_t)li * 4 + x];
                if (!ld.got[slot] || !A) continue;
                const std::string nm = slot_tensor_name(slot, fam_of(ld.got[slot]));
                if (dec && !kv_dim_ok(cfg, A, set.value(SET_HEAD_DIM, 0)))
                    return err(KR_EINVAL, "'%s' with A = %d rows: expected A = kv_heads * %d, kv_heads a divisor of %d, A %% 64 == 0 and A <= %d", nm.c_str(), A, head_w, cfg.heads, q_dim);
                if (!dec && A != cfg.hidden)
                    return err(KR_EINVAL, "'%s' with A = %d rows on a handle without config.decoder_attention: grouped-query k / v projections are accepted on decoder handles only "
                                          "(load the setting before kr_encoder_finalize, or expand the tensor to %d rows)", nm.c_str(), A, cfg.hidden);
                if (first_l < 0) { first_l = li; first_k = x; kv_dim = A; }
                else if (A != kv_dim)
                    return err(KR_EINVAL, "'%s' has A = %d rows but '%s' has %d: k_proj and v_proj (and their biases) of every layer of a handle share one width A", nm.c_str(), A,
                               slot_tensor_name(T_LAYER0 + (size_t)first_l * L_COUNT + ids[first_k], fam_of(ld.got[T_LAYER0 + (size_t)first_l * L_COUNT + ids[first_k]])).c_str(), kv_dim);
            }
    }
    if (deb) {
        if (!set.has(SET_DEB_BUCKETS) || !set.has(SET_DEB_MAX_REL))
            return err(KR_EINVAL, "%s without %s: a DeBERTa handle takes both", SETTINGS[set.has(SET_DEB_BUCKETS) ? SET_DEB_BUCKETS : SET_DEB_MAX_REL].name,
                       SETTINGS[set.has(SET_DEB_BUCKETS) ? SET_DEB_MAX_REL : SET_DEB_BUCKETS].name);
        if (pad_idx >= 0 || rot || modern || local_set || t5 || rel)
            return err(KR_EINVAL, "config.deberta_position_buckets / config.deberta_max_relative_positions next to config.position_padding_idx / config.rotary_inv_freq* / "
                                  "config.local_attention_layers / config.attention_half_window / config.t5_feed_forward / a relative attention bias: a handle has one position scheme");
        if (!(max_rel - 1 > Bk / 2))
            return err(KR_EINVAL, "config.deberta_max_relative_positions = %d with config.deberta_position_buckets = %d: the bucket rule needs M - 1 > position_buckets / 2", max_rel, Bk);
        if (cfg.max_pos > 8192) return err(KR_EINVAL, "max_position_embeddings = %d: a DeBERTa handle's bucket table is built for at most 8192 columns", cfg.max_pos);
        // names and family agree: the attention projections under DeBERTa's names (the score scale 1 / sqrt(3 d_h) is folded into query_proj as it is loaded), no
        // position table, nothing under a third family's name
        for (size_t i = 0; i < ld.got.size(); ++i) {
            const Family g = fam_of(ld.got[i]);
            const int id = i < T_LAYER0 ? -1 : (int)((i - T_LAYER0) % L_COUNT);
            const bool qkv = id >= L_QW && id <= L_VB;
            if (!ld.got[i] || i == T_TYPE || (qkv ? g == DEBERTA : g == BERT && i != T_POS)) continue;
            return i == T_POS ? err(KR_EINVAL, "'embeddings.position_embeddings.weight' on a DeBERTa handle: position_biased_input is not implemented, the positions enter the attention only")
                              : err(KR_EINVAL, "'%s' on a DeBERTa handle (config.deberta_position_buckets): it takes attention.self.{query,key,value}_proj and BERT's names for every other tensor",
                                    slot_tensor_name(i, g).c_str());
        }
        if (!ld.rel_rows) return err(KR_ESTATE, "'encoder.rel_embeddings.weight' was never loaded");
        if (ld.rel_rows != 2 * Bk)
            return err(KR_EINVAL, "'encoder.rel_embeddings.weight' has %d rows, config.deberta_position_buckets = %d needs %d", ld.rel_rows, Bk, 2 * Bk);
        if (ld.rel_ln[0] != ld.rel_ln[1])
            return err(KR_ESTATE, "'encoder.LayerNorm.%s' was never loaded: the norm over the position table takes its weight and its bias or neither", ld.rel_ln[0] ? "bias" : "weight");
    } else {
        if (ld.rel_rows || ld.rel_ln[0] || ld.rel_ln[1])
            return err(KR_EINVAL, "'%s' but config.deberta_position_buckets was never loaded: load it and config.deberta_max_relative_positions before kr_encoder_finalize",
                       ld.rel_rows ? "encoder.rel_embeddings.weight" : ld.rel_ln[0] ? "encoder.LayerNorm.weight" : "encoder.LayerNorm.bias");
        for (size_t i = 0; i < ld.got.size(); ++i)
            if (fam_of(ld.got[i]) == DEBERTA)
                return err(KR_EINVAL, "'%s' but config.deberta_position_buckets was never loaded: load it and config.deberta_max_relative_positions before kr_encoder_finalize",
                           slot_tensor_name(i, DEBERTA).c_str());
    }
    if (t5 && (pad_idx >= 0 || rot || modern || local_set))
        return err(KR_EINVAL, "config.t5_feed_forward next to config.position_padding_idx / config.rotary_inv_freq* / config.local_attention_layers / "
                              "config.attention_half_window: a T5 handle's one position scheme is its relative attention bias");
    if (!modern && local_set)
        return err(KR_EINVAL, "config.rotary_inv_freq_local / config.attention_half_window without config.local_attention_layers: they are settings of a ModernBert handle");
    if (modern) {
        if (pad_idx >= 0 || rel) return err(KR_EINVAL, "config.local_attention_layers next to config.position_padding_idx / a relative attention bias: a handle has one position scheme");
        if (!rot) return err(KR_EINVAL, "config.local_attention_layers without config.rotary_inv_freq: a ModernBert handle rotates q and k");
        if ((int)flags.size() != cfg.layers) return err(KR_EINVAL, "config.local_attention_layers holds %zu flags, the handle has %d layers", flags.size(), cfg.layers);
        bool any_local = false;
        for (float f : flags) any_local = any_local || f != 0.f;
        if (any_local && (!set.has(SET_ROTARY_LOCAL) || !set.has(SET_HALF_WINDOW)))
            return err(KR_EINVAL, "config.local_attention_layers flags local layers, but %s was never loaded", SETTINGS[set.has(SET_ROTARY_LOCAL) ? SET_HALF_WINDOW : SET_ROTARY_LOCAL].name);
    }
    // names and family agree: ModernBert's and T5's names on their own handles only, and nothing but them there (the token-type row has no name of theirs);
    // the bias table under the family's own name
    for (const Family f : {MODERN, T5})
        for (size_t i = 0; i < ld.got.size(); ++i) {
            if (!ld.got[i] || i == T_TYPE || (fam_of(ld.got[i]) == f) == (fam == f) || (dec && i == T_WORD)) continue;
            return fam == f ? err(KR_EINVAL, "weight slot %zu was loaded under another family's name: a handle with %s takes %s's names", i, SETTINGS[f == T5 ? SET_T5_FF : SET_LOCAL_LAYERS].name, family_name(f))
                            : err(KR_EINVAL, "weight slot %zu was loaded under a %s name but %s was never loaded: load it before kr_encoder_finalize", i, family_name(f),
                                  SETTINGS[f == T5 ? SET_T5_FF : SET_LOCAL_LAYERS].name);
        }
    if (rel && (ld.rel_fam == T5) != t5)
        return err(KR_EINVAL, t5 ? "a handle with config.t5_feed_forward takes its bias table as encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"
                                 : "a relative attention bias under T5's name but config.t5_feed_forward was never loaded: load it before kr_encoder_finalize");
    // the heads, in the table's order (a refusal names the first tensor of the head that was loaded): family, neighbours, whole
    for (int h = 0; h < HEAD_ALL; ++h) {
        const HeadDesc& d = HEADS[h];
        const HeadState& s = ld.heads[h];
        if (!s.got) continue;
        if (!(d.families & (1u << fam))) return err(KR_EINVAL, "'%s' on a %s handle: %s", head_first(h, s), family_name(fam), d.accepted);
        for (int x = 0; x < 4 && d.excludes[x] >= 0; ++x)
            if (const int o = d.excludes[x]; ld.heads[o].got)
                return err(KR_EINVAL, "'%s' next to '%s': a handle has %s or %s, not both", head_first(h, s), HEADS[o].subject ? HEADS[o].subject : HEADS[o].t[0].name, d.noun, HEADS[o].noun);
        for (int i = 0; i < d.n; ++i)
            if ((d.t[i].flags & REQUIRED) && !(s.got & (1u << i))) return err(KR_ESTATE, "'%s' was never loaded: %s", d.t[i].name, d.whole);
    }
    // the sentence-transformers tail (its three settings, its Dense head) stands alone: never next to another head
    for (int h = 0; h < HEAD_ALL; ++h) {
        if (h == HEAD_ST_DENSE || !ld.heads[h].got) continue;
        const char* other = HEADS[h].subject ? HEADS[h].subject : HEADS[h].t[0].name;
        if (ld.heads[HEAD_ST_DENSE].got)
            return err(KR_EINVAL, "'%s' next to '%s': a handle has %s or %s, not both", head_first(HEAD_ST_DENSE, ld.heads[HEAD_ST_DENSE]), other, HEADS[HEAD_ST_DENSE].noun, HEADS[h].noun);
        for (const Setting st : {SET_NORMALIZE_OUT, SET_POOL_TOKENS, SET_ST_ACT})
            if (set.has(st))
                return err(KR_EINVAL, "%s next to '%s': the settings of a sentence-transformers pipeline are accepted on handles without %s", SETTINGS[st].name, other, HEADS[h].noun);
    }
    if (set.has(SET_ST_ACT) && !ld.heads[HEAD_ST_DENSE].got)
        return err(KR_EINVAL, "config.st_dense_activation on a handle without st_dense.weight: it selects the activation of the sentence-transformers Dense head");
    if (set.has(SET_CLS_POOLING) && !(modern && ld.heads[HEAD_MODERN_CLS].got))
        return err(KR_EINVAL, "config.classifier_pooling on a %s: it selects the row ModernBert's classification head reads",
                   modern ? "ModernBert handle without head.dense / head.norm / classifier" : "handle that is no ModernBert handle");
    if (t5) {
        for (int li = 0; li < cfg.layers; ++li) {
            const uint8_t* g = &ld.got[T_LAYER0 + (size_t)li * L_COUNT];
            if (g[L_IW] && ((g[L_IW] & GATED_NAME) != 0) != (t5_ff == 1))
                return err(KR_EINVAL, "layer %d: config.t5_feed_forward = %d takes DenseReluDense.%s", li, t5_ff, t5_ff ? "wi_0 / wi_1, not wi" : "wi, not wi_0 / wi_1");
            if (g[L_UW] && t5_ff == 0) return err(KR_EINVAL, "layer %d: config.t5_feed_forward = 0 takes DenseReluDense.wi, not wi_0 / wi_1", li);
        }
        if (!rel) return err(KR_ESTATE, "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight was never loaded");
    }
    if (rot && (pad_idx >= 0 || rel)) return err(KR_EINVAL, "config.rotary_inv_freq next to config.position_padding_idx / a relative attention bias: a handle has one position scheme");
    // q / k and the intermediate projection are packed in another row order under NomicBert's names (enc_load_weight): names and family must agree
    for (int li = 0; li < cfg.layers && !modern && !t5 && !dec; ++li) {
        const uint8_t* g = &ld.got[T_LAYER0 + (size_t)li * L_COUNT];
        auto under = [&](int id, bool nomic) { return g[id] && (fam_of(g[id]) == NOMIC) == nomic; };
        if (rbert) {
            // q / k in the rotary packed-row order (NomicBert's names) and their biases in the same order (the decoders'); fc1 in plain order (its own name)
            const size_t base = T_LAYER0 + (size_t)li * L_COUNT;
            if (under(L_QW, false) || under(L_KW, false))
                return err(KR_EINVAL, "layer %d: a handle with config.rotary_inv_freq takes self_attn.{q,k}_proj under NomicBert's names", li);
            for (const int id : {L_IW, L_UW})
                if (g[id] && fam_of(g[id]) != ROTARY_BERT)
                    return err(KR_EINVAL, "'%s' on a rotary BERT handle (config.rotary_feed_forward = 1): its feed-forward is mlp.fc1 / mlp.fc2, not a gated projection",
                               slot_tensor_name(base + id, fam_of(g[id])).c_str());
            for (const int id : {L_QB, L_KB, L_IB})
                if (g[id] && fam_of(g[id]) != (id == L_IB ? ROTARY_BERT : DECODER))
                    return err(KR_EINVAL, "'%s' on a rotary BERT handle (config.rotary_feed_forward = 1): it takes self_attn.{q,k,v,o}_proj.bias and mlp.{fc1,fc2}.bias",
                               slot_tensor_name(base + id, fam_of(g[id])).c_str());
            continue;
        }
        if (rot && (under(L_QW, false) || under(L_KW, false) || under(L_IW, false)))
            return err(KR_EINVAL, "layer %d: a handle with config.rotary_inv_freq takes self_attn.{q,k}_proj and mlp.{gate,up}_proj under NomicBert's names", li);
        if (rot && (g[L_QB] || g[L_KB] || g[L_IB])) return err(KR_EINVAL, "layer %d: the q / k / gate / up projections of a NomicBert handle have no bias", li);
        if (!rot && (under(L_QW, true) || under(L_KW, true) || under(L_IW, true) || g[L_UW]))
            return err(KR_EINVAL, "layer %d holds tensors under NomicBert's names but config.rotary_inv_freq was never loaded: load it before kr_encoder_finalize", li);
    }
    const FamilyRow& fr = FAMILIES[fam];
    plan = ModelPlan{};
    for (size_t i = 0; i < ld.got.size(); ++i) {
        const int layer = i < T_LAYER0 ? -1 : (int)((i - T_LAYER0) / L_COUNT), id = i < T_LAYER0 ? (int)i : (int)((i - T_LAYER0) % L_COUNT);
        const bool needed = layer < 0 ? (fr.embed >> id) & 1u : ((fr.layer >> id) & 1u) || (id == L_UW && t5_ff == 1);
        if (ld.got[i]) continue;
        if (needed) return err(KR_ESTATE, "weight slot %zu (layer %d, tensor %d) was never loaded", i, layer, id);
        plan.zero_fill.push_back((int)i);
    }
    plan.family = fam; plan.pre_ln = fr.pre_ln; plan.rms = fr.rms; plan.rotary = rot; plan.rotary_local = set.has(SET_ROTARY_LOCAL); plan.rel_bias = rel;
    plan.pos = deb ? POS_DISENT : t5 ? POS_BIAS_ONLY : rot ? POS_ROTARY : pad_idx >= 0 ? POS_FAIRSEQ : POS_COLUMN;
    plan.deb_buckets = Bk; plan.deb_max_rel = max_rel; plan.deb_norm = deb && ld.rel_ln[0]; plan.cls_gelu = deb;
    plan.pad_idx = pad_idx; plan.half_window = set.value(SET_HALF_WINDOW, 0);
    for (int li = 0; li < cfg.layers; ++li)
        plan.layers.push_back({!rot ? QKV_PLAIN : qk_norm ? QKV_SPLIT : (modern && ld.got[T_LAYER0 + (size_t)li * L_COUNT + L_QB]) ||
                                                    ((dec || rbert) && (ld.got[T_LAYER0 + (size_t)li * L_COUNT + L_QB] || ld.got[T_LAYER0 + (size_t)li * L_COUNT + L_KB])) ? QKV_ROT_BIAS : QKV_ROT,
                               dec ? (set.value(SET_DECODER_ATTN) == 1 ? AM_CAUSAL : AM_PLAIN) : deb ? AM_DISENT : rel ? AM_BIAS : modern && flags[li] != 0.f ? AM_WIN : AM_PLAIN});
    plan.ff = t5 ? (t5_ff ? FF_GEGLU_TANH : FF_RELU) : modern ? FF_GEGLU : rot && !rbert ? FF_SWIGLU : FF_GELU;
    plan.ff_gated = plan.ff == FF_GEGLU_TANH || plan.ff == FF_GEGLU || plan.ff == FF_SWIGLU;
    plan.out_dim = cfg.hidden;
    plan.kv_dim = kv_dim; plan.head_w = head_w; plan.q_dim = q_dim; plan.qk_norm = qk_norm;
    for (int h = 0; h < HEAD_ALL; ++h) {
        plan.head[h] = ld.heads[h].got != 0;
        plan.head_dim[h] = ld.heads[h].dim;
        if (plan.head[h]) plan.ws |= HEADS[h].ws;
    }
    if (plan.head[HEAD_DENSE]) plan.out_dim = plan.head_dim[HEAD_DENSE];
    if (plan.head[HEAD_ST_DENSE]) plan.out_dim = plan.head_dim[HEAD_ST_DENSE];
    plan.normalize = set.value(SET_NORMALIZE_OUT, 1) != 0; plan.pool_tokens = set.value(SET_POOL_TOKENS, 0); plan.st_tanh = set.value(SET_ST_ACT, 0) == 1;
    plan.classifier = plan.head[HEAD_CLS] ? (int)HEAD_CLS : plan.head[HEAD_MODERN_CLS] ? (int)HEAD_MODERN_CLS : plan.head[HEAD_SCORE] ? (int)HEAD_SCORE : -1;
    plan.classify_mean = set.value(SET_CLS_POOLING) == 1;
    plan.out_width = plan.classifier >= 0 && plan.head_dim[plan.classifier] > plan.out_dim ? plan.head_dim[plan.classifier] : plan.out_dim;
    return Error{};
}

// What a forward with `pool` (KR_POOL_*, the token-level flags taken off) runs on a finalized handle.  KR_POOL_CLASSIFY, KR_POOL_SPLADE and KR_POOL_LAST pack
// and attend like another pool and differ behind the last layer only:
//   pack      what the packing front end and the attention see: KR_POOL_CLS (a query-only row for a masked column 0, the packed token count) or KR_POOL_MEAN
//   select    the row k_pool reads: KR_POOL_MEAN, KR_POOL_CLS or KR_POOL_LAST (a splade forward does not pool)
//   classify  k_pool leaves the raw row to the classifier (ModelPlan::classifier); score: that head is a decoder's HEAD_SCORE, on the last row;
//             ModernBert's with config.classifier_pooling = 1 reads the masked mean
//   splade    the MLM head on every row in place of pooling
//   one_row   behind the last layer's attention one row per sequence is read, the CLS row or the score head's last row: the layer may finish on those rows alone
struct ForwardPool { int pack, select; bool classify, score, splade, one_row; };
inline ForwardPool resolve_pool(const ModelPlan& p, int pool) {
    ForwardPool f{pool, pool, pool == KR_POOL_CLASSIFY, false, pool == KR_POOL_SPLADE, false};
    f.score = f.classify && p.classifier == HEAD_SCORE;
    if (f.classify) f.select = f.score ? KR_POOL_LAST : p.classify_mean ? KR_POOL_MEAN : KR_POOL_CLS;
    if (f.splade) f.select = KR_POOL_MEAN;
    f.pack = f.select == KR_POOL_LAST ? KR_POOL_MEAN : f.select;
    f.one_row = f.pack == KR_POOL_CLS || f.score;
    return f;
}

}  // namespace model
}  // namespace kr
