// The life of an Encoder handle outside the forward, per operand type (included by encoder.hip behind the handle): creation and destruction, the name-addressed
// loader (where every slot, head tensor and setting of encoder_model.hpp is stored on the device) and finalize (describe() -> the plan, zero fills, tables).
#pragma once

namespace kr {
namespace KR_ENC_NS {

static int refuse(const model::Error& er) { return er.code ? fail(er.code, "%s", er.msg.c_str()) : 0; }

// the head width d_h and Dq = heads d_h, the width of q and of the context: hidden / heads and hidden unless the handle was given config.head_dim
static int head_width(const Encoder* e) { return e->set.value(model::SET_HEAD_DIM, e->cfg.hidden / e->cfg.heads); }
static int64_t q_width(const Encoder* e) { return (int64_t)e->cfg.heads * head_width(e); }

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
    e->ld = model::Loaded(cfg->layers);
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

// a "config.*" name: the values come to the host, the settings table (encoder_model.hpp) does the rest
static int set_config(Encoder* e, const char* name, const float* data, int64_t numel) {
    std::vector<float> v;
    if (model::find_setting(name) >= 0 && numel >= 1 && numel <= model::SETTING_MAX_VALUES) {
        v.resize((size_t)numel);
        KR_HIP(hipMemcpy(v.data(), data, (size_t)numel * 4, hipMemcpyDefault));
    }
    const bool head_dim = model::find_setting(name) == model::SET_HEAD_DIM;
    if (head_dim && !e->finalized_once)      // the packed QKV matrix, o_proj and the bias rows are laid out by it
        for (size_t i = model::T_LAYER0; i < e->ld.got.size(); ++i) {
            const int id = (int)((i - model::T_LAYER0) % model::L_COUNT);
            if (e->ld.got[i] && id >= model::L_QW && id <= model::L_OW) return fail(KR_EINVAL, "config.head_dim behind a layer's attention tensors: load it before the weights");
        }
    bool stored = false;
    KR_TRY(refuse(model::set_setting(e->cfg, e->set, e->ld.heads, e->finalized_once, name, v.data(), numel, stored)));
    if (stored) e->ready = false;
    if (stored && head_dim) {
        // [Dq + 2A, H] with A <= Dq, [H, Dq] and the q | k | v bias rows at the handle's own width (enc_create allocated them for Dq = H)
        const size_t H = e->cfg.hidden, Dq = (size_t)q_width(e);
        free_ws(e);
        for (auto& l : e->L) {
            (void)hipFree(l.wqkv); l.wqkv = nullptr; (void)hipFree(l.wo); l.wo = nullptr; (void)hipFree(l.bqkv); l.bqkv = nullptr;      // (own_bufs keeps pointing at the members)
            KR_HIP(hipMalloc(reinterpret_cast<void**>(&l.wqkv), 3 * Dq * H * 2)); KR_HIP(hipMalloc(reinterpret_cast<void**>(&l.wo), H * Dq * 2));
            KR_HIP(hipMalloc(reinterpret_cast<void**>(&l.bqkv), 3 * Dq * 4));
        }
    }
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

// A DeBERTa handle's tables (encoder_pos.hpp, AttnDisentArgs): the bucket of every column difference the position table allows, and per layer PQ = query_proj(R),
// PK = key_proj(R) of R = LayerNorm(rel_embeddings) (the raw table without encoder.LayerNorm), [heads][TP][d_h] in the 16-bit operand type.  R is normalised
// on the host in double and rounded once; the projections are fp32 sums from the fp32 copies of the two matrices the loader kept (LayerW::wq32 / wk32).  PQ
// carries the score scale log2(e) / sqrt(3 d_h) that the loader folded into query_proj's matrix for the 16-bit copy and into its bias.
static int build_disent_tables(Encoder* e) {
    const model::ModelPlan& p = e->plan;
    const int H = e->cfg.hidden, dh = H / e->cfg.heads, Bk = p.deb_buckets, rows = 2 * Bk, TP = (int)round_up(rows, 32), P = e->cfg.max_pos;
    std::vector<int> bucket((size_t)2 * P - 1);
    for (int r = -(P - 1); r <= P - 1; ++r) bucket[(size_t)(r + P - 1)] = model::deberta_bucket(r, Bk, p.deb_max_rel);
    if (!e->deb_bucket) KR_TRY(dmalloc(e->own_bufs, &e->deb_bucket, bucket.size() * 4));
    KR_HIP(hipMemcpy(e->deb_bucket, bucket.data(), bucket.size() * 4, hipMemcpyHostToDevice));
    std::vector<float> R((size_t)rows * H);
    for (int r = 0; r < rows; ++r) {
        const float* x = &e->rel_emb[(size_t)r * H];
        if (!p.deb_norm) { std::copy(x, x + H, &R[(size_t)r * H]); continue; }
        double mean = 0.0, var = 0.0;
        for (int c = 0; c < H; ++c) mean += x[c];
        mean /= H;
        for (int c = 0; c < H; ++c) var += ((double)x[c] - mean) * ((double)x[c] - mean);
        const double rstd = 1.0 / std::sqrt(var / H + (double)e->cfg.ln_eps);
        for (int c = 0; c < H; ++c) R[(size_t)r * H + c] = (float)(((double)x[c] - mean) * rstd * (double)e->rel_lng[c] + (double)e->rel_lnb[c]);
    }
    const float qscale = (float)(1.4426950408889634 / std::sqrt(3.0 * dh));
    const size_t tab_bytes = (size_t)e->cfg.heads * TP * dh * 2;
    for (auto& l : e->L) {
        if (l.pq16) continue;
        KR_TRY(dmalloc(e->own_bufs, &l.pq16, tab_bytes)); KR_TRY(dmalloc(e->own_bufs, &l.pk16, tab_bytes));
        KR_HIP(hipMemset(l.pq16, 0, tab_bytes)); KR_HIP(hipMemset(l.pk16, 0, tab_bytes));      // the rows behind 2 Bk stay zero
    }
    float* dR = nullptr;
    KR_HIP(hipMalloc(reinterpret_cast<void**>(&dR), R.size() * 4));
    hipError_t rc = hipMemcpy(dR, R.data(), R.size() * 4, hipMemcpyHostToDevice);
    for (auto& l : e->L) {
        if (rc != hipSuccess) break;
        const unsigned g = (unsigned)(((int64_t)rows * H + 255) / 256);
        hipLaunchKernelGGL(k_pos_table, dim3(g), dim3(256), 0, 0, dR, l.wq32, l.bqkv, qscale, rows, TP, H, dh, l.pq16);
        hipLaunchKernelGGL(k_pos_table, dim3(g), dim3(256), 0, 0, dR, l.wk32, l.bqkv + H, 1.f, rows, TP, H, dh, l.pk16);
    }
    if (rc == hipSuccess) rc = hipGetLastError();
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    (void)hipFree(dR);
    KR_HIP(rc);
    return 0;
}

// cos / sin [max_pos][d_h / 2] with HF's arithmetic (NomicBertRotaryEmbedding.forward): the angle is the fp32 product float(pos) * inv_freq[j], the entry the
// cosine / sine of that fp32 angle (evaluated in double and rounded once).  One pair of tables per frequency vector: the handle's (global) one, and for
// ModernBert handles with local layers the local one.
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

static size_t head_tensor_bytes(const Encoder* e, int head, int idx, int dim) {
    const model::HeadTensor& t = model::HEADS[head].t[idx];
    return (size_t)(model::extent(e->cfg, t.store_r, dim) * model::extent(e->cfg, t.c)) * ((t.flags & model::HALF) ? 2 : 4);
}

// one tensor of a head (the rule and the shapes: encoder_model.hpp, HEADS): allocated on first sight, zero behind the tensor's own rows where it is stored with more
static int load_head_tensor(Encoder* e, int head, int idx, const float* data, int64_t numel) {
    const model::HeadDesc& d = model::HEADS[head];
    model::HeadState& s = e->ld.heads[head];
    int dim = 0;
    KR_TRY(refuse(model::check_head_tensor(e->cfg, head, idx, numel, s, e->finalized_once, dim)));
    void*& dst = e->head_p[head][idx];
    if (!dst) {
        KR_TRY(dmalloc(e->own_bufs, &dst, head_tensor_bytes(e, head, idx, dim)));
        if (d.t[idx].store_r != d.t[idx].r) KR_HIP(hipMemset(dst, 0, head_tensor_bytes(e, head, idx, dim)));
    }
    if (d.t[idx].flags & model::HALF) KR_TRY(upload_16bit(data, numel, static_cast<uint16_t*>(dst)));
    else KR_HIP(hipMemcpy(dst, data, (size_t)numel * 4, hipMemcpyDefault));
    if (d.ws && (!s.got || s.dim != dim)) free_ws(e);      // buffers that exist with the head, or are sized by its free dimension
    s.dim = dim;
    s.got |= 1u << idx;
    e->ready = false;
    return 0;
}

// where an fp32 slot (norm parameter, bias, the small embedding tables) lives and how many floats it holds; nullptr: a matrix, or a table this handle never got
static float* slot_f32(Encoder* e, int slot, size_t* count = nullptr) {
    using namespace model;
    const size_t H = e->cfg.hidden;
    size_t n = H;
    float* p = nullptr;
    if (slot < T_LAYER0) {
        float* const emb[] = {nullptr, e->pos, e->type, e->elng, e->elnb};
        p = emb[slot];
        if (slot == T_TYPE) n = (size_t)e->cfg.type_vocab * H;
    } else {
        LayerW& l = e->L[(slot - T_LAYER0) / L_COUNT];
        const size_t Dq = (size_t)q_width(e);      // the q | k | v bias rows: Dq floats each (v's per query head)
        switch ((slot - T_LAYER0) % L_COUNT) {
            case L_QB: p = l.bqkv; n = Dq; break;
            case L_KB: p = l.bqkv + Dq; n = Dq; break;
            case L_VB: p = l.bqkv + 2 * Dq; n = Dq; break;
            case L_OB: p = l.bo; break;
            case L_LN1G: p = l.ln1g; break;
            case L_LN1B: p = l.ln1b; break;
            case L_IB: p = l.b1; n = (size_t)e->cfg.intermediate; break;
            case L_FB: p = l.b2; break;
            case L_LN2G: p = l.ln2g; break;
            case L_LN2B: p = l.ln2b; break;
        }
    }
    if (count) *count = n;
    return p;
}

int enc_load_weight(void* h, const char* hf_name, const float* data, int64_t numel) {
    using namespace model;
    if (!h || !hf_name || !data) return fail(KR_EINVAL, "NULL argument");
    Encoder* e = reinterpret_cast<Encoder*>(h);
    KR_TRY(select_device(e->device));
    if (std::strncmp(hf_name, "config.", 7) == 0) return set_config(e, hf_name, data, numel);
    if (int head, idx; find_head_tensor(hf_name, head, idx)) return load_head_tensor(e, head, idx, data, numel);
    Resolved r;
    KR_TRY(refuse(resolve_name(e->cfg, hf_name, r)));
    const int slot = r.slot, layer = r.layer;
    // NomicBert's and ModernBert's names: q / k (rotary partners) and the gated projection's rows go into tile-pair order; T5's: wi_0 | wi_1 only
    const bool paired = r.fam == NOMIC || r.fam == MODERN, gated = paired || r.gated;
    KR_TRY(refuse(check_tensor(e->cfg, hf_name, r, numel, e->ld, e->finalized_once, e->set.value(SET_HEAD_DIM, 0))));
    if (slot == T_IGNORED) return 0;   // pooler.* / position_ids: not used by the encoders (encoders.py:74,115 take last_hidden_state)
    const int64_t dh = head_width(e), Dq = q_width(e);
    if (slot == T_QNORM || slot == T_KNORM) {
        // the weight of a layer's q / k norm, fp32 [d_h]; q's carries the score scale log2(e) / sqrt(d_h) (k_qk_norm_rope)
        float*& dst = slot == T_QNORM ? e->L[layer].qng : e->L[layer].kng;
        if (!dst) KR_TRY(dmalloc(e->own_bufs, &dst, (size_t)dh * 4));
        std::vector<float> g((size_t)numel);
        KR_HIP(hipMemcpy(g.data(), data, (size_t)numel * 4, hipMemcpyDefault));
        if (slot == T_QNORM) for (float& x : g) x *= (float)(1.4426950408889634 / std::sqrt((double)dh));
        KR_HIP(hipMemcpy(dst, g.data(), (size_t)numel * 4, hipMemcpyHostToDevice));
        mark_loaded(e->ld, r);
        e->ready = false;
        return 0;
    }
    if (slot <= T_RELEMB) {            // DeBERTa's position table and its norm, kept as loaded on the host: finalize builds every layer's PQ / PK from them (build_disent_tables)
        std::vector<float>& dst = slot == T_RELEMB ? e->rel_emb : slot == T_RELLNG ? e->rel_lng : e->rel_lnb;
        dst.resize((size_t)numel);
        KR_HIP(hipMemcpy(dst.data(), data, (size_t)numel * 4, hipMemcpyDefault));
        mark_loaded(e->ld, r);
        e->ready = false;
        return 0;
    }
    if (slot == T_RELBIAS) {           // kept as loaded on the host: finalize builds the table the attention kernels read (build_bias_table)
        e->rel_w.resize((size_t)numel);
        KR_HIP(hipMemcpy(e->rel_w.data(), data, (size_t)numel * 4, hipMemcpyDefault));
        mark_loaded(e->ld, r);
        e->ready = false;
        return 0;
    }
    if ((size_t)numel > e->stage_elems) {
        if (e->stage) (void)hipFree(e->stage);
        e->stage = nullptr; e->stage_elems = 0;
        KR_HIP(hipMalloc(reinterpret_cast<void**>(&e->stage), (size_t)numel * 4));
        e->stage_elems = (size_t)numel;
    }
    KR_HIP(hipMemcpy(e->stage, data, (size_t)numel * 4, hipMemcpyDefault));
    const int64_t H = e->cfg.hidden, FF = e->cfg.intermediate;
    // log2(e) / sqrt(d_h) is folded into the query projection: the attention scores come out in log2 units and the softmax is a bare exp2.  The multiply is
    // fp32, before the 16-bit conversion (d_h = 32: the factor is not a power of two; d_h = 64: the same bits as log2(e) / 8).  T5's scores are q.k + bias,
    // no 1 / sqrt(d_h): under T5's names log2(e) alone is folded in
    // DeBERTa's scores are (q.k + q.PK + k.PQ) / sqrt(3 d_h): under DeBERTa's names that factor
    const float qscale = r.fam == T5 ? (float)1.4426950408889634
                       : r.fam == DEBERTA ? (float)(1.4426950408889634 / std::sqrt(3.0 * (double)(H / e->cfg.heads))) : (float)(1.4426950408889634 / std::sqrt((double)dh));
    // rows [n / H, H] from element `first` of the staged copy; mode >= 0: into tile-pair order (k_f32_to_bf16_rows)
    auto to_bf16 = [&](uint16_t* dst, int64_t first, int64_t n, float scale, int mode) {
        const unsigned g = (unsigned)((n + 255) / 256);
        if (mode < 0) hipLaunchKernelGGL(k_f32_to_bf16, dim3(g), dim3(256), 0, 0, e->stage + first, dst, n, scale);
        else hipLaunchKernelGGL(k_f32_to_bf16_rows, dim3(g), dim3(256), 0, 0, e->stage + first, dst, n, (int)H, scale, mode);
    };
    const int head64 = paired && dh == 64 ? (int)ROWS_HEAD64 : -1;
    // the tensors that fill w1 allocate it: [FF, H], or gated [2 FF, H]; a layer holds one kind
    auto claim_w1 = [&](LayerW& l, int li) -> int {
        if (l.w1 && l.gated != gated)
            return fail(KR_EINVAL, "'%s': layer %d already holds %s", hf_name, li, gated ? "a plain intermediate projection" : "a gated projection (gate_proj / up_proj, wi_0 / wi_1, mlp.Wi)");
        if (!l.w1) KR_TRY(dmalloc(e->own_bufs, &l.w1, (size_t)H * FF * (gated ? 4 : 2)));
        l.gated = gated;
        return 0;
    };
    if (slot == T_WQKV) {
        // Wqkv [3H, H] = q | k | v row blocks (heads contiguous inside each): the blocks the loader fills for the other families
        LayerW& l = e->L[layer];
        to_bf16(l.wqkv, 0, H * H, qscale, head64); to_bf16(l.wqkv + H * H, H * H, H * H, 1.f, head64); to_bf16(l.wqkv + 2 * H * H, 2 * H * H, H * H, 1.f, -1);
    } else if (slot == T_WI) {
        LayerW& l = e->L[layer];
        KR_TRY(claim_w1(l, layer));
        to_bf16(l.w1, 0, H * FF, 1.f, ROWS_GATE); to_bf16(l.w1, H * FF, H * FF, 1.f, ROWS_UP);
    } else if (slot == T_WQKVB || slot == T_WIB) {
        // q | k | v biases: q with the fold, q and k in their rows' order (added before the rotation: EPI_QKV_ROTB), v as always (folded into bo_eff);
        // mlp.Wi.bias: input | gate in the order of w1's rows
        LayerW& l = e->L[layer];
        if (slot == T_WIB && !l.b1p) KR_TRY(dmalloc(e->own_bufs, &l.b1p, (size_t)numel * 4));
        std::vector<float> b((size_t)numel), pb((size_t)numel);
        KR_HIP(hipMemcpy(b.data(), e->stage, (size_t)numel * 4, hipMemcpyDeviceToHost));
        if (slot == T_WQKVB)
            for (int64_t i = 0; i < H; ++i) {
                const int64_t d = head64 >= 0 ? tile_pair_row(i, ROWS_HEAD64) : i;
                pb[(size_t)d] = b[(size_t)i] * qscale; pb[(size_t)(H + d)] = b[(size_t)(H + i)]; pb[(size_t)(2 * H + i)] = b[(size_t)(2 * H + i)];
            }
        else
            for (int64_t i = 0; i < FF; ++i) { pb[(size_t)tile_pair_row(i, ROWS_GATE)] = b[(size_t)i]; pb[(size_t)tile_pair_row(i, ROWS_UP)] = b[(size_t)(FF + i)]; }
        KR_HIP(hipMemcpy(slot == T_WQKVB ? l.bqkv : l.b1p, pb.data(), (size_t)numel * 4, hipMemcpyHostToDevice));
    } else if (slot >= 0) {
        const int li = slot < T_LAYER0 ? -1 : (slot - T_LAYER0) / L_COUNT, id = slot < T_LAYER0 ? -1 : (slot - T_LAYER0) % L_COUNT;
        if (slot == T_POS && !e->pos) KR_TRY(dmalloc(e->own_bufs, &e->pos, (size_t)numel * 4));
        if (id == L_IW || id == L_UW) KR_TRY(claim_w1(e->L[li], li));
        if (r.fam == DECODER && (id == L_QB || id == L_KB)) {
            // a decoder's q / k bias (Qwen2): in the order of the projection's packed rows and, q's, with its fold — added before the rotation (EPI_QKV_ROTB),
            // as ModernBert's attn.Wqkv.bias above
            std::vector<float> b((size_t)numel), pb((size_t)numel);
            KR_HIP(hipMemcpy(b.data(), e->stage, (size_t)numel * 4, hipMemcpyDeviceToHost));
            // (k's comes with its own A = numel entries: whole 64-wide heads, so the row order applies per head as in the matrix)
            const bool h64 = dh == 64;
            for (int64_t i = 0; i < numel; ++i) pb[(size_t)(h64 ? tile_pair_row(i, ROWS_HEAD64) : i)] = b[(size_t)i] * (id == L_QB ? qscale : 1.f);
            KR_HIP(hipMemcpy(slot_f32(e, slot), pb.data(), (size_t)numel * 4, hipMemcpyHostToDevice));
        } else if (r.fam == DECODER && id == L_VB && numel != Dq) {
            // a grouped-query value bias [A]: kept per QUERY head, [H], where the plain one lives — the QKV epilogue never reads it, k_fold_vbias folds
            // Wo . bv into bo_eff over the context's H columns, and column c of the context is head c / d_h, which reads KV head (c / d_h) / group
            const int64_t group = Dq / numel;
            std::vector<float> b((size_t)numel), pb((size_t)Dq);
            KR_HIP(hipMemcpy(b.data(), e->stage, (size_t)numel * 4, hipMemcpyDeviceToHost));
            for (int64_t i = 0; i < Dq; ++i) pb[(size_t)i] = b[(size_t)((i / dh / group) * dh + i % dh)];
            KR_HIP(hipMemcpy(slot_f32(e, slot), pb.data(), (size_t)Dq * 4, hipMemcpyHostToDevice));
        } else if (float* dst = slot == T_WORD ? e->word : slot_f32(e, slot))
            hipLaunchKernelGGL(k_scale_copy, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, 0, e->stage, dst, numel, id == L_QB ? qscale : 1.f);
        else {
            LayerW& l = e->L[li];
            if (r.fam == DEBERTA && (id == L_QW || id == L_KW)) {      // the fp32 matrix stays: finalize projects the position table with it (build_disent_tables)
                float*& keep = id == L_QW ? l.wq32 : l.wk32;
                if (!keep) KR_TRY(dmalloc(e->own_bufs, &keep, (size_t)numel * 4));
                KR_HIP(hipMemcpy(keep, e->stage, (size_t)numel * 4, hipMemcpyDeviceToDevice));
            }
            switch (id) {
                case L_QW: to_bf16(l.wqkv, 0, numel, qscale, head64); l.qfold = qscale; break;
                // the packed matrix is [H + 2A, H]: q's rows, k's from row H, v's from row H + A, A = numel / H the tensor's own row count (H unless it is a
                // grouped-query decoder's: describe() holds k's against v's) — so the load order stays free
                // (Dq rows of q: H unless the handle has config.head_dim)
                case L_KW: to_bf16(l.wqkv + Dq * H, 0, numel, 1.f, head64); break;
                case L_VW: to_bf16(l.wqkv + Dq * H + numel, 0, numel, 1.f, -1); break;
                case L_OW: to_bf16(l.wo, 0, numel, 1.f, -1); break;
                case L_IW: to_bf16(l.w1, 0, numel, 1.f, gated ? (int)ROWS_GATE : -1); break;
                case L_UW: to_bf16(l.w1, 0, numel, 1.f, ROWS_UP); break;
                case L_FW: to_bf16(l.w2, 0, numel, 1.f, -1); break;
            }
        }
    }
    KR_HIP(hipGetLastError());
    KR_HIP(hipDeviceSynchronize());
    mark_loaded(e->ld, r);
    e->ready = false;
    return 0;
}

int enc_finalize(void* h) {
    using namespace model;
    if (!h) return fail(KR_EINVAL, "NULL argument");
    Encoder* e = reinterpret_cast<Encoder*>(h);
    ModelPlan plan;
    KR_TRY(refuse(describe(e->cfg, e->set, e->ld, plan)));
    e->plan = std::move(plan);
    const ModelPlan& p = e->plan;
    if (e->stage) { (void)hipFree(e->stage); e->stage = nullptr; e->stage_elems = 0; }
    KR_TRY(select_device(e->device));
    const int H = e->cfg.hidden;
    auto zeros = [&](auto** buf, size_t bytes) -> int {
        if (!*buf) { KR_TRY(dmalloc(e->own_bufs, buf, bytes)); KR_HIP(hipMemset(*buf, 0, bytes)); }
        return 0;
    };
    // what the family or a head leaves optional is zero unless loaded: linear biases and norm betas, a head's optional tensors, ModernBert's mlp.Wi.bias (in
    // its rows' order: b1p); the zero row the embedding of a rotary handle adds in place of a position row, and k_ln16_head in place of a bias
    for (int slot : p.zero_fill) {
        size_t n = 0;
        if (float* dst = slot_f32(e, slot, &n)) KR_HIP(hipMemset(dst, 0, n * 4));
    }
    for (int hd = 0; hd < HEAD_ALL; ++hd)
        for (int i = 0; p.head[hd] && i < HEADS[hd].n; ++i) KR_TRY(zeros(&e->head_p[hd][i], head_tensor_bytes(e, hd, i, p.head_dim[hd])));
    if (p.ff == FF_GEGLU)
        for (auto& l : e->L) KR_TRY(zeros(&l.b1p, (size_t)2 * e->cfg.intermediate * 4));
    if (p.rotary || p.head[HEAD_MLM] || p.pos == POS_DISENT) KR_TRY(zeros(&e->zero_row, (size_t)H * 4));
    if (p.rotary) KR_TRY(build_rotary_table(e, e->set.v[SET_ROTARY], &e->rot_cos, &e->rot_sin));
    if (p.rotary_local) KR_TRY(build_rotary_table(e, e->set.v[SET_ROTARY_LOCAL], &e->rot_cos_l, &e->rot_sin_l));
    for (auto& l : e->L) hipLaunchKernelGGL(k_fold_vbias, dim3((H + 127) / 128), dim3(128), 0, 0, l.wo, l.bo, l.bqkv + 2 * p.q_dim, l.bo_eff, H, p.q_dim);
    if (p.rel_bias) KR_TRY(build_bias_table(e));
    KR_HIP(hipGetLastError());
    if (p.family == DEBERTA) KR_TRY(build_disent_tables(e));
    KR_HIP(hipDeviceSynchronize());
    e->ready = true;
    e->finalized_once = true;
    return 0;
}

}  // namespace KR_ENC_NS
}  // namespace kr
