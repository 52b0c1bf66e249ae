// Sentence encoder, the attention: device code (AttnState ... k_attn_lds, k_attn_dma) and, behind it, the host code that launches it (launch_attn_lds,
// launch_attn_dma, launch_attention).  Part of encoder.hip (see its header).
#pragma once
#include "encoder_rows.hpp"

#include <type_traits>

namespace kr {
namespace KR_ENC_NS {

// ---------------------------------------------------------------------------------------------------------
// attention.  Two kernels share ONE arithmetic (attn_step64: the same MFMAs, the same softmax operations in the same order), so a sequence's context
// rows are bit-identical whichever kernel its batch selects (the embedding cache and batch invariance rely on it):
//   k_attn_lds  sequences of at most 128 tokens: K / V^T of the block's heads staged through registers, one block per (sequence, HPB heads, 4 / HPB q-tiles)
//   k_attn_dma  longer sequences: K / V^T chunks of 64 keys stream through a 3-stage LDS ring by LDS-DMA (two chunks in flight behind the one being
//               multiplied, one barrier per chunk), one block per (sequence, head, 8 q-tiles): two q-tiles per wave share every staged chunk
// (DeBERTa's disentangled position terms, AttnDisentArgs below, are built into k_attn_lds only: such a handle runs it at every length.)
// Common scheme per wave and 32-query tile: S^T = K.Q^T (keys on accumulator rows, so the softmax row reductions are in-lane + one shfl_xor 32), online
// softmax over 64-key steps, P^T fed from the accumulator straight into the V^T.P^T MFMA.  The key that sits on A-tile row i of a 32-key tile is
// perm(i) = i with bits 2 and 3 exchanged: a lane's registers 8a .. 8a+7 then hold 8 CONSECUTIVE keys (16 a + 8 hf .. + 7), i.e. the P^T fragment of a
// k-step matches one contiguous 16-byte run of a V^T row (without the permutation a lane owns keys {0..3, 8..11} + 4 hf: two 8-byte reads per fragment).
// The permutation maps each ds_read_b128 lane group onto itself, so the K reads stay bank-conflict free.
// Everything is a template on the head width DH (32, 64 or 128): S^T takes DH / 16 k-steps of the 32x32x16 MFMA, O^T is DH / 32 accumulators of 32 d rows.
// (DH = 128 — Qwen3 handles — is built into the register-staged body only and launched as k_attn_wide, at every sequence length; it has no bias-table and no
// disentangled mode.)
//   K image   rows of 2 DH bytes (DH / 8 16-B chunks), chunk index XOR attn_kswz<DH>(key): DH = 64 128-B rows, XOR ((key >> 1) & 7) (same image as the
//             GEMM ring); DH = 32 64-B rows, XOR ((key >> 2) & 3); DH = 128 256-B rows (every row starts on bank 0), XOR (key & 15).  Either way the 16 lanes
//             of a ds_read_b128 group (keys {0..3, 12..15, 20..27} or {4..11, 16..19, 28..31} of a 32-key tile: key & 15 takes 16 different values in both)
//             land on 16 different 16-B slots of a 256-B bank window
//   V^T image k_attn_lds: DH rows, row pitch 2 * cap + 8 bytes (pitch / 8 odd: conflict-free ds_read_b64), keys >= nk stored as zero;
//             k_attn_dma: [DH d][128 B] per chunk, chunk index XOR ((d >> 1) & 7) like the 64-wide K image (one ds_read_b128 per fragment), columns >= nk
//             of the last chunk zeroed in LDS after they landed (no 0 * NaN from rows of other sequences).
// The O tile is staged through a wave-private LDS block of 32 x 2 DH bytes and stored as whole 2 DH-byte rows of ctx at column head * DH.
// ---------------------------------------------------------------------------------------------------------
template <int DH>
struct AttnState {
    static_assert(DH == 32 || DH == 64 || DH == 128, "head width 32, 64 or 128");
    f32x16 o[DH / 32];  // O^T of the tile: d rows 32 j .. 32 j + 31 in o[j]
    float mref, l;      // reference maximum (log2 units) the accumulated o / l are scaled by; running denominator
};

template <int DH>
__device__ __forceinline__ void attn_init(AttnState<DH>& s) {
#pragma unroll
    for (int j = 0; j < DH / 32; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) s.o[j][r] = 0.f;
    s.mref = -INFINITY; s.l = 0.f;
}

__device__ __forceinline__ int attn_perm(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }

// 16-B chunk swizzle of row `key` of a K image with 2 DH-byte rows (128 / DH rows per 256-B bank window; DH = 128: one)
template <int DH>
__device__ __forceinline__ int attn_kswz(int key) { return (key >> (DH == 128 ? 0 : DH == 64 ? 1 : 2)) & (DH / 8 - 1); }

// One 64-key step of a wave's 32-query tile.  Kst: K image (128-B rows, swizzled), k0 = row of the step's first key in it; nvalid = keys of the
// step that exist (MASKED instantiation: < 64; <= 32: the second 32-key tile is skipped — it would only add exact zeros); vfrag(dh, ks) returns the
// V^T A-fragment of d rows 32 dh .. + 31, keys k0 + 16 ks + 8 hf .. + 7.
// Scores are in log2 units (log2(e) / sqrt(d_h) is folded into W_q at load time), so P = exp2(s - mref) is one subtraction and one v_exp_f32 per
// element.  The reference maximum mref of a query is only raised — with the o / l rescale of the online softmax — when a step's maximum exceeds it by
// more than ATTN_RESCALE_THR (2^8: P stays far inside the 16-bit range, and o / l are fp32); any mref gives the same result up to rounding because it
// cancels in o / l.  The slow path is taken by the whole wave (wave-uniform branch), so a tile's P.V is never split.  (Feeding -mref to the S^T MFMAs
// as their C operand would save the subtraction too, but costs 16 more live registers per tile: measured as spills at three blocks per CU.)
constexpr float ATTN_RESCALE_THR = 8.0f;

// Relative attention bias (MPNet): score(head, query, key) += W[bucket(col_key - col_query)][head], col = the token's column in the padded batch (tok_pos).
// The kernels read a per-handle fp32 table built at finalize: `width` floats per head, entry width / 2 + d = log2(e) * W[bucket(d)][head] for every column
// difference d the position table allows (plus 64 entries of slack on both sides for the keys a masked tile reads past the sequence).  The bias TILE of a step
// is loaded into the (dead) score registers and handed to the first S^T MFMA as its C operand in place of the zero tile: no add instruction, no extra live
// registers, and a zero table starts the chain from the same zeros as the instantiation without a bias.  Both kernels and both ways of finding the column
// difference load the same table entries into the same operand, so a sequence's rows do not depend on which of them ran.
//   consecutive columns (right / left padding, ragged input): key column = col0 + packed key index: a lane's 8 consecutive keys are 8 consecutive entries
//   holes in the mask (or KIRAG_AMD_ATTN_BIAS_GATHER=1): the column of every key is read from tok_pos
// The query's column is always read from tok_pos (the extra CLS query row sits behind the keys in the packed order and has column 0).
struct AttnBiasArgs {
    const float* tab;     // [heads][width]
    const int* col;       // tok_pos: column of every packed row
    int width;            // floats per head (even); the entry of difference 0 is width / 2
    int gather;           // != 0: take every key's column from `col` even when they are consecutive
};
struct AttnNoBiasArgs {};
// Sliding-window ("local") attention (ModernBert's sliding_attention layers): key admitted iff |col_key - col_query| <= w, col = the token's column in the
// padded batch (tok_pos), on top of the padding mask.  The key columns come the same two ways as for the bias.  An excluded score becomes -inf after the
// S^T chains; the steps that can hold no admitted key for a wave's whole 32-query tile are skipped (AttnBand), by ONE rule in both kernels.
// The window has a left and a right extent: admitted iff -wl <= col_key - col_query <= wr.  ModernBert's is symmetric (wl = wr = w).  CAUSAL attention (decoder
// handles: key column <= query column) is the same test with wr = 0 and a wl no column difference reaches (max_pos): one compare per score, the band's upper
// end is the tile's own last query, so every 64-key step above a tile's diagonal is skipped and k_attn_dma stages about half the chunks of a long sequence.
struct AttnWinArgs {
    const int* col;       // tok_pos
    int wl, wr;           // extents to the left (keys before the query) and to the right, wl + wr >= 1
    int gather;           // != 0: take every key's column from `col` even when they are consecutive
};
// Disentangled attention (DeBERTa-v2 / v3): score(head, query i, key j) += q_i . PK[p] + k_j . PQ[p], p = deberta_bucket(col_i - col_j) (encoder_model.hpp),
// in the log2 units of q . k (the scale log2(e) / sqrt(3 d_h) is folded into query_proj and into PQ).  Both products of every packed row with every table row a
// batch can reach are computed per layer by k_pos_scores (encoder_pos.hpp) into `sc`: [row][head][C2P | P2C][W] fp32, entry w = bucket p0 + w.  The bias TILE
// of a step is gathered from there — C2P from the lane's own query row, P2C from each key's row (for a fixed key the 32 lanes read consecutive entries) — and
// handed to the first S^T MFMA as its C operand, where attn_bias_tile puts MPNet's values.  Every key's column comes from tok_pos (the gather path), so right
// padding, left padding and holes in the mask are one code path, and a sequence's rows depend on column DIFFERENCES only.
struct AttnDisentArgs {
    const float* sc;      // [rows][heads][2][W]
    const int* col;       // tok_pos
    const int* bucket;    // [2 max_pos - 1]: entry max_pos - 1 + r = deberta_bucket(r)
    int center;           // max_pos - 1
    int p0, W;            // the buckets [p0, p0 + W) are computed for this batch
    int heads;
};
template <bool BIAS, bool WIN = false, bool DIS = false>
using AttnBiasArg = std::conditional_t<DIS, AttnDisentArgs, std::conditional_t<BIAS, AttnBiasArgs, std::conditional_t<WIN, AttnWinArgs, AttnNoBiasArgs>>>;

// BM (mode of a kernel body, block-uniform): 0 plain, 1 bias with consecutive key columns, 2 bias with gathered key columns, 3 window with consecutive key
// columns, 4 / 5 window with gathered key columns (4: k_attn_dma, 16-byte loads; 5: k_attn_lds, one load per key — the same values either way).  The choice between 1 and 2 (3 and 4) is made once per block, outside the key loops (a branch inside them
// costs the accumulators register copies at every join).  6: disentangled position terms (gathered key columns, k_attn_lds only)
template <int BM> using AttnModeArg = AttnBiasArg<BM == 1 || BM == 2, BM >= 3 && BM <= 5, BM == 6>;
struct AttnNoBias { static constexpr bool on = false, win = false; };
template <int GATHER>       // 0: consecutive key columns, 1: gathered with 16-byte loads, 2: gathered key by key
struct AttnWinLane {
    static constexpr bool on = false, win = true;
    const int* col;       // columns of the sequence's packed rows (GATHER)
    int base;             // wl - column of this lane's query (+ 8 hf + the column of key 0 when the columns are consecutive)
    unsigned w2;          // wl + wr: admitted <=> (unsigned)(col_key - col_query + wl) <= wl + wr
    int nk;
};
template <bool GATHER>
struct AttnBiasLane {
    static constexpr bool on = true, win = false;
    const float* tab;     // table of the head (wave-uniform)
    const int* col;       // columns of the sequence's packed rows (GATHER)
    int lane0;            // width / 2 - column of this lane's query + 8 hf (+ the column of key 0 when the columns are consecutive)
    int nk;
};
struct AttnDisentLane {
    static constexpr bool on = true, win = false;
    const float* sc;      // row 0 of the sequence in AttnDisentArgs::sc (wave-uniform)
    const int* col;       // columns of the sequence's packed rows
    const int* bucket;
    int i0;               // center + column of this lane's query: bucket[i0 - col_key] = p
    unsigned qoff;        // this lane's C2P row (query, head) in floats from sc, less p0
    unsigned hoff;        // the head's P2C row of key 0 in floats from sc, less p0 (wave-uniform)
    unsigned stride;      // floats per packed row
    int nk;
};
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte load at a 4-byte aligned address (one global_load_dwordx4)
typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));

// does sequence (off, nk) need the gathered key columns?  (the packers write the attended columns in increasing order: consecutive <=> last - first = nk - 1)
template <class Args>
__device__ __forceinline__ bool attn_bias_gathers(const Args& ba, int64_t off, int nk) {
    return ba.gather != 0 || (nk >= 2 && ba.col[off + nk - 1] - ba.col[off] != nk - 1);
}

template <int BM>
__device__ __forceinline__ auto attn_bias_lane(const AttnModeArg<BM>& ba, int64_t off, int nk, int head, int qi, int hf) {
    if constexpr (BM == 6) {
        // offsets inside one sequence: (max_pos + 1 <= 8193 rows) x (stride <= 2^16 floats) < 2^30 floats
        const int* col = ba.col + off;
        AttnDisentLane dl;
        dl.stride = 2u * (unsigned)ba.W * (unsigned)ba.heads;
        dl.sc = ba.sc + off * (int64_t)dl.stride;
        dl.col = col;
        dl.bucket = ba.bucket;
        dl.i0 = ba.center + col[qi];
        dl.hoff = (unsigned)(head * 2 * ba.W + ba.W - ba.p0);
        dl.qoff = (unsigned)qi * dl.stride + (unsigned)(head * 2 * ba.W - ba.p0);
        dl.nk = nk;
        return dl;
    } else if constexpr (BM >= 3) {
        const int* col = ba.col + off;
        AttnWinLane<BM - 3> wl;
        wl.col = col;
        wl.base = ba.wl - col[qi] + (BM == 3 ? 8 * hf + (nk > 0 ? col[0] : 0) : 0);
        wl.w2 = (unsigned)ba.wl + (unsigned)ba.wr;
        wl.nk = nk;
        return wl;
    } else if constexpr (BM != 0) {
        const int* col = ba.col + off;
        AttnBiasLane<BM == 2> bl;
        bl.tab = ba.tab + (int64_t)head * ba.width;
        bl.col = col;
        bl.lane0 = (ba.width >> 1) - col[qi] + 8 * hf + (BM == 1 && nk > 0 ? col[0] : 0);
        bl.nk = nk;
        return bl;
    } else {
        return AttnNoBias{};
    }
}

// the bias of one 32-key tile in the layout of the score registers: register r = key kb + 16 (r >> 3) + 8 hf + (r & 7) of the sequence, this lane's query
template <bool GATHER>
__device__ __forceinline__ void attn_bias_tile(f32x16& st, const AttnBiasLane<GATHER>& bl, int kb, int hf) {
    __builtin_amdgcn_sched_barrier(0);      // the loads stay behind the previous step: hoisted into it they would need registers next to its live score tiles
    if constexpr (!GATHER) {
        const float* p = bl.tab + (unsigned)(bl.lane0 + kb);     // unsigned 32-bit lane offset on a wave-uniform base: one address register per lane
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const f32x4u x = *reinterpret_cast<const f32x4u*>(p + 16 * a), y = *reinterpret_cast<const f32x4u*>(p + 16 * a + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { st[8 * a + i] = x[i]; st[8 * a + 4 + i] = y[i]; }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kb + 16 * (r >> 3) + 8 * hf + (r & 7);
            st[r] = bl.tab[(unsigned)(bl.lane0 - 8 * hf + bl.col[(unsigned)min(key, bl.nk - 1)])];     // keys >= nk are masked below: any entry will do
        }
    }
}
// the disentangled position terms of one 32-key tile, same register layout
__device__ __forceinline__ void attn_bias_tile(f32x16& st, const AttnDisentLane& dl, int kb, int hf) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = min(kb + 16 * (r >> 3) + 8 * hf + (r & 7), dl.nk - 1);      // keys >= nk are masked below: any entry will do
        const unsigned p = (unsigned)dl.bucket[(unsigned)(dl.i0 - dl.col[(unsigned)key])];
        st[r] = dl.sc[dl.qoff + p] + dl.sc[(unsigned)key * dl.stride + dl.hoff + p];
    }
}
// the window of one 32-key tile: scores of keys outside -wl <= col_key - col_query <= wr become -inf (kb = index of the tile's first key in its sequence)
template <int GATHER>
__device__ __forceinline__ void attn_window_tile(f32x16& st, const AttnWinLane<GATHER>& wl, int kb, int hf) {
    if constexpr (GATHER == 0) {
        const int t0 = wl.base + kb;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = ((unsigned)(t0 + 16 * (r >> 3) + (r & 7)) <= wl.w2) ? st[r] : -INFINITY;
    } else if constexpr (GATHER == 2) {
        // (k_attn_lds runs at its 168-register limit: four consecutive registers per load do not fit there)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kb + 16 * (r >> 3) + 8 * hf + (r & 7);
            st[r] = ((unsigned)(wl.base + wl.col[(unsigned)min(key, wl.nk - 1)]) <= wl.w2) ? st[r] : -INFINITY;     // keys >= nk are masked by the step's MODE
        }
    } else {
        // a lane's 8 consecutive keys of a 16-key group are 8 consecutive entries of the column table: two 16-byte loads on one lane address.  The entries of
        // keys >= nk (other sequences' rows; tok_pos has 64 entries of slack behind the last token, ensure_ws) are masked by the step's MODE
        const int* p = wl.col + (unsigned)(kb + 8 * hf);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const i32x4u x = *reinterpret_cast<const i32x4u*>(p + 16 * a), y = *reinterpret_cast<const i32x4u*>(p + 16 * a + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                st[8 * a + i] = ((unsigned)(wl.base + x[i]) <= wl.w2) ? st[8 * a + i] : -INFINITY;
                st[8 * a + 4 + i] = ((unsigned)(wl.base + y[i]) <= wl.w2) ? st[8 * a + 4 + i] : -INFINITY;
            }
        }
    }
}

// Which 64-key steps a wave's 32-query tile (first query q0) visits under a window.  Attended columns are packed in increasing order, so
// |col_i - col_j| >= |i - j|: every admissible key of packed query i < nk lies in packed [i - wl, i + wr], with or without holes in the mask (causal, wr = 0:
// packed index order IS column order, so the band [0, i] is exact).  The query-only
// CLS row (packed last, index nk, column 0; nq == nk + 1) admits keys of column <= wr: packed [0, wr] (a causal handle never packs one).  A step [kb, kb + 64) is visited iff it meets the
// union of the tile's bands; both kernels apply this rule to the same 64-aligned steps, so they run the same steps on a tile.
struct AttnBand {
    int lo, hi, xhi;      // packed keys [lo, hi] of the tile's key-bearing queries (hi < lo: none); [0, xhi] of the CLS row (xhi < 0: not in this tile)
    __device__ __forceinline__ bool visits(int kb) const { return (kb <= hi && kb + 63 >= lo) || kb <= xhi; }
};
__device__ __forceinline__ AttnBand attn_band(int q0, int q1, int nk, int nq, int wl, int wr) {      // queries [q0, q1] (q1 may lie past nq - 1)
    AttnBand b;
    b.lo = max(q0 - wl, 0);
    b.hi = q0 < nk ? min(q1, nk - 1) + wr : -1;
    b.xhi = (nq > nk && q1 >= nk) ? wr : -1;
    return b;
}

// first half of a step: the shifted-score tiles S^T = K . Q^T (st1 = -inf when the second 32-key tile does not exist)
// MODE (wave-uniform, picked from the number of valid keys of the step): 0 = 64, 1 = fewer than 32 (first tile masked, no second tile),
// 2 = exactly 32 (one full tile: a 32-token sequence), 3 = 33 .. 63 (second tile masked)
// PF (k_attn_dma): all K fragments of the step are requested before the first MFMA (counted lgkmcnt waits instead of one exposed LDS round trip per
// MFMA); same MFMAs in the same order, so the result does not depend on it
// BL: AttnNoBias, or AttnBiasLane with kb = index of the step's first key in its sequence: the chains start from the bias tiles instead of zero
template <int DH, int MODE, bool PF = false, class BL>
__device__ __forceinline__ void attn_scores(f32x16& st0, f32x16& st1, const uint4 (&qf)[DH / 16], const char* Kst, int k0, int nvalid, int c, int hf, const BL& bl, int kb) {
    constexpr bool two = MODE == 0 || MODE == 3;
    constexpr int NK = DH / 16, KR = 2 * DH;              // k-steps of S^T; bytes per K row
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (BL::on) attn_bias_tile(st0, bl, kb, hf);
    auto c0 = [&]() -> const f32x16& { if constexpr (BL::on) return st0; else return zero; };
    auto c1 = [&]() -> const f32x16& { if constexpr (BL::on) return st1; else return zero; };
    if constexpr (PF) {
        const int key = k0 + attn_perm(c);
        const char* krow = Kst + key * KR;
        const int swz = attn_kswz<DH>(key);
        uint4 kf[two ? 2 * NK : NK];
#pragma unroll
        for (int sk = 0; sk < NK; ++sk) kf[sk] = *reinterpret_cast<const uint4*>(krow + (((2 * sk + hf) ^ swz) << 4));
        if constexpr (two) {
#pragma unroll
            for (int sk = 0; sk < NK; ++sk) kf[NK + sk] = *reinterpret_cast<const uint4*>(krow + 32 * KR + (((2 * sk + hf) ^ swz) << 4));
        }
        st0 = ET::mfma(kf[0], qf[0], c0());
#pragma unroll
        for (int sk = 1; sk < NK; ++sk) st0 = ET::mfma(kf[sk], qf[sk], st0);
        if constexpr (two) {
            if constexpr (BL::on) attn_bias_tile(st1, bl, kb + 32, hf);     // after the first chain: its K fragments are dead by now
            st1 = ET::mfma(kf[NK], qf[0], c1());
#pragma unroll
            for (int sk = 1; sk < NK; ++sk) st1 = ET::mfma(kf[NK + sk], qf[sk], st1);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) st1[r] = -INFINITY;
        }
    } else {
        const int key = k0 + attn_perm(c);
        const char* krow = Kst + key * KR;
        const int swz = attn_kswz<DH>(key);
        st0 = ET::mfma(*reinterpret_cast<const uint4*>(krow + (((0 + hf) ^ swz) << 4)), qf[0], c0());
#pragma unroll
        for (int sk = 1; sk < NK; ++sk) st0 = ET::mfma(*reinterpret_cast<const uint4*>(krow + (((2 * sk + hf) ^ swz) << 4)), qf[sk], st0);
        if (two) {
            const char* krow1 = krow + 32 * KR;           // attn_kswz(key + 32) == swz
            if constexpr (BL::on) attn_bias_tile(st1, bl, kb + 32, hf);
            st1 = ET::mfma(*reinterpret_cast<const uint4*>(krow1 + (((0 + hf) ^ swz) << 4)), qf[0], c1());
#pragma unroll
            for (int sk = 1; sk < NK; ++sk) st1 = ET::mfma(*reinterpret_cast<const uint4*>(krow1 + (((2 * sk + hf) ^ swz) << 4)), qf[sk], st1);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) st1[r] = -INFINITY;      // never read (two == false below)
        }
    }
    // register r of this lane: key k0 + 16 (r >> 3) + 8 hf + (r & 7) (+ 32 for st1), query c.  Only the tile that holds key nvalid is partial (wave-uniform
    // cases: a 32-token sequence has exactly one full tile and nothing to mask)
    if constexpr (MODE == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st0[r] = (16 * (r >> 3) + 8 * hf + (r & 7) < nvalid) ? st0[r] : -INFINITY;
    }
    if constexpr (MODE == 3) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st1[r] = (16 * (r >> 3) + 8 * hf + (r & 7) + 32 < nvalid) ? st1[r] : -INFINITY;
    }
    if constexpr (BL::win) {
        attn_window_tile(st0, bl, kb, hf);
        if constexpr (two) attn_window_tile(st1, bl, kb + 32, hf);
    }
}

// second half: online softmax and O^T += V^T . P^T
template <int MODE, bool PF = false, int DH, class VFrag>
__device__ __forceinline__ void attn_softmax_pv(AttnState<DH>& s, const f32x16& st0, const f32x16& st1, VFrag&& vfrag) {
    constexpr bool two = MODE == 0 || MODE == 3;
    constexpr int ND = DH / 32;                          // accumulators of O^T
    uint4 vpre[PF ? (two ? 4 : 2) * ND : 1];
    if constexpr (PF) {                                  // the V^T fragments land under the maximum / rescale arithmetic
#pragma unroll
        for (int ks = 0; ks < (two ? 4 : 2); ++ks)
#pragma unroll
            for (int j = 0; j < ND; ++j) vpre[ND * ks + j] = vfrag(j, ks);
    }
    float tmax = fmaxf(fmaxf(st0[0], st0[1]), st0[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) tmax = fmaxf(fmaxf(tmax, st0[r]), st0[r + 1]);   // v_max3_f32
    tmax = fmaxf(tmax, st0[15]);
    if (two) {
#pragma unroll
        for (int r = 0; r < 16; r += 2) tmax = fmaxf(fmaxf(tmax, st1[r]), st1[r + 1]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const bool fresh = s.mref == -INFINITY;               // nothing accumulated for this query yet
    if (__builtin_amdgcn_ballot_w64(fresh || tmax > s.mref + ATTN_RESCALE_THR) != 0ull) {
        // raise the reference (never lower it)
        const float mnew = fmaxf(s.mref, tmax);
        const float alpha = fresh ? 1.f : __builtin_amdgcn_exp2f(s.mref - mnew);   // fresh: o = l = 0 (and mref - mnew is -inf - x)
        s.l *= alpha;
#pragma unroll
        for (int j = 0; j < ND; ++j) s.o[j] *= alpha;
        s.mref = mnew;
    }
    const float mshift = (s.mref == -INFINITY) ? 0.f : s.mref;   // still -inf: no valid key so far, every score is -inf and stays so
    // P = exp2(s - mref) and O^T += V^T . P^T, one k-step (8 keys per lane: registers 8 a .. 8 a + 7 = keys 16 a + 8 hf .. + 7 of the tile) at a time: the
    // exp2 / pack of a k-step sit between the MFMAs of the previous one, and at most 8 probabilities are live next to the scores
    float psum = 0.f;
    auto pv = [&](const f32x16& stx, int ks0) {
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float e[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) { e[i] = __builtin_amdgcn_exp2f(stx[8 * a + i] - mshift); psum += e[i]; }
            uint4 pf;
            pf.x = pack_bf16x2(e[0], e[1]); pf.y = pack_bf16x2(e[2], e[3]); pf.z = pack_bf16x2(e[4], e[5]); pf.w = pack_bf16x2(e[6], e[7]);
            if constexpr (PF) {
#pragma unroll
                for (int j = 0; j < ND; ++j) s.o[j] = ET::mfma(vpre[ND * (ks0 + a) + j], pf, s.o[j]);
            } else {
#pragma unroll
                for (int j = 0; j < ND; ++j) s.o[j] = ET::mfma(vfrag(j, ks0 + a), pf, s.o[j]);
            }
        }
    };
    pv(st0, 0);
    if (two) pv(st1, 2);
    psum += __shfl_xor(psum, 32, 64);
    s.l += psum;
}

template <int MODE, bool PF = false, int DH, class VFrag, class BL>
__device__ __forceinline__ void attn_step64m(AttnState<DH>& s, const uint4 (&qf)[DH / 16], const char* Kst, int k0, int nvalid, int c, int hf, VFrag&& vfrag, const BL& bl, int kb) {
    f32x16 st0, st1;
    attn_scores<DH, MODE, PF>(st0, st1, qf, Kst, k0, nvalid, c, hf, bl, kb);
    attn_softmax_pv<MODE, PF>(s, st0, st1, vfrag);
}
// MASKED = false: 64 valid keys; true: fewer (nvalid says how many).  bl / kb: the relative attention bias of the lane and the step's first key (attn_scores)
template <bool MASKED, bool PF = false, int DH, class VFrag, class BL>
__device__ __forceinline__ void attn_step64(AttnState<DH>& s, const uint4 (&qf)[DH / 16], const char* Kst, int k0, int nvalid, int c, int hf, VFrag&& vfrag, const BL& bl, int kb) {
    if constexpr (!MASKED) attn_step64m<0, PF>(s, qf, Kst, k0, 64, c, hf, vfrag, bl, kb);
    else if (nvalid == 32) attn_step64m<2>(s, qf, Kst, k0, nvalid, c, hf, vfrag, bl, kb);
    else if (nvalid < 32) attn_step64m<1>(s, qf, Kst, k0, nvalid, c, hf, vfrag, bl, kb);
    else attn_step64m<3>(s, qf, Kst, k0, nvalid, c, hf, vfrag, bl, kb);
}

// (H: the row pitch of ctx, heads * DH)
// normalise a finished 32-query tile and store it as whole 2 DH-byte rows of ctx (columns head * DH ..) through the wave-private LDS block Os of
// 32 x 2 DH bytes (8-byte chunk index XOR the row)
// ZERO_EMPTY (window instantiations): a query whose window holds no attended key (the CLS row of a masked column 0 whose sequence starts beyond column w)
// gets a zero context row instead of 0 / 0
template <int DH, bool ZERO_EMPTY = false>
__device__ __forceinline__ void attn_store_tile(const AttnState<DH>& s, char* Os, uint16_t* __restrict__ ctx, int64_t off, int q0, int nq, int H, int head, int lane) {
    constexpr int RB = 2 * DH, C8 = DH / 4, LR = DH / 8;  // row bytes, 8-byte chunks per row, lanes per row in the store
    asm volatile("" : "+v"(lane));   // opaque: the store addresses are computed here, after the key loop, instead of living in registers (or scratch) across it
    const int c = lane & 31, hf = lane >> 5;
    // a query with no attendable key (all-masked sequence) is 0/0 = NaN, as under HF's -inf masking
    const float inv = (ZERO_EMPTY && s.l == 0.f) ? 0.f : 1.0f / s.l;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        uint2 w[DH / 32];
#pragma unroll
        for (int j = 0; j < DH / 32; ++j) {
            w[j].x = pack_bf16x2(s.o[j][4 * gq + 0] * inv, s.o[j][4 * gq + 1] * inv); w[j].y = pack_bf16x2(s.o[j][4 * gq + 2] * inv, s.o[j][4 * gq + 3] * inv);
        }
#pragma unroll
        for (int j = 0; j < DH / 32; ++j) {
            const int j8 = 8 * j + 2 * gq + hf;     // 8-byte chunk (4 features) of the row of query c
            *reinterpret_cast<uint2*>(Os + c * RB + ((j8 ^ (c & (C8 - 1))) << 3)) = w[j];
        }
    }
#pragma unroll
    for (int p4 = 0; p4 < 32 * LR / 64; ++p4) {
        const int rq = p4 * (64 / LR) + (lane >> (DH == 128 ? 4 : DH == 64 ? 3 : 2)), ch = lane & (LR - 1);
        const uint2 lo = *reinterpret_cast<const uint2*>(Os + rq * RB + (((2 * ch) ^ (rq & (C8 - 1))) << 3));
        const uint2 hi = *reinterpret_cast<const uint2*>(Os + rq * RB + (((2 * ch + 1) ^ (rq & (C8 - 1))) << 3));
        if (q0 + rq < nq) *reinterpret_cast<uint4*>(ctx + (off + q0 + rq) * H + head * DH + ch * 8) = make_uint4(lo.x, lo.y, hi.x, hi.y);
    }
}

// HPB = heads per block: 1 when a sequence has >= 3 q-tiles, 2 / 4 for short sequences so that all four waves have work (the choice follows the q-tiles,
// not the head width).
// __launch_bounds__(256, 3) at DH = 64: at most 168 registers per lane, which makes hipcc keep the MFMA accumulators in VGPRs; with the default bound it
// put them in AGPRs and spent 112 of the 276 VALU instructions of a key tile on v_accvgpr_read / _write around the softmax rescale.  A 32-wide head
// stages half the bytes (<= 25 KiB per block for any HPB, see launch_attn_lds) and keeps half the Q fragments and accumulators: four blocks per CU (<= 128
// registers).
// Grouped-query attention: query head h reads KV head h / group, group = heads / kv_heads.  The kernels take the group as kv_mul = 65536 / group + 1
// (attn_kv_mul, host): (h * kv_mul) >> 16 == h / group for every h < 1024 and group <= 64 (h (kv_mul group - 65536) < 65536) — a multiply and a shift where a
// division by a kernel argument is a reciprocal sequence in every block of the short-sequence launches.  group = 1: kv_mul = 65537, the head itself.
__host__ __device__ inline int attn_kv_mul(int group) { return 65536 / group + 1; }
__device__ __forceinline__ int attn_kv_head(int head, int kv_mul) { return (int)(((unsigned)head * (unsigned)kv_mul) >> 16); }
template <int DH> constexpr int attn_lds_blocks() { return DH == 128 ? 1 : DH == 64 ? 3 : 4; }
template <int DH, int HPB, int BM>
__device__ __forceinline__ void attn_lds_body(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ vT, int64_t ldv,
                                              const int* __restrict__ seq_off, const int* __restrict__ seq_nk, const int* __restrict__ seq_nq,
                                              int H, int heads, int kchunk, uint16_t* __restrict__ ctx, int ldk, int kv_mul, const AttnModeArg<BM>& ba, char* smem) {
    constexpr bool WIN = BM >= 3 && BM <= 5;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction; as a scalar, the head / q-tile / LDS bases derived from it cost no VGPRs
    const int hb = blockIdx.x, b = blockIdx.y;            // heads fastest: the heads of one sequence (same 2-KiB q/k rows) run together
    const int nq = seq_nq[b];
    constexpr int QT = 4 / HPB;                           // q-tiles per block (one per wave and head)
    const int q0 = ((int)blockIdx.z * QT + wave / HPB) * 32;
    if ((int)blockIdx.z * QT * 32 >= nq) return;          // block-uniform: no q-tile of this block exists (nq == 0 included)
    const int nk = seq_nk[b];
    const int64_t off = seq_off[b];
    constexpr int KR = 2 * DH, NC = DH / 8, NCS = DH == 128 ? 4 : DH == 64 ? 3 : 2;   // K row bytes, 16-B chunks per K row (1 << NCS)
    const int vpitch = kchunk * 2 + 8;
    char* Ks = smem;                                      // [HPB][kchunk][KR]
    char* Vs = smem + (size_t)HPB * kchunk * KR;          // [HPB][DH][vpitch]
    // the O staging: behind V^T, or at DH = 128 (4 x 8 KiB) over the K / V^T area once every wave is done with it (the barrier behind the key loop): 65 KiB per
    // block at kchunk = 128 instead of 97 (launch_attn_wide)
    char* Os = (DH == 128 ? smem : Vs + (size_t)HPB * DH * vpitch) + wave * (32 * KR);
    const int hs = wave % HPB;
    const int head = hb * HPB + hs;
    const bool active = head < heads && q0 < nq;          // inactive waves still stage and meet every barrier
    const char* Kh = Ks + (size_t)hs * kchunk * KR;
    const char* Vh = Vs + (size_t)hs * DH * vpitch;
    const int c = lane & 31, hf = lane >> 5;
    // Q^T as the B operand: lane (c, hf) holds Q[q0 + c][16 s + 8 hf .. +7], s = 0 .. DH / 16 - 1
    uint4 qf[DH / 16] = {};
    const auto bl = attn_bias_lane<BM>(ba, off, nk, head, min(q0 + c, nq - 1), hf);    // nq >= 1 here; an inactive wave never reads through it
    if (active) {
        const int qi = (q0 + c < nq) ? (q0 + c) : (nq - 1);
        const uint16_t* qrow = q + (off + qi) * H + head * DH;
#pragma unroll
        for (int s = 0; s < DH / 16; ++s) qf[s] = *reinterpret_cast<const uint4*>(qrow + 16 * s + 8 * hf);
    }
    AttnState<DH> st;
    attn_init(st);
    // window: the steps this wave's tile visits, and the chunks any tile of the block visits (block-uniform: the others are not staged)
    AttnBand band{}, bband{};
    if constexpr (WIN) {
        band = attn_band(q0, q0 + 31, nk, nq, ba.wl, ba.wr);
        bband = attn_band((int)blockIdx.z * QT * 32, (int)blockIdx.z * QT * 32 + QT * 32 - 1, nk, nq, ba.wl, ba.wr);
    }
    constexpr int NB = HPB == 1 ? 4 : 2;                  // loads in flight per thread, head and batch (register budget: 3 blocks per CU = 168 VGPRs; HPB = 4 means <= 32 keys: 2 cover a head)
    for (int kc0 = 0; kc0 < nk; kc0 += kchunk) {
        // ---- stage keys [kc0, kc0 + kchunk) of the block's heads: every global load of a batch is issued before the first LDS store
        // (a load -> store loop would serialise one memory round trip per iteration)
        const int nkc = min(nk - kc0, kchunk);            // keys of this chunk
        if constexpr (WIN) {
            bool any = false;
            for (int k0 = 0; k0 < nkc; k0 += 64) any = any || bband.visits(kc0 + k0);
            if (!any) continue;
        }
        const int nkp = (nkc + 31) & ~31;
        const int cpr = nkp >> 2;                         // 8-byte chunks (4 keys) per V^T row
        const unsigned cpr_magic = 0xFFFFFFFFu / (unsigned)cpr + 1u;
        if (kc0 > 0) __syncthreads();                     // every wave is done with the previous chunk (or nothing was staged yet: harmless)
        {
            // all heads of the block in ONE batch: every global load (K and V^T of up to HPB heads) is issued before the first LDS store, so a block with
            // 2 / 4 heads pays one memory round trip per batch, not one per head (a 32-token sequence is a single batch)
            const int nkcs = nkp * NC, nvc = DH * cpr;
            int tid = threadIdx.x;
            asm volatile("" : "+v"(tid));      // opaque: the staging indices are derived per chunk and die with it (the key loop below runs at the register limit)
            for (int base = 0; base < nkcs || base < nvc; base += 256 * NB) {
                uint4 kv[HPB][NB]; uint2 vv[HPB][NB];
#pragma unroll
                for (int h2 = 0; h2 < HPB; ++h2) {
                    // K [T, ldk] and V^T [ldk, ldv] hold one head per KV head: query head h reads head h / group = attn_kv_head(h, kv_mul) (block-uniform: two
                    // scalar instructions).  The heads of a block are staged one by one even where two of them share a KV head
                    const int head2 = hb * HPB + h2, kvh = attn_kv_head(head2, kv_mul);
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const int i = base + j * 256 + tid;
                        const int key = i >> NCS, ch = i & (NC - 1);
                        kv[h2][j] = make_uint4(0u, 0u, 0u, 0u);
                        if (head2 < heads && i < nkcs && key < nkc) {
                            const uint16_t* kp = k + (off + kc0 + key) * ldk + kvh * DH + ch * 8;
                            kv[h2][j] = *reinterpret_cast<const uint4*>(kp);
                        }
                    }
                }
                // (d row, 8-byte chunk) of element i of the V^T staging: i / cpr and i % cpr (exact: i < 2^16, cpr <= 128); recomputed where needed (two VALU
                // instructions) instead of being kept in registers across the loads — the kernel runs at the 168-register limit of three blocks per CU
                auto vsplit = [&](int i, int& d, int& kc) { d = (int)__umulhi((unsigned)i, cpr_magic); kc = i - d * cpr; };
#pragma unroll
                for (int h2 = 0; h2 < HPB; ++h2) {
                    const int head2 = hb * HPB + h2, kvh = attn_kv_head(head2, kv_mul);
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const int i = base + j * 256 + tid;
                        int vd, vk; vsplit(i, vd, vk);
                        vv[h2][j] = make_uint2(0u, 0u);
                        if (head2 < heads && i < nvc && vk * 4 < nkc) {
                            const uint16_t* vp = vT + (int64_t)(kvh * DH + vd) * ldv + off + kc0 + vk * 4;   // off, kc0 % 4 == 0: 8-B aligned
                            vv[h2][j] = uint2(*reinterpret_cast<const uint2*>(vp));
                        }
                    }
                }
#pragma unroll
                for (int h2 = 0; h2 < HPB; ++h2) {
                    if (hb * HPB + h2 >= heads) continue;
                    char* Kw = Ks + (size_t)h2 * kchunk * KR;
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const int i = base + j * 256 + tid;
                        const int key = i >> NCS, ch = i & (NC - 1);
                        if (i < nkcs) *reinterpret_cast<uint4*>(Kw + key * KR + ((ch ^ attn_kswz<DH>(key)) << 4)) = kv[h2][j];
                    }
                }
#pragma unroll
                for (int h2 = 0; h2 < HPB; ++h2) {
                    if (hb * HPB + h2 >= heads) continue;
                    char* Vw = Vs + (size_t)h2 * DH * vpitch;
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const int i = base + j * 256 + tid;
                        int vd, vk; vsplit(i, vd, vk);
                        const int key0 = vk * 4;
                        uint2 v = vv[h2][j];
                        if (key0 + 4 > nkc) {      // keys >= nk (padding / the next sequence) are stored as zero
                            v.x &= (key0 + 0 < nkc ? 0xffffu : 0u) | (key0 + 1 < nkc ? 0xffff0000u : 0u);
                            v.y &= (key0 + 2 < nkc ? 0xffffu : 0u) | (key0 + 3 < nkc ? 0xffff0000u : 0u);
                        }
                        if (i < nvc) *reinterpret_cast<uint2*>(Vw + vd * vpitch + vk * 8) = v;
                    }
                }
            }
        }
        __syncthreads();
        if (!active) continue;
        // the full 64-key steps run in a loop of their own: with the masked variants inside the same loop the accumulators went through register
        // copies at every join (k0: key offset inside the chunk)
        const int kfull = nkc & ~63;
        for (int k0 = 0; k0 < kfull; k0 += 64) {
            auto vfrag = [&](int dh, int ks) {
                const char* v = Vh + (c + 32 * dh) * vpitch + (k0 + 16 * ks + 8 * hf) * 2;
                const uint2 a0 = *reinterpret_cast<const uint2*>(v), a1 = *reinterpret_cast<const uint2*>(v + 8);
                return make_uint4(a0.x, a0.y, a1.x, a1.y);
            };
            if constexpr (WIN) { if (!band.visits(kc0 + k0)) continue; }
            attn_step64<false>(st, qf, Kh, k0, 64, c, hf, vfrag, bl, kc0 + k0);
        }
        if (kfull < nkc && (!WIN || band.visits(kc0 + kfull))) {
            auto vfrag = [&](int dh, int ks) {
                const char* v = Vh + (c + 32 * dh) * vpitch + (kfull + 16 * ks + 8 * hf) * 2;
                const uint2 a0 = *reinterpret_cast<const uint2*>(v), a1 = *reinterpret_cast<const uint2*>(v + 8);
                return make_uint4(a0.x, a0.y, a1.x, a1.y);
            };
            attn_step64<true>(st, qf, Kh, kfull, nkc - kfull, c, hf, vfrag, bl, kc0 + kfull);
        }
    }
    if constexpr (DH == 128) __syncthreads();             // block-uniform: every wave of a block that got here meets it, active or not
    if (!active) return;
    attn_store_tile<DH, WIN>(st, Os, ctx, off, q0, nq, H, head, lane);
}

template <int DH, int HPB, bool BIAS = false, bool WIN = false, bool DIS = false>
__global__ __launch_bounds__(256, attn_lds_blocks<DH>()) void k_attn_lds(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ vT, int64_t ldv,
                                                  const int* __restrict__ seq_off, const int* __restrict__ seq_nk, const int* __restrict__ seq_nq,
                                                  int H, int heads, int kchunk, uint16_t* __restrict__ ctx, int ldk, int kv_mul, AttnBiasArg<BIAS, WIN, DIS> ba) {
    static_assert(!(BIAS && WIN) && !(DIS && (BIAS || WIN)), "a relative attention bias under a window is not instantiated, nor either next to the disentangled terms");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (DIS) {
        attn_lds_body<DH, HPB, 6>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
    } else if constexpr (WIN) {
        const int b = blockIdx.y;
        if (attn_bias_gathers(ba, seq_off[b], seq_nk[b])) attn_lds_body<DH, HPB, 5>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
        else attn_lds_body<DH, HPB, 3>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
    } else if constexpr (BIAS) {
        const int b = blockIdx.y;
        if (attn_bias_gathers(ba, seq_off[b], seq_nk[b])) attn_lds_body<DH, HPB, 2>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
        else attn_lds_body<DH, HPB, 1>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
    } else {
        attn_lds_body<DH, HPB, 0>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
    }
}

// 128-wide heads (Qwen3 handles): the register-staged body under a name of its own — four O^T accumulators and eight Q fragments per lane do not fit the 168
// registers k_attn_lds is held to.  ONE block per CU by registers: held to 256 VGPRs + AGPRs (__launch_bounds__(256, 2)) hipcc spills 10 vector registers
// in the plain and 31 - 37 in the window / causal instantiations (44 - 88 B of scratch per lane: reloads are VMEM operations inside the key loop), so the bound
// is (256, 1) and the compiler takes 256 VGPRs + 152 - 156 AGPRs.  The LDS side is ready for two (<= 68 KiB per block, launch_attn_wide); getting the
// registers under 256 without spills is the follow-up.  Plain and window / causal modes; every sequence length (the chunked key loop
// serves any S, as for DeBERTa handles).
template <int HPB, bool WIN = false>
__global__ __launch_bounds__(256, attn_lds_blocks<128>()) void k_attn_wide(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ vT, int64_t ldv,
                                                   const int* __restrict__ seq_off, const int* __restrict__ seq_nk, const int* __restrict__ seq_nq,
                                                   int H, int heads, int kchunk, uint16_t* __restrict__ ctx, int ldk, int kv_mul, AttnBiasArg<false, WIN> ba) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (WIN) {
        const int b = blockIdx.y;
        if (attn_bias_gathers(ba, seq_off[b], seq_nk[b])) attn_lds_body<128, HPB, 5>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
        else attn_lds_body<128, HPB, 3>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
    } else {
        attn_lds_body<128, HPB, 0>(q, k, vT, ldv, seq_off, seq_nk, seq_nq, H, heads, kchunk, ctx, ldk, kv_mul, ba, smem);
    }
}

// ---- long sequences: LDS-DMA ring ------------------------------------------------------------------------------------------------------------
constexpr int ADMA_RING = 3;
constexpr int ADMA_WAVES = 4;                              // eight (one block per (sequence, head) up to 512 tokens) measured 5 % faster at 128 x 512,
                                                           // 10-35 % slower at 64 x 512, 256 x 256 and 341 x 192
constexpr int ADMA_THREADS = ADMA_WAVES * 64;
constexpr int ADMA_QT = 2 * ADMA_WAVES;                    // q-tiles per block: TWO per wave (w and w + ADMA_WAVES), so every staged chunk serves 256 queries
// per 64-key chunk: K [64 keys][2 DH B] + V^T [DH d][128 B]; DH = 64: 16 KiB per stage, 48 KiB per block, DH = 32: 8 / 24 KiB.  The O staging
// (4 waves x 32 x 2 DH B) re-uses the ring after the last chunk
template <int DH>
struct AdmaGeom {
    static constexpr int KB = 64 * 2 * DH;                 // K bytes of a chunk (= V^T bytes)
    static constexpr int STAGE = 2 * KB;
    static constexpr int LDS = ADMA_RING * STAGE;
    static constexpr int PIECES = KB / 1024 / ADMA_WAVES;  // K pieces (and V^T pieces) of 1 KiB a wave issues per chunk
};

// Measured at 128 x 512 tokens (us per layer; the register-staged kernel: 344): two q-tiles per wave one after the other 253; one q-tile per wave with
// four waves per block and three waves per SIMD 285 (every chunk then serves 128 queries and the block meets a barrier per step: its waves run in
// lockstep); eight waves x one q-tile at <= 128 registers spills the Q fragments (scratch reloads are VMEM operations: they drain the DMA ring).
// Interleaving a wave's two q-tiles by halves (scores(0), scores(1), softmax + P.V(0), softmax + P.V(1): tile 1's S^T MFMAs under tile 0's softmax)
// needs both score tiles live: 42 spilled registers at the 256-register limit, two of them reloaded per chunk (VMEM: the DMA ring drains) — not kept.
// (the body is a function with __restrict__ K / V^T pointers on purpose: after inlining the LDS-DMA carries their alias scope and the ring's ds_reads are
// marked as not aliasing it, which lets the compiler's waitcnt pass leave the COUNTED vmcnt waits alone; see coarse_q32_body in search.hip)
template <int DH, int BM>
__device__ __forceinline__ void attn_dma_body(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* __restrict__ vT, int64_t ldv,
                                              int64_t off, int nk, int nq, int H, int head, int qg, int64_t capT, uint16_t* __restrict__ ctx, char* smem, int ldk, int kv_mul,
                                              const AttnModeArg<BM>& ba) {
    constexpr bool WIN = BM >= 3;      // (never 6: the disentangled terms are built into k_attn_lds only)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hf = lane >> 5;
    using G = AdmaGeom<DH>;
    constexpr int ADMA_PIECES = G::PIECES, KB = G::KB, ADMA_STAGE = G::STAGE;
    constexpr int NC = DH / 8, NCS = DH == 64 ? 3 : 2, KROWS = 1024 / (2 * DH);  // 16-B chunks per K row (1 << NCS), keys per 1-KiB K piece
    // chunks [c_lo, nchunks) are streamed: all of them, or under a window those that meet the band of the block's 256 queries (at w = 64 at most 7, causal: up to the block's last query; a block
    // that holds the query-only CLS row starts at chunk 0)
    int c_lo = 0, nchunks = (nk + 63) >> 6;
    if constexpr (WIN) {
        const AttnBand bb = attn_band(qg * ADMA_QT * 32, qg * ADMA_QT * 32 + ADMA_QT * 32 - 1, nk, nq, ba.wl, ba.wr);
        c_lo = bb.xhi >= 0 ? 0 : (bb.lo >> 6);
        nchunks = min(nchunks, max(bb.hi, bb.xhi) / 64 + 1);      // hi, xhi >= -1
    }
    // DMA of one chunk: 2 DH / 8 pieces of 1 KiB (DH / 8 K pieces of 1024 / (2 DH) keys each, DH / 8 V^T pieces = 8 d rows x 128 B each); wave w issues
    // pieces w * ADMA_PIECES .. + ADMA_PIECES - 1 of both.  K: lane -> key KROWS p + lane / NC, 16-B chunk (lane % NC) ^ attn_kswz(key); V^T: lane -> d row
    // 8 p + (lane >> 3), 16-B chunk (lane & 7) ^ ((d >> 1) & 7) (the LDS destination is lane-linear: the swizzle sits on the source)
    // addresses = a buffer resource per operand whose base is this (sequence, head)'s first byte (scalar registers) + a wave-uniform chunk offset (the
    // instruction's scalar offset) + a 32-bit per-lane offset that never changes: buffer_load_dwordx4 ... lds.  (With global_load_lds the compiler kept four
    // zero-extended 64-bit lane offsets, spilled them at the 256-register limit and reloaded them — s_waitcnt vmcnt(0) each — in front of the DMA of the
    // partial last chunk.)  Rows past the sequence (last chunk) are read and masked; the K buffer has 64 rows and V^T 64 columns of slack behind the last
    // token (ensure_ws), so nothing is out of range.
    // K [T, ldk] / V^T [ldk, ldv] hold one head per KV head: query head `head` streams head / group (ldk = H, group = 1 on every handle but a grouped-query decoder's)
    const int kvh = attn_kv_head(head, kv_mul);
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(k)) + (int64_t)kvh * 2 * DH + off * ldk * 2, 0, 0xffffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(vT)) + ((int64_t)kvh * DH) * ldv * 2 + off * 2, 0, 0xffffffff, 0x00020000);
    uint32_t klane[ADMA_PIECES], vlane[ADMA_PIECES];
#pragma unroll
    for (int pp = 0; pp < ADMA_PIECES; ++pp) {
        const int p = wave * ADMA_PIECES + pp;
        const int key = KROWS * p + (lane >> NCS), row = 8 * p + (lane >> 3);   // key inside the chunk / d row
        klane[pp] = (uint32_t)(key * ldk * 2 + (((lane & (NC - 1)) ^ attn_kswz<DH>(key)) << 4));
        vlane[pp] = (uint32_t)((int64_t)row * ldv * 2 + (((lane & 7) ^ ((row >> 1) & 7)) << 4));   // < 2^32: DH rows x (tokens + 64) x 2 B, tokens <= 2^24 (ensure_ws)
    }
    auto issue = [&](int cidx) {
        char* stg = smem + (cidx % ADMA_RING) * ADMA_STAGE;
        const int kc = cidx * 64 * ldk * 2, vc = cidx * 128;             // chunk offsets (bytes): 32 MiB / 16 KiB at 8192 tokens and H = 2048
#pragma unroll
        for (int pp = 0; pp < ADMA_PIECES; ++pp) {
            const int p = wave * ADMA_PIECES + pp;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_void*)(stg + p * 1024), 16, klane[pp], kc, 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (lds_void*)(stg + KB + p * 1024), 16, vlane[pp], vc, 0, 0);
        }
    };
    if (!WIN || c_lo < nchunks) issue(c_lo);      // (window: no chunk at all for the CLS row of an all-masked sequence)
    if (c_lo + 1 < nchunks) issue(c_lo + 1);
    // The Q fragments are loaded behind the first two chunks' DMA and waited for HERE with a wait the compiler sees (a builtin, not inline asm):
    // otherwise its waitcnt pass keeps them "possibly pending" around the loop's back edge and puts s_waitcnt vmcnt(0) in front of the first MFMA of
    // every chunk, which drains the DMA ring (one memory round trip per chunk, as without a ring)
    int q0[2]; bool act[2];
    uint4 qf[2][DH / 16] = {};
    AttnState<DH> st[2];
    decltype(attn_bias_lane<BM>(ba, off, nk, head, 0, hf)) bl[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        q0[j] = (qg * ADMA_QT + wave + ADMA_WAVES * j) * 32;
        act[j] = q0[j] < nq;                               // wave-uniform; act[1] implies act[0]
        bl[j] = attn_bias_lane<BM>(ba, off, nk, head, min(q0[j] + c, nq - 1), hf);      // nq >= 1 (k_attn_dma)
        if (act[j]) {
            const int qi = (q0[j] + c < nq) ? (q0[j] + c) : (nq - 1);
            const uint16_t* qrow = q + (off + qi) * H + head * DH;
#pragma unroll
            for (int s = 0; s < DH / 16; ++s) qf[j][s] = *reinterpret_cast<const uint4*>(qrow + 16 * s + 8 * hf);
        }
        attn_init(st[j]);
    }
    AttnBand band[2] = {};
    if constexpr (WIN) {
#pragma unroll
        for (int j = 0; j < 2; ++j) band[j] = attn_band(q0[j], q0[j] + 31, nk, nq, ba.wl, ba.wr);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0): Q fragments (and chunks 0, 1) have landed
    auto turn = [&](int ci) {
        if (ci + 1 < nchunks) wait_vmcnt<2 * ADMA_PIECES>(); else wait_vmcnt<0>();   // this wave's pieces of chunk ci have landed; chunk ci + 1 may be in flight
        __builtin_amdgcn_s_barrier();                      // everybody's pieces of chunk ci landed, everybody is done reading chunk ci - 1
        if (ci + 2 < nchunks) issue(ci + 2);               // into the stage of chunk ci - 1
    };
    // The chunks with 64 valid keys run in loops of their own (one per number of active q-tiles) that hold nothing but the unmasked step: with the masked
    // variants and the act[] tests inside one loop the accumulators of both tiles went through copies at every join (32 v_mov_b64 per step)
    const int nfull = WIN ? min(nk >> 6, nchunks) : nk >> 6;
    auto full_chunk = [&](int ci, auto two_tiles) {
        turn(ci);
        char* stg = smem + (ci % ADMA_RING) * ADMA_STAGE;
        auto vfrag = [&](int dh, int ks) {
            const int d = c + 32 * dh;
            return *reinterpret_cast<const uint4*>(stg + KB + d * 128 + (((2 * ks + hf) ^ ((d >> 1) & 7)) << 4));
        };
        // (gathered key columns: without the fragment prefetch — the gather's indices and the prefetched fragments together do not fit the register file)
        constexpr bool PF = BM != 2 && BM != 4;
        if constexpr (WIN) {
            if (band[0].visits(ci * 64)) attn_step64<false, PF>(st[0], qf[0], stg, 0, 64, c, hf, vfrag, bl[0], ci * 64);
            if constexpr (decltype(two_tiles)::value) { if (band[1].visits(ci * 64)) attn_step64<false, PF>(st[1], qf[1], stg, 0, 64, c, hf, vfrag, bl[1], ci * 64); }
        } else {
            attn_step64<false, PF>(st[0], qf[0], stg, 0, 64, c, hf, vfrag, bl[0], ci * 64);
            if constexpr (decltype(two_tiles)::value) attn_step64<false, PF>(st[1], qf[1], stg, 0, 64, c, hf, vfrag, bl[1], ci * 64);
        }
    };
    if (act[1]) {
        for (int ci = c_lo; ci < nfull; ++ci) full_chunk(ci, std::true_type{});
    } else {
        for (int ci = c_lo; ci < nfull; ++ci) full_chunk(ci, std::false_type{});
    }
    for (int ci = WIN ? max(nfull, c_lo) : nfull; ci < nchunks; ++ci) {             // at most one: the partial last chunk
        turn(ci);
        char* stg = smem + (ci % ADMA_RING) * ADMA_STAGE;
        const int nkc = min(nk - ci * 64, 64);
        auto vfrag = [&](int dh, int ks) {
            const int d = c + 32 * dh;
            return *reinterpret_cast<const uint4*>(stg + KB + d * 128 + (((2 * ks + hf) ^ ((d >> 1) & 7)) << 4));
        };
        if (nkc < 64) {
            // V^T columns >= nkc of the last chunk hold other sequences' values (or padding): zero them, so that P = 0 meets 0 and not a possible NaN / Inf
            for (int i = tid; i < DH * 8; i += ADMA_THREADS) {
                const int d = i >> 3, chk = i & 7;         // (d row, 16-B chunk)
                if (chk * 8 + 8 > nkc) {
                    uint4* w = reinterpret_cast<uint4*>(stg + KB + d * 128 + ((chk ^ ((d >> 1) & 7)) << 4));
                    uint4 v = *w;
                    unsigned int* u = reinterpret_cast<unsigned int*>(&v);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = chk * 8 + 2 * e;
                        u[e] &= (key < nkc ? 0xffffu : 0u) | (key + 1 < nkc ? 0xffff0000u : 0u);
                    }
                    *w = v;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!act[j]) continue;
            if constexpr (WIN) { if (!band[j].visits(ci * 64)) continue; }
            if (nkc < 64) attn_step64<true>(st[j], qf[j], stg, 0, nkc, c, hf, vfrag, bl[j], ci * 64);
            else attn_step64<false>(st[j], qf[j], stg, 0, 64, c, hf, vfrag, bl[j], ci * 64);
        }
    }
    __syncthreads();                                       // the ring is free: re-use it for the O staging
    char* Os = smem + wave * (32 * 2 * DH);
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (act[j]) attn_store_tile<DH, WIN>(st[j], Os, ctx, off, q0[j], nq, H, head, lane);
}

template <int DH, bool BIAS = false, bool WIN = false>
__global__ __launch_bounds__(ADMA_THREADS, 512 / ADMA_THREADS) void k_attn_dma(const uint16_t* q, const uint16_t* k, const uint16_t* vT, int64_t ldv, const int* __restrict__ seq_off,
                                                             const int* __restrict__ seq_nk, const int* __restrict__ seq_nq, int H, int64_t capT, uint16_t* ctx, int heads, int nseq, int qgroups,
                                                             int ldk, int kv_mul, AttnBiasArg<BIAS, WIN> ba) {
    static_assert(!(BIAS && WIN), "a relative attention bias under a window is not instantiated");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // linear block id -> (pair p = b * heads + head, q-group qg).  Consecutive workgroups go to consecutive XCDs (id mod 8), and each XCD has its own L2:
    // the q-groups of one (sequence, head) read the same K / V^T stream, so they are placed 8 ids apart — same XCD, dispatched together — and the second
    // reader finds the chunks in L2 (measured: HBM-side traffic of the kernel 1.6 x -> 1.1 x its algorithmic bytes at 128 x 512 tokens).  Heads fastest
    // inside a group of 8 pairs: the heads of one sequence share their 2-KiB q / k rows.
    const int G = qgroups;                                 // q-groups per pair
    const int L = (int)blockIdx.x;
    const int grp = L / (8 * G), r = L % (8 * G);
    const int qg = r >> 3, p = grp * 8 + (r & 7);
    const int b = p / heads, head = p % heads;
    if (b >= nseq) return;                                 // the grid is padded to whole groups of 8 pairs
    const int nq = seq_nq[b];
    if (qg * ADMA_QT * 32 >= nq) return;                   // block-uniform (nq == 0 included)
    if constexpr (WIN) {
        if (attn_bias_gathers(ba, seq_off[b], seq_nk[b])) attn_dma_body<DH, 4>(q, k, vT, ldv, seq_off[b], seq_nk[b], nq, H, head, qg, capT, ctx, smem, ldk, kv_mul, ba);
        else attn_dma_body<DH, 3>(q, k, vT, ldv, seq_off[b], seq_nk[b], nq, H, head, qg, capT, ctx, smem, ldk, kv_mul, ba);
    } else if constexpr (BIAS) {
        if (attn_bias_gathers(ba, seq_off[b], seq_nk[b])) attn_dma_body<DH, 2>(q, k, vT, ldv, seq_off[b], seq_nk[b], nq, H, head, qg, capT, ctx, smem, ldk, kv_mul, ba);
        else attn_dma_body<DH, 1>(q, k, vT, ldv, seq_off[b], seq_nk[b], nq, H, head, qg, capT, ctx, smem, ldk, kv_mul, ba);
    } else {
        attn_dma_body<DH, 0>(q, k, vT, ldv, seq_off[b], seq_nk[b], nq, H, head, qg, capT, ctx, smem, ldk, kv_mul, ba);
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side: the launchers (the library's forward and tests/capi/attn_probe.hip launch through them)
// ---------------------------------------------------------------------------------------------------------
// The operands of one layer's attention as they lie in the workspace: q / ctx [capT, H], k [capT + 64, kv_dim], vT [kv_dim, ldv], the sequence tables of the
// nseq sequences (offsets: multiples of 4 tokens for k_attn_lds, of 8 for k_attn_dma).  H is the row pitch of q and ctx, heads * DH: the hidden size unless the
// handle has a head width of its own (config.head_dim)
struct AttnOperands {
    const uint16_t *q, *k, *vT; int64_t ldv;
    const int *seq_off, *seq_nk, *seq_nq;
    uint16_t* ctx;
    int H, heads, kv_dim;
    int64_t capT; int nseq;
};
// The mode of a launch is the type of its arguments (AttnNoBiasArgs, AttnBiasArgs, AttnWinArgs — a causal layer's too —, AttnDisentArgs)
template <class BA> constexpr bool attn_is_bias = std::is_same_v<BA, AttnBiasArgs>;
template <class BA> constexpr bool attn_is_win = std::is_same_v<BA, AttnWinArgs>;
template <class BA> constexpr bool attn_is_disent = std::is_same_v<BA, AttnDisentArgs>;

// the register-staged kernel, HPB heads per block.  cap: the batch width rounded up to 32; nqt: q-tiles of the longest sequence
template <int DH, int HPB, class BA>
static int launch_attn_lds(const AttnOperands& o, int cap, int nqt, const BA& ba, int device, hipStream_t st) {
    // keys staged at a time: K kchunk x 2 DH B + V^T DH x (2 kchunk + 8) B per head, plus 4 O tiles of 32 x 2 DH B.  DH = 64: 49-50 KiB per block for any
    // (S, HPB), 3 blocks per CU; DH = 32: 24-25 KiB, 4 blocks per CU (attn_lds_blocks: the registers, not the LDS, bound it)
    const int kchunk = cap < 128 ? cap : 128;
    const int lds = HPB * (kchunk * 2 * DH + DH * (kchunk * 2 + 8)) + 4 * 32 * 2 * DH;
    const auto kern = &k_attn_lds<DH, HPB, attn_is_bias<BA>, attn_is_win<BA>, attn_is_disent<BA>>;
    KR_TRY(set_lds_once(reinterpret_cast<const void*>(kern), lds, device));
    const int qgroups = (nqt + (4 / HPB) - 1) / (4 / HPB);   // blocks per (sequence, head group): 4 / HPB q-tiles each
    hipLaunchKernelGGL(kern, dim3((unsigned)((o.heads + HPB - 1) / HPB), (unsigned)o.nseq, (unsigned)qgroups), dim3(256), lds, st, o.q, o.k, o.vT, o.ldv, o.seq_off, o.seq_nk,
                       o.seq_nq, o.H, o.heads, kchunk, o.ctx, o.kv_dim, attn_kv_mul(o.H / o.kv_dim), ba);
    return 0;
}
// the register-staged kernel at DH = 128.  K kchunk x 256 B + V^T 128 x (2 kchunk + 8) B per head; the O staging (32 KiB) re-uses that area: 65 KiB at
// kchunk = 128 (HPB = 1), 67 KiB at 64 (HPB = 2), 68 KiB at 32 (HPB = 4)
constexpr int attn_wide_lds(int hpb, int kchunk) {
    const int kv = hpb * (kchunk * 256 + 128 * (kchunk * 2 + 8)), os = 4 * 32 * 256;
    return kv > os ? kv : os;
}
template <int HPB, class BA>
static int launch_attn_wide(const AttnOperands& o, int cap, int nqt, const BA& ba, int device, hipStream_t st) {
    static_assert(!attn_is_bias<BA> && !attn_is_disent<BA>, "128-wide heads: plain and window / causal attention only");
    const int kchunk = cap < 128 ? cap : 128;
    const int lds = attn_wide_lds(HPB, kchunk);
    const auto kern = &k_attn_wide<HPB, attn_is_win<BA>>;
    KR_TRY(set_lds_once(reinterpret_cast<const void*>(kern), lds, device));
    const int qgroups = (nqt + (4 / HPB) - 1) / (4 / HPB);
    hipLaunchKernelGGL(kern, dim3((unsigned)((o.heads + HPB - 1) / HPB), (unsigned)o.nseq, (unsigned)qgroups), dim3(256), lds, st, o.q, o.k, o.vT, o.ldv, o.seq_off, o.seq_nk,
                       o.seq_nq, o.H, o.heads, kchunk, o.ctx, o.kv_dim, attn_kv_mul(o.H / o.kv_dim), ba);
    return 0;
}
// the LDS-DMA ring (not built with the disentangled terms)
template <int DH, class BA>
static int launch_attn_dma(const AttnOperands& o, int nqt, const BA& ba, hipStream_t st) {
    const int qgroups = (nqt + ADMA_QT - 1) / ADMA_QT;       // blocks per (sequence, head): 8 q-tiles each
    const int64_t pairs = (int64_t)o.nseq * o.heads;
    const int64_t blocks = (pairs + 7) / 8 * 8 * qgroups;    // whole groups of 8 pairs (see k_attn_dma)
    hipLaunchKernelGGL((k_attn_dma<DH, attn_is_bias<BA>, attn_is_win<BA>>), dim3((unsigned)blocks), dim3(ADMA_THREADS), AdmaGeom<DH>::LDS, st, o.q, o.k, o.vT, o.ldv, o.seq_off,
                       o.seq_nk, o.seq_nq, o.H, o.capT, o.ctx, o.heads, o.nseq, qgroups, o.kv_dim, attn_kv_mul(o.H / o.kv_dim), ba);
    return 0;
}
// the attention of one layer: the LDS-DMA ring for long sequences, else the register-staged kernel with 1 / 2 / 4 heads per block by q-tiles per sequence
// (the disentangled terms are built into the register-staged kernel only: a DeBERTa forward never asks for the ring)
template <int DH, class BA>
static int launch_attention(const AttnOperands& o, int cap, int nqt, bool long_seq, const BA& ba, int device, hipStream_t st) {
    if constexpr (DH == 128) {
        // every length through k_attn_wide (long_seq is never set for such a handle); the bias-table and disentangled modes stay 32 / 64 only
        if constexpr (attn_is_bias<BA> || attn_is_disent<BA>) return fail(KR_ESTATE, "128-wide heads run plain and window / causal attention only");
        else return nqt >= 3 ? launch_attn_wide<1>(o, cap, nqt, ba, device, st) : nqt == 2 ? launch_attn_wide<2>(o, cap, nqt, ba, device, st) : launch_attn_wide<4>(o, cap, nqt, ba, device, st);
    } else {
    if constexpr (!attn_is_disent<BA>) { if (long_seq) return launch_attn_dma<DH>(o, nqt, ba, st); }
    if (nqt >= 3) return launch_attn_lds<DH, 1>(o, cap, nqt, ba, device, st);
    if (nqt == 2) return launch_attn_lds<DH, 2>(o, cap, nqt, ba, device, st);
    return launch_attn_lds<DH, 4>(o, cap, nqt, ba, device, st);
    }
}

}  // namespace KR_ENC_NS
}  // namespace kr
