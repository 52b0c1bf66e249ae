// Sentence encoder, the projections: device code (ProjArgs, the epilogues, k_proj*) and, behind it, the host code that launches it (launch_proj_loop: one
// launch on a given main loop; launch_proj: which loop a launch of a forward takes).  Part of encoder.hip (see its header).
#pragma once
#include "encoder_rows.hpp"

#include <type_traits>

namespace kr {
namespace KR_ENC_NS {

using ShapeBig = GemmShape<256, 256, 2, 4>;     // 8 waves of 128x64, 128 KiB LDS, one block per CU: best main loop (long-K GEMMs)
// Four main loops, one per launch size (launch_proj picks; all give bit-identical rows):
//   256x256 ping-pong (gemm_nt_pingpong)          launches with >= 5/8 of the CUs' worth of 256x256 tiles
//   128x128 producer / consumer (gemm_nt_split)   fewer: at most one tile per CU, or more than two
//   128x128 streaming, 2 slots, 2 blocks per CU   in between (k_proj<.., ShapeSmall, 2>)
//   32x32 / 64x64 skinny (gemm_nt_skinny)         a handful of token rows (<= 4 tiles of 32x32 per CU)

using ShapeSmall = GemmShape<128, 128, 2, 2>;   // 4 waves of 64x64, 64 KiB ring, two blocks per CU: for launches with too few 256x256 tiles to fill the chip

// all main loops run with exchanged MFMA operands (accumulators hold 4 consecutive features per lane)
template <class ShapeE, int STAGES, bool ANT = false, class Coord, class Epilogue>
__device__ __forceinline__ void gemm_main(const uint16_t* __restrict__ A, int64_t lda, int64_t M, const uint16_t* __restrict__ B, int64_t ldb, int64_t N,
                                          int K, int64_t total_tiles, char* smem, Coord&& coord, Epilogue&& epi) {
    if constexpr (ShapeE::BM == 256 && ShapeE::BN == 256) gemm_nt_pingpong<ET, true, ANT>(A, lda, M, B, ldb, N, K, total_tiles, smem, coord, epi);
    else gemm_nt_stream<ET, ShapeE, STAGES, true>(A, lda, M, B, ldb, N, K, total_tiles, smem, coord, epi);
}

// ---------------------------------------------------------------------------------------------------------
// projections: C[token, feature] = X[token, :] . W[feature, :]   (rows = tokens, cols = output features)
// ---------------------------------------------------------------------------------------------------------
struct ProjArgs {
    const uint16_t* W; const uint16_t* X; const int* Tp; int F; int K; int H;   // H: the QKV epilogues' width of q (hidden unless the handle has a head width of its own)
    int A;   // the rotating QKV epilogues and EPI_QKV_SPLIT: columns of k and rows of V^T (F = H + 2A; A = H unless k / v are a grouped-query decoder's, A % 64 == 0)
    const float* bias;
    uint16_t* out0; uint16_t* out1; uint16_t* outT; int64_t ldT;   // QKV: q [T,H], k [T,A] row-major; vT [A, ldT].  Others: out0 [T, F]
    int64_t ldx, ldo;   // row pitch (elements) of X and of out0 (EPI_DENSE / EPI_GELU); 0 = K / F
    int pw;   // feature tiles per XCD patch of the tile walk (patch_coord)
    int epi_prio;   // A/B knob, see proj_epilogue
    int ant;  // activation loads non-temporal (FF2's h: launch_proj)
    int nt;   // epilogue stores non-temporal (large launches: the output is consumed from HBM by the next kernel, keep it out of L2) or plain
              // (small launches: the whole output fits in L2 / Infinity Cache, the next kernel reads it from there)
    // EPI_QKV_ROT (NomicBert handles): cos / sin tables [max_pos][dh / 2] fp32, the position every token row is rotated by (k_rot_pos), the head width (32 or 64)
    const float* rot_cos; const float* rot_sin; const int* tpos; int max_pos; int dh;
    // EPI_SPLADE: the sequence of every packed row or -1 (k_splade_rowseq), the [B, V] reduction buffer (bit patterns, zero-initialised), V <= F real columns
    const int* row_seq; unsigned int* smax; int V;
};

enum { EPI_QKV = 0, EPI_DENSE = 1, EPI_GELU = 2, EPI_QKV_ROT = 3, EPI_SWIGLU = 4, EPI_GEGLU = 5, EPI_QKV_ROTB = 6, EPI_RELU = 7, EPI_GEGLU_TANH = 8, EPI_SPLADE = 9, EPI_QKV_SPLIT = 10 };
constexpr bool epi_rotates(int epi) { return epi == EPI_QKV_ROT || epi == EPI_QKV_ROTB; }
constexpr bool epi_splits(int epi) { return epi_rotates(epi) || epi == EPI_QKV_SPLIT; }   // F = H + 2A: q | k [T, A] | V^T [A, ldT]
constexpr bool epi_gated(int epi) { return epi == EPI_SWIGLU || epi == EPI_GEGLU || epi == EPI_GEGLU_TANH; }   // F = 2 FF GEMM columns -> FF stored

// The two epilogues of NomicBert handles combine feature pairs: a rotary pair (j, j + d_h / 2) of q or k, or gate and up of one intermediate feature.  The
// packed weights are laid out (tile_pair_row, encoder_rows.hpp) so that on EVERY main loop both partners sit in one 32x32 accumulator tile, column cc < 16 with
// cc + 16: in the swapped layout that is register r with register r + 8 of the same lane.  No cross-lane traffic, and the skinny loop's one-tile waves work too.
//   EPI_QKV_ROT: tile columns 0..15 are the head's features jb .. jb + 15 and columns 16..31 their partners jb + d_h / 2 ..; jb = 0 for 32-wide heads (a tile is
//   a head) and 0 / 16 for the even / odd tile of a 64-wide head.  q and k are STORED in that order (a 64-wide head as 0..15, 32..47, 16..31, 48..63): the
//   attention kernels only ever dot q with k over a head, and both carry the same order.
__device__ __forceinline__ int rot_jbase(int dh, int f) { return dh == 64 ? ((f >> 5) & 1) << 4 : 0; }

// x'[j] = x[j] cos - x[j + d_h/2] sin,  x'[j + d_h/2] = x[j + d_h/2] cos + x[j] sin  (HF apply_rotary_pos_emb, NeoX pairing), fp32, on one tile of one lane:
// cs / sn point at the lane's token row of the tables, at jb + 4 h
__device__ __forceinline__ void rotate_tile(f32x16& v, const float* __restrict__ cs, const float* __restrict__ sn) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cs + 8 * g), s = *reinterpret_cast<const f32x4*>(sn + 8 * g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float a = v[4 * g + i], b = v[4 * g + 8 + i];
            v[4 * g + i] = a * c[i] - b * s[i];
            v[4 * g + 8 + i] = b * c[i] + a * s[i];
        }
    }
}
// the table row of token t: its column relative to its sequence's first row (k_rot_pos).  Rows past the packed total hold none (partial last tile): row 0
__device__ __forceinline__ int64_t rot_row(const ProjArgs& a, int64_t t) {
    const int p = a.tpos[t];
    return (int64_t)((unsigned)p < (unsigned)a.max_pos ? p : 0) * (a.dh >> 1);
}

// the gated products of one register quad of a tile in tile-pair order (registers 4g .. 4g + 3 with 4g + 8 ..): silu(gate) * up, and ModernBert's
// erf_gelu(input + b) * (gate + b') with EPI_GELU's erf-GELU (bi / bg: the biases of the quad's input and gate features)
__device__ __forceinline__ float silu_mul(float g, float u);
__device__ __forceinline__ f32x2 gelu_erf_fast2(f32x2 x);
__device__ __forceinline__ f32x4 swiglu_quad(const f32x16& v, int g) {
    return f32x4{silu_mul(v[4 * g], v[4 * g + 8]), silu_mul(v[4 * g + 1], v[4 * g + 9]), silu_mul(v[4 * g + 2], v[4 * g + 10]), silu_mul(v[4 * g + 3], v[4 * g + 11])};
}
__device__ __forceinline__ f32x4 geglu_quad(const f32x16& v, int g, f32x4 bi, f32x4 bg) {
    const f32x4 x = f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]} + bi, u = f32x4{v[4 * g + 8], v[4 * g + 9], v[4 * g + 10], v[4 * g + 11]} + bg;
    const f32x2 lo = gelu_erf_fast2(f32x2{x.x, x.y}), hi = gelu_erf_fast2(f32x2{x.z, x.w});
    return f32x4{lo.x, lo.y, hi.x, hi.y} * u;
}

// T5 v1.1 / flan handles: gelu_new(wi_0 x) * wi_1 x, no bias.  HF's gelu_new is the tanh form 0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), and
// 0.5 (1 + tanh(u)) = 1 / (1 + exp(-2 u)) exactly: one v_exp_f32 and one v_rcp_f32 per element like silu_mul (exp overflows to +inf for very negative x:
// the quotient is then -0, the limit of the tanh form)
__device__ __forceinline__ float gelu_tanh_mul(float x, float u) {
    const float t = 0.7978845608028654f * (x + 0.044715f * (x * x * x));
    return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(t * -2.8853900817779268f)) * u;
}
__device__ __forceinline__ f32x4 geglu_tanh_quad(const f32x16& v, int g) {
    return f32x4{gelu_tanh_mul(v[4 * g], v[4 * g + 8]), gelu_tanh_mul(v[4 * g + 1], v[4 * g + 9]), gelu_tanh_mul(v[4 * g + 2], v[4 * g + 10]),
                 gelu_tanh_mul(v[4 * g + 3], v[4 * g + 11])};
}

// relu of a register quad; NaN stays NaN (fmaxf would drop it, and a non-finite activation has to reach the error word)
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{v.x < 0.f ? 0.f : v.x, v.y < 0.f ? 0.f : v.y, v.z < 0.f ? 0.f : v.z, v.w < 0.f ? 0.f : v.w}; }

// silu(g) u = g u / (1 + exp(-g)) in fp32: one v_exp_f32 and one v_rcp_f32 per element (exp overflows to +inf for g < -88: the quotient is then -0)
__device__ __forceinline__ float silu_mul(float g, float u) {
    return g * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(g * -1.4426950408889634f)) * u;
}

// erf-GELU x Phi(x) = max(x, 0) - 0.5 |x| erfc(|x| / sqrt 2), with erfc(a / sqrt 2) = 2^-Q(a), Q(a) = a (c1 + c2 a + c3 a^2 + c4 a^3 + c5 a^4) a weighted
// minimax fit of -log2 erfc on [0, 8] (weight a erfc(a / sqrt 2) = the sensitivity of the result; fitted offline, c5 > 0 so Q keeps growing and the
// tail underflows to the exact limit max(x, 0)).  |error| <= 9.4e-7 absolute on the whole line in fp32 arithmetic (the result is rounded to bf16:
// 2^-9 relative), no sign handling, and ONE quarter-rate transcendental (v_exp_f32) per element instead of two: 13 VALU instructions per element
// pair (76 issue cycles) against 22 (136) for the Abramowitz-Stegun 7.1.26 form used before, in an epilogue that nothing overlaps with (the GELU
// was 1557 VALU instructions per wave and 256x256 tile, with both waves of a SIMD in it at the same time).
// two elements at once: the polynomial / products run as packed fp32 (v_pk_fma_f32 / v_pk_mul_f32), only exp2 / abs / max stay scalar
__device__ __forceinline__ f32x2 gelu_erf_fast2(f32x2 x) {
    const f32x2 ax = {fabsf(x.x), fabsf(x.y)};
    f32x2 q = __builtin_elementwise_fma(ax, f32x2{4.881049150e-04f, 4.881049150e-04f}, f32x2{-7.198719129e-03f, -7.198719129e-03f});
    q = __builtin_elementwise_fma(q, ax, f32x2{5.214659068e-02f, 5.214659068e-02f});
    q = __builtin_elementwise_fma(q, ax, f32x2{4.595959239e-01f, 4.595959239e-01f});
    q = __builtin_elementwise_fma(q, ax, f32x2{1.151000505e+00f, 1.151000505e+00f});
    q = q * ax;
    const f32x2 e = {__builtin_amdgcn_exp2f(-q.x), __builtin_amdgcn_exp2f(-q.y)};
    const f32x2 r = {fmaxf(x.x, 0.f), fmaxf(x.y, 0.f)};
    return __builtin_elementwise_fma(ax * e, f32x2{-0.5f, -0.5f}, r);
}

// A 32x32 MFMA accumulator has its COLUMN on the lane, so a direct store writes 2-byte elements (128 store instructions per lane per
// 256x256 tile, the epilogue then costs as much as a third of the main loop).  Instead every wave owns a private 4-KiB LDS stage
// behind the ring (no barrier: only this wave touches it, LDS operations of one wave complete in order):
//   rows:  the wave's 32 x 64 block (one mi, both ni) is written as bf16 [32 rows][128 B] and read back 16 B per lane, so each global
//          store instruction writes eight whole 128-B lines of the output;
//   V^T:   each 32x32 tile is written TRANSPOSED ([feature][token], 4 consecutive tokens of a lane packed into 8 B, 80-B rows) and
//          read back 16 B per lane: a store instruction writes 64-B runs of sixteen V^T rows.
constexpr int EPI_STAGE_BYTES = 4096;

// Both helpers take the SWAPPED accumulator layout of gemm_nt_pingpong / gemm_nt_split / gemm_nt_stream / gemm_nt_skinny with SWAP = true: tile (mi, ni), register r,
// lane (c = l & 31, h = l >> 5) is token mi*32 + c, feature ni*32 + (r & 3) + 8 (r >> 2) + 4 h of the wave's (TM*32 tokens) x (TN*32 features).
//
// rows: for one mi the wave's 32 tokens x 64 features are staged as bf16 [32 tokens][128 B]; registers 4g .. 4g+3 of a lane are 4
// consecutive features -> one packed ds_write_b64 (16-B chunk index XOR (token & 7): 2-way instead of 16-way conflicts), read back 16 B
// per lane: every global store instruction writes eight whole 128-B rows.  f(v, mi, ni, g) maps 4 features (bias / GELU / row scale) before packing.
template <class Shape, bool NT, class F>
__device__ __forceinline__ void store_rows_bf16(AccTile<Shape>& acc, char* stage, uint16_t* __restrict__ out, int64_t ld, int64_t row0, int col0, F&& f) {
    static_assert(Shape::TN == 2, "stage geometry assumes 64 features per wave");
    const int c = acc.lane & 31, h = acc.lane >> 5;
    const int r8 = acc.lane >> 3, ch = acc.lane & 7;
    const char* st_rd = stage + r8 * 128 + ((ch ^ r8) << 4);
    uint16_t* g_base = out + (row0 + r8) * ld + col0 + ch * 8;
    // software pipeline over the mi blocks: write(mi), read(mi), THEN the global stores of mi-1 — LDS operations of one wave complete in order, so
    // the single 4-KiB stage is safe to overwrite right after the reads were issued, and the stores of block mi-1 only wait for their own reads
    // (counted lgkmcnt) while the LDS round trip of block mi is in flight (one exposed round trip per tile instead of one per block)
    uint4 d[2][4];
#pragma unroll
    for (int mi = 0; mi <= Shape::TM; ++mi) {
        if (mi < Shape::TM) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 v = f(f32x4{acc.v[mi][ni][4 * g], acc.v[mi][ni][4 * g + 1], acc.v[mi][ni][4 * g + 2], acc.v[mi][ni][4 * g + 3]}, mi, ni, g);
                    uint2 w;
                    w.x = pack_bf16x2(v.x, v.y); w.y = pack_bf16x2(v.z, v.w);
                    *reinterpret_cast<uint2*>(stage + c * 128 + (((ni * 4 + g) ^ (c & 7)) << 4) + h * 8) = w;
                }
#pragma unroll
            for (int p = 0; p < 4; ++p) d[mi & 1][p] = *reinterpret_cast<const uint4*>(st_rd + p * 8 * 128);
        }
        if (mi > 0) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {  // rl & 7 == lane >> 3 for every p: one lane-dependent LDS / global base, the rest are wave-uniform steps (8 rows per store)
                u32x4_t* dst = reinterpret_cast<u32x4_t*>(g_base + (int64_t)((mi - 1) * 32 + p * 8) * ld);
                if constexpr (NT) __builtin_nontemporal_store(__builtin_bit_cast(u32x4_t, d[(mi - 1) & 1][p]), dst);
                else *dst = __builtin_bit_cast(u32x4_t, d[(mi - 1) & 1][p]);
            }
        }
    }
}

// EPI_SWIGLU: the wave's 64 GEMM columns are 2 tiles of (16 gate | 16 up) = 32 consecutive intermediate features: out[token, col0 + ni*16 + 8g + 4h ..] =
// silu(gate) * up from registers 4g.. and 4g + 8.. (g < 2).  Staged like store_rows_bf16, as bf16 [32 tokens][64 B] (16-B chunk index XOR (token >> 2) & 3: 2-way
// conflicts), read back 16 B per lane: every global store instruction writes sixteen whole aligned 64-B runs.  Same software pipeline over the mi blocks.
// f(v, ni, g) = the 4 products of registers 4g .. 4g + 3 of tile v with their partners 4g + 8 .. (EPI_SWIGLU: silu_mul; EPI_GEGLU: erf-GELU, with the biases)
template <class Shape, bool NT, class F>
__device__ __forceinline__ void store_rows_gated(AccTile<Shape>& acc, char* stage, uint16_t* __restrict__ out, int64_t ld, int64_t row0, int col0, F&& f) {
    static_assert(Shape::TN == 2, "stage geometry assumes 64 GEMM columns per wave");
    const int c = acc.lane & 31, h = acc.lane >> 5;
    const int r4 = acc.lane >> 2, ch = acc.lane & 3;
    const char* st_rd = stage + r4 * 64 + ((ch ^ ((r4 >> 2) & 3)) << 4);
    uint16_t* g_base = out + (row0 + r4) * ld + col0 + ch * 8;
    uint4 d[2][2];
#pragma unroll
    for (int mi = 0; mi <= Shape::TM; ++mi) {
        if (mi < Shape::TM) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const f32x4 p = f(acc.v[mi][ni], ni, g);
                    uint2 w;
                    w.x = pack_bf16x2(p.x, p.y);
                    w.y = pack_bf16x2(p.z, p.w);
                    *reinterpret_cast<uint2*>(stage + c * 64 + (((ni * 2 + g) ^ ((c >> 2) & 3)) << 4) + h * 8) = w;
                }
#pragma unroll
            for (int p = 0; p < 2; ++p) d[mi & 1][p] = *reinterpret_cast<const uint4*>(st_rd + p * 16 * 64);
        }
        if (mi > 0) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {  // (row >> 2) & 3 == (lane >> 4) & 3 for both p: one lane-dependent LDS / global base (16 rows per store)
                u32x4_t* dst = reinterpret_cast<u32x4_t*>(g_base + (int64_t)((mi - 1) * 32 + p * 16) * ld);
                if constexpr (NT) __builtin_nontemporal_store(__builtin_bit_cast(u32x4_t, d[(mi - 1) & 1][p]), dst);
                else *dst = __builtin_bit_cast(u32x4_t, d[(mi - 1) & 1][p]);
            }
        }
    }
}

// V^T[feature, token]: each 32x32 tile is staged as [32 features][32 tokens] (80-B rows), lanes = consecutive tokens of a feature row,
// read back 16 B per lane: a store instruction writes 64-B runs of sixteen V^T rows.
template <class Shape, bool NT>
__device__ __forceinline__ void store_transposed_bf16(AccTile<Shape>& acc, char* stage, uint16_t* __restrict__ outT, int64_t ldT, int64_t t0, int f0) {
    // the lane id is made opaque HERE: everything below that depends on it (LDS offsets, the 64-bit V^T addresses) is then recomputed per tile (a few VALU
    // instructions) instead of being hoisted out of the persistent tile loop into registers the main loop has no room for — hipcc spilled them, and the
    // scratch reloads (VMEM, followed by s_waitcnt vmcnt(0)) drained the LDS-DMA ring in every V^T tile (tests/test_capi_and_host.py: no spills allowed)
    int ln = acc.lane;
    asm volatile("" : "+v"(ln));
    const int c = ln & 31, h = ln >> 5;
#pragma unroll
    for (int mi = 0; mi < Shape::TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < Shape::TN; ++ni) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                *reinterpret_cast<uint16_t*>(stage + ((r & 3) + 8 * (r >> 2) + 4 * h) * 80 + c * 2) = ET::from_f32(acc.v[mi][ni][r]);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int fl = p * 16 + (ln >> 2), ch = ln & 3;
                const uint4 d = *reinterpret_cast<const uint4*>(stage + fl * 80 + ch * 16);
                u32x4_t* dst = reinterpret_cast<u32x4_t*>(outT + (int64_t)(f0 + ni * 32 + fl) * ldT + t0 + mi * 32 + ch * 8);
                if constexpr (NT) __builtin_nontemporal_store(__builtin_bit_cast(u32x4_t, d), dst);
                else *dst = __builtin_bit_cast(u32x4_t, d);
            }
        }
}

// EPI_SPLADE (the MLM decoder of a SPLADE handle, KR_POOL_SPLADE): nothing is stored per token.  log1p(relu(.)) is monotone and the decoder's bias is constant per
// column, so w[b, v] = log1p(max(0, bias[v] + max over the sequence's rows of acc[row, v])): the epilogue reduces the fp32 accumulators over the token rows of
// each sequence and hands max(0, max + bias) to smax[b, v] by atomicMax on its BIT PATTERN — non-negative floats order like unsigned integers, a zeroed buffer
// is the identity, a NaN (either sign) is larger than every finite value and so survives to k_splade_finish.  Max is exact and order-independent: the result
// does not depend on the tiling, the batch or the order of the atomics.
// In the exchanged layout a lane holds 16 features of ONE token row per (mi, ni) and lane & 31 is the row, so the reduction runs across the 32 lanes of a
// half-wave.  row_seq[row] names the row's sequence (-1: an alignment row between two sequences, or a row >= T of a partial tile, computed from clamped
// loads: such a row never enters a max).  Per 32-row block mi:
//   all 32 rows in one sequence (the common case): when the next block belongs to the same sequence the block is folded into it in the registers (no
//     cross-lane traffic); else every register is reduced over the half-wave (4 DPP steps + one cross-row shuffle) and lanes 0..15 of each half issue one
//     atomicMax each per tile: 32 consecutive columns per instruction.  A zero is never sent (it is the identity): with a trained model most columns are.
//   anything else (a sequence boundary or the end of the packed rows inside the block): every lane sends its own row's values.
template <int CTRL>
__device__ __forceinline__ float dpp_fmax(float x) {
    const int xi = __builtin_bit_cast(int, x);
    return fmaxf(x, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(xi, xi, CTRL, 0xf, 0xf, false)));
}
// max over the 32 lanes of each half-wave, in every lane: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror (every group of 4 / 8 lanes is
// uniform by then, so a mirror pairs it with its neighbour), then lanes l and l ^ 16.  fmaxf keeps a NaN only when both sides are NaN: a column of NaN
// (a NaN in the weights) survives, a single NaN row is caught where it arises (k_ln16_head)
__device__ __forceinline__ float half_wave_max(float x) {
    x = dpp_fmax<0xB1>(x); x = dpp_fmax<0x4E>(x); x = dpp_fmax<0x141>(x); x = dpp_fmax<0x140>(x);
    return fmaxf(x, __shfl_xor(x, 16, 64));
}
__device__ __forceinline__ unsigned int splade_key(float v) { return (v > 0.f || v != v) ? __builtin_bit_cast(unsigned int, v) : 0u; }

template <class Shape>
__device__ __forceinline__ void splade_reduce(const ProjArgs& a, AccTile<Shape>& acc, int64_t t0, int f0) {
    const int c = acc.lane & 31, h = acc.lane >> 5;
    int s[Shape::TM];
#pragma unroll
    for (int mi = 0; mi < Shape::TM; ++mi) s[mi] = a.row_seq[t0 + mi * 32 + c];
#pragma unroll
    for (int mi = 0; mi < Shape::TM; ++mi) {
        const int sf = __builtin_amdgcn_readfirstlane(s[mi]);
        if (__ballot(s[mi] != sf) == 0ull) {             // wave-uniform from here on: all 64 lanes are active in the DPP steps
            if (sf < 0) continue;
            if (mi + 1 < Shape::TM) {
                const int mn = mi + 1 < Shape::TM ? mi + 1 : mi;      // (an index inside the array for the unrolled last block, where this branch is dead)
                const int sn = __builtin_amdgcn_readfirstlane(s[mn]);
                if (sn == sf && __ballot(s[mn] != sn) == 0ull) {
#pragma unroll
                    for (int ni = 0; ni < Shape::TN; ++ni)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc.v[mn][ni][r] = fmaxf(acc.v[mn][ni][r], acc.v[mi][ni][r]);
                    continue;
                }
            }
#pragma unroll
            for (int ni = 0; ni < Shape::TN; ++ni) {
                float m = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float x = half_wave_max(acc.v[mi][ni][r]);
                    if ((c & 15) == r) m = x;
                }
                const int f = f0 + ni * 32 + (c & 3) + 8 * ((c >> 2) & 3) + 4 * h;      // the feature of register c & 15
                if (c < 16 && f < a.V) {
                    const unsigned int key = splade_key(m + a.bias[f]);
                    if (key) atomicMax(a.smax + (int64_t)sf * a.V + f, key);
                }
            }
        } else if (s[mi] >= 0) {
            unsigned int* dst = a.smax + (int64_t)s[mi] * a.V;
#pragma unroll
            for (int ni = 0; ni < Shape::TN; ++ni)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int f = f0 + ni * 32 + 8 * g + 4 * h;
                    const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + f);      // the bias is padded to F like the weight
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned int key = splade_key(acc.v[mi][ni][4 * g + i] + b[i]);
                        if (key && f + i < a.V) atomicMax(dst + f + i, key);
                    }
                }
        }
    }
}

// persistent streaming projections (256x256 ping-pong or 128x128 streaming main loop).  rows = tokens, cols = output features; bias is
// one value per lane and ni.  Token-indexed buffers are allocated in multiples of 256 rows, so a partial last token tile needs no bounds
// test (rows >= T are written with values computed from clamped loads and never read).
// Tiles are walked in patches of (token tiles x 8 feature tiles) per XCD so operand slices are reused from that XCD's L2.
//   EPI_QKV:   F = 3H: features [0,H) -> q (bias, log2(e) / sqrt(d_h) folded into the weights), [H,2H) -> k, [2H,3H) -> V^T (its bias lives in bo_eff)
//   EPI_DENSE: out0[T,F] = acc as bf16 (k_ln adds the bias and the residual in fp32)
//   EPI_GELU:  out0[T,F] = gelu(acc + bias)
//   EPI_QKV_ROTB: EPI_QKV_ROT with the bias of q and k (in the rows' order, q's with the log2(e) / sqrt(d_h) fold) added BEFORE the rotation, as HF rotates
//              Wqkv x + b (ModernBert handles that were given attn.Wqkv.bias)
//   EPI_QKV_ROT: EPI_QKV without a bias, q and k rotated by the token's column before they are rounded (NomicBert handles; V^T as in EPI_QKV).  Both rotating
//              epilogues take F = H + 2A: [0,H) -> q, [H,H+A) -> k [T,A], [H+A,F) -> V^T [A,ldT] (A < H: a grouped-query decoder handle, one k / V^T per KV head)
//   EPI_QKV_SPLIT: the same three regions of F = H + 2A with nothing done to them: no bias, no rotation (handles with q / k norms: k_qk_norm_rope normalises and
//              rotates q and k in place behind this launch)
//   EPI_SWIGLU:  F = 2 FF, gate | up interleaved per tile: out0[T, F / 2] = silu(gate) * up, no bias (NomicBert handles)
//   EPI_GEGLU:   F = 2 FF, input | gate interleaved the same way: out0[T, F / 2] = erf_gelu(input + b) * (gate + b') (ModernBert handles; bias in the rows' order)
//   EPI_RELU:    out0[T,F] = max(acc, 0), no bias (T5 v1.0 handles: DenseReluDense.wi)
//   EPI_GEGLU_TANH: F = 2 FF, wi_0 | wi_1 interleaved like EPI_GEGLU: out0[T, F / 2] = gelu_new(wi_0 x) * wi_1 x, no bias (T5 v1.1 / flan handles)
//   EPI_SPLADE:  nothing stored per token: smax[seq, f] = max(smax, max(0, acc + bias)) over the rows of each sequence (splade_reduce)
template <int EPI, class ShapeE, bool NT>
__device__ __forceinline__ void proj_epilogue(const ProjArgs& a, AccTile<ShapeE>& acc, int64_t m0, int64_t n0, char* stage) {
    const int64_t t0 = m0 + acc.m_wave;
    const int f0 = (int)n0 + acc.n_wave;          // first feature of this wave's 64 columns; F % 64 == 0, so a wave is never partial
    if (f0 >= a.F) return;
    // A/B knob (KIRAG_AMD_EPI_PRIO, profiles/r03/tried_ab_epi_prio.txt): the two wave groups of the ping-pong loop run their epilogues side by side and the
    // younger group (tile rows 128 ..) loses the issue arbitration (its epilogue takes ~2x as long): 1 = that group at priority 1, 2 = the older group
    if (a.epi_prio && ((a.epi_prio == 1) == (acc.m_wave >= 128))) __builtin_amdgcn_s_setprio(1);
    const int h = acc.lane >> 5;
    f32x4 b[2][4];                                // bias of the lane's 32 features: (ni, g) -> features ni*32 + 8g + 4h .. +3
    if constexpr (EPI == EPI_QKV || EPI == EPI_GELU || EPI == EPI_GEGLU) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) b[ni][g] = *reinterpret_cast<const f32x4*>(a.bias + f0 + ni * 32 + 8 * g + 4 * h);
    }
    if constexpr (EPI == EPI_QKV) {
        const int region = f0 / a.H;              // H % 64 == 0: a wave's columns never straddle q | k | v
        if (region == 2) {
            store_transposed_bf16<ShapeE, NT>(acc, stage, a.outT, a.ldT, t0, f0 - 2 * a.H);   // value bias lives in bo_eff
        } else {
            store_rows_bf16<ShapeE, NT>(acc, stage, region ? a.out1 : a.out0, a.H, t0, f0 - region * a.H,
                                    [&](f32x4 v, int mi, int ni, int g) { return v + b[ni][g]; });
        }
    } else if constexpr (EPI == EPI_QKV_SPLIT) {
        const int region = f0 < a.H ? 0 : f0 < a.H + a.A ? 1 : 2;
        if (region == 2) store_transposed_bf16<ShapeE, NT>(acc, stage, a.outT, a.ldT, t0, f0 - a.H - a.A);
        else store_rows_bf16<ShapeE, NT>(acc, stage, region ? a.out1 : a.out0, region ? a.A : a.H, t0, f0 - region * a.H, [&](f32x4 v, int, int, int) { return v; });
    } else if constexpr (epi_rotates(EPI)) {
        // F = H + 2A: q below H, k below H + A (stored with pitch A), V^T behind; H % 64 == 0 and A % 64 == 0, so a wave's columns never straddle them
        const int region = f0 < a.H ? 0 : f0 < a.H + a.A ? 1 : 2;
        if (region == 2) {
            store_transposed_bf16<ShapeE, NT>(acc, stage, a.outT, a.ldT, t0, f0 - a.H - a.A);
        } else {
            // the rotation rides in store_rows_bf16's map: the table rows of ONE mi block are live at a time (requested at its first call; all of them up front
            // left the 256x256 tile's 128 accumulator registers no room), the token columns of all blocks are fetched before the first
            int64_t row[ShapeE::TM];
#pragma unroll
            for (int mi = 0; mi < ShapeE::TM; ++mi) row[mi] = rot_row(a, t0 + mi * 32 + (acc.lane & 31)) + 4 * h;
            const int jb1 = rot_jbase(a.dh, f0 + 32);     // f0 % 64 == 0: tile ni = 0 starts at 0
            f32x4 cs[2][2], sn[2][2];
            store_rows_bf16<ShapeE, NT>(acc, stage, region ? a.out1 : a.out0, region ? a.A : a.H, t0, f0 - region * a.H, [&](f32x4 v, int mi, int ni, int g) {
                if (ni == 0 && g == 0) {
                    if constexpr (EPI == EPI_QKV_ROTB) {
                        // the bias of this block's 64 features goes into its accumulators first, a quad at a time.  The offset is opaque per block: hoisted
                        // out of the store loop, the eight bias quads would be 32 more live registers next to the accumulators (the 256 x 256 tile, with 128 of them, has no
                        // room even so: launch_proj gives this epilogue the 128 x 128 loops)
                        int boff = f0 + 4 * h;
                        asm volatile("" : "+v"(boff));
#pragma unroll
                        for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                            for (int g2 = 0; g2 < 4; ++g2) {
                                const f32x4 bq = *reinterpret_cast<const f32x4*>(a.bias + boff + n2 * 32 + 8 * g2);
#pragma unroll
                                for (int i = 0; i < 4; ++i) acc.v[mi][n2][4 * g2 + i] += bq[i];
                            }
                        v = f32x4{acc.v[mi][0][0], acc.v[mi][0][1], acc.v[mi][0][2], acc.v[mi][0][3]};
                    }
#pragma unroll
                    for (int n2 = 0; n2 < 2; ++n2)
#pragma unroll
                        for (int g2 = 0; g2 < 2; ++g2) {
                            const int64_t o = row[mi] + (n2 ? jb1 : 0) + 8 * g2;
                            cs[n2][g2] = *reinterpret_cast<const f32x4*>(a.rot_cos + o);
                            sn[n2][g2] = *reinterpret_cast<const f32x4*>(a.rot_sin + o);
                        }
                }
                // v = registers 4g ..: the first halves (g < 2) take - partner * sin, the second halves + partner * sin (see rotate_tile)
                const int gp = g ^ 2;
                const f32x4 o = {acc.v[mi][ni][4 * gp], acc.v[mi][ni][4 * gp + 1], acc.v[mi][ni][4 * gp + 2], acc.v[mi][ni][4 * gp + 3]};
                return g < 2 ? v * cs[ni][g & 1] - o * sn[ni][g & 1] : v * cs[ni][g & 1] + o * sn[ni][g & 1];
            });
        }
    } else if constexpr (EPI == EPI_SWIGLU) {
        store_rows_gated<ShapeE, NT>(acc, stage, a.out0, a.ldo, t0, f0 >> 1, [](const f32x16& v, int, int g) { return swiglu_quad(v, g); });
    } else if constexpr (EPI == EPI_GEGLU) {
        // bias (tile-pair order like the rows): b[ni][g] are the input features of quad g < 2, b[ni][g + 2] their gates
        store_rows_gated<ShapeE, NT>(acc, stage, a.out0, a.ldo, t0, f0 >> 1, [&](const f32x16& v, int ni, int g) { return geglu_quad(v, g, b[ni][g], b[ni][g + 2]); });
    } else if constexpr (EPI == EPI_GEGLU_TANH) {
        store_rows_gated<ShapeE, NT>(acc, stage, a.out0, a.ldo, t0, f0 >> 1, [](const f32x16& v, int, int g) { return geglu_tanh_quad(v, g); });
    } else if constexpr (EPI == EPI_DENSE) {
        store_rows_bf16<ShapeE, NT>(acc, stage, a.out0, a.ldo, t0, f0, [&](f32x4 v, int, int, int) { return v; });   // the bias is added in k_ln (fp32)
    } else if constexpr (EPI == EPI_RELU) {
        store_rows_bf16<ShapeE, NT>(acc, stage, a.out0, a.ldo, t0, f0,
                                    [&](f32x4 v, int, int, int) { return relu4(v); });
    } else if constexpr (EPI == EPI_SPLADE) {
        splade_reduce<ShapeE>(a, acc, t0, f0);
    } else {
        store_rows_bf16<ShapeE, NT>(acc, stage, a.out0, a.ldo, t0, f0, [&](f32x4 v, int mi, int ni, int g) {
            const f32x4 x = v + b[ni][g];
            const f32x2 lo = gelu_erf_fast2(f32x2{x.x, x.y}), hi = gelu_erf_fast2(f32x2{x.z, x.w});
            return f32x4{lo.x, lo.y, hi.x, hi.y};
        });
    }
    if (a.epi_prio) __builtin_amdgcn_s_setprio(0);
}

// ANT: the activation operand is loaded non-temporally (FF2's h: launch_proj)
template <int EPI, class ShapeE, int STAGES, bool NT, bool ANT = false>
__global__ __launch_bounds__(ShapeE::NTHREADS, 2) void k_proj(ProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = *a.Tp;
    const int64_t tm_count = (T + ShapeE::BM - 1) / ShapeE::BM, tn_count = (a.F + ShapeE::BN - 1) / ShapeE::BN;
    char* stage = smem + STAGES * ShapeE::STAGE_BYTES + (threadIdx.x >> 6) * EPI_STAGE_BYTES;
    auto coord = [&](int64_t nat, int64_t& m0, int64_t& n0) {
        int64_t tm, tn;
        patch_coord(nat, tm_count, tn_count, tm, tn, (uint32_t)a.pw);
        m0 = tm * ShapeE::BM; n0 = tn * ShapeE::BN;
    };
    gemm_main<ShapeE, STAGES, ANT>(a.X, a.ldx, T, a.W, a.K, a.F, a.K, tm_count * tn_count, smem, coord,
                                   [&](AccTile<ShapeE>& acc, int64_t m0, int64_t n0, int64_t) { proj_epilogue<EPI, ShapeE, NT>(a, acc, m0, n0, stage); });
}

// the same projections on the producer / consumer 128x128 loop (gemm_nt_split): 4 multiplying + 4 staging waves, 4-slot ring + one 4-KiB epilogue
// stage per multiplying wave = 144 KiB, one persistent block per CU
template <int EPI>
__global__ __launch_bounds__(SPLIT_THREADS) void k_proj_split(ProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int T = *a.Tp;
    const int64_t tm_count = (T + 127) / 128, tn_count = (a.F + 127) / 128;
    char* stage = smem + SPLIT_RING * ShapeSplit::STAGE_BYTES + ((threadIdx.x >> 6) & 3) * EPI_STAGE_BYTES;
    gemm_nt_split<ET, true>(
        a.X, a.ldx, T, a.W, a.K, a.F, a.K, tm_count * tn_count, smem,
        [&](int64_t nat, int64_t& m0, int64_t& n0) {
            int64_t tm, tn;
            patch_coord(nat, tm_count, tn_count, tm, tn, (uint32_t)a.pw);
            m0 = tm * 128; n0 = tn * 128;
        },
        [&](AccTile<ShapeSplit>& acc, int64_t m0, int64_t n0, int64_t) { proj_epilogue<EPI, ShapeSplit, false>(a, acc, m0, n0, stage); });
}

// the same projections for a handful of token rows on the skinny loop (gemm_nt_skinny): one (32 WM)-token x (32 WN)-feature tile per block,
// grid = (F / (32 WN), T / (32 WM)).  Epilogue straight from the accumulator (swapped layout: a lane holds 4 consecutive features of one token per register
// quad): 8-byte row stores, 2-byte stores for V^T — at these sizes the stores are noise next to the operand stream.
// (Round 5 built the LayerNorm behind a dense projection as the TAIL of this launch — write-through y, an arrival counter per token tile, the last
// arriver normalises the tile's rows — bit-identical and SLOWER: the one block that finds itself last works through 32 rows alone, 26.8 us per launch
// against 9.2 + 5.3 for the two launches; profiles/r05/tried_ln_tail.txt.)
template <int EPI, int RING, int WM = 1, int WN = 1>
__global__ __launch_bounds__((WM * WN + 4) * 64) void k_proj_skinny(ProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int64_t m0 = (int64_t)blockIdx.y * (32 * WM), n0 = (int64_t)blockIdx.x * (32 * WN);
    f32x4 bias4[4];                                       // multiplying waves: the bias of the lane's 16 features, requested before the main loop
    gemm_nt_skinny<ET, RING, WM, WN, true>(a.X, a.ldx, a.Tp, m0, a.W, a.K, a.F, n0, a.K, smem,
        [&](int64_t, int64_t f0) {
            if constexpr (EPI == EPI_QKV || EPI == EPI_GELU || EPI == EPI_GEGLU || EPI == EPI_QKV_ROTB) {
                const int h = (threadIdx.x & 63) >> 5;
#pragma unroll
                for (int g = 0; g < 4; ++g) bias4[g] = *reinterpret_cast<const f32x4*>(a.bias + f0 + 8 * g + 4 * h);   // QKV: the V third's slots are never used
            }
        },
        [&](AccTile<ShapeSkinny>& acc, int64_t t0, int64_t f0) {
        const int c = acc.lane & 31, h = acc.lane >> 5;
        if constexpr (EPI == EPI_SPLADE) {
            splade_reduce<ShapeSkinny>(a, acc, t0, (int)f0);
            return;
        }
        if constexpr (epi_gated(EPI)) {      // the tile's 16 features: 8-byte row stores of silu(gate) * up / erf_gelu(input) * gate / gelu_new(wi_0 x) * wi_1 x
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                f32x4 p;
                if constexpr (EPI == EPI_SWIGLU) p = swiglu_quad(acc.v[0][0], g);
                else if constexpr (EPI == EPI_GEGLU_TANH) p = geglu_tanh_quad(acc.v[0][0], g);
                else p = geglu_quad(acc.v[0][0], g, bias4[g], bias4[g + 2]);
                uint2 w;
                w.x = pack_bf16x2(p.x, p.y);
                w.y = pack_bf16x2(p.z, p.w);
                *reinterpret_cast<uint2*>(a.out0 + (t0 + c) * a.ldo + ((int)f0 >> 1) + 8 * g + 4 * h) = w;
            }
            return;
        }
        if constexpr (epi_rotates(EPI)) {
            if ((int)f0 < a.H + a.A) {                    // q and k: (biased and) rotated in place, then stored like EPI_QKV's
                if constexpr (EPI == EPI_QKV_ROTB) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc.v[0][0][r] += bias4[r >> 2][r & 3];
                }
                const int64_t o = rot_row(a, t0 + c) + 4 * h + rot_jbase(a.dh, (int)f0);
                rotate_tile(acc.v[0][0], a.rot_cos + o, a.rot_sin + o);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = {acc.v[0][0][4 * g], acc.v[0][0][4 * g + 1], acc.v[0][0][4 * g + 2], acc.v[0][0][4 * g + 3]};
            const int f = (int)f0 + 8 * g + 4 * h;        // first of the lane's 4 consecutive features
            if constexpr (EPI == EPI_QKV || epi_splits(EPI)) {
                // EPI_QKV: thirds of 3H.  The rotating epilogues and EPI_QKV_SPLIT: q below H, k below H + A with pitch A, V^T behind (proj_epilogue)
                const int kv = epi_splits(EPI) ? a.A : a.H;
                const int region = (int)f0 < a.H ? 0 : (int)f0 < a.H + kv ? 1 : 2;
                if (region == 2) {                        // V^T [feature, token]; its bias lives in bo_eff
#pragma unroll
                    for (int j = 0; j < 4; ++j) a.outT[(int64_t)(f - a.H - kv + j) * a.ldT + t0 + c] = ET::from_f32(v[j]);
                    continue;
                }
                if constexpr (EPI == EPI_QKV) v = v + bias4[g];
                uint2 w; w.x = pack_bf16x2(v.x, v.y); w.y = pack_bf16x2(v.z, v.w);
                *reinterpret_cast<uint2*>((region ? a.out1 : a.out0) + (t0 + c) * (region ? kv : a.H) + (f - region * a.H)) = w;
            } else {
                if constexpr (EPI == EPI_GELU) {
                    v = v + bias4[g];
                    const f32x2 lo = gelu_erf_fast2(f32x2{v.x, v.y}), hi = gelu_erf_fast2(f32x2{v.z, v.w});
                    v = f32x4{lo.x, lo.y, hi.x, hi.y};
                }
                if constexpr (EPI == EPI_RELU) v = relu4(v);
                uint2 w; w.x = pack_bf16x2(v.x, v.y); w.y = pack_bf16x2(v.z, v.w);
                *reinterpret_cast<uint2*>(a.out0 + (t0 + c) * a.ldo + f) = w;
            }
        }
    });
}

// ---------------------------------------------------------------------------------------------------------
// host side: the launchers (the library's forward and tests/capi/proj_probe.hip launch through them)
// ---------------------------------------------------------------------------------------------------------
// The runtime epilogue as a compile-time constant: f(std::integral_constant<int, EPI>{}) for the epilogues above.  What a launch site does not build for an
// epilogue, it excludes itself with `if constexpr`.
template <class F>
static int with_epilogue(int epi, F&& f) {
    switch (epi) {
        case EPI_QKV: return f(std::integral_constant<int, EPI_QKV>{});
        case EPI_DENSE: return f(std::integral_constant<int, EPI_DENSE>{});
        case EPI_GELU: return f(std::integral_constant<int, EPI_GELU>{});
        case EPI_QKV_ROT: return f(std::integral_constant<int, EPI_QKV_ROT>{});
        case EPI_QKV_ROTB: return f(std::integral_constant<int, EPI_QKV_ROTB>{});
        case EPI_SWIGLU: return f(std::integral_constant<int, EPI_SWIGLU>{});
        case EPI_GEGLU: return f(std::integral_constant<int, EPI_GEGLU>{});
        case EPI_RELU: return f(std::integral_constant<int, EPI_RELU>{});
        case EPI_GEGLU_TANH: return f(std::integral_constant<int, EPI_GEGLU_TANH>{});
        case EPI_SPLADE: return f(std::integral_constant<int, EPI_SPLADE>{});
        case EPI_QKV_SPLIT: return f(std::integral_constant<int, EPI_QKV_SPLIT>{});
        default: return fail(KR_EINVAL, "projection epilogue %d is not built into this library", epi);
    }
}

// one launch: the LDS attribute once per (kernel, device), then the kernel
template <class Kern>
static int launch_proj_kernel(Kern kern, dim3 grid, int threads, int lds, const ProjArgs& a, int device, hipStream_t st) {
    KR_TRY(set_lds_once(reinterpret_cast<const void*>(kern), lds, device));
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, st, a);
    return 0;
}

// the persistent loops over whole tiles (k_proj): `blocks` blocks walk the tiles
template <class Shape, int STAGES, bool NT>
static int launch_proj_shape_nt(int epi, const ProjArgs& a, int blocks, int device, hipStream_t st) {
    constexpr int lds = STAGES * Shape::STAGE_BYTES + Shape::NWAVE * EPI_STAGE_BYTES;   // 160 KiB for the 256x256 tile: the whole LDS of a CU
    auto go = [&](auto kern) -> int { return launch_proj_kernel(kern, dim3(blocks), Shape::NTHREADS, lds, a, device, st); };
    const bool ant = a.ant && Shape::BM == 256;   // the non-temporal activation operand exists for the ping-pong loop only
    return with_epilogue(epi, [&](auto tag) -> int {
        constexpr int EPI = decltype(tag)::value;
        if constexpr (EPI == EPI_QKV_ROTB && Shape::BM == 256)      // not on the 256 x 256 tile (launch_proj): the bias quads next to its 128 accumulators spill
            return fail(KR_EINVAL, "projection epilogue %d is not built for the 256 x 256 tile", epi);
        else if constexpr (EPI == EPI_SPLADE && NT)                 // stores no rows: one instantiation per shape (launch_proj clears nt)
            return fail(KR_EINVAL, "projection epilogue %d has no non-temporal stores", epi);
        else if constexpr (EPI == EPI_DENSE) return ant ? go(&k_proj<EPI_DENSE, Shape, STAGES, NT, true>) : go(&k_proj<EPI_DENSE, Shape, STAGES, NT>);
        else return go(&k_proj<EPI, Shape, STAGES, NT>);
    });
}
// the skinny loop: one (32 WM)^2 tile per block, a ring of 16 / 8 K-tiles
template <int WM>
static int launch_proj_skinny(int epi, const ProjArgs& a, int64_t max_tokens, int device, hipStream_t st) {
    constexpr int RING = WM == 1 ? 16 : 8;
    using G = SkinnyGeom<WM, WM>;
    const dim3 grid((unsigned)(a.F / (32 * WM)), (unsigned)((max_tokens + 32 * WM - 1) / (32 * WM)));
    return with_epilogue(epi, [&](auto tag) -> int {
        return launch_proj_kernel(&k_proj_skinny<decltype(tag)::value, RING, WM, WM>, grid, G::THREADS, RING * G::STAGE, a, device, st);
    });
}

// Mechanism.  One projection launch on the main loop `loop` (the values of KIRAG_AMD_PROJ_TILE: 256 ping-pong, 128 streaming, 130 producer / consumer, 64 / 32
// skinny) with `a` as given (nt, ant, pw, epi_prio, ldx, ldo): grid, block size, LDS bytes, the LDS attribute, the instantiation, the launch.  blocks: the
// persistent grid of 256 / 128 / 130; max_tokens: the token rows the skinny grid covers.  What a loop is not built for is refused: EPI_QKV_ROTB on the 256 tile,
// EPI_SPLADE with non-temporal stores; ant is honoured by EPI_DENSE on the ping-pong loop only.
static int launch_proj_loop(int epi, const ProjArgs& a, int loop, int blocks, int64_t max_tokens, int device, hipStream_t st) {
    switch (loop) {
        case 256: return a.nt ? launch_proj_shape_nt<ShapeBig, 2, true>(epi, a, blocks, device, st) : launch_proj_shape_nt<ShapeBig, 2, false>(epi, a, blocks, device, st);
        case 128: return a.nt ? launch_proj_shape_nt<ShapeSmall, 2, true>(epi, a, blocks, device, st) : launch_proj_shape_nt<ShapeSmall, 2, false>(epi, a, blocks, device, st);
        case 130: {
            constexpr int lds = SPLIT_RING * ShapeSplit::STAGE_BYTES + 4 * EPI_STAGE_BYTES;
            return with_epilogue(epi, [&](auto tag) -> int { return launch_proj_kernel(&k_proj_split<decltype(tag)::value>, dim3(blocks), SPLIT_THREADS, lds, a, device, st); });
        }
        case 64: return launch_proj_skinny<2>(epi, a, max_tokens, device, st);
        case 32: return launch_proj_skinny<1>(epi, a, max_tokens, device, st);
        default: return fail(KR_EINVAL, "projection loop %d: 256, 128, 130, 64 or 32", loop);
    }
}

// Policy.  What a forward's projection launches with: the CUs the persistent grids are sized for, the device, and the A/B switches read once per forward
// (KIRAG_AMD_PATCH_W, KIRAG_AMD_EPI_PRIO, KIRAG_AMD_PROJ_TILE)
struct ProjLaunch { int num_cu, device, pw, epi_prio, force_tile; };

// tile shape per launch: when the 256x256 tiling has fewer tiles than ~5/8 of the CUs (small batches: the reference's per_gpu_batch_size 4-8, the KiRAG
// loop's triple batches, a 1/8 slice of a query batch) the 128x128 tiling gives 4x the parallelism at a quarter of the per-tile latency
static int launch_proj(int epi, const ProjArgs& a_in, int64_t max_tokens, const ProjLaunch& ctx, hipStream_t st) {
    const int num_cu = ctx.num_cu, device = ctx.device;
    ProjArgs a = a_in;
    if (a.ldx == 0) a.ldx = a.K;
    if (a.ldo == 0) a.ldo = a.F;
    a.pw = ctx.pw;
    a.epi_prio = ctx.epi_prio;
    // store policy by output size (see ProjArgs::nt)
    a.nt = epi != EPI_SPLADE && max_tokens * (int64_t)(epi_gated(epi) ? a.F / 2 : a.F) * 2 > ((int64_t)96 << 20) ? 1 : 0;
    // FF2 (K = FF > H): its activation operand h is a once-through stream four times the size of every other activation (256 MiB at 32 k tokens); loaded
    // non-temporally it leaves the L2 / Infinity Cache to the weights and to the residual stream the LayerNorm behind it reads: -0.7 % forward time at
    // 1000 x 32 tokens, neutral elsewhere (profiles/r04/tried_nt_activations.txt; outputs bit-identical).
    a.ant = a.K > a.H ? 1 : 0;
    const int64_t big_tiles = ((max_tokens + 255) / 256) * ((a.F + 255) / 256);
    const int64_t small_tiles = ((max_tokens + 127) / 128) * ((a.F + 127) / 128);
    const int force = ctx.force_tile;
    const bool small = force == 128 || (force != 256 && big_tiles * 8 < (int64_t)num_cu * 5) || epi == EPI_QKV_ROTB;   // measured crossover: ~5/8 of the CUs busy with 256x256 tiles
    // a handful of token rows: the skinny loop, one tile per block (latency chain: the operand stream of the launch spread over as many CUs as it has
    // tiles).  32 x 32 tiles while there is at most one per CU, 64 x 64 (four multiplying waves share every staged K-tile: half the L2 -> LDS bytes per
    // output element) up to four 32 x 32 tiles' worth per CU — the crossover against the 128x128 producer / consumer loop measured in round 1.
    // KIRAG_AMD_PROJ_TILE = 32 / 64 forces one of the two.
    const int64_t skinny_tiles = ((max_tokens + 31) / 32) * (a.F / 32);
    if (force == 32 || force == 64 || (force == 0 && skinny_tiles <= 4 * (int64_t)num_cu && (max_tokens + 31) / 32 <= 65535)) {
        const bool one = force == 32 || (force == 0 && skinny_tiles <= num_cu);
        return launch_proj_loop(epi, a, one ? 32 : 64, 0, max_tokens, device, st);
    }
    if (!small) return launch_proj_loop(epi, a, 256, num_cu, max_tokens, device, st);
    // producer/consumer loop (one persistent block per CU): at most one tile per CU, or more than two (measured: 600 tiles -7 % vs the streaming loop
    // with two blocks per CU; between one and two tiles per CU the two co-resident streaming blocks quantise better).  130 forces it, 128 the streaming loop
    if (((small_tiles <= num_cu || small_tiles > 2 * num_cu) && force != 128) || force == 130) return launch_proj_loop(epi, a, 130, num_cu, max_tokens, device, st);
    return launch_proj_loop(epi, a, 128, 2 * num_cu, max_tokens, device, st);
}

}  // namespace KR_ENC_NS
}  // namespace kr
