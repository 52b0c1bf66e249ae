// Sentence encoder, device code over token rows: weight conversion, the residual stream's byte codec, embedding + LayerNorm, LayerNorm, pooling and the
// CLS gather.  Part of encoder.hip (see its header); defines the namespace of the build's operand type and ET for the other encoder_*.hpp.
#pragma once
#include "gemm_nt.hpp"

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

// This file is compiled TWICE (kirag_amd/csrc/Makefile): once per 16-bit operand type of the MFMAs and of every stored activation —
//   bf16 (8 significand bits, fp32 range)  and  f16 (11 significand bits, |x| <= 65504; -DKR_ENC_F16)
// — into the namespaces kr::enc_bf16 / kr::enc_f16; encoder_api.hip holds the C entry points and picks one per handle (kr_encoder_create_ex).
// Why both exist: DESIGN.md section 4.2 "operand precision" (weights with outlier channels need the 11 bits to stay within the 1e-3 score tolerance).
#ifdef KR_ENC_BUILD_F16
#define KR_ENC_NS enc_f16
#else
#define KR_ENC_NS enc_bf16
#endif

namespace kr {
namespace KR_ENC_NS {

#ifdef KR_ENC_BUILD_F16
using ET = F16;
#else
using ET = BF16;
#endif

// ---------------------------------------------------------------------------------------------------------
// small kernels
// ---------------------------------------------------------------------------------------------------------
__global__ void k_f32_to_bf16(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = ET::from_f32(src[i] * scale);
}
// the same conversion of a [rows, cols] matrix whose rows change place (NomicBert handles: every 32-column MFMA tile of a projection holds 16 features and
// their 16 partners, so that the rotary / gated epilogues combine register r with r + 8 of ONE tile on every main loop, see encoder_proj.hpp):
//   ROWS_HEAD64:  q / k with 64-wide heads: the four 16-row blocks of a head in the order 0, 2, 1, 3 (feature j next to its rotary partner j + 32)
//   ROWS_GATE / ROWS_UP:  gate_proj / up_proj into one [2 FF, H] matrix: tile t = gate rows 16 t .. 16 t + 15, then the up rows of the same features
enum { ROWS_HEAD64 = 0, ROWS_GATE = 1, ROWS_UP = 2 };
__host__ __device__ inline int64_t tile_pair_row(int64_t r, int mode) {
    if (mode == ROWS_HEAD64) {
        const int64_t b = (r >> 4) & 3;
        return (r & ~(int64_t)63) + ((((b & 1) << 1) | (b >> 1)) << 4) + (r & 15);
    }
    return ((r >> 4) << 5) + (mode == ROWS_UP ? 16 : 0) + (r & 15);
}
__global__ void k_f32_to_bf16_rows(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n, int cols, float scale, int mode) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[tile_pair_row(i / cols, mode) * cols + i % cols] = ET::from_f32(src[i] * scale);
}
__global__ void k_scale_copy(const float* __restrict__ src, float* __restrict__ dst, int64_t n, float scale) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i] * scale;
}

// b_o' = b_o + W_o . b_v : softmax rows sum to 1, so P (X W_v^T + b_v) = P X W_v^T + b_v and the value bias moves into the output projection
// (wo [H, K], bv [K]: K = the width of the context, H unless the handle has a head width of its own)
__global__ void k_fold_vbias(const uint16_t* __restrict__ wo, const float* __restrict__ bo, const float* __restrict__ bv, float* __restrict__ out, int H, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= H) return;
    float s = 0.f;
    for (int j = 0; j < K; ++j) s += ET::to_f32(wo[(int64_t)i * K + j]) * bv[j];
    out[i] = bo[i] + s;
}

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
// two floats -> packed 16-bit pair (lo in bits 0..15), round-to-nearest-even, NaN stays NaN: ONE v_cvt_pk_bf16_f32 / the f16 conversions of the target
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
#ifdef KR_ENC_BUILD_F16
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, f16x2_t));
#else
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{lo, hi}, bf16x2_t));
#endif
}
// the two halves of a packed pair as fp32
__device__ __forceinline__ float unpack_lo16(unsigned int w) {
#ifdef KR_ENC_BUILD_F16
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
#else
    return __builtin_bit_cast(float, w << 16);
#endif
}
__device__ __forceinline__ float unpack_hi16(unsigned int w) {
#ifdef KR_ENC_BUILD_F16
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
#else
    return __builtin_bit_cast(float, w & 0xffff0000u);
#endif
}

// Low half of the residual stream: x = hi + lo with hi = the 16-bit operand the GEMMs read (round-to-nearest of x) and lo = ONE byte: the distance from hi to
// x in units of ulp(hi) / 256, biased by 128 (19 significand bits with f16 operands, 16 with bf16).  Round 2 kept lo as a second 16-bit word (10 B per
// element through a LayerNorm instead of 6); the byte makes it 8 B — on the emulation of the rounding points (tools/precision_probe.py, G10 out3 / out16) the
// worst score error is unchanged (9.1e-5 vs 8.6e-5 / 1.2e-3 vs 9.5e-4).
// The byte is computed ON THE BIT PATTERNS (round 4): x and hi have the same sign and neighbouring magnitudes, so bits(x) - bits(hi) (both as fp32) is their
// distance in fp32 ulps, signed towards larger magnitude, and 2^LO_SH of those are ulp(hi) / 256 (a unit half as large when hi rounded up into the next
// binade: still within +-128).  Encode = subtract, add the rounding constant, shift, clamp (4 integer instructions); decode = shift-add + constant (3, the
// byte extraction included) — a third of the floating-point form (exponent extraction, two constructed powers of two, rint, min, max, conversions) that made
// round 4's fused residual epilogue VALU-bound (profiles/r04/tried_fused_layernorm.txt).  |x| < 2^-25 (hi = +-0) clamps to a denormal: an absolute error below 2^-25.
#ifdef KR_ENC_BUILD_F16
constexpr int LO_SH = 5;        // 23 - 10 stored mantissa bits - 8
#else
constexpr int LO_SH = 8;        // 23 - 7 - 8
#endif
__device__ __forceinline__ unsigned int lo_encode(float o, float hf) {
    const int d = (int)(__builtin_bit_cast(unsigned int, o) - __builtin_bit_cast(unsigned int, hf));
    // round to nearest, biased by 128; clamped BEFORE the shift.  (Shift-then-clamp of two neighbours is selected to v_ashr_pk_u8_i32, which on gfx950 writes only
    // bits 15:0 of its destination — the compiler assumes the upper half is zero and ORs the stale bits into the neighbouring bytes: tools/ashr_pk_check.hip)
    const int t = min(max(d + ((1 << (LO_SH - 1)) + (128 << LO_SH)), 0), (256 << LO_SH) - 1);
    return (unsigned int)t >> LO_SH;
}
__device__ __forceinline__ float lo_decode(unsigned int byte, float hf) {
    return __builtin_bit_cast(float, __builtin_bit_cast(unsigned int, hf) + (byte << LO_SH) - (128u << LO_SH));
}
// lo_decode for readers of the FINAL hidden state (pooling, kr_encoder_last_hidden): a non-finite hi (a LayerNorm output beyond the f16 range, or NaN) decodes
// to ITSELF — on the bit patterns inf - 4096 would be a finite 3.4e38.  Inside the stack the overflow travels with the 16-bit stream itself (the next GEMM reads
// hi = inf and every LayerNorm behind it sees NaN through y), so the LayerNorm's residual decode keeps the 3-instruction form (its two extra VALU instructions per
// element cost 0.3 % of the 1000-query step); behind the LAST LayerNorm there is no GEMM, only this decode (tests/test_lo_codec_spec.py,
// tests/test_gpu_lifecycle.py: an overflow in the last LayerNorm must raise KR_ERANGE).
__device__ __forceinline__ float lo_decode_final(unsigned int byte, float hf) {
    const unsigned int hb = __builtin_bit_cast(unsigned int, hf);
    return (hb & 0x7f800000u) == 0x7f800000u ? hf : lo_decode(byte, hf);
}

// LayerNorm of one row held as up to 8 float4 per lane (H <= 2048); writes fp32 and bf16 copies
__device__ __forceinline__ void ln_row_store(float4 (&v)[8], int H, int lane, const float* __restrict__ g, const float* __restrict__ bta, float eps,
                                             uint8_t* __restrict__ xlo_row, uint16_t* __restrict__ xb_row) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (lane * 4 + j * 256 < H) s += v[j].x + v[j].y + v[j].z + v[j].w;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    const float mu = s / (float)H;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (lane * 4 + j * 256 < H) {
            const float a = v[j].x - mu, b = v[j].y - mu, c = v[j].z - mu, d = v[j].w - mu;
            q += a * a + b * b + c * c + d * d;
        }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m, 64);
    const float rstd = 1.0f / sqrtf(q / (float)H + eps);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = lane * 4 + j * 256;
        if (i < H) {
            const float4 gg = *reinterpret_cast<const float4*>(g + i);
            const float4 bb = *reinterpret_cast<const float4*>(bta + i);
            float4 o;
            o.x = (v[j].x - mu) * rstd * gg.x + bb.x; o.y = (v[j].y - mu) * rstd * gg.y + bb.y;
            o.z = (v[j].z - mu) * rstd * gg.z + bb.z; o.w = (v[j].w - mu) * rstd * gg.w + bb.w;
            ushort4 ob;
            ob.x = ET::from_f32(o.x); ob.y = ET::from_f32(o.y); ob.z = ET::from_f32(o.z); ob.w = ET::from_f32(o.w);
            *reinterpret_cast<ushort4*>(xb_row + i) = ob;
            if (xlo_row)                                                      // optional low half (kernel-uniform branch): one byte per element
                *reinterpret_cast<unsigned int*>(xlo_row + i) = lo_encode(o.x, ET::to_f32(ob.x)) | (lo_encode(o.y, ET::to_f32(ob.y)) << 8) |
                                                                (lo_encode(o.z, ET::to_f32(ob.z)) << 16) | (lo_encode(o.w, ET::to_f32(ob.w)) << 24);
        }
    }
}

// embeddings: word[id] + position[pos] + token_type[0] -> LayerNorm       (one wave per token; tok_pos = the handle's embedding-position table: the column
// under BERT's rule, tok_epos under fairseq's)
__global__ __launch_bounds__(256) void k_embed_ln(const int* __restrict__ tok_id, const int* __restrict__ tok_pos, const int* __restrict__ tok_type, const int* __restrict__ Tp,
                                                  const float* __restrict__ word, const float* __restrict__ pos, const float* __restrict__ type,
                                                  const float* __restrict__ g, const float* __restrict__ bta, float eps, int H,
                                                  uint8_t* __restrict__ xlo, uint16_t* __restrict__ xb) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= *Tp) return;
    const float* w = word + (int64_t)tok_id[t] * H;
    const float* p = pos + (int64_t)tok_pos[t] * H;
    const float* ty = type + (int64_t)tok_type[t] * H;       // token_type_embeddings row (0 for every KiRAG caller)
    float4 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int i = lane * 4 + j * 256;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < H) {
            const float4 a = *reinterpret_cast<const float4*>(w + i);
            const float4 b = *reinterpret_cast<const float4*>(p + i);
            const float4 c = *reinterpret_cast<const float4*>(ty + i);
            v[j] = make_float4((a.x + b.x) + c.x, (a.y + b.y) + c.y, (a.z + b.z) + c.z, (a.w + b.w) + c.w);
        }
    }
    ln_row_store(v, H, lane, g, bta, eps, xlo ? xlo + t * H : nullptr, xb + t * H);
}

// Rotary handles: the position a token is rotated by = its column minus the smallest column among its sequence's rows (attended rows are packed in column
// order; the query-only CLS row of a masked column 0 has column 0 and sits last).  Scores depend on column differences only, so the shift changes nothing in
// exact arithmetic; in 16-bit storage it makes a sequence's rows the same bits wherever it stands in the padded batch, and keeps the angles small.  One wave per
// sequence; the alignment rows behind a sequence get 0.
__global__ __launch_bounds__(64) void k_rot_pos(const int* __restrict__ seq_off, const int* __restrict__ seq_nq, int align, const int* __restrict__ tok_pos,
                                                 int* __restrict__ rpos) {
    const int o = seq_off[blockIdx.x], n = seq_nq[blockIdx.x];
    if (n <= 0) return;
    const int first = min(tok_pos[o], tok_pos[o + n - 1]);
    const int padded = (n + align - 1) & ~(align - 1);
    for (int i = threadIdx.x; i < padded; i += 64) rpos[o + i] = i < n ? tok_pos[o + i] - first : 0;
}

// Handles with q / k norms (Qwen3): behind the EPI_QKV_SPLIT projection, in place on q [T, heads DH] and k [T, kv_heads DH], per (token, head) in fp32
//   x <- x * rsqrt(mean(x^2) + eps) * g, then the NeoX rotation by the token's position (x'[j] = x[j] cos - x[j + DH/2] sin, x'[j + DH/2] = x[j + DH/2] cos +
//   x[j] sin) — HF's order, norm before rope.  gq carries the score scale log2(e) / sqrt(DH): a scale folded in FRONT of an RMS norm is undone by it.  (W_q does
//   carry the loader's fold s all the same — the loader cannot know that norms will follow: eps_q = s^2 eps makes the norm of s x the norm of x.)
// DH / 8 lanes per head, a lane owns features 4 i .. 4 i + 3 and their rotary partners (+ DH / 2): two 8-byte accesses, a rotary pair never leaves its lane,
// the sum of squares is log2(DH / 8) shuffles.  A 64-wide head lies in tile-pair order (ROWS_HEAD64: its 16-feature blocks as 0, 2, 1, 3), as the rotating
// epilogues store it, and stays so; 32- and 128-wide heads in plain order.  The rows past the packed total are not touched.
template <int DH>
__global__ __launch_bounds__(256) void k_qk_norm_rope(uint16_t* __restrict__ q, uint16_t* __restrict__ k, const int* __restrict__ Tp, int heads, int kv_heads,
                                                      const float* __restrict__ gq, const float* __restrict__ gk, float eps_q, float eps_k,
                                                      const float* __restrict__ rot_cos, const float* __restrict__ rot_sin, const int* __restrict__ tpos, int max_pos) {
    static_assert(DH == 32 || DH == 64 || DH == 128, "head width 32, 64 or 128");
    constexpr int LPH = DH / 8, HPW = 64 / LPH;           // lanes per head, heads per wave
    const int lane = threadIdx.x & 63, i = lane % LPH;
    const int nh = heads + kv_heads;
    const int64_t u = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * HPW + lane / LPH;
    const bool live = u < (int64_t)*Tp * nh;              // whole LPH-lane groups are live or not; the others ride along for the shuffles
    const int64_t t = live ? u / nh : 0;
    const int hd = live ? (int)(u % nh) : 0;
    const bool isq = hd < heads;
    uint16_t* row = isq ? q + (t * heads + hd) * DH : k + (t * kv_heads + (hd - heads)) * DH;
    const int f = 4 * i;                                  // the lane's first feature; where it and its partner lie in the row
    const int pa = DH == 64 ? (f < 16 ? f : f + 16) : f, pb = DH == 64 ? (f < 16 ? f + 16 : f + 32) : f + DH / 2;
    const uint2 wa = *reinterpret_cast<const uint2*>(row + pa), wb = *reinterpret_cast<const uint2*>(row + pb);
    float x[4] = {unpack_lo16(wa.x), unpack_hi16(wa.x), unpack_lo16(wa.y), unpack_hi16(wa.y)};
    float y[4] = {unpack_lo16(wb.x), unpack_hi16(wb.x), unpack_lo16(wb.y), unpack_hi16(wb.y)};
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) ss += x[j] * x[j] + y[j] * y[j];
#pragma unroll
    for (int m = LPH / 2; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    const float rs = rsqrtf(ss * (1.0f / DH) + (isq ? eps_q : eps_k));
    const float* g = isq ? gq : gk;
    const float4 ga = *reinterpret_cast<const float4*>(g + f), gb = *reinterpret_cast<const float4*>(g + f + DH / 2);
    const int p = tpos[t];
    const int64_t ro = (int64_t)((unsigned)p < (unsigned)max_pos ? p : 0) * (DH / 2) + f;
    const float4 cs = *reinterpret_cast<const float4*>(rot_cos + ro), sn = *reinterpret_cast<const float4*>(rot_sin + ro);
    const float gav[4] = {ga.x, ga.y, ga.z, ga.w}, gbv[4] = {gb.x, gb.y, gb.z, gb.w}, c[4] = {cs.x, cs.y, cs.z, cs.w}, s[4] = {sn.x, sn.y, sn.z, sn.w};
    float oa[4], ob[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = x[j] * rs * gav[j], b = y[j] * rs * gbv[j];
        oa[j] = a * c[j] - b * s[j];
        ob[j] = b * c[j] + a * s[j];
    }
    if (!live) return;
    *reinterpret_cast<uint2*>(row + pa) = make_uint2(pack_bf16x2(oa[0], oa[1]), pack_bf16x2(oa[2], oa[3]));
    *reinterpret_cast<uint2*>(row + pb) = make_uint2(pack_bf16x2(ob[0], ob[1]), pack_bf16x2(ob[2], ob[3]));
}

// LayerNorm(y + bias + residual) with 16-byte accesses: a lane owns 8 consecutive elements per 512-element step (one global_load_dwordx4 per tensor and step:
// 8-byte accesses reach 0.54-0.70 of the 16-byte rate, MI355X_MICROARCH.md).  NS 512-element steps cover a row (H <= 512 NS, H % 8 == 0).
// The row arithmetic lives in Ln16<NS> (one definition for every kernel that normalises a row).
// RMS (T5 handles, T5LayerNorm): w * x * rsqrt(mean(x^2) + eps) — no mean is subtracted and there is no beta (bta is never read).
template <int NS, bool RMS = false>
struct Ln16 {
    float gg[NS][8], bb[NS][8], yb[NS][8];     // gamma, beta, the projection's bias (added in fp32) of the lane's elements
    __device__ __forceinline__ void load_params(const float* __restrict__ g, const float* __restrict__ bta, const float* __restrict__ ybias, int H, int lane) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int i = lane * 8 + j * 512;
#pragma unroll
            for (int c = 0; c < 8; ++c) { gg[j][c] = 0.f; bb[j][c] = 0.f; yb[j][c] = 0.f; }
            if (i < H) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float4 a = *reinterpret_cast<const float4*>(g + i + 4 * h), c = *reinterpret_cast<const float4*>(ybias + i + 4 * h);
                    gg[j][4 * h] = a.x; gg[j][4 * h + 1] = a.y; gg[j][4 * h + 2] = a.z; gg[j][4 * h + 3] = a.w;
                    if constexpr (!RMS) {
                        const float4 b = *reinterpret_cast<const float4*>(bta + i + 4 * h);
                        bb[j][4 * h] = b.x; bb[j][4 * h + 1] = b.y; bb[j][4 * h + 2] = b.z; bb[j][4 * h + 3] = b.w;
                    }
                    yb[j][4 * h] = c.x; yb[j][4 * h + 1] = c.y; yb[j][4 * h + 2] = c.z; yb[j][4 * h + 3] = c.w;
                }
            }
        }
    }
    // v = (y + bias) + residual, the residual decoded from its 16-bit half and its low-half byte.  KEEP_INF (k_ln16_pre): a non-finite high half decodes to
    // itself (lo_decode_final).  The post-LN stack needs no such care — its residual is the GEMM operand, so an overflow reaches the next LayerNorm through y —
    // but nothing else ever reads the pre-LN residual stream: decoded on the bit patterns, an overflowed element would come back as a finite 3.4e38, the row
    // would normalise to beta and the overflow would never reach the error word
    template <bool KEEP_INF = false>
    __device__ __forceinline__ void combine(const uint4 (&a)[NS], const uint4 (&rh)[NS], const uint2 (&rl)[NS], float (&v)[NS][8]) const {
        auto dec = [](unsigned int byte, float hf) { if constexpr (KEEP_INF) return lo_decode_final(byte, hf); else return lo_decode(byte, hf); };
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const unsigned int aw[4] = {a[j].x, a[j].y, a[j].z, a[j].w}, hw[4] = {rh[j].x, rh[j].y, rh[j].z, rh[j].w}, lw[2] = {rl[j].x, rl[j].y};
#pragma unroll
            for (int c = 0; c < 4; ++c) {   // elements 2c, 2c + 1: low-half bytes 2c, 2c + 1 of the 8
                v[j][2 * c] = (unpack_lo16(aw[c]) + yb[j][2 * c]) + dec((lw[c >> 1] >> (16 * (c & 1))) & 0xffu, unpack_lo16(hw[c]));
                v[j][2 * c + 1] = (unpack_hi16(aw[c]) + yb[j][2 * c + 1]) + dec((lw[c >> 1] >> (16 * (c & 1) + 8)) & 0xffu, unpack_hi16(hw[c]));
            }
        }
    }
    // pre-LN residual stream: the 16-bit high half of v and (rlo_row != nullptr) its low-half bytes, the same codec as the LayerNorm output's
    __device__ __forceinline__ void store_residual(const float (&v)[NS][8], int H, int lane, uint16_t* rb_row, uint8_t* rlo_row) const {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int i = lane * 8 + j * 512;
            if (i < H) {
                unsigned int ob[4], ol[2] = {0u, 0u};
#pragma unroll
                for (int c = 0; c < 4; ++c) ob[c] = pack_bf16x2(v[j][2 * c], v[j][2 * c + 1]);
                *reinterpret_cast<uint4*>(rb_row + i) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
                if (rlo_row) {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        ol[c >> 1] |= (lo_encode(v[j][2 * c], unpack_lo16(ob[c])) | (lo_encode(v[j][2 * c + 1], unpack_hi16(ob[c])) << 8)) << (16 * (c & 1));
                    *reinterpret_cast<uint2*>(rlo_row + i) = make_uint2(ol[0], ol[1]);
                }
            }
        }
    }
    // mean / variance over the wave, normalise, store the 16-bit row and (xlo_row != nullptr) its low-half bytes.  NTS: the low half stored non-temporally
    template <bool NTS>
    __device__ __forceinline__ void normalize_store(const float (&v)[NS][8], int H, float eps, int lane, uint16_t* xb_row, uint8_t* xlo_row) const {
        typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
        float s = 0.f;
        if constexpr (!RMS) {
#pragma unroll
            for (int j = 0; j < NS; ++j)
                if (lane * 8 + j * 512 < H)
#pragma unroll
                    for (int c = 0; c < 8; ++c) s += v[j][c];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        }
        const float mu = s / (float)H;      // RMS: 0, and x - 0 is x bit for bit
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NS; ++j)
            if (lane * 8 + j * 512 < H)
#pragma unroll
                for (int c = 0; c < 8; ++c) { const float dlt = v[j][c] - mu; q += dlt * dlt; }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m, 64);
        const float rstd = 1.0f / sqrtf(q / (float)H + eps);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int i = lane * 8 + j * 512;
            if (i < H) {
                float o[8];
                unsigned int ob[4], ol[4];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    if constexpr (RMS) o[c] = v[j][c] * rstd * gg[j][c];
                    else o[c] = (v[j][c] - mu) * rstd * gg[j][c] + bb[j][c];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) ob[c] = pack_bf16x2(o[2 * c], o[2 * c + 1]);
                *reinterpret_cast<uint4*>(xb_row + i) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
                if (xlo_row) {   // optional low half: one byte per element (lo_encode)
                    ol[0] = ol[1] = 0u;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        ol[c >> 1] |= (lo_encode(o[2 * c], unpack_lo16(ob[c])) | (lo_encode(o[2 * c + 1], unpack_hi16(ob[c])) << 8)) << (16 * (c & 1));
                    if constexpr (NTS) __builtin_nontemporal_store(u32x2_t{ol[0], ol[1]}, reinterpret_cast<u32x2_t*>(xlo_row + i));
                    else *reinterpret_cast<uint2*>(xlo_row + i) = make_uint2(ol[0], ol[1]);
                }
            }
        }
    }
};

// one wave per token row, grid-stride.  Same arithmetic per element as round 1's 8-byte k_ln; the row sums add the elements in the lane order of Ln16
// (rows stay independent of the batch).
// POL (cache policy of the streams; profiles/r04/tried_ln_policies.txt): bit 0 = y loaded non-temporally (dead after this kernel), bit 1 = the low half loaded
// non-temporally, bit 2 = the low half stored non-temporally (its next reader is the next LayerNorm, ~600 MiB of traffic later)
template <int NS, int POL = 0>
__global__ __launch_bounds__(256) void k_ln16(const uint16_t* __restrict__ y, const float* __restrict__ ybias, const int* __restrict__ Tp, const float* __restrict__ g,
                                              const float* __restrict__ bta, float eps, int H, const uint8_t* xlo_in, uint8_t* xlo, uint16_t* xb) {
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2_t;
    const int lane = threadIdx.x & 63;
    const int T = *Tp;
    Ln16<NS> ln;
    ln.load_params(g, bta, ybias, H, lane);
    const int64_t step = (int64_t)gridDim.x * 4;
    int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint4 a[NS], rh[NS]; uint2 rl[NS];
    auto load_row = [&](int64_t row) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int i = lane * 8 + j * 512;
            a[j] = rh[j] = make_uint4(0u, 0u, 0u, 0u); rl[j] = make_uint2(0x80808080u, 0x80808080u);      // byte 128 = a zero low half
            if (i < H && row < T) {
                a[j] = (POL & 1) ? __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(y + row * H + i))) : *reinterpret_cast<const uint4*>(y + row * H + i);
                rh[j] = *reinterpret_cast<const uint4*>(xb + row * H + i);
                if (xlo_in) rl[j] = (POL & 2) ? __builtin_bit_cast(uint2, __builtin_nontemporal_load(reinterpret_cast<const u32x2_t*>(xlo_in + row * H + i))) : *reinterpret_cast<const uint2*>(xlo_in + row * H + i);
            }
        }
    };
    load_row(t);
    for (; t < T; t += step) {
        float v[NS][8];
        ln.combine(a, rh, rl, v);
        load_row(t + step);                                   // next row's loads in flight while this one is reduced and stored
        ln.template normalize_store<(POL & 4) != 0>(v, H, eps, lane, xb + t * H, xlo ? xlo + t * H : nullptr);
    }
}

// Pre-LN stacks (ModernBert handles): the residual stream r (rb 16-bit high half + optional rlo low-half bytes) is kept apart from the normalised MFMA operand
// xb.  One launch does  r = (y + bias) + r_in;  store r (rb_out != nullptr: not behind the last layer);  xb = LayerNorm(r)  (+ its low half into xlo, the final
// LayerNorm only: pooling and kr_encoder_last_hidden read it).  r_in may be the embedding LayerNorm's output in xb itself (layer 0): a wave reads its whole row
// before it stores it.  Same row arithmetic as k_ln16 (Ln16).  RMS: T5 handles (Ln16<NS, true>); everything around the row arithmetic is the same.
template <int NS, int POL = 0, bool RMS = false>
__global__ __launch_bounds__(256) void k_ln16_pre(const uint16_t* __restrict__ y, const float* __restrict__ ybias, const int* __restrict__ Tp, const float* __restrict__ g,
                                                  const float* __restrict__ bta, float eps, int H, const uint16_t* rb_in, const uint8_t* rlo_in, uint16_t* rb_out,
                                                  uint8_t* rlo_out, uint8_t* xlo, uint16_t* xb) {
    const int lane = threadIdx.x & 63;
    const int T = *Tp;
    Ln16<NS, RMS> ln;
    ln.load_params(g, bta, ybias, H, lane);
    const int64_t step = (int64_t)gridDim.x * 4;
    int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    uint4 a[NS], rh[NS]; uint2 rl[NS];
    auto load_row = [&](int64_t row) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int i = lane * 8 + j * 512;
            a[j] = rh[j] = make_uint4(0u, 0u, 0u, 0u); rl[j] = make_uint2(0x80808080u, 0x80808080u);      // byte 128 = a zero low half
            if (i < H && row < T) {
                a[j] = (POL & 1) ? __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(y + row * H + i))) : *reinterpret_cast<const uint4*>(y + row * H + i);
                rh[j] = *reinterpret_cast<const uint4*>(rb_in + row * H + i);
                if (rlo_in) rl[j] = *reinterpret_cast<const uint2*>(rlo_in + row * H + i);
            }
        }
    };
    load_row(t);
    for (; t < T; t += step) {
        float v[NS][8];
        ln.template combine<true>(a, rh, rl, v);          // an overflowed residual element stays inf: the row becomes NaN and reaches the error word (k_pool)
        load_row(t + step);                                   // next row's loads in flight while this one is reduced and stored
        if (rb_out) ln.store_residual(v, H, lane, rb_out + t * H, rlo_out ? rlo_out + t * H : nullptr);
        ln.template normalize_store<false>(v, H, eps, lane, xb + t * H, xlo ? xlo + t * H : nullptr);
    }
}

// pooling + L2 normalisation: one block per sequence.  Mean pooling: wave w sums the tokens t = w, w+4, ... (8-byte loads of the (hi, lo)
// stream, 4 columns per lane and step), the four partial sums are combined in a fixed order (w = 0..3), so the result is deterministic.
// pooling + L2 normalisation: one block of 16 waves per sequence.  Masked mean: wave w sums tokens w, w + 16, ... (in that order), the 16 partial rows are added
// in wave order — a fixed order per sequence, whatever the batch.  (Rounds 1-4 used 4 waves: the kernel is bound by the VALU work of decoding and adding
// 262 k elements for a 256-token sequence on ONE block, 37 us — 2.7 % of a one-sequence forward; 16 waves: see profiles/r05.)
// KR_POOL_LAST (decoder handles): the sequence's last packed row in the CLS row's place.
// RAW (KR_POOL_CLASSIFY, the input of k_cls_head): the pooled row is written as it is, not divided by its norm; the norm is still formed, for the error word.
constexpr int POOL_WAVES = 16;
template <int NJ, bool RAW = false>     // 256-element steps that cover a row: H <= 256 NJ
__global__ __launch_bounds__(POOL_WAVES * 64) void k_pool(const uint16_t* __restrict__ xb, const uint8_t* __restrict__ xlo, const int* __restrict__ seq_off,
                                                         const int* __restrict__ seq_nk, const int* __restrict__ seq_cls, int H, int pool, float* __restrict__ out,
                                                         int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* part = reinterpret_cast<float*>(smem);                     // [POOL_WAVES][NJ * 256]
    float* red = part + POOL_WAVES * NJ * 256;                        // [POOL_WAVES]
    constexpr int HP = NJ * 256;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = seq_off[b];
    const int nk = seq_nk[b];
    float4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    // one row — the CLS row, or KR_POOL_LAST's last packed row (attended columns are packed in increasing order: the highest attended column; nk == 0: none,
    // and the row is NaN like the mean of nothing) — is wave 0's alone
    const bool one_row = pool == KR_POOL_CLS || pool == KR_POOL_LAST;
    const int row = pool == KR_POOL_CLS ? seq_cls[b] : nk - 1;
    const int t_begin = one_row ? (wave == 0 && row >= 0 ? row : 1 << 30) : wave;
    const int t_end = one_row ? (wave == 0 && row >= 0 ? row + 1 : 0) : nk;
    // PU of the wave's tokens per step: all their loads are issued before the first add; the adds keep the order t, t + 16, t + 32, ... so the result does
    // not depend on the unrolling
    constexpr int PU = NJ <= 4 ? 4 : 2;       // 16 waves per block: 128 registers per lane
    for (int t = t_begin; t < t_end; t += POOL_WAVES * PU) {
        ushort4 hi[PU][NJ]; unsigned int lo[PU][NJ];
#pragma unroll
        for (int u = 0; u < PU; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = lane * 4 + j * 256;
                if (i < H && t + POOL_WAVES * u < t_end) {
                    hi[u][j] = *reinterpret_cast<const ushort4*>(xb + (off + t + POOL_WAVES * u) * H + i);
                    lo[u][j] = xlo ? *reinterpret_cast<const unsigned int*>(xlo + (off + t + POOL_WAVES * u) * H + i) : 0x80808080u;
                }
            }
#pragma unroll
        for (int u = 0; u < PU; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = lane * 4 + j * 256;
                if (i < H && t + POOL_WAVES * u < t_end) {
                    acc[j].x += lo_decode_final(lo[u][j] & 0xffu, ET::to_f32(hi[u][j].x)); acc[j].y += lo_decode_final((lo[u][j] >> 8) & 0xffu, ET::to_f32(hi[u][j].y));
                    acc[j].z += lo_decode_final((lo[u][j] >> 16) & 0xffu, ET::to_f32(hi[u][j].z)); acc[j].w += lo_decode_final(lo[u][j] >> 24, ET::to_f32(hi[u][j].w));
                }
            }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = lane * 4 + j * 256;
        if (i < H) *reinterpret_cast<float4*>(&part[wave * HP + i]) = acc[j];
    }
    __syncthreads();
    constexpr int VJ = (NJ * 256 + POOL_WAVES * 64 - 1) / (POOL_WAVES * 64);      // elements per thread of the pooled row
    float v[VJ];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
        const int i = tid + j * POOL_WAVES * 64;
        v[j] = 0.f;
        if (i < H) {
            float s = part[i];
#pragma unroll
            for (int w = 1; w < POOL_WAVES; ++w) s += part[w * HP + i];
            v[j] = pool == KR_POOL_CLS ? s : pool == KR_POOL_LAST ? (nk > 0 ? s : NAN) : s / (float)nk;   // nk == 0 -> 0/0 = NaN like average_pool (encoders.py:56-58)
            ss += v[j] * v[j];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    float n2 = red[0];
#pragma unroll
    for (int w = 1; w < POOL_WAVES; ++w) n2 += red[w];
    const float nrm = sqrtf(n2);
    // A sequence WITH attended tokens whose pooled vector is not finite: an activation left the 16-bit operand range upstream (f16: |x| > 65504 becomes
    // inf, the next LayerNorm row NaN) or the weights hold NaN / Inf.  Recorded in the sticky error word (bit 1) and reported like an out-of-vocabulary
    // token id (kr_encoder_check: KR_ERANGE) instead of being returned as an embedding.  nk == 0 is the reference's own NaN (average_pool of nothing).
    if (tid == 0 && nk > 0 && !(nrm < INFINITY)) atomicOr(err, 2);
    const float den = fmaxf(nrm, 1e-12f);   // F.normalize eps; NaN norm stays NaN (fmaxf would drop it)
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
        const int i = tid + j * POOL_WAVES * 64;
        if constexpr (RAW) { if (i < H) out[(int64_t)b * H + i] = (nrm == nrm) ? v[j] : NAN; }
        else if (i < H) out[(int64_t)b * H + i] = (nrm == nrm) ? v[j] / den : NAN;
    }
}

// config.pool_tokens (k_pool_tok): what a KR_POOL_MEAN forward makes of the attended tokens where it is not their mean.  k_pool's walk over all tokens, without its
// one-row pools (KR_POOL_CLS / KR_POOL_LAST keep k_pool under every setting):  TOK = 1 the element-wise MAX — the accumulators start at -inf, wave w folds tokens
// w, w + 16, ..., the 16 partial rows are folded in wave order; a maximum does not depend on the order, and a NaN element is kept (pool_max);  TOK = 2
// sum / sqrt(n), the mean's sums in the mean's order, divided once.  A sequence without attended tokens is NaN under both, without an error bit, like the mean
// of nothing.  RAW, the norm and the error word: k_pool's.
__device__ __forceinline__ float pool_max(float acc, float v) { return (v > acc || v != v) ? v : acc; }      // a NaN arrives and stays (fmaxf would drop it)
template <int NJ, bool RAW, int TOK>     // 256-element steps that cover a row: H <= 256 NJ
__global__ __launch_bounds__(POOL_WAVES * 64) void k_pool_tok(const uint16_t* __restrict__ xb, const uint8_t* __restrict__ xlo, const int* __restrict__ seq_off,
                                                             const int* __restrict__ seq_nk, int H, float* __restrict__ out, int* __restrict__ err) {
    static_assert(TOK == 1 || TOK == 2, "the max or sum / sqrt(n); the mean is k_pool");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* part = reinterpret_cast<float*>(smem);                     // [POOL_WAVES][NJ * 256]
    float* red = part + POOL_WAVES * NJ * 256;                        // [POOL_WAVES]
    constexpr int HP = NJ * 256;
    constexpr float ACC0 = TOK == 1 ? -INFINITY : 0.f;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t off = seq_off[b];
    const int nk = seq_nk[b];
    auto fold = [](float a, float v) { if constexpr (TOK == 1) return pool_max(a, v); else return a + v; };
    float4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = make_float4(ACC0, ACC0, ACC0, ACC0);
    constexpr int PU = NJ <= 4 ? 4 : 2;       // tokens of the wave per step, all their loads issued before the first fold (k_pool)
    for (int t = wave; t < nk; t += POOL_WAVES * PU) {
        ushort4 hi[PU][NJ]; unsigned int lo[PU][NJ];
#pragma unroll
        for (int u = 0; u < PU; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = lane * 4 + j * 256;
                if (i < H && t + POOL_WAVES * u < nk) {
                    hi[u][j] = *reinterpret_cast<const ushort4*>(xb + (off + t + POOL_WAVES * u) * H + i);
                    lo[u][j] = xlo ? *reinterpret_cast<const unsigned int*>(xlo + (off + t + POOL_WAVES * u) * H + i) : 0x80808080u;
                }
            }
#pragma unroll
        for (int u = 0; u < PU; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = lane * 4 + j * 256;
                if (i < H && t + POOL_WAVES * u < nk) {
                    acc[j].x = fold(acc[j].x, lo_decode_final(lo[u][j] & 0xffu, ET::to_f32(hi[u][j].x))); acc[j].y = fold(acc[j].y, lo_decode_final((lo[u][j] >> 8) & 0xffu, ET::to_f32(hi[u][j].y)));
                    acc[j].z = fold(acc[j].z, lo_decode_final((lo[u][j] >> 16) & 0xffu, ET::to_f32(hi[u][j].z))); acc[j].w = fold(acc[j].w, lo_decode_final(lo[u][j] >> 24, ET::to_f32(hi[u][j].w)));
                }
            }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = lane * 4 + j * 256;
        if (i < H) *reinterpret_cast<float4*>(&part[wave * HP + i]) = acc[j];
    }
    __syncthreads();
    constexpr int VJ = (NJ * 256 + POOL_WAVES * 64 - 1) / (POOL_WAVES * 64);      // elements per thread of the pooled row
    float v[VJ];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
        const int i = tid + j * POOL_WAVES * 64;
        v[j] = 0.f;
        if (i < H) {
            float s = part[i];
#pragma unroll
            for (int w = 1; w < POOL_WAVES; ++w) s = fold(s, part[w * HP + i]);
            v[j] = nk <= 0 ? NAN : TOK == 1 ? s : s / sqrtf((float)nk);
            ss += v[j] * v[j];
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    float n2 = red[0];
#pragma unroll
    for (int w = 1; w < POOL_WAVES; ++w) n2 += red[w];
    const float nrm = sqrtf(n2);
    if (tid == 0 && nk > 0 && !(nrm < INFINITY)) atomicOr(err, 2);      // a non-finite row of a sequence with attended tokens: KR_ERANGE (k_pool)
    const float den = fmaxf(nrm, 1e-12f);   // F.normalize eps; NaN norm stays NaN (fmaxf would drop it)
#pragma unroll
    for (int j = 0; j < VJ; ++j) {
        const int i = tid + j * POOL_WAVES * 64;
        if constexpr (RAW) { if (i < H) out[(int64_t)b * H + i] = (nrm == nrm) ? v[j] : NAN; }
        else if (i < H) out[(int64_t)b * H + i] = (nrm == nrm) ? v[j] / den : NAN;
    }
}

// T5 handles: the embedding row IS the residual stream (no embedding norm, no positions, no token types): r = shared[id] -> rb / rlo, and
// xb = RMS(block 0's attention norm)(r).  One wave per token, the row arithmetic and the residual codec of k_ln16_pre.
template <int NS>
__global__ __launch_bounds__(256) void k_embed_rms(const int* __restrict__ tok_id, const int* __restrict__ Tp, const float* __restrict__ word, const float* __restrict__ g,
                                                   float eps, int H, uint16_t* __restrict__ rb, uint8_t* __restrict__ rlo, uint16_t* __restrict__ xb) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= *Tp) return;
    Ln16<NS, true> ln;
    const float* w = word + (int64_t)tok_id[t] * H;
    float v[NS][8];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int i = lane * 8 + j * 512;
#pragma unroll
        for (int c = 0; c < 8; ++c) { v[j][c] = 0.f; ln.gg[j][c] = 0.f; }
        if (i < H) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 a = *reinterpret_cast<const float4*>(w + i + 4 * h), b = *reinterpret_cast<const float4*>(g + i + 4 * h);
                v[j][4 * h] = a.x; v[j][4 * h + 1] = a.y; v[j][4 * h + 2] = a.z; v[j][4 * h + 3] = a.w;
                ln.gg[j][4 * h] = b.x; ln.gg[j][4 * h + 1] = b.y; ln.gg[j][4 * h + 2] = b.z; ln.gg[j][4 * h + 3] = b.w;
            }
        }
    }
    ln.store_residual(v, H, lane, rb + t * H, rlo ? rlo + t * H : nullptr);
    ln.template normalize_store<false>(v, H, eps, lane, xb + t * H, nullptr);
}

// The sentence-transformers Dense head behind the pooling (T5 handles with "dense.weight"): out[b, :] = normalize(W . p_b), W [P, H] fp32 without a bias,
// p = k_pool's normalised [B, H] rows (normalize(W . p / |p|) = normalize(W . p)), fp32 throughout, F.normalize's 1e-12 floor; a NaN pooled row stays NaN.
// One block of 4 waves per PD_SEQ sequences: the pooled rows sit in LDS, wave w computes features w, w + 4, ... (a lane owns 4 consecutive columns per
// 256-column step, the partial sums are added in a fixed order), so a W row is read once per PD_SEQ sequences and a row does not depend on its batch.
constexpr int PD_SEQ = 4;      // = the block's waves: wave s reduces sequence s's norm
__global__ __launch_bounds__(256) void k_pool_dense(const float* __restrict__ pooled, const float* __restrict__ W, int B, int H, int P, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* p = reinterpret_cast<float*>(smem);          // [PD_SEQ][H]
    float* y = p + PD_SEQ * H;                          // [PD_SEQ][P]
    float* red = y + PD_SEQ * P;                        // [PD_SEQ][4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * PD_SEQ;
    for (int i = tid; i < PD_SEQ * H; i += 256) {
        const int s = i / H;
        p[i] = b0 + s < B ? pooled[(int64_t)(b0 + s) * H + (i - s * H)] : 0.f;
    }
    __syncthreads();
    for (int f = wave; f < P; f += 4) {
        float acc[PD_SEQ];
#pragma unroll
        for (int s = 0; s < PD_SEQ; ++s) acc[s] = 0.f;
        for (int i = lane * 4; i < H; i += 256) {
            const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)f * H + i);
#pragma unroll
            for (int s = 0; s < PD_SEQ; ++s) {
                const float4 x = *reinterpret_cast<const float4*>(p + s * H + i);
                acc[s] += (w.x * x.x + w.y * x.y) + (w.z * x.z + w.w * x.w);
            }
        }
#pragma unroll
        for (int s = 0; s < PD_SEQ; ++s) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) acc[s] += __shfl_xor(acc[s], m, 64);
            if (lane == 0) y[s * P + f] = acc[s];
        }
    }
    __syncthreads();
    // |y_s|^2: wave w sums sequence w's features (lane-strided, then across the wave): one fixed order per row
    {
        float ss = 0.f;
        for (int f = lane; f < P; f += 64) ss += y[wave * P + f] * y[wave * P + f];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
        if (lane == 0) red[wave] = ss;
    }
    __syncthreads();
    for (int i = tid; i < PD_SEQ * P; i += 256) {
        const int s = i / P;
        if (b0 + s >= B) continue;
        const float nrm = sqrtf(red[s]);
        const float den = fmaxf(nrm, 1e-12f);           // NaN norm stays NaN (fmaxf would drop it)
        out[(int64_t)(b0 + s) * P + (i - s * P)] = (nrm == nrm) ? y[i] / den : NAN;
    }
}

// sentence-transformers' Dense module behind the pooling of any family (HEAD_ST_DENSE: "st_dense.weight" [P, H], "st_dense.bias" [P], zero unless loaded):
// out[b, :] = act(W . x_b + bias) of k_pool's RAW rows x [B, H] (k_pool<NJ, true> / k_pool_tok<NJ, true, TOK>), act = tanhf or the identity, then divided by its
// norm (F.normalize's 1e-12 floor) unless the handle has config.normalize_output = 0; fp32 throughout.  k_pool_dense's layout and summation order: PD_SEQ
// sequences per block with their rows in LDS, wave w computes features w, w + 4, ... from ONE read of the W row, a lane's partial sums are added in column
// order and folded by a shuffle butterfly — a row does not depend on its batch.  A NaN pooled row stays NaN; a non-finite output of a sequence WITH attended
// tokens sets bit 1 of the error word (the norm is formed either way).
__global__ __launch_bounds__(256) void k_st_dense(const float* __restrict__ pooled, const float* __restrict__ W, const float* __restrict__ bias, int B, int H, int P, int act_tanh,
                                                  int normalize, const int* __restrict__ seq_nk, float* __restrict__ out, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* p = reinterpret_cast<float*>(smem);          // [PD_SEQ][H]
    float* y = p + PD_SEQ * H;                          // [PD_SEQ][P]
    float* red = y + PD_SEQ * P;                        // [PD_SEQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * PD_SEQ;
    for (int i = tid; i < PD_SEQ * H; i += 256) {
        const int s = i / H;
        p[i] = b0 + s < B ? pooled[(int64_t)(b0 + s) * H + (i - s * H)] : 0.f;
    }
    __syncthreads();
    for (int f = wave; f < P; f += 4) {
        float acc[PD_SEQ];
#pragma unroll
        for (int s = 0; s < PD_SEQ; ++s) acc[s] = 0.f;
        for (int i = lane * 4; i < H; i += 256) {
            const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)f * H + i);
#pragma unroll
            for (int s = 0; s < PD_SEQ; ++s) {
                const float4 x = *reinterpret_cast<const float4*>(p + s * H + i);
                acc[s] += (w.x * x.x + w.y * x.y) + (w.z * x.z + w.w * x.w);
            }
        }
        const float bf = bias[f];
#pragma unroll
        for (int s = 0; s < PD_SEQ; ++s) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) acc[s] += __shfl_xor(acc[s], m, 64);
            if (lane == 0) y[s * P + f] = act_tanh ? tanhf(acc[s] + bf) : acc[s] + bf;
        }
    }
    __syncthreads();
    // |y_s|^2: wave w sums sequence w's features (lane-strided, then across the wave): one fixed order per row
    {
        float ss = 0.f;
        for (int f = lane; f < P; f += 64) ss += y[wave * P + f] * y[wave * P + f];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
        if (lane == 0) {
            red[wave] = ss;
            if (b0 + wave < B && seq_nk[b0 + wave] > 0 && !(sqrtf(ss) < INFINITY)) atomicOr(err, 2);
        }
    }
    __syncthreads();
    for (int i = tid; i < PD_SEQ * P; i += 256) {
        const int s = i / P;
        if (b0 + s >= B) continue;
        const float nrm = sqrtf(red[s]);
        const float den = fmaxf(nrm, 1e-12f);           // NaN norm stays NaN (fmaxf would drop it)
        out[(int64_t)(b0 + s) * P + (i - s * P)] = !normalize ? y[i] : (nrm == nrm) ? y[i] / den : NAN;
    }
}

// The sequence-classification head behind the raw CLS row (KR_POOL_CLASSIFY; RobertaClassificationHead, and BertForSequenceClassification's pooler + classifier
// under the same names): logits[b, :] = Wo . tanh(Wd . x_b + bd) + bo, x = k_pool<NJ, true>'s [B, H] rows, Wd [H, H], Wo [L, H], fp32 throughout.
// One block of CH_WAVES waves per CH_SEQ sequences, their rows in LDS.  Stage 1: a wave takes CH_ROWS rows of Wd at a time and computes those features of
// all CH_SEQ sequences from ONE read of the rows — a lane owns 4 consecutive columns per 256-column step and adds its products with fp32 FMAs in column
// order, the 64 lane sums are folded by a shuffle butterfly in a fixed order — and stores t = tanhf(sum + bd) to LDS.  Stage 2: the same over Wo and t, + bo,
// to out [B, L].  Every slot of the group runs the same instructions on its own row and a feature is summed by one wave whatever its row's place in the
// wave's batch, so a sequence's logits depend neither on its slot nor on the batch around it.
// The weights stay fp32 (4 MiB at H = 1024, re-read from L2 by every group): 2 H^2 flops per sequence are not a GEMM worth the MFMA units at a few hundred
// sequences, and fp32 keeps the head inside an a-priori bound of (H + 2) 2^-24 per sum (tests/test_gpu_reranker.py).  What bounds the kernel is the latency of
// the weight rows — one block streams all of Wd — hence 16 waves with CH_ROWS x NJ row loads each in flight before the first FMA (4 waves with one row each:
// 0.6 ms at any batch size; profiles/reranker/measurements.txt).
//
// GLN (ModernBert handles; ModernBertForSequenceClassification's head.dense -> gelu -> head.norm -> classifier): logits[b, :] = Wo . LayerNorm(erf_gelu(Wd . x_b + bd)) + bo.
// Stage 1 stores the exact erf-GELU where the tanh stood; then wave s < CH_SEQ takes the H values of slot s in LDS: lane l sums columns l, l + 64, ... in
// that order and a shuffle butterfly folds the 64 sums — first the mean, then the variance of the values centred on it (two passes, fp32), then
// t = (t - mean) / sqrt(var + eps) * g + beta in place — a fixed order per sequence whatever its slot.  Stage 2 is the same code.  This variant also
// guards its result: a non-finite logit of a sequence with attended tokens (seq_nk > 0) sets bit 1 of the error word, like a non-finite embedding (k_pool).
//
// GELU without GLN (DeBERTa handles; DebertaV2ForSequenceClassification's ContextPooler + classifier under HEAD_CLS's names): logits[b, :] =
// Wo . erf_gelu(Wd . x_b + bd) + bo — the erf-GELU of the GLN variant where the tanh stands, no norm, and the same guard of the result.
constexpr int CH_SEQ = 4, CH_WAVES = 16;
template <int NJ, bool GLN = false, bool GELU = GLN>     // 256-column steps that cover a row: H <= 256 NJ
__global__ __launch_bounds__(CH_WAVES * 64) void k_cls_head(const float* __restrict__ pooled, const float* __restrict__ Wd, const float* __restrict__ bd,
                                                           const float* __restrict__ Wo, const float* __restrict__ bo, int B, int H, int L,
                                                           float* __restrict__ out, const float* __restrict__ ng = nullptr, const float* __restrict__ nb = nullptr,
                                                           float eps = 0.f, const int* __restrict__ seq_nk = nullptr, int* __restrict__ err = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* x = reinterpret_cast<float*>(smem);          // [CH_SEQ][H]
    float* t = x + CH_SEQ * H;                          // [CH_SEQ][H]
    constexpr int CH_ROWS = NJ <= 2 ? 4 : 2;            // weight rows per wave and step: CH_ROWS * NJ float4 per lane (16 waves per block: 128 registers per lane)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * CH_SEQ;
    for (int i = tid; i < CH_SEQ * H; i += CH_WAVES * 64) {
        const int s = i / H;
        x[i] = b0 + s < B ? pooled[(int64_t)(b0 + s) * H + (i - s * H)] : 0.f;
    }
    __syncthreads();
    // y[f][s] = W[f, :] . v[s, :] for every row f < rows of W and the CH_SEQ rows of v (LDS); lane 0 of the wave that owns f hands the sums to `store`
    auto rows_dot = [&](const float* __restrict__ W, int rows, const float* v, auto&& store) {
        for (int f0 = wave * CH_ROWS; f0 < rows; f0 += CH_WAVES * CH_ROWS) {
            float4 w[CH_ROWS][NJ];
#pragma unroll
            for (int r = 0; r < CH_ROWS; ++r)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int i = lane * 4 + j * 256;
                    w[r][j] = (i < H && f0 + r < rows) ? *reinterpret_cast<const float4*>(W + (int64_t)(f0 + r) * H + i) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            float acc[CH_ROWS][CH_SEQ];
#pragma unroll
            for (int r = 0; r < CH_ROWS; ++r)
#pragma unroll
                for (int s = 0; s < CH_SEQ; ++s) acc[r][s] = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = lane * 4 + j * 256;
                if (i < H) {
#pragma unroll
                    for (int s = 0; s < CH_SEQ; ++s) {
                        const float4 a = *reinterpret_cast<const float4*>(v + s * H + i);
#pragma unroll
                        for (int r = 0; r < CH_ROWS; ++r)
                            acc[r][s] = fmaf(w[r][j].w, a.w, fmaf(w[r][j].z, a.z, fmaf(w[r][j].y, a.y, fmaf(w[r][j].x, a.x, acc[r][s]))));
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < CH_ROWS; ++r) {
#pragma unroll
                for (int s = 0; s < CH_SEQ; ++s)
#pragma unroll
                    for (int m = 32; m >= 1; m >>= 1) acc[r][s] += __shfl_xor(acc[r][s], m, 64);
                if (lane == 0 && f0 + r < rows) store(f0 + r, acc[r]);
            }
        }
    };
    rows_dot(Wd, H, x, [&](int f, const float (&y)[CH_SEQ]) {
        const float b = bd[f];
#pragma unroll
        for (int s = 0; s < CH_SEQ; ++s) {
            if constexpr (GELU) { const float a = y[s] + b; t[s * H + f] = 0.5f * a * (1.f + erff(a * 0.70710678118654752f)); }
            else t[s * H + f] = tanhf(y[s] + b);
        }
    });
    __syncthreads();
    if constexpr (GLN) {
        if (wave < CH_SEQ) {
            float* ts = t + wave * H;
            float sum = 0.f;
            for (int i = lane; i < H; i += 64) sum += ts[i];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
            const float mean = sum / (float)H;
            float sq = 0.f;
            for (int i = lane; i < H; i += 64) { const float d = ts[i] - mean; sq = fmaf(d, d, sq); }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) sq += __shfl_xor(sq, m, 64);
            const float rstd = 1.f / sqrtf(sq / (float)H + eps);
            for (int i = lane; i < H; i += 64) ts[i] = (ts[i] - mean) * rstd * ng[i] + nb[i];
        }
        __syncthreads();
    }
    rows_dot(Wo, L, t, [&](int l, const float (&y)[CH_SEQ]) {
        const float b = bo[l];
#pragma unroll
        for (int s = 0; s < CH_SEQ; ++s)
            if (b0 + s < B) {
                const float v = y[s] + b;
                out[(int64_t)(b0 + s) * L + l] = v;
                if constexpr (GELU) { if (!(fabsf(v) < INFINITY) && seq_nk[b0 + s] > 0) atomicOr(err, 2); }
            }
    });
}

// The score head of a decoder cross-encoder (KR_POOL_CLASSIFY on a decoder handle with "score.weight"; the Linear without a bias behind the last token in
// Qwen2 / Llama / MistralForSequenceClassification): logits[b, l] = W[l, :] . x_b, x = k_pool<NJ, true>'s [B, H] rows under KR_POOL_LAST's row rule, W [L, H],
// fp32 throughout.  One stage — no Wd, no activation, no bias — so there is nothing to keep in LDS: one wave per (sequence, group of SH_LABELS labels) reads its
// row of x once and SH_LABELS rows of W, a lane owns 4 consecutive columns per 256-column step and adds its products with fp32 FMAs in column order, and a
// shuffle butterfly folds the 64 lane sums in a fixed order.  A logit is summed by one wave from its own sequence's row alone, so it depends neither on the
// batch around it nor on the grid; its sum has H / 64 + 6 additions in a chain, inside the a-priori bound gamma_H sum |w_i x_i| (tests/test_gpu_decoder_reranker.py).
// A non-finite logit of a sequence with attended tokens (seq_nk > 0) sets bit 1 of the error word, as k_cls_head's guarded variants do; the NaN row of an
// all-masked sequence passes through.
constexpr int SH_LABELS = 4, SH_WAVES = 4;
__global__ __launch_bounds__(SH_WAVES * 64) void k_score_head(const float* __restrict__ pooled, const float* __restrict__ W, int B, int H, int L, float* __restrict__ out,
                                                             const int* __restrict__ seq_nk, int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int groups = (L + SH_LABELS - 1) / SH_LABELS;
    const int64_t wv = (int64_t)blockIdx.x * SH_WAVES + (threadIdx.x >> 6);
    if (wv >= (int64_t)B * groups) return;
    const int b = (int)(wv / groups), l0 = (int)(wv % groups) * SH_LABELS;
    const float* x = pooled + (int64_t)b * H;
    float acc[SH_LABELS];
#pragma unroll
    for (int r = 0; r < SH_LABELS; ++r) acc[r] = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const float4 a = *reinterpret_cast<const float4*>(x + i);
#pragma unroll
        for (int r = 0; r < SH_LABELS; ++r)
            if (l0 + r < L) {
                const float4 w = *reinterpret_cast<const float4*>(W + (int64_t)(l0 + r) * H + i);
                acc[r] = fmaf(w.w, a.w, fmaf(w.z, a.z, fmaf(w.y, a.y, fmaf(w.x, a.x, acc[r]))));
            }
    }
#pragma unroll
    for (int r = 0; r < SH_LABELS; ++r) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc[r] += __shfl_xor(acc[r], m, 64);
        if (lane == 0 && l0 + r < L) {
            out[(int64_t)b * L + l0 + r] = acc[r];
            if (!(fabsf(acc[r]) < INFINITY) && seq_nk[b] > 0) atomicOr(err, 2);
        }
    }
}

// bge-m3's token-level heads (KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT).  Both blocks are laid out by the columns of the padded [B, S] input, so the kernels
// run one wave per SLOT (b, s) and find their packed row through slot_row: k_m3_slots writes off[b] + (rank of column s among the attended columns of its
// row) — the order fill_seq packs them in — or -1 for a masked column.  The query-only row of a masked column 0 (CLS pooling) sits behind the attended ones
// and has no slot.  No slot is written twice and none is skipped: no atomics, no zero-fill pass.
__global__ __launch_bounds__(64) void k_m3_slots(const int64_t* __restrict__ mask, const int* __restrict__ seq_off, int S, int* __restrict__ slot_row) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t* m = mask + (int64_t)b * S;
    const int off = seq_off[b];
    int run = 0;
    for (int base = 0; base < S; base += 64) {
        const int p = base + lane;
        const bool v = p < S && m[p] != 0;
        const unsigned long long bal = __ballot(v);
        if (p < S) slot_row[(int64_t)b * S + p] = v ? off + run + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
        run += __popcll(bal);
    }
}

// colbert rows: y [T, P] = colbert_linear.weight . x as the projection loops stored it (EPI_DENSE: 16-bit, no bias) -> out[b, s, :] = (y + bias) / max(|y + bias|, 1e-12)
// in fp32, or P times +0.0 for a masked slot.  One wave per slot, lane l owns columns l, l + 64, ...: 4-byte stores (the block starts wherever the caller's
// dense and sparse blocks end, so nothing wider is aligned), 256 contiguous bytes per store instruction.  The row is read twice (norm, then values: the second
// pass hits the cache) instead of being held in P / 64 registers; squares are added in column order per lane, then by a shuffle butterfly: one order per row.
__global__ __launch_bounds__(256) void k_m3_rows(const uint16_t* __restrict__ y, const float* __restrict__ bias, const int* __restrict__ slot_row, int64_t slots, int P,
                                                 float* __restrict__ out, int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= slots) return;
    float* o = out + slot * P;
    const int r = slot_row[slot];
    if (r < 0) {
        for (int c = lane; c < P; c += 64) o[c] = 0.f;
        return;
    }
    const uint16_t* yr = y + (int64_t)r * P;
    float ss = 0.f;
    for (int c = lane; c < P; c += 64) {
        const float v = ET::to_f32(yr[c]) + bias[c];
        ss += v * v;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    const float nrm = sqrtf(ss);
    if (lane == 0 && !(nrm < INFINITY)) atomicOr(err, 2);      // an attended token's vector is not finite: KR_ERANGE, like a non-finite embedding (k_pool)
    const float den = fmaxf(nrm, 1e-12f);                       // F.normalize's floor; a NaN norm stays NaN below
    for (int c = lane; c < P; c += 64) {
        const float v = ET::to_f32(yr[c]) + bias[c];
        o[c] = (nrm == nrm) ? v / den : NAN;
    }
}

// sparse weights: out[b, s] = max(0, w . x + bias) over the decoded final row x (the (hi, lo) stream, read as k_pool reads it), +0.0 for a masked slot.  One
// wave per slot: a lane owns 4 consecutive columns per 256-column step and adds its products with fp32 FMAs in column order, the 64 lane sums are folded by a
// shuffle butterfly — one order per token, whatever the batch.
__global__ __launch_bounds__(256) void k_m3_sparse(const uint16_t* __restrict__ xb, const uint8_t* __restrict__ xlo, const float* __restrict__ w, const float* __restrict__ bias,
                                                   const int* __restrict__ slot_row, int64_t slots, int H, float* __restrict__ out, int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= slots) return;
    const int r = slot_row[slot];
    if (r < 0) { if (lane == 0) out[slot] = 0.f; return; }
    float acc = 0.f;
    for (int i = lane * 4; i < H; i += 256) {
        const ushort4 hi = *reinterpret_cast<const ushort4*>(xb + (int64_t)r * H + i);
        const unsigned int lo = *reinterpret_cast<const unsigned int*>(xlo + (int64_t)r * H + i);
        const float4 ww = *reinterpret_cast<const float4*>(w + i);
        acc = fmaf(ww.x, lo_decode_final(lo & 0xffu, ET::to_f32(hi.x)), acc);
        acc = fmaf(ww.y, lo_decode_final((lo >> 8) & 0xffu, ET::to_f32(hi.y)), acc);
        acc = fmaf(ww.z, lo_decode_final((lo >> 16) & 0xffu, ET::to_f32(hi.z)), acc);
        acc = fmaf(ww.w, lo_decode_final(lo >> 24, ET::to_f32(hi.w)), acc);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    const float v = acc + bias[0];
    if (lane == 0) {
        if (!(fabsf(v) < INFINITY)) atomicOr(err, 2);          // NaN / Inf weight of an attended token: KR_ERANGE
        out[slot] = (v != v) ? v : (v > 0.f ? v : 0.f);
    }
}

// SPLADE's MLM head (KR_POOL_SPLADE).  k_ln16_head: the transform LayerNorm, t = LayerNorm(y) of rows that already hold gelu(Wt x + bt) (EPI_GELU), no
// residual: Ln16's row arithmetic with a zero residual ((y + 0) + 0 is y bit for bit; `zero` = H zeros in the place of the projection's bias), 16-bit out for
// the decoder's MFMAs.  A row OF A SEQUENCE (row_seq >= 0: the alignment rows between two sequences hold whatever the attention left there, nobody reads them)
// with a non-finite element raises the error word here: behind the decoder the max over a sequence would drop a lone NaN.
template <int NS>
__global__ __launch_bounds__(256) void k_ln16_head(const uint16_t* __restrict__ y, const float* __restrict__ zero, const int* __restrict__ Tp, const float* __restrict__ g,
                                                   const float* __restrict__ bta, float eps, int H, const int* __restrict__ row_seq, uint16_t* __restrict__ out,
                                                   int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int T = *Tp;
    Ln16<NS> ln;
    ln.load_params(g, bta, zero, H, lane);
    const int64_t step = (int64_t)gridDim.x * 4;
    for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < T; t += step) {
        uint4 a[NS], rh[NS]; uint2 rl[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int i = lane * 8 + j * 512;
            a[j] = rh[j] = make_uint4(0u, 0u, 0u, 0u); rl[j] = make_uint2(0x80808080u, 0x80808080u);      // byte 128 = a zero low half
            if (i < H) a[j] = *reinterpret_cast<const uint4*>(y + t * H + i);
        }
        float v[NS][8];
        ln.combine(a, rh, rl, v);
        float chk = 0.f;
#pragma unroll
        for (int j = 0; j < NS; ++j)
#pragma unroll
            for (int c = 0; c < 8; ++c) chk += v[j][c] * 0.f;      // 0 for finite elements, NaN for NaN / Inf
        if (__ballot(chk != chk) != 0ull && lane == 0 && row_seq[t] >= 0) atomicOr(err, 2);
        ln.template normalize_store<false>(v, H, eps, lane, out + t * H, nullptr);
    }
}
// row_seq[row] = b for the nk[b] attended rows of sequence b (the buffer was filled with -1: alignment rows and everything behind the packed rows stay -1)
__global__ __launch_bounds__(64) void k_splade_rowseq(const int* __restrict__ seq_off, const int* __restrict__ seq_nk, int* __restrict__ row_seq) {
    const int b = blockIdx.x, off = seq_off[b], n = seq_nk[b];
    for (int i = threadIdx.x; i < n; i += 64) row_seq[off + i] = b;
}
// in place over the [B, V] reduction buffer: the bit pattern of m = max(0, bias + max over the rows) -> w = log1p(m); a sequence without attended rows kept its
// zeros: +0.0.  A non-finite m (NaN / Inf weights) is passed on and raises the error word: KR_ERANGE, like a non-finite embedding (k_pool)
__global__ __launch_bounds__(256) void k_splade_finish(float* __restrict__ w, int64_t n, int* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float m = w[i];
    if (!(m < INFINITY)) { atomicOr(err, 2); return; }
    if (m != 0.f) w[i] = log1pf(m);
}

// CLS shortcut: row seq_off[b] + seq_cls[b] of ctx / the residual stream (hi, lo) -> row b of the compact buffers; also the compact "sequence" tables
// (one token per sequence) and the row count for the B-row kernels that follow.  last_row != 0 (the last-row shortcut of a decoder handle's KR_POOL_CLASSIFY):
// the sequence's last packed row seq_off[b] + seq_nk[b] - 1 in the CLS row's place — k_pool's KR_POOL_LAST row; an all-masked sequence has none and gathers
// its first row slot (inside the workspace, whatever it holds: c_nk == 0 makes the pooled row NaN)
__global__ __launch_bounds__(256) void k_gather_cls(const uint16_t* __restrict__ ctx, const uint16_t* __restrict__ xb, const uint8_t* __restrict__ xlo,
                                                    const int* __restrict__ seq_off, const int* __restrict__ seq_cls, const int* __restrict__ seq_nk, int H, uint16_t* __restrict__ c_ctx,
                                                    uint16_t* __restrict__ c_xb, uint8_t* __restrict__ c_xlo, int* __restrict__ c_off, int* __restrict__ c_nk,
                                                    int* __restrict__ c_cls, int* __restrict__ d_B, int last_row, int Dq) {
    const int b = blockIdx.x;
    const int64_t src = (int64_t)seq_off[b] + (last_row ? (seq_nk[b] > 0 ? seq_nk[b] - 1 : 0) : seq_cls[b]);
    // the context rows are Dq = heads d_h wide (H unless the handle has a head width of its own), the residual stream H
    for (int i = threadIdx.x * 8; i < Dq; i += 256 * 8) *reinterpret_cast<uint4*>(c_ctx + (int64_t)b * Dq + i) = *reinterpret_cast<const uint4*>(ctx + src * Dq + i);
    for (int i = threadIdx.x * 8; i < H; i += 256 * 8) {
        *reinterpret_cast<uint4*>(c_xb + (int64_t)b * H + i) = *reinterpret_cast<const uint4*>(xb + src * H + i);
        if (xlo) *reinterpret_cast<uint2*>(c_xlo + (int64_t)b * H + i) = *reinterpret_cast<const uint2*>(xlo + src * H + i);
    }
    if (threadIdx.x == 0) {
        c_off[b] = b; c_nk[b] = seq_nk[b] > 0 ? 1 : 0; c_cls[b] = 0;   // c_nk == 0: an all-masked sequence (its NaN is the reference's own, not an overflow: k_pool)
        if (b == 0) *d_B = (int)gridDim.x;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize), the one place that sets it: function attributes belong to the device's code-object instance, so the
// largest `lds` set so far is remembered per (kernel, device) and the attribute is raised only by a launch that needs more.  Safe against concurrent first
// launches from several host threads (a query encoder and a corpus encoder on one device: ADVICE r04) and with the outcome cached, so that a failing
// attribute is reported by every launch
static int set_lds_once(const void* kern, int lds, int device) {
    struct Ent { const void* k; int dev; int lds; hipError_t rc; };
    static std::mutex mu;
    static std::vector<Ent> done;
    std::lock_guard<std::mutex> lock(mu);
    Ent* ent = nullptr;
    for (Ent& x : done)
        if (x.k == kern && x.dev == device) { ent = &x; break; }
    if (ent && ent->rc != hipSuccess) return fail(KR_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(ent->rc));
    if (ent && lds <= ent->lds) return 0;
    const hipError_t rc = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (ent) { ent->lds = lds; ent->rc = rc; } else done.push_back({kern, device, lds, rc});
    if (rc != hipSuccess) return fail(KR_EHIP, "hipFuncSetAttribute failed: %s", hipGetErrorString(rc));
    return 0;
}

// Row width as a compile-time constant, f(std::integral_constant<int, N>{}) in the manner of with_epilogue: the LayerNorm family of kernels covers a row in
// NS steps of 512 elements (the pool and head family in NJ steps of 256: with_pool_width, encoder.hip)
template <int N> using width_c = std::integral_constant<int, N>;
template <class F> static auto with_ln_width(int H, F&& f) { return H <= 512 ? f(width_c<1>{}) : H <= 1024 ? f(width_c<2>{}) : f(width_c<4>{}); }

// The launches of the row kernels above: which instantiation a width or a head width gets, its cache policy and its block size, as plain functions of
// pointers, sizes, a grid and a stream — a forward (encoder.hip) and the kernels' own tests (tests/capi/rows_probe.hip) go through the same lines.  The grids
// of a forward: one wave per row (row_grid) for the embedding kernels; the grid-stride LayerNorms at most 8 blocks per CU (ln_grid; profiles/r04/
// tried_ln_policies.txt); the q / k norm one DH / 8-lane group per (row, head) unit (qk_norm_grid).
static unsigned row_grid(int64_t rows) { return (unsigned)((rows + 3) / 4); }
static unsigned ln_grid(int64_t rows, int num_cu) { return std::min(row_grid(rows), (unsigned)num_cu * 8u); }
static unsigned qk_norm_grid(int64_t rows, int heads, int kv_heads, int head_w) {
    const int64_t units = rows * (heads + kv_heads), per_block = 4 * (64 / (head_w / 8));
    return (unsigned)((units + per_block - 1) / per_block);
}
static void launch_rot_pos(const int* seq_off, const int* seq_nq, int align, const int* tok_pos, int* rpos, unsigned B, hipStream_t st) {
    hipLaunchKernelGGL(k_rot_pos, dim3(B), dim3(64), 0, st, seq_off, seq_nq, align, tok_pos, rpos);
}
static void launch_embed_rms(const int* tok_id, const int* Tp, const float* word, const float* g, float eps, int H, uint16_t* rb, uint8_t* rlo, uint16_t* xb, unsigned grid,
                             hipStream_t st) {
    const auto embed_kernel = with_ln_width(H, [](auto ns) { return &k_embed_rms<decltype(ns)::value>; });
    hipLaunchKernelGGL(embed_kernel, dim3(grid), dim3(256), 0, st, tok_id, Tp, word, g, eps, H, rb, rlo, xb);
}
static void launch_embed_ln(const int* tok_id, const int* tok_pos, const int* tok_type, const int* Tp, const float* word, const float* pos, const float* type, const float* g,
                            const float* bta, float eps, int H, uint8_t* xlo, uint16_t* xb, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL(k_embed_ln, dim3(grid), dim3(256), 0, st, tok_id, tok_pos, tok_type, Tp, word, pos, type, g, bta, eps, H, xlo, xb);
}
// LayerNorm streams: y (dead after the kernel) and the low half (next read by the next LayerNorm, ~600 MiB of traffic later) are loaded / stored
// non-temporally — they do not displace the 16-bit stream the next GEMM reads: -1.3 % forward at 1024 x 128 tokens, -0.1...0.5 % at 1000 x 32; 8 blocks
// per CU instead of 4: -0.25 % (profiles/r04/tried_ln_policies.txt; outputs bit-identical)
static void launch_ln_post(const uint16_t* y, const float* bias, const int* Tp, const float* g, const float* b, float eps, int H, const uint8_t* xlo_in, uint8_t* xlo,
                           uint16_t* xb, unsigned grid, hipStream_t st) {
    const auto ln_kernel = with_ln_width(H, [](auto ns) { return &k_ln16<decltype(ns)::value, 7>; });
    hipLaunchKernelGGL(ln_kernel, dim3(grid), dim3(256), 0, st, y, bias, Tp, g, b, eps, H, xlo_in, xlo, xb);
}
static void launch_ln_pre(bool rms, const uint16_t* y, const float* bias, const int* Tp, const float* g, const float* b, float eps, int H, const uint16_t* rb_in,
                          const uint8_t* rlo_in, uint16_t* rb_out, uint8_t* rlo_out, uint8_t* xlo, uint16_t* xb, unsigned grid, hipStream_t st) {
    const auto ln_tail_kernel = rms ? with_ln_width(H, [](auto ns) { return &k_ln16_pre<decltype(ns)::value, 1, true>; })
                                    : with_ln_width(H, [](auto ns) { return &k_ln16_pre<decltype(ns)::value, 1>; });
    hipLaunchKernelGGL(ln_tail_kernel, dim3(grid), dim3(256), 0, st, y, bias, Tp, g, b, eps, H, rb_in, rlo_in, rb_out, rlo_out, xlo, xb);
}
static void launch_ln_head(const uint16_t* y, const float* zero, const int* Tp, const float* g, const float* b, float eps, int H, const int* row_seq, uint16_t* out, int* err,
                           unsigned grid, hipStream_t st) {
    const auto head_ln = with_ln_width(H, [](auto ns) { return &k_ln16_head<decltype(ns)::value>; });
    hipLaunchKernelGGL(head_ln, dim3(grid), dim3(256), 0, st, y, zero, Tp, g, b, eps, H, row_seq, out, err);
}
static void launch_qk_norm_rope(int head_w, uint16_t* q, uint16_t* k, const int* Tp, int heads, int kv_heads, const float* gq, const float* gk, float eps_q, float eps_k,
                                const float* rot_cos, const float* rot_sin, const int* tpos, int max_pos, unsigned grid, hipStream_t st) {
    const auto norm_kernel = head_w == 128 ? &k_qk_norm_rope<128> : head_w == 64 ? &k_qk_norm_rope<64> : &k_qk_norm_rope<32>;
    hipLaunchKernelGGL(norm_kernel, dim3(grid), dim3(256), 0, st, q, k, Tp, heads, kv_heads, gq, gk, eps_q, eps_k, rot_cos, rot_sin, tpos, max_pos);
}
static void launch_gather_cls(const uint16_t* ctx, const uint16_t* xb, const uint8_t* xlo, const int* seq_off, const int* seq_cls, const int* seq_nk, int H, uint16_t* c_ctx,
                              uint16_t* c_xb, uint8_t* c_xlo, int* c_off, int* c_nk, int* c_cls, int* d_B, int last_row, int Dq, unsigned B, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_cls, dim3(B), dim3(256), 0, st, ctx, xb, xlo, seq_off, seq_cls, seq_nk, H, c_ctx, c_xb, c_xlo, c_off, c_nk, c_cls, d_B, last_row, Dq);
}

}  // namespace KR_ENC_NS
}  // namespace kr
