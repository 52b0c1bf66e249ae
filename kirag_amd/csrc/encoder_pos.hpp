// Sentence encoder, device code of DeBERTa's position terms (k_pos_table, k_pos_scores).  Part of encoder.hip (see its header).
#pragma once
#include "encoder_rows.hpp"

namespace kr {
namespace KR_ENC_NS {

// ---------------------------------------------------------------------------------------------------------
// Disentangled attention (DebertaV2Model): s(i, j) = (q_i . k_j + q_i . PK[p] + k_j . PQ[p]) / sqrt(3 d_h), p = deberta_bucket(col_i - col_j), with
// PQ = query_proj(R), PK = key_proj(R) of the layer and R the (normalised) position table [2 Bk, H].  PQ and PK depend on the weights only:
//   k_pos_table   at finalize, per layer and projection: out[head][p][d] = (W . R[p] + b) of the head's d_h features, fp32 sums in column order, stored in the
//                 handle's 16-bit operand type with TP = 2 Bk rounded up to 32 rows per head (the rows behind 2 Bk are zero)
//   k_pos_scores  per forward and layer, behind the QKV projection: C2P[t][h][w] = q_t . PK[h][p0 + w] and P2C[t][h][w] = k_t . PQ[h][p0 + w] for every packed
//                 row t and the W buckets the batch's widest possible column difference reaches, from the 16-bit q / k rows the attention reads (q carries
//                 log2(e) / sqrt(3 d_h), and so does PQ), fp32 out [t][h][C2P | P2C][W] — what the AM_DISENT instantiation of k_attn_lds gathers its bias
//                 tiles from (encoder_attn.hpp)
// k_pos_scores is a tile kernel of its own: K = d_h (two or four k-steps of the 32x32x16 MFMA), so the H-deep loops of encoder_proj.hpp have nothing to
// pipeline.  One block = 128 packed rows (a 32-row tile per wave, its q and k fragments in registers for the whole block) x one head; the head's tables pass
// through LDS 64 buckets at a time (rows padded by 16 B: the 16-B fragment reads of 32 consecutive rows spread over the banks), every wave multiplies its tile
// with both 32-bucket halves of both tables.  Token rows on the A side, buckets on the B side: a lane holds one bucket of 16 rows, so each store instruction
// writes 128 contiguous bytes of a row.  An element is one dot product over d_h in the MFMA's fixed order: it depends neither on the batch around its row nor
// on p0 / W.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pos_table(const float* __restrict__ R, const float* __restrict__ Wm, const float* __restrict__ bias, float wscale, int rows, int TP,
                                                   int H, int dh, uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * H) return;
    const int p = (int)(i / H), f = (int)(i % H);
    float acc = 0.f;
    for (int c = 0; c < H; ++c) acc = fmaf(R[(int64_t)p * H + c], Wm[(int64_t)f * H + c], acc);
    // (the bias arrives as the loader stored it: query_proj's already carries the score scale)
    out[((int64_t)(f / dh) * TP + p) * dh + f % dh] = ET::from_f32(acc * wscale + bias[f]);
}

constexpr int POS_ROWS = 128, POS_CHUNK = 64;      // packed rows per block; buckets staged at a time
template <int DH>
__global__ __launch_bounds__(256) void k_pos_scores(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const int* __restrict__ Tp, int H, int heads,
                                                    const uint16_t* __restrict__ pk, const uint16_t* __restrict__ pq, int TP, int p0, int W, float* __restrict__ out) {
    constexpr int NK = DH / 16, NC = DH / 8, PITCH = 2 * DH + 16;      // k-steps; 16-B chunks per table row; bytes per staged row
    __shared__ __attribute__((aligned(16))) char tab[2 * POS_CHUNK * PITCH];
    const int T = *Tp;
    const int t0 = (int)blockIdx.x * POS_ROWS, head = (int)blockIdx.y;
    if (t0 >= T) return;                                   // block-uniform (the grid covers the largest possible token count)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, hf = lane >> 5;
    // A fragments: lane (c, hf) holds features 16 s + 8 hf .. + 7 of row t0 + 32 wave + c (rows past T are read — the buffers hold whole 256-row tiles — and never stored)
    const int64_t trow = (int64_t)t0 + 32 * wave + c;
    uint4 qa[NK], ka[NK];
#pragma unroll
    for (int s = 0; s < NK; ++s) {
        qa[s] = *reinterpret_cast<const uint4*>(q + trow * H + head * DH + 16 * s + 8 * hf);
        ka[s] = *reinterpret_cast<const uint4*>(k + trow * H + head * DH + 16 * s + 8 * hf);
    }
    const uint16_t* tsrc[2] = {pk + (int64_t)head * TP * DH, pq + (int64_t)head * TP * DH};
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int pc = 0; pc < W; pc += POS_CHUNK) {
        if (pc > 0) __syncthreads();                       // every wave is done with the previous chunk
        for (int i = tid; i < 2 * POS_CHUNK * NC; i += 256) {
            const int which = i / (POS_CHUNK * NC), row = (i / NC) % POS_CHUNK, ch = i % NC;
            if (pc + row < W)                              // p0 + W <= TP (pos_span): inside the table
                *reinterpret_cast<uint4*>(tab + (which * POS_CHUNK + row) * PITCH + ch * 16) =
                    *reinterpret_cast<const uint4*>(tsrc[which] + (int64_t)(p0 + pc + row) * DH + ch * 8);
        }
        __syncthreads();
#pragma unroll
        for (int pt = 0; pt < POS_CHUNK / 32; ++pt) {
            if (pc + 32 * pt >= W) break;                  // W is a multiple of 32
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                const char* brow = tab + (which * POS_CHUNK + 32 * pt + c) * PITCH + hf * 16;
                f32x16 acc = ET::mfma(which ? ka[0] : qa[0], *reinterpret_cast<const uint4*>(brow), zero);
#pragma unroll
                for (int s = 1; s < NK; ++s) acc = ET::mfma(which ? ka[s] : qa[s], *reinterpret_cast<const uint4*>(brow + 32 * s), acc);
                // register r of lane (c, hf): row 8 (r >> 2) + 4 hf + (r & 3) of the wave's tile, bucket p0 + pc + 32 pt + c
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t t = (int64_t)t0 + 32 * wave + 8 * (r >> 2) + 4 * hf + (r & 3);
                    if (t < T) out[((t * heads + head) * 2 + which) * W + pc + 32 * pt + c] = acc[r];
                }
            }
        }
    }
}

}  // namespace KR_ENC_NS
}  // namespace kr
