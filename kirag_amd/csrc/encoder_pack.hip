// Token-packing front end of the sentence encoder: see encoder_pack.hpp.  Every rule is ONE __device__ function run by one wave; the kernels below only
// decide which wave runs it and where the tables live (a small batch keeps them in LDS and is a single launch: a 32-token forward is launch-bound).
#include "encoder_pack.hpp"

namespace kr {
namespace pack {

constexpr int SMALL_B = 64;   // batches up to here are packed by one block

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
    return v;
}

// one row of a padded batch: number of attended positions and whether position 0 is attended
__device__ __forceinline__ void count_row(const int64_t* __restrict__ mask, int S, int lane, int* nk, int* has0) {
    int c = 0;
    for (int p = lane; p < S; p += 64) c += (mask[p] != 0) ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
    if (lane == 0) { *nk = c; *has0 = (mask[0] != 0) ? 1 : 0; }
}

// ragged input, any B: nk, has0 and where each sequence starts in ids32 (exclusive scan of the raw lengths).  A length outside [0, S], or lengths that do not
// add up to `total`, set error bit 8 and the sequence is read as empty: nothing is read past `total` (the following starts keep the caller's lengths)
__device__ __forceinline__ void scan_lens(const int* __restrict__ lens, int B, int S, int total, const SeqTables& t, int* in_off, int* err, int lane) {
    int carry = 0;
    bool bad = false;
    for (int base = 0; base < B; base += 64) {
        const int b = base + lane;
        int len = (b < B) ? lens[b] : 0;
        if (len < 0 || len > S) { bad = true; len = 0; }
        const int incl = wave_incl_scan(len, lane);
        const int start = carry + incl - len;
        if (start + len > total) { bad = true; len = 0; }
        if (b < B) { t.nk[b] = len; t.has0[b] = len > 0 ? 1 : 0; in_off[b] = start; }
        carry += __shfl(incl, 63, 64);
    }
    if (__ballot(bad) != 0ull || carry != total) { if (lane == 0) atomicOr(err, 8); }
}

// any B, from nk / has0: nq = nk (+1 query-only row for position 0 when CLS pooling needs it), cls, offsets = exclusive scan of round_up(nq, align), T
__device__ __forceinline__ void scan_seqs(const SeqTables& t, int B, const PackRules& r, int lane) {
    int carry = 0;
    for (int base = 0; base < B; base += 64) {
        const int b = base + lane;
        int n = 0;
        if (b < B) {
            n = t.nk[b] + ((r.pool == KR_POOL_CLS && !t.has0[b]) ? 1 : 0);
            t.nq[b] = n;
            t.cls[b] = t.has0[b] ? 0 : t.nk[b];
        }
        const int padded = (n + r.align - 1) & ~(r.align - 1);
        const int incl = wave_incl_scan(padded, lane);
        if (b < B) t.off[b] = carry + incl - padded;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) *t.T = carry;
}

// The two sources of one sequence's tokens: `cols` columns, of which fill_seq keeps the attended ones
struct PaddedRow {
    const int64_t *ids, *mask, *tt;   // tt: nullptr = all zero
    int cols;
    __device__ bool attended(int p) const { return mask[p] != 0; }
    __device__ int64_t id(int p) const { return ids[p]; }
    __device__ int64_t type(int p) const { return tt ? tt[p] : 0; }
};
struct RaggedRun {
    const int* src;
    int cols;
    __device__ bool attended(int) const { return true; }
    __device__ int64_t id(int p) const { return src[p]; }
    __device__ int64_t type(int) const { return 0; }
};

// The packed token list of ONE sequence: attended positions in order, the optional query-only row for position 0, zero rows up to round_up(n, align).
// The query-only row reads column 0; an empty ragged run has none and reads what its padded twin holds there: [PAD] = 0 under BERT's rule, id P under fairseq's.
// Fairseq's rule (k.epos): a second ballot counts the ids != P over ALL columns of the source, attended or not (the count the attended-only `run` cannot
// give), and epos gets P + that count (P where the id is P).
template <class Src>
__device__ __forceinline__ void fill_seq(const Src& s, const PackRules& r, const TokTables& k, int o, int n_att, int n, int lane) {
    auto put = [&](int row, int64_t id, int pos, int64_t ty, int epos) {
        if (id < 0 || id >= r.vocab) { atomicOr(k.err, 1); id = 0; }
        if (ty < 0 || ty >= r.type_vocab) { atomicOr(k.err, 4); ty = 0; }
        k.id[row] = (int)id; k.pos[row] = pos; k.type[row] = (int)ty;
        if (k.epos) k.epos[row] = epos;
    };
    int run = 0, erun = 0;
    for (int base = 0; base < s.cols; base += 64) {
        const int p = base + lane;
        const bool in = p < s.cols, v = in && s.attended(p);
        const unsigned long long bal = __ballot(v);
        const int64_t id = (v || (k.epos && in)) ? s.id(p) : 0;
        const bool m = k.epos && in && id != r.P;
        const unsigned long long mbal = __ballot(m);
        if (v) put(o + run + __popcll(bal & ((1ull << lane) - 1ull)), id, p, s.type(p), r.P + (m ? erun + __popcll(mbal & ((2ull << lane) - 1ull)) : 0));
        run += __popcll(bal);
        erun += __popcll(mbal);
    }
    if (lane == 0 && n > n_att) {
        const int64_t id = s.cols > 0 ? s.id(0) : k.epos ? r.P : 0;
        put(o + n_att, id, 0, s.cols > 0 ? s.type(0) : 0, r.P + (id != r.P ? 1 : 0));
    }
    const int padded = (n + r.align - 1) & ~(r.align - 1);
    if (lane < padded - n) put(o + n + lane, 0, 0, 0, 0);
}

__device__ __forceinline__ PaddedRow padded_row(const int64_t* ids, const int64_t* mask, const int64_t* tt, int S, int b) {
    return PaddedRow{ids + (int64_t)b * S, mask + (int64_t)b * S, tt ? tt + (int64_t)b * S : nullptr, S};
}

// ---- large batches: one wave per sequence around the one-wave scan ----
__global__ __launch_bounds__(64) void k_pack_count(const int64_t* __restrict__ mask, int S, SeqTables t) {
    count_row(mask + (int64_t)blockIdx.x * S, S, threadIdx.x, t.nk + blockIdx.x, t.has0 + blockIdx.x);
}
__global__ __launch_bounds__(64) void k_pack_scan(int B, PackRules r, SeqTables t) { scan_seqs(t, B, r, threadIdx.x); }
__global__ __launch_bounds__(64) void k_pack_fill(const int64_t* ids, const int64_t* mask, const int64_t* tt, int S, PackRules r, SeqTables t, TokTables k) {
    const int b = blockIdx.x;
    fill_seq(padded_row(ids, mask, tt, S, b), r, k, t.off[b], t.nk[b], t.nq[b], threadIdx.x);
}
__global__ __launch_bounds__(64) void k_rag_scan(const int* lens, int* in_off, int B, int S, int total, PackRules r, SeqTables t, TokTables k) {
    scan_lens(lens, B, S, total, t, in_off, k.err, threadIdx.x);
    scan_seqs(t, B, r, threadIdx.x);   // each lane reads back what it wrote itself
}
__global__ __launch_bounds__(64) void k_rag_fill(const int* ids32, const int* in_off, PackRules r, SeqTables t, TokTables k) {
    const int b = blockIdx.x;
    fill_seq(RaggedRun{ids32 + in_off[b], t.nk[b]}, r, k, t.off[b], t.nk[b], t.nq[b], threadIdx.x);
}

// ---- B <= SMALL_B: the same steps by one block of 16 waves on tables in LDS, copied out once the scan is done ----
struct SmallTables {
    int nk[SMALL_B], has0[SMALL_B], nq[SMALL_B], off[SMALL_B], cls[SMALL_B], in_off[SMALL_B], T;
    __device__ SeqTables view() { return SeqTables{nk, has0, nq, off, cls, &T}; }
    __device__ void publish(const SeqTables& t, int B) const {
        const int b = threadIdx.x;
        if (b < B) { t.nk[b] = nk[b]; t.has0[b] = has0[b]; t.nq[b] = nq[b]; t.off[b] = off[b]; t.cls[b] = cls[b]; }
        if (b == 0) *t.T = T;
    }
};
__global__ __launch_bounds__(1024) void k_pack_small(const int64_t* ids, const int64_t* mask, const int64_t* tt, int B, int S, PackRules r, SeqTables t, TokTables k) {
    __shared__ SmallTables s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = wave; b < B; b += 16) count_row(mask + (int64_t)b * S, S, lane, s.nk + b, s.has0 + b);
    __syncthreads();
    if (wave == 0) scan_seqs(s.view(), B, r, lane);
    __syncthreads();
    s.publish(t, B);
    for (int b = wave; b < B; b += 16) fill_seq(padded_row(ids, mask, tt, S, b), r, k, s.off[b], s.nk[b], s.nq[b], lane);
}
__global__ __launch_bounds__(1024) void k_rag_small(const int* ids32, const int* lens, int B, int S, int total, PackRules r, SeqTables t, TokTables k) {
    __shared__ SmallTables s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        scan_lens(lens, B, S, total, s.view(), s.in_off, k.err, lane);
        scan_seqs(s.view(), B, r, lane);
    }
    __syncthreads();
    s.publish(t, B);
    for (int b = wave; b < B; b += 16) fill_seq(RaggedRun{ids32 + s.in_off[b], s.nk[b]}, r, k, s.off[b], s.nk[b], s.nq[b], lane);
}

}  // namespace pack
using namespace pack;

void pack_padded(const int64_t* ids, const int64_t* mask, const int64_t* tt, int B, int S, const PackRules& r, const SeqTables& t, const TokTables& k, hipStream_t st) {
    if (B <= SMALL_B) hipLaunchKernelGGL(k_pack_small, dim3(1), dim3(1024), 0, st, ids, mask, tt, B, S, r, t, k);
    else {
        hipLaunchKernelGGL(k_pack_count, dim3(B), dim3(64), 0, st, mask, S, t);
        hipLaunchKernelGGL(k_pack_scan, dim3(1), dim3(64), 0, st, B, r, t);
        hipLaunchKernelGGL(k_pack_fill, dim3(B), dim3(64), 0, st, ids, mask, tt, S, r, t, k);
    }
}

void pack_ragged(const int* ids32, const int* lens, int* in_off, int B, int S, int total, const PackRules& r, const SeqTables& t, const TokTables& k, hipStream_t st) {
    if (B <= SMALL_B) hipLaunchKernelGGL(k_rag_small, dim3(1), dim3(1024), 0, st, ids32, lens, B, S, total, r, t, k);
    else {
        hipLaunchKernelGGL(k_rag_scan, dim3(1), dim3(64), 0, st, lens, in_off, B, S, total, r, t, k);
        hipLaunchKernelGGL(k_rag_fill, dim3(B), dim3(64), 0, st, ids32, in_off, r, t, k);
    }
}

}  // namespace kr
