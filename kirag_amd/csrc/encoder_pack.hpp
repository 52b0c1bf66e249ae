// Token-packing front end of the sentence encoder (encoder_pack.hip): the [B,S] batch, or its ragged form, becomes the per-sequence and per-token tables
// every kernel of the forward reads.  Nothing here depends on the operand type, so it is compiled once (encoder.hip is compiled per type).
#pragma once
#include "common.hpp"

namespace kr {

// per sequence b: attended positions, whether position 0 is attended, token rows (nk + the query-only row for position 0 when CLS pooling needs it), first
// token row (exclusive scan of round_up(nq, align)), the row CLS pooling reads; T = token rows of the batch
struct SeqTables { int *nk, *has0, *nq, *off, *cls, *T; };
// per token row: id, column, token type, embedding position under fairseq's rule (epos == nullptr: BERT's rule, pos is all there is); err: the sticky error
// word (bit 1: id outside the vocabulary, 4: token type outside its vocabulary, 8: bad ragged lengths), cleared by the host once it has been reported
struct TokTables { int *id, *pos, *type, *epos, *err; };
// align = 4, or 8 when the long-sequence attention kernel stages V^T by 16-byte LDS-DMA; P: fairseq's padding index (read only with epos)
struct PackRules { int vocab, type_vocab, pool, align, P; };      // pool: KR_POOL_MEAN or KR_POOL_CLS (KR_POOL_CLASSIFY packs as KR_POOL_CLS: enqueue_forward passes that)

// padded input: ids / mask / tt [B,S] int64 on the device, tt or nullptr (= all zero).  One launch for a small batch, three otherwise.
void pack_padded(const int64_t* ids, const int64_t* mask, const int64_t* tt, int B, int S, const PackRules& r, const SeqTables& t, const TokTables& k, hipStream_t st);
// ragged input: ids32 = the attended tokens of every sequence back to back (`total` of them), lens[b] = how many belong to sequence b, at positions
// 0 .. lens[b]-1; in_off: B ints of scratch.  Fills exactly the tables pack_padded fills for the equivalent [B,S] batch (mask[b,p] = p < lens[b]).
// One launch for a small batch, two otherwise.
void pack_ragged(const int* ids32, const int* lens, int* in_off, int B, int S, int total, const PackRules& r, const SeqTables& t, const TokTables& k, hipStream_t st);

}  // namespace kr
