/*
 * kirag_amd — C ABI of the MI355X-native dense-retrieval core (libkirag_amd.so).
 *
 * The reference (jyfang6/kirag) is pure Python and has no FFI of its own: its boundary for this path is the
 * duck-typed Python surface of retriever/{encoders,index,retrievers,e5}.py, underneath which the arithmetic is
 * done by third-party libraries (HF BertModel.forward, faiss.IndexFlatIP).  Each entry point below names the
 * reference call it replaces (paths relative to the reference root).  The Python shims in kirag_amd/ bind these
 * through ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative KR_E* code; it never throws across the ABI;
 *     kr_last_error() returns a thread-local message for the last failure on the calling thread.
 *   - data pointers may be HOST or DEVICE pointers (hipMemcpyDefault semantics); device pointers must belong to
 *     the handle's device.  The caller owns every I/O buffer; handles own their device allocations.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls on one handle are serialised
 *     by the caller (one thread per rank, as in the reference).
 *   - there is NO CPU fallback: without a gfx950 device every compute call fails with KR_ENODEV.
 */
#ifndef KIRAG_AMD_H
#define KIRAG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KR_OK 0
#define KR_EINVAL (-22)   /* bad argument (shape, k, dtype, unknown weight name ...) */
#define KR_ENOMEM (-12)   /* hipMalloc failed */
#define KR_ENODEV (-19)   /* no usable HIP device */
#define KR_EHIP (-5)      /* a HIP runtime call failed; see kr_last_error() */
#define KR_ESTATE (-1)    /* handle not ready (e.g. encoder weights missing) */
#define KR_ERANGE (-34)   /* the encoder met non-finite activations (a value outside the f16 operand range, or NaN / Inf weights): results unusable */

#define KR_ABI_VERSION 9
int kr_abi_version(void);
const char* kr_last_error(void);
int kr_device_count(void);
/* process-wide test / diagnostic switches.  "force_exact_scores" (0/1): every canonical score goes through the integer
 * super-accumulator instead of the certified fp64 fast path (same results by definition; exercises the rare path).
 * "byte_prescan" (0/1, default 1): blocks of at most 32 queries on an index of >= 2^19 rows (256 < d <= 1024 with a 16-bit row pitch of 384 / 512 / 768 / 1024) stream an int8 copy of the rows
 * (1 KiB per row at d = 1024, built by the first such search) in the final round of the coarse scan and 16-bit-score only the rows it marks;
 * results are the same exact top-k either way.  KIRAG_AMD_NO_BYTE_SCAN in the environment at kr_index_create: never for that index.
 * "debug_byte_min_rows" (rows; < 0 = default 2^19): test hook, the index size from which small blocks take that path.
 * "debug_eps8_permille" (default 1000; <= 0 restores it): MUTATION hook of the tests — the pre-scan's error bound eps8 is multiplied by value / 1000.  With a value
 * below 1000 the pre-scan is no longer exact (tests/test_gpu_search.py builds a row that a 750-permille bound misses and the real bound finds); never set it in production.
 * Regimes the pre-scan does not serve: blocks of 33-128 queries, and 16-32-query blocks over anisotropic (e5-like) rows that mark more than n/8 rows four times
 * in a row (the index then pauses the pre-scan for 1024 calls): those run the 2-byte stream at ~0.66-0.69 of HBM.  No reference caller sits there
 * (knowledge_graph/models.py:1645 searches 1-2 queries per hop, retrieve.py whole query sets).
 * "debug_va_retired_tib" (TiB) / "debug_vmm_min_reserve_mib" (MiB; 0 = default): test hooks of the large-index address-space
 * budget and of the smallest address range reserved per large index.  Unknown names: KR_EINVAL. */
int kr_set_option(const char* name, int value);
/* frees the per-device scratch buffers kr_score_topk keeps between calls */
void kr_release_scratch(void);

/* ------------------------------------------------------------------------------------------------------------
 * Flat inner-product index — replaces faiss.IndexFlatIP behind retriever/index.py (Indexer, :17-83).
 * Stores, per row, the fp32 master (exact re-rank) and a 16-bit copy (MFMA coarse scan); rows live in HBM.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct kr_index kr_index;

#define KR_METRIC_INNER_PRODUCT 0  /* retriever/index.py:13  FAISSINDEX_DICT["inner_product"] */
#define KR_COARSE_BF16 0
#define KR_COARSE_F16 1

/* Indexer.__init__ (index.py:19-24): faiss.IndexFlatIP(vector_sz).  d % 4 == 0, 4 <= d <= 4096. */
int kr_index_create(int d, int metric, int coarse_dtype, int device, kr_index** out);
void kr_index_destroy(kr_index* ix);
/* capacity hint (rows); avoids regrowth copies when the final size is known (faiss_index_corpus.py:42-45 loop) */
int kr_index_reserve(kr_index* ix, int64_t n_rows);
/* Indexer.index_data -> index.add(embeddings.astype('float32')) (index.py:26-34): append n fp32 rows [n,d]. */
int kr_index_add(kr_index* ix, const float* x, int64_t n, void* stream);
/* index.ntotal (index.py:75,79) */
int64_t kr_index_ntotal(const kr_index* ix);
int kr_index_dim(const kr_index* ix);
/* read back fp32 rows [start, start+n) (serialisation: index.py:55-64 writes the flat storage) */
int kr_index_get_rows(kr_index* ix, int64_t start, int64_t n, float* out, void* stream);

/* Native shard files (SURVEY 8f-1 "native sharded bf16 format"; kirag_amd/retriever/index.py ShardedIndexer.serialize /
 * deserialize_from, next to the reference's index.py:55-79 formats): the stored state of rows, exactly — fp32 master, 16-bit
 * scan copy [n, coarse_dim] and the two quantisation bounds — so that a saved shard reloads without re-quantising. */
int kr_index_coarse_dim(const kr_index* ix);      /* row length of the 16-bit copy (d rounded up to 64) */
int kr_index_coarse_dtype(const kr_index* ix);    /* KR_COARSE_BF16 / KR_COARSE_F16 */
int kr_index_get_coarse(kr_index* ix, int64_t start, int64_t n, uint16_t* out, void* stream);
int kr_index_get_bounds(kr_index* ix, float* out2 /* max |x - c(x)|, max |c(x)| over the stored rows */);
int kr_index_add_raw(kr_index* ix, const float* xf, const uint16_t* xc, int64_t n, const float* bounds2, void* stream);

/* Indexer.search_knn -> index.search(q, top_docs) (index.py:47): exact inner-product top-k.
 *   q       [nq,d] fp32;  scores [nq,k] fp32 (descending);  rows [nq,k] int64 = internal row numbers
 *   (the caller maps them through index_id_to_db_id exactly as index.py:49 does).
 * Result definition (identical to oracle/search_c.c): score = the EXACT inner product of the fp32 inputs rounded once to
 * fp32 (round-to-nearest-even; independent of any summation order); ranking by (score desc, row asc); rows whose score is
 * NaN are never returned.  0 < k <= min(ntotal, 1024), else KR_EINVAL.
 * Magnitudes: the guarantee covers ALL of fp32 - rows and queries of any norm, subnormal elements, scores that round to zero, to a subnormal
 * or to +-inf, rows and queries with +-inf or NaN elements (a score is then +-inf or NaN as in IEEE arithmetic; +inf scores tie and resolve by
 * row asc).  The certificate's error bounds are computed in fp64 and rounded up, so no magnitude makes pass 1 claim more than it knows.
 * Zero rule: -0.0 and +0.0 are ONE score.  They tie (the lower row wins), and a zero score may come back with either sign (today: +0.0
 * from every search and from kr_score_topk; the merges pass on what they are given).  Every non-zero score is bit-exact.
 * `mode`: 0 = auto: pass 1 = 16-bit MFMA scan + certified exact re-rank for all queries; pass 2 = fp64 MFMA scan of the fp32 rows
 *             + certified re-rank for the queries pass 1 could not certify (they share one pass over the corpus per group of
 *             32); pass 3 = exact scan, query by query, for what is left (mass ties);
 *         1 = exact scan only, 2 = pass 2 (+3) only — slow; used by tests as on-device cross-checks.
 * Small calls (ABI 8, nq <= 32, mode 0): when q, scores and rows are all addressable by the device (device memory of the index's GPU, pinned host
 * memory) the kernels read the queries and write the results in place — no staging copies; any other combination goes through the workspace as before.
 * On an index of >= 2^19 rows the final coarse round of such a call streams an int8 copy of the rows (kr_set_option "byte_prescan"). */
int kr_index_search(kr_index* ix, const float* q, int nq, int k, float* scores, int64_t* rows, int mode, void* stream);
/* The same search (mode 0) in two halves.  kr_index_search_async ENQUEUES pass 1 of every 1024-query block on `stream` and returns without waiting
 * for the device (given device pointers it performs no host synchronisation at all): the results of every query whose exactness certificate holds
 * are written to scores / rows in stream order, and the per-query certificate flags are copied to pinned memory behind them.
 * kr_index_search_finish waits for that point, reads the flags and - only for queries pass 1 could not certify - runs passes 2 / 3 and overwrites
 * their rows; after it returns the results are final and the statistics are updated.  q, scores and rows must stay valid until then.
 * Up to 16 calls may be outstanding per handle as long as they use ONE stream (ABI 5; the row-sharded search of bench.py --gpus N enqueues the W
 * batches of a block back to back and looks at the certificates once): a call on another stream, a 17th call, and any other call that touches the
 * handle's rows (add, reserve, get_rows ...) finish the outstanding ones first.  kr_index_search_finish finishes ALL outstanding calls, oldest first;
 * kr_index_search_finish_ex does the same and reports, per call (oldest first, the first `cap` of them), how many of its queries pass 1 could not
 * certify — i.e. whether rows of that call's result buffers were re-written after whatever the caller enqueued behind the call had consumed them.
 * kr_index_search(mode 0) == kr_index_search_async + kr_index_search_finish. */
int kr_index_search_async(kr_index* ix, const float* q, int nq, int k, float* scores, int64_t* rows, void* stream);
int kr_index_search_finish(kr_index* ix);
int kr_index_search_finish_ex(kr_index* ix, int64_t* flagged, int cap, int* ncalls);
/* ... and only the OLDEST outstanding call (ABI 8): a host that converts block i's results while block i + 1 is already being searched keeps two calls
 * in flight and finishes them one at a time (Indexer.search_knn).  *flagged (may be NULL) as in kr_index_search_finish_ex; no call outstanding: 0, nothing done. */
int kr_index_search_finish_one(kr_index* ix, int64_t* flagged);
int kr_index_search_pending(const kr_index* ix);   /* number of outstanding asynchronous calls */

/* Row-sharded search with the exchange BEFORE the re-rank (replaces the gather of utils/utils.py:145-155 together with kr_topk_merge_device /
 * kr_shard_allgather_topk).  Every shard certifies and re-ranks its OWN top-k in kr_index_search_async: ~0.3 ms of scattered fp32 row gathers per 1000-query
 * batch on every rank whatever the number of shards, although only ~k / W of a shard's rows reach the global top-k.  Split form, one block of nq <= 1024 queries,
 * all three calls enqueue-only on ONE stream with nothing else on the handle in between:
 *   kr_index_search_coarse_async   pass 1's coarse scan; topk [nq, k + 1] (DEVICE memory) receives the k best coarse scores of this shard per query
 *                                  (unsorted, -inf where the shard has fewer candidates) followed by the query's error bound on this shard;
 *   [the host gathers the shards' topk blocks: gathered [nshards][nq][k + 1], rank order irrelevant]
 *   kr_index_search_global_theta   theta[q] = (k-th best coarse score of ALL shards) - (largest error bound of any shard + this shard's): a row of this shard
 *                                  with a coarse score below it cannot be in the global exact top-k;
 *   kr_index_search_rerank_async   certificate + exact re-rank of the candidates above max(local bound, theta); scores / rows [nq, k] as in
 *                                  kr_index_search_async, but a query may get FEWER than k rows: the tail is (-inf, -1) (kr_topk_merge* treat id < 0 as padding).
 *                                  theta == NULL: exactly kr_index_search_async's result.
 * The call is outstanding from the first half on (kr_index_search_finish* as usual; queries pass 1 could not certify are re-answered with the shard's own
 * exact top-k, which merges just as well); a first half whose second half never comes makes the next finish return KR_ESTATE. */
int kr_index_search_coarse_async(kr_index* ix, const float* q, int nq, int k, float* topk, void* stream);
int kr_index_search_global_theta(kr_index* ix, const float* gathered, int nshards, float* theta, void* stream);
int kr_index_search_rerank_async(kr_index* ix, const float* theta, float* scores, int64_t* rows, void* stream);

typedef struct {
    int64_t queries;          /* queries answered since creation / last reset */
    int64_t certified;        /* answered by the fast path with the exactness certificate holding */
    int64_t fallback;         /* not certified by pass 1 (= fine + exact) */
    int64_t overflow;         /* candidate-buffer overflows in pass 1 (subset of fallback) */
    int64_t reranked_rows;    /* fp32 rows gathered by the re-rank kernel */
    int64_t coarse_rounds;    /* coarse GEMM launches */
    double last_coarse_ms;    /* device time of the coarse launches of the last search call (HIP events) */
    double last_total_ms;     /* device time of the whole last search call */
    int64_t fine;             /* answered by pass 2 (fp64 MFMA scan, certified) */
    int64_t exact;            /* answered by pass 3 (exact scan) */
    int64_t fine_rounds;      /* pass-2 scan launches */
    double last_fine_ms;      /* device time of pass 2 in the last search call */
    int64_t marked_passes;    /* pass-2 groups that were pre-scanned (16-bit stream marking the rows the fp64 scan has to visit) */
    int64_t marked_rows;      /* rows marked by those pre-scans, summed over the groups */
    int64_t va_retired_bytes; /* process-wide: virtual addresses retired by released / moved indexes (never reused) */
    int64_t grow_mode;        /* this index: -1 undecided (< 256 MiB), 0 hipMalloc + copy-on-grow, 1 chunks mapped into a reserved address range */
    int64_t byte_scans;       /* query blocks whose final coarse round went through the int8 copy (kr_set_option "byte_prescan") */
    int64_t byte_marked_rows; /* rows those pre-scans marked (then scored from the 16-bit copy), summed */
    int64_t byte_rows;        /* this index: rows its int8 copy currently covers (0: none - never built, released, or not affordable; kr_index_prepare) */
} kr_search_stats;
int kr_index_stats(kr_index* ix, kr_search_stats* out, int reset);
/* Do now what the FIRST search of blocks of `nq` queries x top-`k` would otherwise do on the spot: allocate that shape's search workspaces, set the kernels'
 * function attributes and - when such blocks take the byte pre-scan on this index (kr_set_option "byte_prescan") - build the int8 copy of the rows (8.6 ms at
 * 5M x 1024 rows + 1 KiB per row of HBM; extended by the rows added since an earlier call) with its row bitmap.  The copy is only built while it leaves
 * max(2 GiB, 1/16 of the device) free and is released again when kr_index_add needs the memory (derived data: results never depend on it).  Called by
 * Indexer.index_data / deserialize_from (retriever/index.py:26-34,66-79) so that the first KiRAG hop after a load (knowledge_graph/models.py:1645) costs what
 * every later one costs.  Enqueues on `stream`; waits for searches in flight on the handle.  An empty index: no-op. */
int kr_index_prepare(kr_index* ix, int nq, int k, void* stream);

/* Exact top-k of q . x^T for a small transient candidate set — replaces the torch.matmul + torch.topk of the KiRAG loop's aligner step
 * (knowledge_graph/models.py:1532-1538: [1-2 queries] x [T triples], top-20) and the matmul + argsort of the exemplar / dev-MRR ranking
 * (models.py:1315-1316, kg_generator.py:119-120, trainer/aligner_trainer.py:112-113).
 *   q [nq,d], x [n,d] fp32 (host or device pointers), scores [nq,k] fp32 descending, rows [nq,k] int64 row numbers of x.
 * Same result definition as kr_index_search (canonical score, ties by row asc); 0 < k <= min(n, 1024), nq <= 65535. */
int kr_score_topk(const float* q, int nq, const float* x, int64_t n, int d, int k, float* scores, int64_t* rows, int device, void* stream);

/* Host-side final merge of per-shard results (north_star: "host-side final merge" after the RCCL all-gather).
 *   scores [nshards,nq,k], ids [nshards,nq,k] (GLOBAL ids) -> out_scores/out_ids [nq,k] by (score desc, id asc).
 *   Host pointers only. */
int kr_topk_merge(const float* scores, const int64_t* ids, int nshards, int nq, int k, float* out_scores, int64_t* out_ids);

/* Decimal ASCII of n int64 ids, joined by `sep`, no trailing separator: the bulk form of the `str(id)` per hit that Indexer.search_knn returns
 * (index.py:49 builds 100 k Python strings per 1024-query x top-100 block one at a time — as long as the GPU's whole search of the block; the
 * host mirror splits this buffer instead).  Host pointers.  cap >= 21 * n always suffices; KR_EINVAL when `out` is too small. */
int kr_format_ids(const int64_t* ids, int64_t n, char sep, char* out, int64_t cap, int64_t* written);

/* The same merge on the device, for lists that are already in HBM (the output of the all-gather): asynchronous on `stream`, no host round trip.
 *   scores + s * score_shard_stride -> list block [nq,k] of shard s (strides in elements), likewise ids; out_* [nq,k] device (or pinned host) pointers.
 *   nshards * k <= 8192.  Result identical to kr_topk_merge (lists sorted by (score desc, id asc), id < 0 = padding at the tail, ids unique). */
int kr_topk_merge_device(const float* scores, int64_t score_shard_stride, const int64_t* ids, int64_t id_shard_stride, int nshards, int nq, int k,
                         float* out_scores, int64_t* out_ids, int device, void* stream);

/* The exchange step of the row-sharded search for hosts without their own collective library (the reference gathers to rank 0 with
 * torch.distributed, utils/utils.py:145-155): one process per GPU, every rank holds rows [row_offset, row_offset + ntotal) of the corpus.
 *   kr_comm_unique_id  rank 0 fills a KR_COMM_ID_BYTES buffer and hands it to the other ranks by any means (file, socket, MPI, torch.distributed ...).
 *   kr_comm_create     collective: blocks until all `world` ranks (one per GPU of the node) have called it with the same id.  RCCL is loaded at run time
 *                      (librccl.so.1, override with KIRAG_AMD_RCCL_LIB); KR_ESTATE if it cannot be loaded.
 *   kr_shard_allgather_topk   collective, enqueue-only on `stream`: all-gather (RCCL over xGMI) of every rank's [nq,k] lists (scores fp32 descending, rows
 *                      int64 GLOBAL row numbers, (-inf, -1) padding at the tail) + the device merge; every rank gets the global top-k in out_* (device
 *                      pointers, [nq,k]).  world * k <= 8192.  Same result as kr_topk_merge of the W lists. */
#define KR_COMM_ID_BYTES 128
typedef struct kr_comm kr_comm;
int kr_comm_unique_id(void* id128);
int kr_comm_create(const void* id128, int rank, int world, int device, kr_comm** out);
int kr_comm_destroy(kr_comm* c);
int kr_comm_rank(const kr_comm* c);
int kr_comm_world(const kr_comm* c);
int kr_shard_allgather_topk(kr_comm* c, const float* scores_local, const int64_t* rows_local, int nq, int k, float* out_scores, int64_t* out_rows,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * BERT-family sentence encoder — replaces HF BertModel.forward + pooling + F.normalize behind
 * retriever/encoders.py (E5Encoder.forward :67-77, BGEEncoder.forward :106-118) and retriever/e5.py:51-61.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct kr_encoder kr_encoder;

typedef struct {
    int hidden;        /* H   (1024 for e5-large-v2 / bge-large-en, 384 for e5-small-v2 / bge-small-en / MiniLM); multiple of 128, <= 2048 */
    int layers;        /* L   (24; 12 / 6 for the small models) */
    int heads;         /* 16 (12 for the small models); hidden / heads (the head width) must be 32 or 64, anything else is KR_EINVAL */
    int intermediate;  /* FF  (4096) */
    int vocab;         /* 30522 (250002 for XLM-R: multilingual-e5, bge-m3) */
    int max_pos;       /* 512 (XLM-R: 514 position rows = 512 tokens; bge-m3: 8194 = 8192 tokens) */
    int type_vocab;    /* 2 (XLM-R: 1) */
    float ln_eps;      /* 1e-12 (XLM-R: 1e-5) */
} kr_bert_cfg;

#define KR_POOL_MEAN 0 /* E5: average_pool (encoders.py:56-58) then F.normalize */
#define KR_POOL_CLS 1  /* BGE: last_hidden[:,0] (encoders.py:116) then F.normalize */
#define KR_POOL_CLASSIFY 2 /* cross-encoder rerankers: last_hidden[:,0] -> the classification head -> raw logits [B, L] (needs "classifier.*", below); on a
                            * decoder handle with "score.weight": the row of the highest attended column -> the score head (below) */
/* bge-m3's token-level heads: flag bits ORed onto a base pool of KR_POOL_MEAN or KR_POOL_CLS (kr_encoder_forward / kr_encoder_forward_tt only).  `out` then
 * holds, back to back and all fp32: the dense block [B, hidden] (the bits of the unflagged call with the same base pool), with KR_POOL_WITH_SPARSE the sparse
 * block [B, S], with KR_POOL_WITH_COLBERT the colbert block [B, S, P] ("sparse_linear.*" / "colbert_linear.*" under kr_encoder_load_weight below).  Any other
 * bit, the flags on KR_POOL_CLASSIFY or in kr_encoder_forward_packed: KR_EINVAL; a flag whose head was never loaded: KR_ESTATE. */
/* SPLADE (learned sparse retrieval): the MLM head of a BertForMaskedLM checkpoint, max-pooled over the attended tokens.  `out` is [B, vocab] fp32, every entry
 * >= 0 (needs the six "cls.predictions.*" tensors, below; without them KR_ESTATE).  Accepted by kr_encoder_forward, kr_encoder_forward_tt and
 * kr_encoder_forward_packed; combined with KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT: KR_EINVAL.  The value 3 stays refused. */
#define KR_POOL_SPLADE 4
/* Last-token pooling (decoder-LLM embedders): out [B, hidden] = normalize(the final row of the sequence's highest attended column).  Accepted by the three
 * forward entry points on decoder handles ("config.decoder_attention", below) only — on every other handle it stays KR_EINVAL, and the message says so —
 * and never with KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT.  Packing, attention and the last layer (on every row) are KR_POOL_MEAN's; a sequence without
 * attended tokens gives a NaN row (not an error), like the mean. */
#define KR_POOL_LAST 5
#define KR_POOL_WITH_SPARSE 0x10
#define KR_POOL_WITH_COLBERT 0x20

/* 16-bit type of the MFMA operands and of every stored activation (weights, residual stream, q / k / v, P, ctx, h); accumulation is fp32 and the
 * LayerNorms run in fp32 either way.  f16 has 11 significand bits (|x| <= 65504), bf16 8: with outlier hidden channels (what real BERT-family
 * checkpoints have) only f16 + the residual low half stays inside the 1e-3 score tolerance with margin (tests/golden G10). */
#define KR_ENC_BF16 0
#define KR_ENC_F16 1
#define KR_ENC_DEFAULT_DTYPE KR_ENC_F16
#define KR_ENC_DEFAULT_RESIDUAL_LO 1
int kr_encoder_create(const kr_bert_cfg* cfg, int device, kr_encoder** out);   /* = kr_encoder_create_ex(cfg, device, -1, -1, out) */
/* operand_dtype: KR_ENC_BF16 / KR_ENC_F16 / -1 = default (environment KIRAG_AMD_ENCODER_DTYPE=bf16|f16, else KR_ENC_DEFAULT_DTYPE);
 * residual_lo: 1 = the residual stream between layers keeps a second 16-bit word (the remainder: 16+ significand bits together), 0 = one word,
 * -1 = default (environment KIRAG_AMD_RESIDUAL_LO=0|1, else KR_ENC_DEFAULT_RESIDUAL_LO). */
int kr_encoder_create_ex(const kr_bert_cfg* cfg, int device, int operand_dtype, int residual_lo, kr_encoder** out);
int kr_encoder_operand_dtype(const kr_encoder* enc);   /* what the handle was created with */
int kr_encoder_residual_lo(const kr_encoder* enc);
void kr_encoder_destroy(kr_encoder* enc);
/* one call per HF state_dict tensor of BertModel ("embeddings.word_embeddings.weight",
 * "encoder.layer.3.attention.self.query.bias", ...), fp32, numel checked; "pooler.*" / "*position_ids" ignored.  XLMRobertaModel / RobertaModel have the
 * same names.
 * Names that start with "config." are reserved for settings of the handle (no state-dict tensor starts so); an unknown one is KR_EINVAL.
 *   "config.position_padding_idx": data = ONE float holding an integer P, 0 <= P <= max_pos - 2 (anything else is KR_EINVAL).  The handle then follows
 *   fairseq's position rule (RoBERTa / XLM-R, pad_token_id = P = 1): the position embedding of column i of a row is P + (number of ids != P in columns
 *   0..i, attended or not) where ids[i] != P, and P where ids[i] == P; the forwards then take S <= max_pos - P - 1.  Without it the handle follows BERT's
 *   rule (position = column), bit for bit as before.  Accepted before the handle's first finalize and kept for the handle's life: later the same value is
 *   a no-op, another value KR_EINVAL.  kr_encoder_last_hidden keeps placing rows at their columns under both rules.
 *   "config.rotary_inv_freq": data = d_h / 2 floats (d_h = hidden / heads; any other count is KR_EINVAL), HF's rotary_emb.inv_freq.  Loading it before the
 *   handle's first finalize makes the handle a NomicBert handle for life (nomic-embed-text-v1 / -v1.5, transformers.NomicBertModel); afterwards the same
 *   values are a no-op and other values, or loading it onto a handle that was finalized without it, are KR_EINVAL.  kr_encoder_finalize then builds cos / sin
 *   tables [max_pos][d_h / 2] (max_pos <= 8192): the angle is the fp32 product float(pos) * inv_freq[j], the entries its cosine / sine.  On such a handle
 *     - there is no position table ("embeddings.position_embeddings.weight" is not required; the embedding LayerNorm sums word + token type), and the
 *       forwards take S <= max_pos;
 *     - q and k of every head are rotated after the projection and before they are rounded to 16 bits, NeoX pairing over the whole head width:
 *           x'[j] = x[j] cos - x[j + d_h/2] sin,   x'[j + d_h/2] = x[j + d_h/2] cos + x[j] sin,   cos / sin = table[pos][j],  j < d_h / 2,
 *       where pos is the token's column in the padded [B, S] batch (in kr_encoder_forward_packed, its index inside its sequence) minus the smallest column
 *       among its sequence's rows (the first attended column; 0 when CLS pooling adds the query row of a masked column 0).  Scores depend on column
 *       differences only, so the shift changes no exact score, left padding and masks with holes need no further rule, and a sequence gives the same
 *       bits wherever it stands in the padded batch;
 *     - the MLP is gated: down_proj(silu(gate_proj(x)) * up_proj(x)), gate | up as one projection of 2 * intermediate columns;
 *     - NomicBertModel's state dict loads unchanged: "layers.N.self_attn.{q,k,v,o}_proj.weight" fill the slots of BERT's attention.self.{query,key,value} /
 *       attention.output.dense, "layers.N.post_attention_layernorm.*" / "layers.N.post_mlp_layernorm.*" those of attention.output.LayerNorm / output.LayerNorm,
 *       "layers.N.mlp.down_proj.weight" that of output.dense, and "layers.N.mlp.gate_proj.weight" + "layers.N.mlp.up_proj.weight" together that of the
 *       intermediate projection (a missing one fails finalize as "never loaded"); "embeddings.{word_embeddings,token_type_embeddings,LayerNorm}.*" as in BERT.
 *       q_proj / k_proj / gate_proj / up_proj must come under these names (their packed copies have another row order) and have no bias; the biases of
 *       v / o / down (BERT's names) are zero unless loaded.  A handle without the setting refuses these names at finalize.  It combines with neither
 *       "config.position_padding_idx" nor MPNet's bias tensor.
 *   "config.local_attention_layers": data = one float per layer, 0 or 1 (1 = sliding-window attention).  Loading it before the handle's first finalize makes
 *   the handle a ModernBert handle for life (transformers.ModernBertModel: gte-modernbert-base, modernbert-embed, granite-embedding-english-r2); it needs
 *   "config.rotary_inv_freq" (the frequencies of the global layers; all layers when none is local) and, when any flag is 1,
 *   "config.rotary_inv_freq_local": data = d_h / 2 floats, the frequencies of the local layers (a second pair of cos / sin tables), and
 *   "config.attention_half_window": data = ONE float holding an integer w >= 1: a local layer admits key column j for query column i iff |i - j| <= w
 *   (HF: config.sliding_window = local_attention / 2, inclusive), on top of the padding mask; columns are those of the padded [B, S] batch, so with holes in
 *   the mask the distance counts columns, not attended tokens.
 *   All three follow the rule of the other settings: before the first finalize; later the same values are a no-op, anything else KR_EINVAL.
 *   kr_encoder_finalize refuses (KR_EINVAL, naming the setting) a flag count other than cfg.layers, local layers without frequencies or half-window, the
 *   flags without "config.rotary_inv_freq", the two local settings without the flags, any of them next to "config.position_padding_idx" or MPNet's bias
 *   tensor, ModernBert's tensor names on a handle of another kind and other names on this one.  On such a handle
 *     - the stack is PRE-LN: x += attn.Wo . attention(rot(attn.Wqkv . attn_norm_l(x))), x += mlp.Wo . (erf_gelu(input) * gate) with
 *       input | gate = mlp.Wi . mlp_norm_l(x), attn_norm_0 = identity, output = final_norm(x); the embedding is LayerNorm(tok_embeddings[id]) (the token-type
 *       table is one row: load zeros under BERT's name "embeddings.token_type_embeddings.weight");
 *     - ModernBertModel's state dict loads unchanged: "embeddings.tok_embeddings.weight", "embeddings.norm.*", "layers.N.attn_norm.*" (N >= 1),
 *       "layers.N.attn.Wqkv.weight" [3H, H], "layers.N.attn.Wo.*", "layers.N.mlp_norm.*", "layers.N.mlp.Wi.*" [2 FF, H], "layers.N.mlp.Wo.*" [H, FF],
 *       "final_norm.*".  LayerNorm biases and the biases of attn.Wqkv [3H] / attn.Wo / mlp.Wi / mlp.Wo are zero unless loaded (the q and k thirds of
 *       attn.Wqkv.bias are added before the rotation, as HF rotates Wqkv x + b).  cfg.intermediate must be a multiple of 128 like everywhere (the Python layer zero-pads ModernBERT-large's 2624);
 *     - a query whose window holds no attended column (the CLS row of a MASKED column 0 whose sequence starts beyond column w) gets a zero attention
 *       output in the local layers.
 * MPNetModel (all-mpnet-base-v2, multi-qa-mpnet-*): its state dict loads unchanged.  The layer names "encoder.layer.N.attention.attn.{q,k,v,o}.{weight,bias}"
 * and "encoder.layer.N.attention.LayerNorm.{weight,bias}" fill the slots of BERT's attention.self.{query,key,value} / attention.output.{dense,LayerNorm}
 * (last write wins when a caller uses both spellings for one slot).  MPNet has no token types: create the handle with type_vocab = 1 and load ONE row of
 * zeros as "embeddings.token_type_embeddings.weight"; its embedding positions follow fairseq's rule with P = 1 ("config.position_padding_idx" above).
 *   "encoder.relative_attention_bias.weight": 32 x heads floats ([bucket][head]; any other count is KR_EINVAL — MPNet always uses 32 buckets and
 *   max_distance 128, whatever its config says).  Loading it makes the handle an MPNet handle: every attention score becomes
 *       q.k / sqrt(d_h) + W[bucket(d)][head],   d = column of the key - column of the query,
 *   where a token's column is its index in the padded [B, S] batch (not its position id and not its rank among the attended tokens; in
 *   kr_encoder_forward_packed, the index inside its sequence), and with n = |d|:  bucket = n for n < 8, else min(15, 8 + max{ j >= 0 : 64 * 2^j <= n * n });
 *   plus 16 when d > 0 (key after query).  Buckets 8 .. 15 begin at n = 8, 12, 16, 23, 32, 46, 64, 91.  Like the position rule this is fixed at the first
 *   finalize: a handle finalized with the tensor takes new values for it later (followed by kr_encoder_finalize, as for every tensor), a handle finalized
 *   without it refuses it with KR_EINVAL.  Handles without it run the same kernels, bit for bit, as before the tensor was known.
 * T5EncoderModel (sentence-transformers/gtr-t5-*, sentence-t5-*, hkunlp/instructor-*: the encoder half of T5 v1.0 / v1.1 / flan):
 *   "config.t5_feed_forward": data = ONE float, 0 = the feed-forward wo(relu(wi x)), 1 = the gated wo(gelu_new(wi_0 x) * wi_1 x) with HF's gelu_new
 *   0.5 x (1 + tanh(sqrt(2 / pi) (x + 0.044715 x^3))); anything else is KR_EINVAL.  Loading it before the handle's first finalize makes the handle a T5 handle
 *   for life; afterwards the same value is a no-op and another value, or loading it onto a handle that was finalized without it, is KR_EINVAL.
 *   kr_encoder_finalize refuses it (KR_EINVAL, naming it) next to any of "config.position_padding_idx", "config.rotary_inv_freq*",
 *   "config.local_attention_layers" and "config.attention_half_window", refuses T5's tensor names on a handle of another kind and other families' names on
 *   this one.  In kr_bert_cfg: hidden = d_model, heads = num_heads (d_kv * num_heads must be d_model, d_kv 32 or 64), intermediate = d_ff, type_vocab = 1,
 *   ln_eps = layer_norm_epsilon; max_pos only bounds S (no table is sized by it).  On such a handle
 *     - the stack is PRE-LN with RMS norms (T5LayerNorm: w * x * rsqrt(mean(x^2) + eps), no mean subtracted, no bias): x = shared[id] — no embedding norm,
 *       no positions, no token types —, x += o . attention(q, k, v of layer_norm_0(x)), x += wo . ff(layer_norm_1(x)), output = final_layer_norm(x);
 *     - every attention score is q.k + W[bucket(d)][head] — NO 1 / sqrt(d_h) —, with the ONE table that block 0 holds, in every layer; d, the columns and the
 *       bucket rule are those of the MPNet handles above (T5's bidirectional rule with 32 buckets and max_distance 128 gives the same bucket for every d);
 *     - no linear layer has a bias;
 *     - T5EncoderModel's state dict loads unchanged: "shared.weight" (and its tied alias "encoder.embed_tokens.weight": last write wins),
 *       "encoder.block.N.layer.0.SelfAttention.{q,k,v,o}.weight", "encoder.block.N.layer.0.layer_norm.weight",
 *       "encoder.block.N.layer.1.DenseReluDense.{wi,wo}.weight" (setting 0) or "....DenseReluDense.{wi_0,wi_1,wo}.weight" (setting 1; the other spelling is
 *       KR_EINVAL at finalize), "encoder.block.N.layer.1.layer_norm.weight", "encoder.final_layer_norm.weight" and
 *       "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": 32 x heads floats ([bucket][head]; any other count, or a block other than 0, is
 *       KR_EINVAL).  A missing tensor, the table included, fails finalize as "never loaded"; no position table and no token-type table are required.
 *   "dense.weight": optional, T5 handles only (KR_EINVAL at finalize elsewhere): data = [P, hidden] fp32, 4 <= P <= 2048, P % 4 == 0 — the bias-free
 *   sentence_transformers.models.Dense module with an identity activation that GTR / Sentence-T5 / Instructor put between the pooling and the normalisation
 *   (P = 768 for every GTR size).  A count that is no multiple of hidden, or a P outside that range, is KR_EINVAL.  With it EVERY forward entry point writes
 *   out [B, P] = normalize(W . pooled) instead of [B, hidden] (the caller knows P from the tensor it loaded); an all-masked sequence still gives a NaN row.
 *   Like the settings it is fixed at the first finalize: later the same P takes new values, another P — or the tensor on a handle finalized without it — is
 *   KR_EINVAL.  kr_encoder_last_hidden is not affected (it stays [B, S, hidden]).
 *   "config.rotary_feed_forward": data = ONE float, the feed-forward of a handle with "config.rotary_inv_freq": 0 = NomicBert's SwiGLU (also when never
 *   loaded), 1 = fc2 . gelu(fc1 . x + b1) + b2 with linear biases — a rotary BERT handle (transformers JinaEmbeddingsV3Model: jina-embeddings-v3); anything
 *   else is KR_EINVAL, and the usual rule of the settings holds.  The value 1 needs "config.rotary_inv_freq" and is refused at finalize (KR_EINVAL) next to
 *   every other position scheme and next to "config.decoder_attention".  Such a handle is NomicBert's post-LN stack (word + token-type embedding rows ->
 *   LayerNorm, no position table, q and k rotated) with "layers.N.self_attn.{q,k,v,o}_proj.{weight,bias}", "layers.N.post_attention_layernorm.{weight,bias}",
 *   "layers.N.mlp.{fc1,fc2}.{weight,bias}" and "layers.N.post_mlp_layernorm.{weight,bias}": every bias is zero unless loaded, q's and k's are added before
 *   the rotation; "mlp.gate_proj" / "mlp.up_proj" there, "mlp.fc1" / "mlp.fc2" / "self_attn.o_proj.bias" on any other handle, and grouped-query k / v
 *   tensors are KR_EINVAL at finalize, naming the tensor.
 *   "config.decoder_attention": data = ONE float, 1 = causal attention, 0 = bidirectional attention on the same stack; anything else is KR_EINVAL.  Loading it
 *   before the handle's first finalize makes the handle a DECODER handle for life (transformers Qwen2Model / LlamaModel / MistralModel used as embedders:
 *   the Qwen2.5-0.5B family such as KaLM-embedding-multilingual-mini, Llama-3.2-1B, TinyLlama, SmolLM2 fine-tunes); the usual rule of the settings holds.  It
 *   needs "config.rotary_inv_freq" (max_pos <= 8192; max_pos only bounds S) and is refused at finalize (KR_EINVAL) next to
 *   "config.position_padding_idx", "config.local_attention_layers" and its two companions, "config.t5_feed_forward", the DeBERTa settings or a relative
 *   attention bias: a handle has one position scheme.  In kr_bert_cfg: ln_eps = rms_norm_eps, type_vocab = 1.  On such a handle
 *     - the stack is PRE-LN with RMS norms: x = embed_tokens[id] — no embedding norm, no position table, no token types —,
 *       x += o_proj . attention(rot(q), rot(k), v of input_layernorm(x)), x += down_proj . (silu(gate_proj . n) * up_proj . n) with
 *       n = post_attention_layernorm(x), output = norm(x); rotation and pairing are those of "config.rotary_inv_freq" above;
 *     - with the value 1 a key is admitted iff its column <= the query's column (columns of the padded [B, S] batch, so masks with holes and left padding
 *       need no further rule), on top of the padding mask; the 64-key steps above a 32-query tile's diagonal are skipped;
 *     - the state dict loads unchanged, with or without a leading "model.": "embed_tokens.weight", "layers.N.input_layernorm.weight",
 *       "layers.N.self_attn.{q,k,v,o}_proj.weight" [hidden, hidden], "layers.N.post_attention_layernorm.weight", "layers.N.mlp.{gate,up,down}_proj.weight",
 *       "norm.weight", and optionally "layers.N.self_attn.{q,k,v}_proj.bias" (Qwen2; zero unless loaded; q's and k's are added before the rotation).  o_proj and
 *       the MLP have no bias.  Grouped-query checkpoints load as they are: "layers.N.self_attn.{k,v}_proj.weight" may come as [A, hidden] and
 *       "layers.N.self_attn.{k,v}_proj.bias" as [A], A = kv_heads * d_h, with kv_heads a divisor of heads and A % 64 == 0 (any other count is KR_EINVAL at
 *       load).  kv_heads is read off the element count; k and v (and their biases) of every layer must agree (else KR_EINVAL at finalize, naming the
 *       tensor), and A is fixed at the first finalize.  K and V^T then exist once per KV head and query head h reads KV head h / (heads / kv_heads).  The
 *       EXPANDED form — each KV head's rows repeated heads / kv_heads times, [hidden, hidden] — is accepted as before and computes the same bits; the
 *       expansion is no longer needed, except for a checkpoint whose A is no multiple of 64.  A grouped count on a handle without the setting is KR_EINVAL
 *       at finalize.  k's rows sit in front of v's in the handle's packed matrix, so before the first finalize a k_proj or v_proj matrix that is loaded AGAIN
 *       with another A than it had makes its partner count as never loaded (finalize then reports the partner by its weight slot): after correcting a
 *       k / v mismatch, load both matrices of that layer again;
 *       any other name on the handle, a head's tensors included, is KR_EINVAL at finalize, and these names' decoder-only rows on another handle likewise;
 *     - the forwards take KR_POOL_MEAN and KR_POOL_LAST; KR_POOL_CLS / KR_POOL_SPLADE are KR_EINVAL, and so is KR_POOL_CLASSIFY unless the handle holds
 *       the score head ("score.weight", below: the one head's tensor a decoder handle takes).
 *   "config.head_dim": data = ONE float, 32, 64 or 128: the head width d_h of a decoder handle where it is a config field of its own (transformers Qwen3Model:
 *   Qwen3-Embedding-0.6B, Qwen3-Reranker-0.6B); anything else is KR_EINVAL, and so is the setting on a handle without "config.decoder_attention" (at finalize).
 *   Send it before "config.rotary_inv_freq" — which then takes d_h / 2 values — and before the weights (behind a layer's attention tensors it is KR_EINVAL);
 *   the usual rule of the settings holds.  Never loaded: d_h = hidden / heads and the handle is what it always was.  With it
 *     - q and the context are Dq = heads * d_h wide, a multiple of 128 up to 4096 (else KR_EINVAL at finalize): "layers.N.self_attn.q_proj.weight" is
 *       [Dq, hidden], "o_proj.weight" [hidden, Dq], "k_proj.weight" / "v_proj.weight" [A, hidden] with A = kv_heads * d_h <= Dq, kv_heads a divisor of heads and
 *       A % 64 == 0; any other element count is KR_EINVAL at load, naming the tensor.  kr_bert_cfg is unchanged: hidden / heads must still be 32 or 64 at
 *       kr_encoder_create, so Qwen3-0.6B (1024 / 16 = 64, d_h = 128) loads and Qwen3-1.7B (2048 / 16) does not;
 *     - "layers.N.self_attn.q_norm.weight" and "layers.N.self_attn.k_norm.weight", fp32 [d_h] each, are the RMS norms Qwen3 applies to every head of q and of
 *       k behind the projection and in front of the rotation: x * rsqrt(mean(x^2) + ln_eps) * weight over the head's d_h features.  Decoder handles only
 *       (with or without "config.head_dim"), every layer's two or none (a partial set is KR_ESTATE at finalize, naming the missing tensor), never next to a
 *       q_proj / k_proj bias, fixed at the first finalize like a head.  The value 128 needs them (KR_EINVAL at finalize without).  Such a handle runs one more
 *       kernel per layer, in place on q and k; 128-wide heads run a kernel of their own (k_attn_wide) at every sequence length.
 *   "config.deberta_position_buckets" + "config.deberta_max_relative_positions": data = ONE float each, Bk (even, 2 .. 256) and M (M - 1 > Bk / 2):
 *   DebertaV2Config's position_buckets and max_relative_positions (max_position_embeddings where that is < 1).  The two together, loaded before the first
 *   finalize, make the handle a DeBERTa handle (DebertaV2Model: microsoft/deberta-v3-* and their fine-tunes) for life; the usual rule of the settings holds
 *   (later the same value is a no-op, another is KR_EINVAL); one without the other, or either next to any other position scheme, is KR_EINVAL at finalize;
 *   max_pos <= 8192.  On such a handle
 *     - the stack is BERT's post-LN layer with erf-GELU; the embedding is LayerNorm(word[id]): no position table and no token-type table are required (a
 *       position table is refused), type_vocab = 1;
 *     - every attention score is (q_i . k_j + q_i . PK[p] + k_j . PQ[p]) / sqrt(3 d_h), p = clamp(delta(c_i - c_j) + Bk, 0, 2 Bk - 1), c = the token's column
 *       in the padded [B, S] batch, delta(r) = r for |r| <= Bk / 2, else sign(r) (ceil(ln(|r| / mid) / ln((M - 1) / mid) (mid - 1)) + mid), mid = Bk / 2
 *       (make_log_bucket_position); PQ = query_proj(R), PK = key_proj(R) with the layer's OWN projections, biases included (share_att_key), R =
 *       LayerNorm(rel_embeddings) or, without "encoder.LayerNorm.*", the raw table.  PQ / PK are built at finalize; only column differences enter, so a
 *       sequence gives the same rows under right and left padding;
 *     - DebertaV2Model's state dict loads unchanged: "embeddings.word_embeddings.weight", "embeddings.LayerNorm.{weight,bias}",
 *       "encoder.layer.N.attention.self.{query_proj,key_proj,value_proj}.{weight,bias}", every other layer tensor under BERT's names,
 *       "encoder.rel_embeddings.weight" [2 Bk, hidden] (missing: KR_ESTATE "never loaded"; another row count: KR_EINVAL) and "encoder.LayerNorm.{weight,bias}"
 *       [hidden] (both or neither).  These names on a handle of another kind, and other families' names for q / k / v on this one, are KR_EINVAL at
 *       finalize, naming the tensor;
 *     - pools 0, 1 and (with the head below) 2 run through all three forward entry points, kr_encoder_forward_packed included; S <= max_pos; under CLS
 *       pooling / classify a row whose column 0 is masked is finite but has no HF counterpart (HF attends uniformly over masked columns there);
 *     - "classifier.dense.*" / "classifier.out_proj.*" (below) are accepted and compute DebertaV2ForSequenceClassification's ContextPooler + classifier:
 *       logits = out_proj.weight . gelu(dense.weight . x + dense.bias) + out_proj.bias — erf-GELU where BERT's head has tanh; bge-m3's heads, the MLM head
 *       and "dense.weight" are refused;
 *     - the workspace holds heads x 2 x W fp32 position scores per token (W <= 512: the buckets the batch's S reaches, rounded up to 32), the handle one
 *       fp32 copy of every layer's query_proj / key_proj matrix.
 * Sequence classification (cross-encoder rerankers: BAAI/bge-reranker-base / -large / -v2-m3 = XLMRobertaForSequenceClassification,
 * cross-encoder/ms-marco-MiniLM-L-6-v2 / -L-12-v2 / ms-marco-TinyBERT = BertForSequenceClassification): the head travels under ONE spelling,
 * RobertaClassificationHead's,
 *   "classifier.dense.weight" [hidden, hidden], "classifier.dense.bias" [hidden], "classifier.out_proj.weight" [L, hidden], "classifier.out_proj.bias" [L],
 *   fp32, 1 <= L <= 64 (L = the rows of out_proj; any other count is KR_EINVAL).  All four or none: a partial set fails kr_encoder_finalize as "never loaded".
 *   With the head, pool = KR_POOL_CLASSIFY is accepted by the three forward entry points and writes out [B, L] fp32,
 *       logits = out_proj.weight . tanh(dense.weight . x + dense.bias) + out_proj.bias,     x = last_hidden[:, 0] (NOT normalised),
 *   raw logits (a sigmoid / softmax is the caller's), fp32 arithmetic throughout; a sequence's logits do not depend on the batch around it.  For the packing
 *   front end, the attention kernel choice and the last layer on the CLS rows it behaves exactly as KR_POOL_CLS; an all-masked sequence gives a NaN row; a
 *   non-finite CLS row is reported as KR_ERANGE like a non-finite embedding.  Pools 0 and 1 on such a handle run as on a handle without the head and still
 *   write [B, hidden].  KR_POOL_CLASSIFY on a handle without the head is KR_ESTATE, naming the missing tensors.  The head follows the rule of "dense.weight":
 *   fixed at the first finalize — later the same L takes new values, another L, or any of the four on a handle finalized without them, is KR_EINVAL.
 *   kr_encoder_finalize refuses it (KR_EINVAL, naming it) on NomicBert, ModernBert and T5 handles — their classification heads are other functions — and next
 *   to "dense.weight".  BertForSequenceClassification's spelling of the same arithmetic (pooler.dense.* -> tanh -> classifier.{weight,bias}) is mapped onto
 *   these names by the Python layer (kirag_amd.retriever.rerankers.BertReranker); the library itself keeps ignoring "pooler.*".
 * ModernBertForSequenceClassification (Alibaba-NLP/gte-reranker-modernbert-base, ibm-granite/granite-embedding-reranker-english-r2, CrossEncoder fine-tunes of
 * answerdotai/ModernBERT-*): on ModernBert handles the head travels under HF's own names, fp32,
 *   "head.dense.weight" [hidden, hidden], "head.norm.weight" [hidden], "classifier.weight" [L, hidden], "classifier.bias" [L], 1 <= L <= 64: together or not at
 *   all (a partial set fails kr_encoder_finalize with KR_ESTATE as "never loaded", naming the missing tensor); "head.dense.bias" [hidden] (classifier_bias) and
 *   "head.norm.bias" [hidden] (norm_bias): optional, zero unless loaded.  L outside 1 .. 64, a "classifier.weight" count that is no multiple of hidden or a
 *   "classifier.bias" count other than L is KR_EINVAL at load.  With the head, KR_POOL_CLASSIFY writes out [B, L] fp32,
 *       logits = classifier.weight . LayerNorm_{ln_eps}(erf_gelu(head.dense.weight . x + head.dense.bias)) + classifier.bias     (head.norm's weight and bias),
 *   raw logits in fp32 arithmetic that do not depend on the batch around a sequence, its slot or the entry point.
 *   "config.classifier_pooling": data = ONE float selecting x: 0 (the default) = last_hidden[:, 0], the forward of KR_POOL_CLS up to the pooled row; 1 = the
 *   masked mean, the forward of KR_POOL_MEAN up to the pooled row (kr_encoder_forward_packed then packs without a CLS query row); x is NOT normalised.  Any
 *   other number is KR_EINVAL.  Accepted before the first finalize; later the same value is a no-op and another value is KR_EINVAL.  kr_encoder_finalize
 *   refuses it (KR_EINVAL, naming it) on a handle without this head or of another kind.
 *   An all-masked sequence gives a NaN row; a non-finite pooled row or logit of a sequence with attended tokens is KR_ERANGE.  Pools 0 and 1 write the
 *   [B, hidden] rows of a handle without the head.  The rule of "classifier.*" above holds: fixed at the first finalize — the same L takes new values, another
 *   L or a head arriving on a handle finalized without one is KR_EINVAL.  KR_POOL_CLASSIFY without the head is KR_ESTATE, naming the four required tensors.
 *   kr_encoder_finalize refuses these six names (KR_EINVAL, naming the tensor) on a handle of any other kind; RobertaClassificationHead's four names stay
 *   refused on ModernBert handles.
 * Qwen2ForSequenceClassification / LlamaForSequenceClassification / MistralForSequenceClassification (decoder-LLM cross-encoders, and causal-LM "yes / no"
 * rerankers folded into one label by the Python layer): on decoder handles ("config.decoder_attention" 1 or 0) the head is ONE tensor, fp32, without a bias,
 *   "score.weight" [L, hidden], 1 <= L <= 64 (any other count is KR_EINVAL at load).  With it, pool = KR_POOL_CLASSIFY is accepted by the three forward
 *   entry points (kr_encoder_forward_packed included: decoder pairs carry no token types) and writes out [B, L] fp32,
 *       logits = score.weight . x,     x = the final-norm row of the sequence's HIGHEST ATTENDED COLUMN (KR_POOL_LAST's row, NOT normalised),
 *   raw logits, fp32 arithmetic, independent of the batch around a sequence and of the entry point.  HF picks the rightmost column whose id is not
 *   pad_token_id; the two agree whenever attention_mask == (input_ids != pad_token_id), and the library follows the mask.  Only that row is read behind the
 *   last layer, so its out-projection, norms and feed-forward run on B gathered rows (KIRAG_AMD_CLS_FULL=1 at create: on every row, same bits); after such a
 *   forward kr_encoder_last_hidden is KR_ESTATE.  KR_POOL_MEAN and KR_POOL_LAST run as on a handle without the head and write [B, hidden].  An all-masked
 *   sequence gives a NaN row; a non-finite logit of a sequence with attended tokens is KR_ERANGE.  KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT on it stay
 *   KR_EINVAL.  The rule of "classifier.*" holds: fixed at the first finalize — the same L takes new values, another L, or the tensor arriving on a handle
 *   finalized without it, is KR_EINVAL — and a decoder handle WITHOUT it keeps refusing KR_POOL_CLASSIFY with KR_EINVAL.  kr_encoder_finalize refuses
 *   "score.weight" (KR_EINVAL, naming it) on a handle of any other kind.
 * The tail of a sentence-transformers pipeline (what a checkpoint folder's modules.json states behind the transformer: Pooling, an optional Dense, Normalize or
 * not), on handles of EVERY family and through all three forward entry points.  Three settings, under the usual rule (accepted before the first finalize;
 * later the same value is a no-op and another is KR_EINVAL), ONE float each:
 *   "config.normalize_output": 1 (also when never loaded) = the row of KR_POOL_MEAN / KR_POOL_CLS / KR_POOL_LAST — and the output of the Dense head below — is
 *       divided by its norm; 0 = it is written as pooled (checkpoints trained for the dot product: facebook/contriever, msmarco-distilbert-base-tas-b,
 *       multi-qa-mpnet-base-dot-v1).  The norm is formed either way: a non-finite row of a sequence with attended tokens stays KR_ERANGE.
 *   "config.pool_tokens": what a KR_POOL_MEAN forward makes of the attended tokens: 0 (also when never loaded) = their mean, 1 = the element-wise max,
 *       2 = sum / sqrt(n) (sentence-transformers' mean_sqrt_len_tokens).  KR_POOL_CLS and KR_POOL_LAST keep their row.  A sequence without attended tokens
 *       gives a NaN row under all three and raises no error.
 *   "config.st_dense_activation": 0 (also when never loaded) = identity, 1 = tanh: the activation of the head below; KR_EINVAL at finalize on a handle without
 *       it, and after the first finalize it is known to handles with the head only.
 *   Any other number, or more than one, is KR_EINVAL at load.
 *   "st_dense.weight" [P, hidden], P % 4 == 0 and 4 <= P <= 2048 (any other count is KR_EINVAL at load), and "st_dense.bias" [P], optional, zero unless loaded
 *   (alone it fails kr_encoder_finalize as "'st_dense.weight' was never loaded"): sentence-transformers' Dense module.  With it the three pools above write
 *   out [B, P] fp32,
 *       out = act(st_dense.weight . x + st_dense.bias),     x = the pooled row, NOT normalised,
 *   then divided by its norm (F.normalize's 1e-12 floor) unless "config.normalize_output" is 0; fp32 arithmetic in an order that does not depend on the batch
 *   around a sequence; a NaN pooled row stays NaN, a non-finite output of a sequence with attended tokens is KR_ERANGE.  The rule of every head holds: fixed at
 *   the first finalize — the same P takes new values, another P, or the head arriving on a handle finalized without it, is KR_EINVAL.
 *   kr_encoder_finalize refuses the three settings and the head (KR_EINVAL, naming both sides) on a handle that holds ANY other head: the MLM head, bge-m3's two,
 *   "dense.weight", the three classification heads.  (A T5 checkpoint whose Dense has no bias and no activation keeps "dense.weight".)
 * BAAI/bge-m3's sparse and multi-vector heads (an XLM-R backbone; the same two Linear modules on a BERT backbone are accepted too), fp32:
 *   "colbert_linear.weight" [P, hidden], "colbert_linear.bias" [P]: P % 128 == 0 and 128 <= P <= 2048, any other count is KR_EINVAL;
 *   "sparse_linear.weight" [1, hidden], "sparse_linear.bias" [1].
 *   The two heads are independent; each is weight + bias or nothing (a partial pair fails kr_encoder_finalize as "never loaded").  They follow the rule of
 *   "classifier.*" and "dense.weight": a head is fixed at the first finalize — later the same P takes new values, another P, or a head arriving on a handle
 *   that was finalized without it, is KR_EINVAL.  kr_encoder_finalize refuses them (KR_EINVAL, naming the tensor) on MPNet, NomicBert, ModernBert and T5
 *   handles, next to "classifier.*" and next to "dense.weight".  With x[b, s] = the row of last_hidden_state,
 *       KR_POOL_WITH_SPARSE:   w[b, s] = max(0, sparse_linear.weight . x[b, s] + bias)                    out block [B, S]
 *       KR_POOL_WITH_COLBERT:  v[b, s] = normalize(colbert_linear.weight . x[b, s] + bias)                out block [B, S, P]   (F.normalize, 1e-12 floor)
 *   for an attended column and +0.0 for a masked one.  Columns are those of the padded [B, S] input (left padding and masks with holes place rows where
 *   their columns are); column 0 (<s> / [CLS]) is written like any attended column — dropping it is the caller's business —, and the extra query row
 *   that CLS pooling packs for a MASKED column 0 is never emitted.  A flagged forward runs its last layer on every row (the CLS-rows-only shortcut is off);
 *   its dense block still equals the unflagged call bit for bit.  The colbert product runs on the MFMA projection loops from the 16-bit rows the stack itself
 *   reads (a 16-bit copy of the weight, fp32 accumulation) and is STORED IN THE HANDLE'S 16-BIT OPERAND TYPE, like every projection output of the stack (f16: 11
 *   significand bits, bf16: 8), before bias, norm and division run in fp32: the head is not fp32 end to end, and on a bf16 handle a vector's elements carry that
 *   rounding (measured figures for both types: profiles/m3/measurements.txt).  The sparse dot product reads the final rows with their low
 *   half, in fp32 with a fixed order.  A token's weight and vector do not depend on the batch around it.  A non-finite weight or vector of an attended
 *   token is reported as KR_ERANGE like a non-finite embedding.  A device `out` receives the token-level blocks straight from the kernels; a host `out` is
 *   staged on the device.  kr_encoder_forward_packed refuses the flags: the corpus pipeline behind it stores no token vectors, so the refusal costs nothing.
 * SPLADE's MLM head (transformers.BertForMaskedLM: naver/splade-cocondenser-ensembledistil, naver/splade-v3, ...), fp32, V = cfg.vocab:
 *   "cls.predictions.transform.dense.weight" [hidden, hidden], "cls.predictions.transform.dense.bias" [hidden],
 *   "cls.predictions.transform.LayerNorm.weight" [hidden], "cls.predictions.transform.LayerNorm.bias" [hidden],
 *   "cls.predictions.decoder.weight" [V, hidden], "cls.predictions.decoder.bias" [V]: any other row count is KR_EINVAL.
 *   The decoder weight is loaded explicitly — that HF ties it to the word table is the caller's business ("cls.predictions.bias" is HF's alias of the decoder
 *   bias: send one).  All six or none (a partial set fails kr_encoder_finalize as "never loaded"); under the rule of "classifier.*" the head is fixed at the
 *   first finalize — later the same shapes take new values, a head arriving on a handle finalized without it is KR_EINVAL.  kr_encoder_finalize refuses it
 *   (KR_EINVAL, naming the tensor) on MPNet, NomicBert, ModernBert and T5 handles, next to "classifier.*", next to "dense.weight" and next to bge-m3's heads.
 *   With x[b, s] = the row of last_hidden_state, the LayerNorm at cfg.ln_eps and the erf-GELU of the stack:
 *       t      = LayerNorm(gelu(transform.dense.weight . x + bias))
 *       w[b,v] = max over the ATTENDED tokens s of log(1 + relu(decoder.weight[v] . t[b, s] + decoder.bias[v]))          out [B, V]
 *   computed as log1p(max(0, bias[v] + max_s acc[b, s, v])) — log1p(relu(.)) is monotone —: the decoder runs on the MFMA projection loops over a 16-bit copy
 *   [Vpad, hidden] of the weight (V rounded up to a multiple of 128 by zero rows that never reach `out`; t is rounded to the 16-bit operand type like every
 *   activation of the stack) and its epilogue reduces the fp32 accumulators over the rows of each sequence: no [tokens, V] logits exist in any precision.
 *   The last layer runs on every row; packing and attention are those of KR_POOL_MEAN.  A sequence without attended tokens yields V times +0.0.  The
 *   result is exact in the sense that max is: a sequence's row does not depend on the batch, the tiling or the call.  A non-finite value (NaN / Inf in the head's
 *   weights, a non-finite row of t) is reported as KR_ERANGE like a non-finite embedding.  A device `out` is the reduction buffer itself; a host `out` is staged.
 *   (The definition is recalled from naver's Splade module and sentence-transformers' SpladePooling("max"); neither was at hand to compare against.) */
int kr_encoder_load_weight(kr_encoder* enc, const char* hf_name, const float* data, int64_t numel);
/* verifies every tensor was supplied and builds the fused/packed device copies */
int kr_encoder_finalize(kr_encoder* enc);
/* forward(input_ids, attention_mask) (encoders.py:67-77 / :106-118); token_type_ids are 0 as in every caller.
 *   input_ids, attention_mask [B,S] int64 (S <= max_pos), out [B,hidden] fp32 L2-normalised ([B,P] on a handle that was given "dense.weight" [P, hidden];
 *   [B,L] raw logits with pool = KR_POOL_CLASSIFY; [B,vocab] with pool = KR_POOL_SPLADE; with KR_POOL_WITH_SPARSE / KR_POOL_WITH_COLBERT the blocks [B,hidden] | [B,S] | [B,S,P], see above).
 *   A sequence whose mask is all zero yields NaN (mean pool) exactly like the reference. */
int kr_encoder_forward(kr_encoder* enc, const int64_t* input_ids, const int64_t* attention_mask, int B, int S,
                       int pool, float* out, void* stream);
/* The same with token_type_ids [B,S] int64 (HF BertModel.forward's third input; NULL = all zero = kr_encoder_forward).  No KiRAG caller passes non-zero
 * types (the collators encode single texts), but the encoders' forward signature has the argument (encoders.py:67,106).  A value outside
 * [0, type_vocab) is reported as KR_EINVAL through the same deferred channel as token ids.  out is [B,P] on a handle with "dense.weight" [P, hidden]. */
int kr_encoder_forward_tt(kr_encoder* enc, const int64_t* input_ids, const int64_t* attention_mask, const int64_t* token_type_ids, int B, int S,
                          int pool, float* out, void* stream);
/* The same forward from RAGGED input: token_ids = int32 ids of the attended positions of every sequence back to back (total_tokens of them, host or device),
 * seq_lens [B] int32 = how many belong to each sequence, occupying positions 0 .. len-1 - what the reference's collator yields for a right-padding tokenizer
 * (dataset/collators.py:59-81, padding=True: input_ids[b, :len], attention_mask[b] = 1^len 0^(S-len)) without the padding: 4-16x fewer bytes from the tokenizer
 * processes of compute_corpus_embeddings.py:77-81 to the GPU.  S = the padded width the equivalent [B,S] call would have (>= every length, <= max_pos; it selects
 * the attention kernel exactly as kr_encoder_forward does).  Rows are BIT-IDENTICAL to kr_encoder_forward on the equivalent padded batch (the same kernels run
 * on the same packed token tables).  A length outside [0, S] or lengths that do not add up to total_tokens are reported as KR_EINVAL through the deferred
 * channel below (the sequence is read as empty, nothing is read out of bounds); an empty sequence yields NaN (mean pool) like an all-zero mask.
 * out is [B,P] on a handle with "dense.weight" [P, hidden]. */
int kr_encoder_forward_packed(kr_encoder* enc, const int32_t* token_ids, const int32_t* seq_lens, int B, int S, int64_t total_tokens, int pool, float* out,
                              void* stream);
/* kr_encoder_forward with a DEVICE `out` pointer only enqueues work on `stream` and returns (no host synchronisation); with a host `out`
 * it returns when the result is in the caller's buffer.  The one thing a forward can get wrong at run time - a token id outside [0, vocab)
 * - is recorded by the kernels (the offending token is read as id 0) and reported as KR_EINVAL by the host-output call itself, or, for
 * device-output calls, by the NEXT call on the handle once that forward has finished, or by kr_encoder_check(), which waits for it.
 * The same channel reports KR_ERANGE when a LayerNorm row of the forward was not finite: with f16 operands (the default) an activation beyond
 * +-65504 becomes inf and the embedding NaN; nothing saturates silently. */
int kr_encoder_check(kr_encoder* enc);
/* debugging / parity: last_hidden_state of the previous forward, fp32 [B*S_packed...] see DESIGN.md */
int kr_encoder_last_hidden(kr_encoder* enc, float* out /* [B,S,hidden] */, int B, int S);

#ifdef __cplusplus
}
#endif
#endif /* KIRAG_AMD_H */
