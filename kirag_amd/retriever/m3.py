"""BAAI/bge-m3's three outputs from ONE forward of the HIP encoder — the dense ``<s>`` vector, a learned sparse weight per token (``sparse_linear``, H -> 1,
ReLU) and a normalised vector per token (``colbert_linear``, H -> P, scored by MaxSim) — and hybrid M3 scoring on top of them.

``XLMRobertaM3Encoder`` / ``BertM3Encoder`` ARE the sentence encoders of ``kirag_amd.retriever.encoders`` (CLS pooling) with the two ``nn.Linear`` heads as
sub-modules: ``named_parameters()`` carries ``colbert_linear.{weight,bias}`` / ``sparse_linear.{weight,bias}`` through the ordinary weight sync, and
``forward_m3`` asks the library for the extra blocks (``KR_POOL_WITH_SPARSE`` / ``KR_POOL_WITH_COLBERT``, ``include/kirag_amd.h``).  ``BGEM3Model`` is the
user-facing object: ``encode``, ``compute_score``, ``rerank``, and — over an ``Indexer`` and a ``late.MultiVectorStore`` — ``index_passages`` / ``retrieve``;
over a ``sparse_index.SparseIndexer``, ``retrieve_sparse``; over all three, ``retrieve_hybrid`` (the weighted ``colbert+sparse+dense`` of the dense top-n, from the
stored forms) and ``retrieve_rrf`` (rank fusion of the dense and the sparse ranking, ``fusion.rrf``).

UNVERIFIED OFFLINE.  FlagEmbedding is not a dependency of this project and was not at hand when this was written: the arithmetic below is THIS PROJECT'S
definition, recalled from ``FlagEmbedding.BGEM3FlagModel``, not checked against it.  The recalled points:

  * the ``[:, 1:]`` slice: token vectors are those of columns 1 .. len - 1 of a right-padded row (without ``<s>``, with ``</s>``);
  * the special-token exclusion: ``lexical_weights`` skips the tokenizer's cls / eos / pad / unk ids (and weights <= 0) and keeps the max per token id;
  * MaxSim: ``colbert_score = mean over query tokens of max over passage tokens of q_i . p_j``;
  * the weight normalisation: a combined score is the weighted sum of its parts divided by the sum of their weights;
  * the file names ``colbert_linear.pt`` / ``sparse_linear.pt``: torch state dicts with ``weight`` / ``bias`` next to the backbone's files.

No real bge-m3 weights were available either: real-checkpoint numerics are unmeasured (``tools/checkpoint_check.py <dir>`` measures them).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from transformers import PretrainedConfig

from .encoders import (POOL_CLS, POOL_WITH_COLBERT, POOL_WITH_SPARSE, ROBERTA_TYPES, BGEEncoder, XLMRobertaBGEEncoder, _st_file, check_colbert_dim,
                       checkpoint_model_type)

COLBERT_FILE, SPARSE_FILE = "colbert_linear.pt", "sparse_linear.pt"
SCORE_KEYS = ("dense", "sparse", "colbert", "sparse+dense", "colbert+sparse+dense")


def check_head_state(name: str, state: Dict[str, Tensor], hidden: int) -> Tuple[Tensor, Tensor]:
    """``weight`` / ``bias`` of a head file (``name``: ``colbert_linear`` or ``sparse_linear``) as fp32, refused by field before a handle exists: a weight that
    does not read the backbone's hidden size, a colbert width outside the library's rule, a sparse head with more than one output, a bias of another length."""
    if "weight" not in state or "bias" not in state:
        raise ValueError(f"{name}: the state dict holds {sorted(state)}, expected 'weight' and 'bias'")
    w, b = state["weight"].float(), state["bias"].float()
    if w.dim() != 2 or w.shape[1] != hidden:
        raise ValueError(f"{name}.in_features={tuple(w.shape)[-1]}: the head must read the backbone's hidden_size={hidden}")
    if name == "colbert_linear":
        check_colbert_dim(int(w.shape[0]))
    elif w.shape[0] != 1:
        raise ValueError(f"sparse_linear.out_features={w.shape[0]}: one weight per token is implemented")
    if tuple(b.shape) != (w.shape[0],):
        raise ValueError(f"{name}.bias has shape {tuple(b.shape)}, its weight has {w.shape[0]} rows")
    return w, b


class _M3HeadsMixin:
    """The two heads on a CLS-pooling sentence encoder.  ``colbert_linear`` / ``sparse_linear`` are ``nn.Linear`` sub-modules or ``None`` (head not offered);
    a handle's heads are fixed at its first finalize, so installing or removing one drops the handle."""
    _pool = POOL_CLS
    _model_types: Tuple[str, ...] = ()

    def __init__(self, config, add_pooling_layer=True, **kwargs):
        super().__init__(config, add_pooling_layer, **kwargs)
        self.colbert_linear: Optional[nn.Linear] = None
        self.sparse_linear: Optional[nn.Linear] = None

    def set_heads(self, colbert: Optional[Dict[str, Tensor]] = None, sparse: Optional[Dict[str, Tensor]] = None) -> None:
        """install the heads from state dicts (``weight`` / ``bias``); ``None`` removes that head"""
        H = int(self.config.hidden_size)
        p = next(self.parameters())
        for name, state in (("colbert_linear", colbert), ("sparse_linear", sparse)):
            if state is None:
                setattr(self, name, None)
                continue
            w, b = check_head_state(name, state, H)
            lin = nn.Linear(H, int(w.shape[0]), device=p.device, dtype=p.dtype)
            with torch.no_grad():
                lin.weight.copy_(w); lin.bias.copy_(b)
            setattr(self, name, lin)
        self._hip = None

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, **kwargs):
        model_type, config = checkpoint_model_type(pretrained_model_name_or_path, kwargs)
        if model_type not in cls._model_types:
            raise NotImplementedError(f"model_type={model_type!r}: {cls.__name__} runs {cls._model_types} checkpoints (bge-m3's heads on other families are not "
                                      "implemented)")
        states = {}
        for name, fname in (("colbert_linear", COLBERT_FILE), ("sparse_linear", SPARSE_FILE)):
            path = _st_file(pretrained_model_name_or_path, fname, kwargs)
            if path is None:
                continue
            state = torch.load(path, map_location="cpu", weights_only=True)
            hidden = int(config.hidden_size if isinstance(config, PretrainedConfig) else config["hidden_size"])
            check_head_state(name, state, hidden)         # refused before the backbone is read
            states[name] = state
        model = super().from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        model.set_heads(states.get("colbert_linear"), states.get("sparse_linear"))
        return model

    def save_pretrained(self, save_directory, *args, **kwargs):
        heads = {"colbert_linear": self.colbert_linear, "sparse_linear": self.sparse_linear}
        self.colbert_linear = self.sparse_linear = None     # the backbone's own files hold the backbone's state dict and nothing else
        try:
            out = super().save_pretrained(save_directory, *args, **kwargs)
        finally:
            self.colbert_linear, self.sparse_linear = heads["colbert_linear"], heads["sparse_linear"]
        for name, fname in (("colbert_linear", COLBERT_FILE), ("sparse_linear", SPARSE_FILE)):
            lin = heads[name]
            if lin is not None:
                torch.save({"weight": lin.weight.detach().float().cpu().contiguous(), "bias": lin.bias.detach().float().cpu().contiguous()},
                           os.path.join(save_directory, fname))
        return out

    @torch.no_grad()
    def forward_m3(self, input_ids: Tensor, attention_mask: Tensor, return_sparse: bool = True, return_colbert: bool = True):
        """ONE HIP forward: ``(dense [B, H], sparse [B, S] or None, colbert [B, S, P] or None)`` on the GPU, views into one tensor.  Token-level blocks are laid
        out by the columns of the padded input; masked columns are zero; column 0 is present.  Eval mode only."""
        if self.training:
            raise RuntimeError("forward_m3 is the inference (HIP) path: call model.eval() first")
        if return_sparse and self.sparse_linear is None:
            raise ValueError("return_sparse: this checkpoint has no sparse_linear head")
        if return_colbert and self.colbert_linear is None:
            raise ValueError("return_colbert_vecs: this checkpoint has no colbert_linear head")
        pool = self._pool | (POOL_WITH_SPARSE if return_sparse else 0) | (POOL_WITH_COLBERT if return_colbert else 0)
        hip = self._synced_hip()
        with torch.cuda.device(hip.device_index):
            out = hip.forward(input_ids, attention_mask, pool)
        return out if isinstance(out, tuple) else (out, None, None)


class XLMRobertaM3Encoder(_M3HeadsMixin, XLMRobertaBGEEncoder):
    """XLMRobertaModel -> ``<s>`` row + sparse_linear + colbert_linear (BAAI/bge-m3)"""
    _model_types = ROBERTA_TYPES


class BertM3Encoder(_M3HeadsMixin, BGEEncoder):
    """BertModel -> ``[CLS]`` row + the same two heads (an M3-style fine-tune of a BERT backbone)"""
    _model_types = ("bert",)
    _dispatch_by_model_type = False  # no dispatch to another family's class: from_pretrained refuses other model types by name


def build_lexical_weights(token_ids: Sequence[int], weights: Sequence[float], skip_ids) -> Dict[str, float]:
    """``str(token_id) -> max weight`` over one sequence's attended tokens, without the ids in ``skip_ids`` and without weights <= 0"""
    out: Dict[str, float] = {}
    skip = set(int(i) for i in skip_ids if i is not None)
    for i, w in zip(token_ids, weights):
        i, w = int(i), float(w)
        if i in skip or not w > 0.0:
            continue
        k = str(i)
        if w > out.get(k, 0.0):
            out[k] = w
    return out


def compute_lexical_matching_score(lw_a: Dict[str, float], lw_b: Dict[str, float]) -> float:
    """sum of ``w_a * w_b`` over the token ids both hold"""
    if len(lw_b) < len(lw_a):
        lw_a, lw_b = lw_b, lw_a
    return float(sum(w * lw_b[k] for k, w in lw_a.items() if k in lw_b))


def colbert_score(q_vecs, p_vecs, device=None) -> float:
    """MaxSim: ``mean_i max_j q_i . p_j`` over the query's token vectors ``[n_q, P]`` and the passage's ``[n_p, P]`` (torch, on ``device``)"""
    q = torch.as_tensor(np.asarray(q_vecs) if not isinstance(q_vecs, Tensor) else q_vecs, dtype=torch.float32)
    p = torch.as_tensor(np.asarray(p_vecs) if not isinstance(p_vecs, Tensor) else p_vecs, dtype=torch.float32)
    if device is not None:
        q, p = q.to(device), p.to(device)
    if q.shape[0] == 0 or p.shape[0] == 0:
        return 0.0
    return float((q @ p.T).max(dim=1).values.mean())


def combine_scores(dense: float, sparse: float, colbert: float, weights: Sequence[float]) -> Dict[str, float]:
    """the five scores of one pair: each combination is the weighted sum of its parts divided by the sum of their weights"""
    wd, ws, wc = (float(w) for w in weights)
    return {"dense": dense, "sparse": sparse, "colbert": colbert,
            "sparse+dense": (wd * dense + ws * sparse) / (wd + ws),
            "colbert+sparse+dense": (wd * dense + ws * sparse + wc * colbert) / (wd + ws + wc)}


class BGEM3Model:
    """``encode`` / ``compute_score`` / ``rerank`` over an M3 encoder.  ``model_name_or_path``: a checkpoint folder (its ``model_type`` picks the twin) or an
    already built ``XLMRobertaM3Encoder`` / ``BertM3Encoder``."""

    def __init__(self, model_name_or_path, tokenizer=None, normalize_embeddings: bool = True, device=None, **kwargs):
        if not normalize_embeddings:
            raise ValueError("normalize_embeddings=False: the library's dense block is L2-normalised")
        if isinstance(model_name_or_path, nn.Module) or hasattr(model_name_or_path, "forward_m3"):
            self.model = model_name_or_path
        else:
            mt, _ = checkpoint_model_type(model_name_or_path, kwargs)
            if mt in ROBERTA_TYPES:
                cls = XLMRobertaM3Encoder
            elif mt == "bert":
                cls = BertM3Encoder
            else:
                raise NotImplementedError(f"model_type={mt!r}: bge-m3's heads run on 'bert' and {ROBERTA_TYPES} checkpoints")
            self.model = cls.from_pretrained(model_name_or_path, **kwargs)
        self.model_name_or_path = model_name_or_path
        self.tokenizer = tokenizer
        if device is None:
            device = "cuda" if torch.cuda.is_available() else None
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and isinstance(self.model, nn.Module):
            self.model.to(self.device)
        if isinstance(self.model, nn.Module):
            self.model.eval()

    @classmethod
    def from_pretrained(cls, model_name_or_path, **kwargs):
        """the registry's call (``rerankers.load_reranker("BGEM3", path)``)"""
        return cls(model_name_or_path, **kwargs)

    def _tokenizer(self):
        if self.tokenizer is None:
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(self.model_name_or_path)
        if getattr(self.tokenizer, "padding_side", "right") != "right":
            raise ValueError(f"tokenizer.padding_side={self.tokenizer.padding_side!r}: token vectors are the columns 1 .. len - 1 of a RIGHT-padded row")
        return self.tokenizer

    def _skip_ids(self):
        t = self._tokenizer()
        return {i for i in (t.cls_token_id, t.eos_token_id, t.pad_token_id, t.unk_token_id) if i is not None}

    @torch.no_grad()
    def encode(self, sentences, batch_size: int = 32, max_length: int = 512, return_dense: bool = True, return_sparse: bool = False,
               return_colbert_vecs: bool = False) -> dict:
        """``{"dense_vecs": [N, H] or None, "lexical_weights": list of dicts or None, "colbert_vecs": list of [len_i - 1, P] arrays or None}``; one forward per
        batch whatever is asked for."""
        single = isinstance(sentences, str)
        if single:
            sentences = [sentences]
        tok, skip = self._tokenizer(), self._skip_ids()
        dense_all, lex_all, col_all = [], [], []
        for s in range(0, len(sentences), batch_size):
            enc = tok(list(sentences[s:s + batch_size]), padding=True, truncation=True, max_length=max_length, return_tensors="pt")
            ids, mask = enc["input_ids"], enc["attention_mask"]
            dense, sparse, colbert = self.model.forward_m3(ids, mask, return_sparse=return_sparse, return_colbert=return_colbert_vecs)
            if return_dense:
                dense_all.append(dense.float().cpu().numpy())
            lens = mask.sum(dim=1).tolist()
            if return_sparse:
                w = sparse.float().cpu().numpy()
                ids_np = ids.numpy()
                for b, n in enumerate(lens):
                    lex_all.append(build_lexical_weights(ids_np[b, :n], w[b, :n], skip))
            if return_colbert_vecs:
                v = colbert.float().cpu().numpy()
                for b, n in enumerate(lens):
                    col_all.append(np.ascontiguousarray(v[b, 1:n]))
        out = {"dense_vecs": np.concatenate(dense_all) if return_dense else None,
               "lexical_weights": lex_all if return_sparse else None, "colbert_vecs": col_all if return_colbert_vecs else None}
        if single:
            out = {k: (v[0] if v is not None else None) for k, v in out.items()}
        return out

    compute_lexical_matching_score = staticmethod(compute_lexical_matching_score)

    def colbert_score(self, q_vecs, p_vecs) -> float:
        return colbert_score(q_vecs, p_vecs, self.device)

    def _pair_scores(self, q: dict, qi: Sequence[int], p: dict, weights) -> Dict[str, List[float]]:
        out: Dict[str, List[float]] = {k: [] for k in SCORE_KEYS}
        for j, i in enumerate(qi):
            one = combine_scores(float(np.dot(q["dense_vecs"][i].astype(np.float64), p["dense_vecs"][j].astype(np.float64))),
                                 compute_lexical_matching_score(q["lexical_weights"][i], p["lexical_weights"][j]),
                                 self.colbert_score(q["colbert_vecs"][i], p["colbert_vecs"][j]), weights)
            for k in SCORE_KEYS:
                out[k].append(one[k])
        return out

    def compute_score(self, pairs, weights=(1.0, 1.0, 1.0), batch_size: int = 32, max_query_length: int = 512, max_passage_length: int = 512) -> Dict[str, List[float]]:
        """the five score lists of ``(query, passage)`` pairs under FlagEmbedding's keys; ``weights = (w_dense, w_sparse, w_colbert)``"""
        if isinstance(pairs, tuple) and len(pairs) == 2 and isinstance(pairs[0], str):
            pairs = [pairs]
        q = self.encode([a for a, _ in pairs], batch_size, max_query_length, True, True, True)
        p = self.encode([b for _, b in pairs], batch_size, max_passage_length, True, True, True)
        return self._pair_scores(q, range(len(pairs)), p, weights)

    def rerank(self, query: str, passages: List[str], top_k: Optional[int] = None, weights=(1.0, 1.0, 1.0), batch_size: int = 64) -> Tuple[Tensor, Tensor]:
        """The shape of ``BaseReranker.rerank``: ``(indices, scores)`` of the best ``top_k`` passages (all when ``None``) by (``colbert+sparse+dense`` descending,
        index ascending), both on the CPU.  The query is encoded once."""
        assert isinstance(passages, list) and len(passages) > 0   # must provide passages
        q = self.encode([query], 1, 512, True, True, True)
        p = self.encode(passages, batch_size, 512, True, True, True)
        s = np.asarray(self._pair_scores(q, [0] * len(passages), p, weights)[SCORE_KEYS[-1]], dtype=np.float64)
        order = torch.from_numpy(np.lexsort((np.arange(len(s)), -s)))
        if top_k is not None:
            order = order[:top_k]
        return order, torch.from_numpy(s.astype(np.float32))[order]

    # ---- dense top-n from the index, MaxSim over the stored token vectors of those n (kirag_amd.retriever.late) ----
    @torch.no_grad()
    def index_passages(self, ids, passages: Sequence[str], indexer, store, batch_size: int = 64, max_length: int = 512, sparse_index=None) -> None:
        """ONE flagged forward per batch: the dense block goes to ``indexer.index_data`` (an ``Indexer``), the colbert block to ``store.add_block`` (a
        ``MultiVectorStore`` on the encoder's GPU) — the token vectors of columns 1 .. len - 1, converted to float16 and packed on the device.  Neither block
        visits the host.  With a ``sparse_index`` (a ``sparse_index.SparseIndexer``) the same forward also asks for the sparse block and the passages'
        ``lexical_weights`` (``build_lexical_weights``, as ``encode`` builds them) go to ``sparse_index.index_data``; without one, sparse weights are not stored.

        The two containers are kept in step: every id of the call is checked before the first forward (not a decimal number, twice in the call, already in
        the store: ``ValueError``, nothing indexed); a batch the store refuses (a non-finite vector) never reaches the index; a batch the index refuses after
        the store took it is taken out of the store again before the error is passed on.  Batches before the failing one stay in both.  The sparse index is
        the container in the middle: its ids are checked before the first forward too, a batch it refuses is taken out of the store, a batch the index refuses
        is taken out of both."""
        ids = list(ids)
        if len(ids) != len(passages):
            raise ValueError(f"{len(ids)} ids for {len(passages)} passages")
        store.check_new_ids(ids)
        if sparse_index is not None:
            sparse_index.check_new_ids(ids)
        tok = self._tokenizer()
        skip = self._skip_ids() if sparse_index is not None else ()
        for s in range(0, len(passages), batch_size):
            enc = tok(list(passages[s:s + batch_size]), padding=True, truncation=True, max_length=max_length, return_tensors="pt")
            dense, sparse, colbert = self.model.forward_m3(enc["input_ids"], enc["attention_mask"], return_sparse=sparse_index is not None, return_colbert=True)
            batch_ids = ids[s:s + batch_size]
            if sparse_index is not None:
                w, ids_np, lens = sparse.float().cpu().numpy(), enc["input_ids"].numpy(), enc["attention_mask"].sum(dim=1).tolist()
                lex = [build_lexical_weights(ids_np[b, :n], w[b, :n], skip) for b, n in enumerate(lens)]
                if colbert.data_ptr() % 16:       # behind the [B, S] sparse block the colbert view starts where B * S left it; add_block's kernel reads 16-byte pieces
                    colbert = colbert.clone()
            store.add_block(batch_ids, colbert, enc["attention_mask"], skip_first=True)
            taken = [store]
            try:
                if sparse_index is not None:
                    sparse_index.index_data(batch_ids, lex)
                    taken.append(sparse_index)
                indexer.index_data(batch_ids, dense)
            except BaseException:
                for c in taken:
                    c._drop_last(len(batch_ids))
                raise

    def retrieve(self, queries, indexer, store, top_k: int = 10, n_candidates: int = 100, weights=(1.0, 1.0),
                 max_length: int = 512) -> List[Tuple[List[str], np.ndarray]]:
        """Per query: ``indexer.search_knn`` gives ``n_candidates`` ids (at most the index's size) with their exact dense scores, ``store.maxsim`` scores
        those passages' stored token vectors against the query's (all queries in one launch), and the best ``top_k`` by (combined descending, dense rank
        ascending) come back as ``(ids, float32 scores)``; combined = ``(w_d dense + w_c colbert) / (w_d + w_c)``, ``weights = (w_d, w_c)``.  An empty
        index, or ``n_candidates <= 0``, gives every query an empty result.  The sparse head takes no part: its weights are not stored."""
        if isinstance(queries, str):
            queries = [queries]
        wd, wc = (float(w) for w in weights)
        n = min(int(n_candidates), int(indexer.index.ntotal))
        if n <= 0:
            return [([], np.empty(0, np.float32)) for _ in queries]
        q = self.encode(list(queries), max_length=max_length, return_dense=True, return_sparse=False, return_colbert_vecs=True)
        hits = indexer.search_knn(q["dense_vecs"], n, verbose=False)
        colbert = store.maxsim(q["colbert_vecs"], [h[0] for h in hits], reduce="mean")
        out = []
        for (cand, dense), col in zip(hits, colbert):
            s = (wd * np.asarray(dense, np.float64) + wc * col.astype(np.float64)) / (wd + wc)
            order = np.lexsort((np.arange(len(s)), -s))[:top_k]
            out.append(([str(cand[i]) for i in order], s[order].astype(np.float32)))
        return out

    def retrieve_sparse(self, queries, sparse_index, top_k: int = 10, max_length: int = 512) -> List[Tuple[List[str], List[float]]]:
        """Per query the best ``top_k`` stored passages by lexical matching score, exact, over the whole ``sparse_index`` (``SparseIndexer.search_knn``): the
        query's ``lexical_weights`` against the stored ones (rounded to float16).  A passage that shares no token with the query is no result."""
        if isinstance(queries, str):
            queries = [queries]
        q = self.encode(list(queries), max_length=max_length, return_dense=False, return_sparse=True, return_colbert_vecs=False)
        return sparse_index.search_knn(q["lexical_weights"], top_k)

    # ---- all three stored forms: dense top-n, then the exact sparse score and MaxSim of those n (sparse_index.score_pairs, store.maxsim) ----
    def retrieve_hybrid(self, queries, indexer, store, sparse_index, top_k: int = 10, n_candidates: int = 100, weights=(1.0, 1.0, 1.0),
                        max_length: int = 512) -> List[Tuple[List[str], np.ndarray]]:
        """``compute_score``'s ``colbert+sparse+dense`` over the stored forms.  ONE flagged forward encodes the queries (dense, sparse and colbert together);
        per query ``indexer.search_knn`` gives ``n_candidates`` ids (at most the index's size) with their exact dense scores, ``sparse_index.score_pairs``
        gives those passages' lexical matching scores against the stored (float16) weights and ``store.maxsim`` their MaxSim, each in one launch for all
        queries.  The best ``top_k`` by (combined descending, dense rank ascending) come back as ``(ids, float32 scores)``; combined =
        ``(w_d dense + w_s sparse + w_c colbert) / (w_d + w_s + w_c)`` in float64, ``weights = (w_d, w_s, w_c)``.  ``store=None`` gives ``sparse+dense``:
        ``(w_d dense + w_s sparse) / (w_d + w_s)``, ``w_c`` is ignored and the colbert head is not asked for.  An empty index, or ``n_candidates <= 0``, gives
        every query an empty result.  A candidate that one container lacks raises that container's ``KeyError`` before any scoring launch."""
        if isinstance(queries, str):
            queries = [queries]
        wd, ws, wc = (float(w) for w in weights)
        n = min(int(n_candidates), int(indexer.index.ntotal))
        if n <= 0:
            return [([], np.empty(0, np.float32)) for _ in queries]
        q = self.encode(list(queries), max_length=max_length, return_dense=True, return_sparse=True, return_colbert_vecs=store is not None)
        hits = indexer.search_knn(q["dense_vecs"], n, verbose=False)
        cands = [h[0] for h in hits]
        for c in cands:                           # both containers know every candidate before either scores
            sparse_index.rows_of(c)
            if store is not None:
                store._rows(c)
        sparse = sparse_index.score_pairs(q["lexical_weights"], cands)
        colbert = store.maxsim(q["colbert_vecs"], cands, reduce="mean") if store is not None else [None] * len(cands)
        out = []
        for (cand, dense), sp, col in zip(hits, sparse, colbert):
            if col is None:
                s = (wd * np.asarray(dense, np.float64) + ws * sp.astype(np.float64)) / (wd + ws)
            else:
                s = (wd * np.asarray(dense, np.float64) + ws * sp.astype(np.float64) + wc * col.astype(np.float64)) / (wd + ws + wc)
            order = np.lexsort((np.arange(len(s)), -s))[:top_k]
            out.append(([str(cand[i]) for i in order], s[order].astype(np.float32)))
        return out

    def retrieve_rrf(self, queries, indexer, sparse_index, top_k: int = 10, n_candidates: int = 100, k: float = 60.0,
                     store=None) -> List[Tuple[List[str], np.ndarray]]:
        """Reciprocal rank fusion (``fusion.rrf``, constant ``k``) of the dense top-``n_candidates`` ranking (``indexer.search_knn``) and the sparse
        top-``n_candidates`` ranking (``sparse_index.search_knn``; at most 1024).  With a ``store`` a third ranking enters: MaxSim (``reduce="mean"``) over
        the union of the two lists — the dense list, then the sparse ids it lacks — ordered by (colbert descending, position in the union ascending), so a
        candidate only the sparse search found reaches the multi-vector head without a dense score.  Per query ``(ids, float64 scores)`` as ``rrf`` gives
        them, the best ``top_k``.  ``n_candidates <= 0`` gives every query an empty result."""
        from .fusion import rrf
        if isinstance(queries, str):
            queries = [queries]
        n = int(n_candidates)
        if n <= 0:
            return [([], np.empty(0, np.float64)) for _ in queries]
        q = self.encode(list(queries), max_length=512, return_dense=True, return_sparse=True, return_colbert_vecs=store is not None)
        nd = min(n, int(indexer.index.ntotal))
        dense = [h[0] for h in indexer.search_knn(q["dense_vecs"], nd, verbose=False)] if nd > 0 else [[] for _ in queries]
        sparse = [h[0] for h in sparse_index.search_knn(q["lexical_weights"], n)]
        rankings = [[[str(i) for i in d], [str(i) for i in s]] for d, s in zip(dense, sparse)]
        if store is not None:
            unions = []
            for d, s in rankings:
                have = set(d)
                unions.append(d + [i for i in s if i not in have])
            for r, u, col in zip(rankings, unions, store.maxsim(q["colbert_vecs"], unions, reduce="mean")):
                order = np.lexsort((np.arange(len(col)), -col.astype(np.float64)))
                r.append([u[i] for i in order])
        return [rrf(r, k=k, top_k=top_k) for r in rankings]
