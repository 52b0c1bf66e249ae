"""SPLADE, the learned sparse encoder, on the HIP encoder: a ``BertForMaskedLM`` checkpoint (naver/splade-cocondenser-ensembledistil, naver/splade-v3,
prithivida/Splade_PP_en_v1, opensearch-project/opensearch-neural-sparse-encoding-v1) turned into ONE vocabulary-sized non-negative vector per text,

    t      = LayerNorm(gelu(Wt . x + bt))                                        cls.predictions.transform
    logit  = Wd . t + bd                                                         cls.predictions.decoder (tied to the word embeddings)
    w[b,v] = max over the ATTENDED tokens s of log(1 + relu(logit[b, s, v]))     -> [B, vocab_size]

from one forward of ``libkirag_amd.so`` (``KR_POOL_SPLADE``, ``include/kirag_amd.h``): the ``[tokens, vocab]`` logits never exist, the decoder's epilogue
reduces them over each sequence's rows.

``BertSpladeEncoder`` IS ``transformers.BertForMaskedLM`` (``from_pretrained`` / ``save_pretrained`` / ``.to()`` keep working, ``forward`` stays HF's own and
returns token logits — that is what ``train()`` mode uses); ``forward_splade`` is the inference path, eval mode and GPU only, no CPU fallback.  ``SpladeModel`` is
the user-facing object in the shape of ``BGEM3Model``: ``encode``, ``encode_dense``, ``compute_score``, ``rerank``, ``index_passages``, ``retrieve``.

UNVERIFIED OFFLINE.  Neither naver's ``splade`` package nor ``sentence_transformers`` is a dependency of this project, and neither was at hand when this was
written: the formula above is recalled from naver's ``Splade`` module and from sentence-transformers' ``SpladePooling("max")``, not checked against them.  The
arithmetic under test is ``transformers.BertForMaskedLM(...).logits`` followed by that formula.  No SPLADE weights were available either: real-checkpoint numerics
are unmeasured (``tools/checkpoint_check.py <dir>`` measures them).

``index_passages`` / ``retrieve`` fill and search a ``sparse_index.SparseIndexer``: the ``[B, vocab]`` rows of a forward are compacted on the GPU and stored
as float16 postings, a query is scored against every stored passage by ``libkirag_sparse.so``.

Not covered: DistilBERT- / RoBERTa-based MLM heads (refused by ``model_type``), SPLADE's sum pooling, FLOPS-regularised training.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from transformers import BertForMaskedLM, PretrainedConfig

from .encoders import POOL_SPLADE, HipBertForward, _HipModuleMixin, checkpoint_model_type

DECODER_WEIGHT, DECODER_BIAS = "cls.predictions.decoder.weight", "cls.predictions.decoder.bias"


def splade_rename(name: str) -> str:
    """``BertForMaskedLM`` parameter name -> the library's: the backbone loses its ``bert.`` prefix, ``cls.predictions.bias`` is HF's alias of the decoder's
    bias (one Parameter under two names: ``named_parameters()`` yields it once, under either)"""
    if name.startswith("bert."):
        name = name[len("bert."):]
    return DECODER_BIAS if name == "cls.predictions.bias" else name


def splade_extra(module) -> List[Tuple[str, Tensor]]:
    """the decoder's weight: tied to the word embeddings it does not appear in ``named_parameters()``, and the library takes it explicitly"""
    return [(DECODER_WEIGHT, module.cls.predictions.decoder.weight)]


def check_splade_config(cfg: dict) -> None:
    """Refuse by field, before a handle (or a model) exists, what ``KR_POOL_SPLADE`` does not compute.  ``cfg``: the checkpoint's ``config.json`` as a dict."""
    mt = cfg.get("model_type", "bert")
    if mt != "bert":
        raise NotImplementedError(f"model_type={mt!r}: the SPLADE head runs on 'bert' checkpoints (BertForMaskedLM); DistilBERT- and RoBERTa-based MLM heads are "
                                  "other functions and are not implemented")
    act = cfg.get("hidden_act", "gelu")
    if act != "gelu":
        raise NotImplementedError(f"hidden_act={act!r}: the stack and the MLM head's transform implement erf-GELU only")
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        raise NotImplementedError(f"position_embedding_type={cfg.get('position_embedding_type')!r}: only absolute position embeddings are implemented")
    H, heads, FF = int(cfg.get("hidden_size", 768)), int(cfg.get("num_attention_heads", 12)), int(cfg.get("intermediate_size", 3072))
    if H % 128 or H > 2048:
        raise NotImplementedError(f"hidden_size={H}: the HIP encoder needs a multiple of 128, at most 2048")
    if heads <= 0 or H // heads not in (32, 64) or H % heads:
        raise NotImplementedError(f"hidden_size={H} / num_attention_heads={heads}: the attention kernels are built for heads of width 32 and 64")
    if FF % 128:
        raise NotImplementedError(f"intermediate_size={FF}: the projections need a multiple of 128")


class BertSpladeEncoder(_HipModuleMixin, BertForMaskedLM):
    """BertModel -> cls.predictions (transform + decoder) -> log1p(relu(.)) -> max over the attended tokens (SPLADE's "max" pooling)"""
    _pool = POOL_SPLADE
    _hf_base = BertForMaskedLM
    _hip_rename = staticmethod(splade_rename)
    _hip_extra = staticmethod(splade_extra)

    def __init__(self, config, **kwargs):
        check_splade_config(config.to_dict())
        super().__init__(config)
        self.kwargs = kwargs
        self._hip: Optional[HipBertForward] = None

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, **kwargs):
        _, config = checkpoint_model_type(pretrained_model_name_or_path, kwargs)
        check_splade_config(config.to_dict() if isinstance(config, PretrainedConfig) else config)          # refused by name before any weight is read
        return super().from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)

    @torch.no_grad()
    def forward_splade(self, input_ids: Tensor, attention_mask: Optional[Tensor] = None, token_type_ids: Optional[Tensor] = None) -> Tensor:
        """ONE HIP forward: ``[B, vocab_size]`` fp32 on the GPU, every entry >= 0; a row without attended tokens is all +0.0.  Eval mode only."""
        if self.training:
            raise RuntimeError("forward_splade is the inference (HIP) path: call model.eval() first")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if int(getattr(self.config, "type_vocab_size", 1)) <= 1:
            token_type_ids = None
        return self._hip_forward(input_ids, attention_mask, token_type_ids)


def build_token_weights(vec: np.ndarray, id_to_token, skip_ids=(), top_k: Optional[int] = None) -> Dict[str, float]:
    """``{token string: weight}`` of one ``[vocab]`` vector: weights > 0 only, without the ids in ``skip_ids`` (the tokenizer's pad id), optionally the ``top_k``
    largest (ties by the smaller id).  ``id_to_token``: callable id -> str."""
    v = np.asarray(vec, dtype=np.float32)
    idx = np.flatnonzero(v > 0)
    skip = {int(i) for i in skip_ids if i is not None}
    if skip:
        idx = idx[~np.isin(idx, list(skip))]
    if top_k is not None and len(idx) > top_k:
        idx = idx[np.lexsort((idx, -v[idx]))[:max(int(top_k), 0)]]
    return {id_to_token(int(i)): float(v[i]) for i in idx}


def sparse_dot(a: Dict[str, float], b: Dict[str, float]) -> float:
    """sum of ``w_a * w_b`` over the tokens both hold"""
    if len(b) < len(a):
        a, b = b, a
    return float(sum(w * b[k] for k, w in a.items() if k in b))


class SpladeModel:
    """``encode`` / ``encode_dense`` / ``compute_score`` / ``rerank`` over a ``BertSpladeEncoder``.  ``model_name_or_path``: a checkpoint folder or an already
    built encoder."""

    def __init__(self, model_name_or_path, tokenizer=None, device=None, **kwargs):
        if isinstance(model_name_or_path, nn.Module) or hasattr(model_name_or_path, "forward_splade"):
            self.model = model_name_or_path
        else:
            self.model = BertSpladeEncoder.from_pretrained(model_name_or_path, **kwargs)
        self.model_name_or_path = model_name_or_path
        self.tokenizer = tokenizer
        if device is None:
            device = "cuda" if torch.cuda.is_available() else None
        self.device = torch.device(device) if device is not None else None
        if isinstance(self.model, nn.Module):
            if self.device is not None:
                self.model.to(self.device)
            self.model.eval()

    @classmethod
    def from_pretrained(cls, model_name_or_path, **kwargs):
        """the registry's call (``rerankers.load_reranker("SPLADE", path)``)"""
        return cls(model_name_or_path, **kwargs)

    def _tokenizer(self):
        if self.tokenizer is None:
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(self.model_name_or_path)
        return self.tokenizer

    @torch.no_grad()
    def encode_dense(self, texts, batch_size: int = 32, max_length: int = 512) -> Tensor:
        """``[N, vocab_size]`` fp32 on the model's device, one forward per batch"""
        if isinstance(texts, str):
            texts = [texts]
        tok = self._tokenizer()
        out = []
        for s in range(0, len(texts), batch_size):
            enc = tok(list(texts[s:s + batch_size]), padding=True, truncation=True, max_length=max_length, return_tensors="pt")
            out.append(self.model.forward_splade(enc["input_ids"], enc["attention_mask"], enc.get("token_type_ids")))
        return torch.cat(out)

    def encode(self, texts, batch_size: int = 32, max_length: int = 512, top_k: Optional[int] = None) -> List[Dict[str, float]]:
        """one ``{token string: weight}`` per text: weights > 0, the tokenizer's pad id skipped, optionally the ``top_k`` largest"""
        single = isinstance(texts, str)
        tok = self._tokenizer()
        vecs = self.encode_dense(texts, batch_size, max_length).float().cpu().numpy()
        out = [build_token_weights(v, tok.convert_ids_to_tokens, (tok.pad_token_id,), top_k) for v in vecs]
        return out[0] if single else out

    def compute_score(self, pairs, batch_size: int = 32, max_query_length: int = 512, max_passage_length: int = 512) -> List[float]:
        """the dot product of the two sparse vectors of every ``(query, passage)`` pair"""
        if isinstance(pairs, tuple) and len(pairs) == 2 and isinstance(pairs[0], str):
            pairs = [pairs]
        q = self.encode([a for a, _ in pairs], batch_size, max_query_length)
        p = self.encode([b for _, b in pairs], batch_size, max_passage_length)
        return [sparse_dot(a, b) for a, b in zip(q, p)]

    def rerank(self, query: str, passages: List[str], top_k: Optional[int] = None, batch_size: int = 64) -> Tuple[Tensor, Tensor]:
        """The shape of ``BaseReranker.rerank``: ``(indices, scores)`` of the best ``top_k`` passages (all when ``None``) by (score descending, index ascending),
        both on the CPU.  The query is encoded once."""
        assert isinstance(passages, list) and len(passages) > 0   # must provide passages
        q = self.encode([query], 1)[0]
        s = np.asarray([sparse_dot(q, p) for p in self.encode(passages, batch_size)], dtype=np.float64)
        order = torch.from_numpy(np.lexsort((np.arange(len(s)), -s)))
        if top_k is not None:
            order = order[:top_k]
        return order, torch.from_numpy(s.astype(np.float32))[order]

    # ---- exact retrieval over a resident sparse index (kirag_amd.retriever.sparse_index) ----
    @torch.no_grad()
    def index_passages(self, ids, passages: Sequence[str], sparse_index, batch_size: int = 64, max_length: int = 512) -> None:
        """ONE forward per batch; its ``[B, vocab]`` block goes to ``sparse_index.index_block`` with the tokenizer's pad id skipped, as ``encode`` skips it: the
        rows are compacted on the GPU and only the kept (term, float16 weight) entries visit the host.  Every id of the call is checked before the first
        forward (not a decimal number, twice in the call, already stored: ``ValueError``, nothing indexed)."""
        ids = list(ids)
        if len(ids) != len(passages):
            raise ValueError(f"{len(ids)} ids for {len(passages)} passages")
        sparse_index.check_new_ids(ids)
        tok = self._tokenizer()
        for s in range(0, len(passages), batch_size):
            enc = tok(list(passages[s:s + batch_size]), padding=True, truncation=True, max_length=max_length, return_tensors="pt")
            block = self.model.forward_splade(enc["input_ids"], enc["attention_mask"], enc.get("token_type_ids"))
            sparse_index.index_block(ids[s:s + batch_size], block, (tok.pad_token_id,))

    def retrieve(self, queries, sparse_index, top_k: int = 10, max_length: int = 512) -> List[Tuple[List[str], List[float]]]:
        """Per query the best ``top_k`` stored passages by the dot product of the two sparse vectors, exact, over the whole index
        (``SparseIndexer.search_knn``'s shape): the query's fp32 weights (pad id skipped) against the stored float16 ones.  A passage that shares no term with
        the query is no result."""
        if isinstance(queries, str):
            queries = [queries]
        pad = self._tokenizer().pad_token_id
        vecs = self.encode_dense(list(queries), max_length=max_length).float().cpu().numpy()
        sparse = []
        for v in vecs:
            idx = np.flatnonzero(v > 0)
            if pad is not None:
                idx = idx[idx != pad]
            sparse.append((idx.astype(np.int32), v[idx]))
        return sparse_index.search_knn(sparse, top_k)
