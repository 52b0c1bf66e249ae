"""Cross-encoder rerankers on the HIP encoder: the model the reference's loop names but never defines (``knowledge_graph/models.py:208-225`` loads
``BaseReranker("BGEReranker", ...)``, ``:424-447`` scores (question, reasoning chain + triple) pairs with ``reranker.score(args=batch_args)``).

A cross-encoder is the encoder stack plus a head on the ``[CLS]`` / ``<s>`` row, ``logits = Wo . tanh(Wd . x + bd) + bo``:

  * ``XLMRobertaForSequenceClassification`` (BAAI/bge-reranker-base / -large / -v2-m3): ``RobertaClassificationHead``, ``classifier.dense`` and
    ``classifier.out_proj`` — the names the library knows (``include/kirag_amd.h``);
  * ``BertForSequenceClassification`` (cross-encoder/ms-marco-MiniLM-L-6-v2 / -L-12-v2 / ms-marco-TinyBERT): the same arithmetic spelled
    ``classifier(tanh(pooler.dense(x)))``, mapped onto those names, with token types for the second segment;
  * ``ModernBertForSequenceClassification`` (Alibaba-NLP/gte-reranker-modernbert-base, ibm-granite/granite-embedding-reranker-english-r2, CrossEncoder
    fine-tunes of answerdotai/ModernBERT-*): another function, ``classifier(LayerNorm(gelu(head.dense(x))))`` on the ``[CLS]`` row or the masked mean
    (``config.classifier_pooling``), under HF's own names; no token types, up to 8192 tokens.

``XLMRobertaReranker`` / ``BertReranker`` / ``ModernBertReranker`` ARE those HF classes (``from_pretrained`` / ``save_pretrained`` / ``.to()`` keep working); in ``eval()`` mode their
forward runs in ``libkirag_amd.so`` (``KR_POOL_CLASSIFY``) and returns ``SequenceClassifierOutput(logits=[B, num_labels])`` on the GPU without autograd
history; in ``train()`` mode it is HF's own forward (dropout included).  There is no CPU fallback, as for the encoders.  Raw logits: a sigmoid or softmax is
the caller's.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from transformers import (BertForSequenceClassification, DebertaV2ForSequenceClassification, ModernBertConfig, ModernBertForSequenceClassification,
                          XLMRobertaForSequenceClassification)
from transformers.modeling_outputs import SequenceClassifierOutput

from ..collators import RerankerCollator
from .encoders import (DEBERTA_TYPE, MODERN_LAYER_TYPES, MODERN_TYPE, POOL_CLASSIFY, ROBERTA_TYPES, HipBertForward, _HipModuleMixin, _refuser, check_deberta_config,
                       check_heads, check_hidden, checkpoint_model_type)
from .m3 import BGEM3Model
from .splade import SpladeModel

MAX_LABELS = 64          # the library's bound on the rows of classifier.out_proj (include/kirag_amd.h)


def _strip(name: str, prefix: str) -> str:
    return name[len(prefix):] if name.startswith(prefix) else name


def xlmr_rename(name: str) -> str:
    """``XLMRobertaForSequenceClassification`` parameter name -> the library's: the backbone loses its ``roberta.`` prefix, the head has the library's spelling"""
    return _strip(name, "roberta.")


_BERT_HEAD = {"pooler.dense.weight": "classifier.dense.weight", "pooler.dense.bias": "classifier.dense.bias",
              "classifier.weight": "classifier.out_proj.weight", "classifier.bias": "classifier.out_proj.bias"}


def bert_rename(name: str) -> str:
    """``BertForSequenceClassification`` parameter name -> the library's: the backbone loses its ``bert.`` prefix, ``pooler.dense`` (the Linear in front of
    BERT's tanh) is the head's ``classifier.dense`` and ``classifier`` its ``classifier.out_proj``"""
    name = _strip(name, "bert.")
    return _BERT_HEAD.get(name, name)


class _HipClassifierMixin(_HipModuleMixin):
    """What the rerankers add to their HF base class (``_hf_base``, the next class in the MRO): the HIP eval forward on ``KR_POOL_CLASSIFY``.  Weight sync and
    its invalidation are the encoders' (``_HipModuleMixin``)."""
    _pool = POOL_CLASSIFY
    _hf_base = None

    def __init__(self, config, **kwargs):
        if int(config.num_labels) > MAX_LABELS:
            raise NotImplementedError(f"num_labels={config.num_labels}: the classification head of the HIP encoder holds at most {MAX_LABELS} labels")
        super().__init__(config)
        self.kwargs = kwargs
        self._hip: Optional[HipBertForward] = None

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, **kwargs):
        if self.training:
            return self._hf_base.forward(self, input_ids=input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, **kwargs)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if int(getattr(self.config, "type_vocab_size", 1)) <= 1:
            token_type_ids = None                       # one token-type row: whatever a tokenizer emits there selects it
        return SequenceClassifierOutput(logits=self._hip_forward(input_ids, attention_mask, token_type_ids))


class XLMRobertaReranker(_HipClassifierMixin, XLMRobertaForSequenceClassification):
    """XLMRobertaModel -> ``<s>`` row -> RobertaClassificationHead (BAAI/bge-reranker-base / -large / -v2-m3)"""
    _hf_base = XLMRobertaForSequenceClassification
    _hip_rename = staticmethod(xlmr_rename)


class BertReranker(_HipClassifierMixin, BertForSequenceClassification):
    """BertModel -> ``[CLS]`` row -> pooler.dense -> tanh -> classifier (cross-encoder/ms-marco-MiniLM-*, ms-marco-TinyBERT)"""
    _hf_base = BertForSequenceClassification
    _hip_rename = staticmethod(bert_rename)


MODERN_POOLINGS = {"cls": 0.0, "mean": 1.0}       # config.classifier_pooling -> the library's setting "config.classifier_pooling"
MODERN_POOLING_SETTING = "config.classifier_pooling"


def modern_rename(name: str) -> str:
    """``ModernBertForSequenceClassification`` parameter name -> the library's: the backbone loses its ``model.`` prefix, ``head.*`` and ``classifier.*`` are
    the library's own spelling"""
    return _strip(name, "model.")


def check_modern_config(config) -> None:
    """``NotImplementedError`` beginning ``model_type='modernbert':`` and naming the field, for everything the kernels do not compute — from the config alone:
    no weight has been read and the library is not loaded.  ``config``: a ``ModernBertConfig`` or the dict of a ``config.json`` (HF's defaults fill the rest)."""
    refuse = _refuser(MODERN_TYPE)
    is_dict = isinstance(config, dict)
    get = (lambda k, d: config.get(k, d)) if is_dict else (lambda k, d: getattr(config, k, d))
    # the raw fields first: HF's own config class validates some of them with errors of its own
    H, heads = int(get("hidden_size", 768)), int(get("num_attention_heads", 12))
    check_hidden(refuse, H)
    check_heads(refuse, H, heads)
    if get("classifier_activation", "gelu") != "gelu":
        refuse(f"classifier_activation={get('classifier_activation', None)!r}: the classification head implements erf-GELU only")
    if get("classifier_pooling", "cls") not in MODERN_POOLINGS:
        refuse(f"classifier_pooling={get('classifier_pooling', None)!r}: {tuple(MODERN_POOLINGS)} are implemented")
    labels = len(config["id2label"]) if is_dict and config.get("id2label") is not None else int(get("num_labels", 2))
    if labels > MAX_LABELS:
        refuse(f"num_labels={labels}: the classification head of the HIP encoder holds at most {MAX_LABELS} labels")
    types = get("layer_types", None)
    if types is not None and set(types) - set(MODERN_LAYER_TYPES):
        refuse(f"layer_types={list(types)!r}: one of {MODERN_LAYER_TYPES} per layer is implemented")
    if is_dict:
        config = ModernBertConfig.from_dict(config)
    try:
        with torch.device("cpu"):                      # (from_pretrained constructs the model under a meta-device context)
            HipBertForward._modern_settings(config)    # hidden_activation, head_dim, layer_types, attention_scaling: the encoders' own rules
    except NotImplementedError as e:
        refuse(str(e))


class ModernBertReranker(_HipClassifierMixin, ModernBertForSequenceClassification):
    """ModernBertModel -> ``[CLS]`` row or masked mean (``config.classifier_pooling``) -> head.dense -> gelu -> head.norm -> classifier
    (Alibaba-NLP/gte-reranker-modernbert-base, ibm-granite/granite-embedding-reranker-english-r2).  Frequencies, half-window, layer types and the FF
    zero-padding are the encoders' ModernBERT path (``HipBertForward``); the pooling travels as the library's setting next to the parameters."""
    _hf_base = ModernBertForSequenceClassification
    _hip_rename = staticmethod(modern_rename)

    def __init__(self, config, **kwargs):
        check_modern_config(config)
        super().__init__(config, **kwargs)
        # one float on the host, sent with every weight sync under the setting's reserved name (no parameter, no buffer: the state dict stays HF's)
        self._hip_pooling = torch.tensor([MODERN_POOLINGS[config.classifier_pooling]], dtype=torch.float32, device="cpu")

    @staticmethod
    def _hip_extra(module):
        return [(MODERN_POOLING_SETTING, module._hip_pooling)]

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, **kwargs):
        if self.training:        # ModernBERT has no token types: whatever a tokenizer emits there is dropped
            return ModernBertForSequenceClassification.forward(self, input_ids=input_ids, attention_mask=attention_mask, **kwargs)
        return super().forward(input_ids=input_ids, attention_mask=attention_mask, token_type_ids=None)


def deberta_rename(name: str) -> str:
    """``DebertaV2ForSequenceClassification`` parameter name -> the library's: the backbone loses its ``deberta.`` prefix, ``pooler.dense`` (the Linear in
    front of the ContextPooler's GELU) is the head's ``classifier.dense`` and ``classifier`` its ``classifier.out_proj``, as for ``BertReranker``"""
    name = _strip(name, "deberta.")
    return _BERT_HEAD.get(name, name)


class DebertaV2Reranker(_HipClassifierMixin, DebertaV2ForSequenceClassification):
    """DebertaV2Model -> ``[CLS]`` row -> pooler.dense -> gelu -> classifier (mixedbread-ai/mxbai-rerank-*-v1, cross-encoder/nli-deberta-v3-*,
    naver/trecdl22-crossencoder-debertav3).  On a DeBERTa handle the library's ``classifier.*`` names compute the erf-GELU of the ContextPooler where BERT's
    head computes tanh."""
    _hf_base = DebertaV2ForSequenceClassification
    _hip_rename = staticmethod(deberta_rename)

    def __init__(self, config, **kwargs):
        check_deberta_config(config, head=True)
        super().__init__(config, **kwargs)

    @staticmethod
    def _hip_extra(module):
        # the weight sync leaves out every parameter named ``pooler.*`` (the encoders never read a pooler); here it is half of the head
        return [("classifier.dense.weight", module.pooler.dense.weight), ("classifier.dense.bias", module.pooler.dense.bias)]


class BGEReranker:
    """The registry's entry: ``from_pretrained`` reads the checkpoint's ``config.json`` and returns the twin of its ``model_type``."""

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, **kwargs):
        model_type, cfg_dict = checkpoint_model_type(pretrained_model_name_or_path, kwargs)
        if model_type == "bert":
            return BertReranker.from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        if model_type in ROBERTA_TYPES:
            return XLMRobertaReranker.from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        if model_type == MODERN_TYPE:
            check_modern_config(cfg_dict)          # from config.json alone: before a weight is read
            return ModernBertReranker.from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        if model_type in (DEBERTA_TYPE, "deberta"):
            check_deberta_config(cfg_dict, head=True)      # from config.json alone: before a weight is read
            return DebertaV2Reranker.from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        raise NotImplementedError(f"model_type={model_type!r}: cross-encoder rerankers run for 'bert', {MODERN_TYPE!r}, {DEBERTA_TYPE!r} and {ROBERTA_TYPES} checkpoints "
                                  "(the classification heads of other families are other functions)")


RERANKER_MAP = {"BGEReranker": BGEReranker}
# second stages that are no cross-encoder, reached through load_reranker under these names.  "BGEM3": hybrid dense + sparse + multi-vector scoring with the
# retriever's own bge-m3 checkpoint (kirag_amd.retriever.m3), no second model in HBM.  Kept apart from RERANKER_MAP: that map lists the models
# BaseReranker.score() can drive (a forward that returns logits), which a BGEM3Model is not.
# "SPLADE": learned sparse scoring with a BertForMaskedLM checkpoint (kirag_amd.retriever.splade), the dot product of two vocabulary-sized vectors.
HYBRID_RERANKER_MAP = {"BGEM3": BGEM3Model, "SPLADE": SpladeModel}


def load_reranker(reranker_name, model_name_or_path, **kwargs):
    known = {**RERANKER_MAP, **HYBRID_RERANKER_MAP}
    if reranker_name not in known:
        raise KeyError(f"{reranker_name} is not implemented! Current available rerankers: {list(known.keys())}")
    print(f"loading {reranker_name} model from {model_name_or_path} ...")
    return known[reranker_name].from_pretrained(model_name_or_path, **kwargs)


def rank_order(scores: Sequence[float]) -> np.ndarray:
    """indices by (score descending, index ascending)"""
    s = np.asarray(scores, dtype=np.float64)
    return np.lexsort((np.arange(len(s)), -s))


class BaseReranker(nn.Module):
    """What ``knowledge_graph/models.py:219-225,438`` call — ``.to()``, ``.eval()``, ``.device``, ``.score(args)`` — plus ``save_model`` / ``load_model`` as
    ``BaseRetriever`` has them, and ``rerank``: the call a ``DenseRetriever`` user makes after ``search_knn``."""

    def __init__(self, reranker_name, model_name_or_path, reranker_kwargs={}, tokenizer=None, maxlength: int = 512, **kwargs):
        super().__init__()
        self.reranker = load_reranker(reranker_name, model_name_or_path, **reranker_kwargs, **kwargs)
        self.reranker_name = reranker_name
        self.model_name_or_path = model_name_or_path
        self.reranker_kwargs = reranker_kwargs
        self.tokenizer, self.maxlength = tokenizer, maxlength       # rerank() only; None: the checkpoint's own tokenizer, loaded on first use
        self.kwargs = kwargs

    @property
    def device(self):
        for _, p in self.named_parameters():
            return p.device

    def score(self, args, **kwargs) -> Tensor:
        """``args``: the collator's ``input_ids`` / ``attention_mask`` (/ ``token_type_ids``), on the host or the GPU.  ``[B]`` for one label
        (``logits.view(-1)``), ``[B, num_labels]`` otherwise."""
        logits = self.reranker(**args, **kwargs).logits
        return logits.view(-1) if logits.shape[-1] == 1 else logits

    def save_model(self, save_path):
        self.reranker.save_pretrained(save_path)

    def load_model(self, save_path):
        self.reranker = load_reranker(self.reranker_name, save_path, **self.reranker_kwargs, **self.kwargs)

    def _collator(self) -> RerankerCollator:
        if self.tokenizer is None:
            from transformers import AutoTokenizer
            self.tokenizer = AutoTokenizer.from_pretrained(self.model_name_or_path)
        return RerankerCollator(self.tokenizer, maxlength=self.maxlength)

    @torch.no_grad()
    def rerank(self, query: str, passages: List[str], top_k: Optional[int] = None, batch_size: int = 64) -> Tuple[Tensor, Tensor]:
        """Score ``(query, passage)`` for every passage and return ``(indices, scores)`` of the best ``top_k`` (all when ``None``) by (score descending,
        index ascending), both on the CPU.  The pairs run in batches of ``batch_size`` sorted by token count: a pair's logit does not depend on its batch, so
        the sort only saves padding and every ``batch_size`` gives the same scores.  One-label checkpoints only."""
        assert isinstance(passages, list) and len(passages) > 0   # must provide passages
        col = self._collator()
        rows = col.tokenize_pairs([query] * len(passages), passages)
        by_len = sorted(range(len(passages)), key=lambda i: (len(rows[i]["input_ids"]), i))
        scores = torch.empty(len(passages), dtype=torch.float32)
        for s in range(0, len(by_len), batch_size):
            idx = by_len[s:s + batch_size]
            out = self.score(col.pad([rows[i] for i in idx]))
            if out.dim() != 1:
                raise ValueError(f"rerank needs one score per pair: this checkpoint has {out.shape[-1]} labels (use score())")
            scores[torch.tensor(idx)] = out.detach().float().cpu()
        order = torch.from_numpy(rank_order(scores.numpy()))
        if top_k is not None:
            order = order[:top_k]
        return order, scores[order]
