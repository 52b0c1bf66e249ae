"""Cross-encoder rerankers on the HIP encoder: the model the reference's loop names but never defines (``knowledge_graph/models.py:208-225`` loads
``BaseReranker("BGEReranker", ...)``, ``:424-447`` scores (question, reasoning chain + triple) pairs with ``reranker.score(args=batch_args)``).

A cross-encoder is the encoder stack plus a head on the ``[CLS]`` / ``<s>`` row, ``logits = Wo . tanh(Wd . x + bd) + bo``:

  * ``XLMRobertaForSequenceClassification`` (BAAI/bge-reranker-base / -large / -v2-m3): ``RobertaClassificationHead``, ``classifier.dense`` and
    ``classifier.out_proj`` — the names the library knows (``include/kirag_amd.h``);
  * ``BertForSequenceClassification`` (cross-encoder/ms-marco-MiniLM-L-6-v2 / -L-12-v2 / ms-marco-TinyBERT): the same arithmetic spelled
    ``classifier(tanh(pooler.dense(x)))``, mapped onto those names, with token types for the second segment;
  * ``ModernBertForSequenceClassification`` (Alibaba-NLP/gte-reranker-modernbert-base, ibm-granite/granite-embedding-reranker-english-r2, CrossEncoder
    fine-tunes of answerdotai/ModernBERT-*): another function, ``classifier(LayerNorm(gelu(head.dense(x))))`` on the ``[CLS]`` row or the masked mean
    (``config.classifier_pooling``), under HF's own names; no token types, up to 8192 tokens;
  * ``Qwen2ForSequenceClassification`` / ``LlamaForSequenceClassification`` / ``MistralForSequenceClassification`` (decoder-LLM cross-encoders, what
    sentence-transformers' ``CrossEncoder`` trains from Qwen2.5-0.5B, Llama-3.2-1B, TinyLlama or SmolLM2): the decoder stack of the embedders, no ``[CLS]``
    row — ``score.weight . x`` of the LAST token, a Linear without a bias (``DecoderReranker``, below).

``XLMRobertaReranker`` / ``BertReranker`` / ``ModernBertReranker`` ARE those HF classes (``from_pretrained`` / ``save_pretrained`` / ``.to()`` keep working); in ``eval()`` mode their
forward runs in ``libkirag_amd.so`` (``KR_POOL_CLASSIFY``) and returns ``SequenceClassifierOutput(logits=[B, num_labels])`` on the GPU without autograd
history; in ``train()`` mode it is HF's own forward (dropout included).  There is no CPU fallback, as for the encoders.  Raw logits: a sigmoid or softmax is
the caller's.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import json
import os

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from transformers import (BertForSequenceClassification, DebertaV2ForSequenceClassification, LlamaForSequenceClassification, MistralForSequenceClassification,
                          ModernBertConfig, ModernBertForSequenceClassification, Qwen2ForSequenceClassification, Qwen3ForSequenceClassification,
                          XLMRobertaForSequenceClassification)
from transformers.modeling_outputs import SequenceClassifierOutput

from ..collators import RerankerCollator
from .encoders import (DEBERTA_TYPE, DECODER_ATTENTIONS, EUROBERT_TYPE, QWEN3_TYPE, MODERN_LAYER_TYPES, MODERN_TYPE, POOL_CLASSIFY, ROBERTA_TYPES, ST_ATTENTION_FILE,
                       ST_POOLING_DIR, HipBertForward, _HipModuleMixin, _refuser, _st_file, check_decoder_config, check_deberta_config, check_heads, check_hidden,
                       checkpoint_model_type)
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


DECODER_RERANKER_TYPES = ("qwen2", "llama", "mistral")
QWEN3_RERANKER_TYPES = (QWEN3_TYPE,)     # Qwen3ForSequenceClassification, and Qwen3ForCausalLM "yes / no" rerankers through ``DecoderReranker.from_causal_lm``


def decoder_rename(name: str) -> str:
    """``Qwen2ForSequenceClassification`` / ``Llama...`` / ``Mistral...`` parameter name -> the library's: the backbone loses its ``model.`` prefix (the names
    the decoder embedders send), ``score.weight`` is the library's own spelling"""
    return _strip(name, "model.")


def config_num_labels(config) -> int:
    """``num_labels`` of an HF config or of the dict of a ``config.json`` (where it is the length of ``id2label``; HF's default is 2)"""
    if isinstance(config, dict):
        return len(config["id2label"]) if config.get("id2label") is not None else int(config.get("num_labels", 2))
    return int(config.num_labels)


def check_decoder_reranker_config(config) -> dict:
    """``NotImplementedError`` beginning ``model_type='<type>':`` for a decoder cross-encoder the kernels do not compute — from the config alone: no weight has
    been read and the library is not loaded.  Everything ``check_decoder_config`` refuses for the embedders, in its order (128-wide heads included), then
    ``num_labels`` > 64.  EuroBERT is a decoder stack for the embedders, but ``EuroBertForSequenceClassification`` has another head (dense -> activation ->
    classifier over ``clf_pooling``) and is refused by name.  ``config``: the HF config or the dict of a ``config.json``."""
    mt = config.get("model_type") if isinstance(config, dict) else config.model_type
    refuse = _refuser(mt)
    if mt == EUROBERT_TYPE:
        refuse("EuroBertForSequenceClassification's head is dense -> activation -> classifier over clf_pooling, not the score head of the decoder "
               f"rerankers: they run for {DECODER_RERANKER_TYPES}")
    if mt not in DECODER_RERANKER_TYPES + QWEN3_RERANKER_TYPES:
        refuse(f"the decoder rerankers run for {DECODER_RERANKER_TYPES + QWEN3_RERANKER_TYPES}")
    d = check_decoder_config(config)
    labels = config_num_labels(config)
    if labels > MAX_LABELS:
        refuse(f"num_labels={labels}: the score head of the HIP encoder holds at most {MAX_LABELS} labels")
    return d


class _HipDecoderClassifierMixin(_HipClassifierMixin):
    """A decoder LLM used as a cross-encoder: ``logits = score.weight . x`` with x the final-norm row of the LAST token, no bias (HF's
    ``GenericForSequenceClassification``).  ``train()`` mode is HF's own forward; eval mode sends the backbone under the decoder embedders' names plus
    ``score.weight`` and runs ``KR_POOL_CLASSIFY`` with the attention mask.

    The last token.  HF picks the rightmost column with ``input_ids != config.pad_token_id``; the library picks the HIGHEST ATTENDED COLUMN of
    ``attention_mask``.  The two agree whenever ``attention_mask == (input_ids != pad_token_id)`` — what a tokenizer's padding produces, right or left — and
    where they differ (a pad id inside the text, a mask with its own idea of the end) the library follows the mask.  A config without ``pad_token_id`` is
    served as HF serves it, from the last column: the eval forward then needs an all-ones mask (or none) or batch 1, like HF's.

    ``attention`` ("causal", the default, / "bidirectional") is the ``from_pretrained`` kwarg of the decoder embedders with the same meaning, else the
    checkpoint's ``1_Pooling/attention.json``; ``save_pretrained`` writes that file for a bidirectional twin only, so a causal one saves an ordinary
    ``...ForSequenceClassification`` folder.  ``train()`` mode of a bidirectional twin feeds HF the 4-D mask that admits every attended key."""
    _hip_rename = staticmethod(decoder_rename)

    def __init__(self, config, **kwargs):
        check_decoder_reranker_config(config)          # refuses what the kernels do not compute when the model is made, not at its first forward
        super().__init__(config, **kwargs)
        self._decoder_attention = 1.0

    @staticmethod
    def _check_attention(attention) -> None:
        if attention not in DECODER_ATTENTIONS:
            raise ValueError(f"attention={attention!r}: one of {sorted(DECODER_ATTENTIONS)}")

    def set_attention(self, attention: str) -> None:
        self._check_attention(attention)
        if DECODER_ATTENTIONS[attention] != self._decoder_attention:
            self._decoder_attention = DECODER_ATTENTIONS[attention]
            self._hip = None                            # the mask of a handle is fixed at its first finalize

    @property
    def attention(self) -> str:
        return {v: k for k, v in DECODER_ATTENTIONS.items()}[self._decoder_attention]

    def last_token_index(self, input_ids: Tensor, attention_mask: Tensor) -> Tensor:
        """[B] the column the eval forward reads: the highest attended one (0 for a row without any; its logits are NaN)"""
        cols = torch.arange(attention_mask.shape[1], device=attention_mask.device)
        return ((attention_mask != 0) * (cols + 1)).argmax(dim=1)

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, **kwargs):
        if not self.training:
            if attention_mask is None:
                attention_mask = torch.ones_like(input_ids)
            if self.config.pad_token_id is None and input_ids.shape[0] != 1 and not bool((attention_mask != 0).all()):
                raise ValueError("Cannot handle a padded batch if no padding token is defined (config.pad_token_id is None): pass an all-ones mask or batch 1")
            return SequenceClassifierOutput(logits=self._hip_forward(input_ids, attention_mask, None))      # decoders have no token types
        if self._decoder_attention == 0.0 and attention_mask is not None:
            # [B, 1, S, S] additive: every attended key column for every query column, in the place of HF's causal mask
            dtype = next(self.parameters()).dtype
            m = torch.zeros(attention_mask.shape, dtype=dtype, device=attention_mask.device).masked_fill(attention_mask == 0, torch.finfo(dtype).min)
            attention_mask = m[:, None, None, :].expand(-1, 1, attention_mask.shape[1], -1).contiguous()
        return self._hf_base.forward(self, input_ids=input_ids, attention_mask=attention_mask, **kwargs)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, **kwargs):
        attention = kwargs.pop("attention", None)
        if attention is not None:
            cls._check_attention(attention)
        check_decoder_reranker_config(checkpoint_model_type(pretrained_model_name_or_path, kwargs)[1])     # from config.json alone, before a weight is read
        if attention is None:
            path = _st_file(pretrained_model_name_or_path, f"{ST_POOLING_DIR}/{ST_ATTENTION_FILE}", kwargs)
            if path is not None:
                with open(path) as f:
                    attention = json.load(f).get("attention")
                cls._check_attention(attention)
        model = super().from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        if attention is not None:
            model.set_attention(attention)
        return model

    def save_pretrained(self, save_directory, *args, **kwargs):
        out = super().save_pretrained(save_directory, *args, **kwargs)
        if self._decoder_attention == 0.0:
            os.makedirs(os.path.join(save_directory, ST_POOLING_DIR), exist_ok=True)
            with open(os.path.join(save_directory, ST_POOLING_DIR, ST_ATTENTION_FILE), "w") as f:
                json.dump({"attention": self.attention}, f, indent=2)
        return out


class Qwen2Reranker(_HipDecoderClassifierMixin, Qwen2ForSequenceClassification):
    """Qwen2Model (causal) -> last attended token -> score (CrossEncoder fine-tunes of Qwen2 / Qwen2.5-0.5B ... 1.5B)"""
    _hf_base = Qwen2ForSequenceClassification


class Qwen3Reranker(_HipDecoderClassifierMixin, Qwen3ForSequenceClassification):
    """Qwen3Model (causal, q / k norms, head_dim of its own) -> last attended token -> score (Qwen3-Reranker-0.6B folded by ``DecoderReranker.from_causal_lm``)"""
    _hf_base = Qwen3ForSequenceClassification


class LlamaReranker(_HipDecoderClassifierMixin, LlamaForSequenceClassification):
    """LlamaModel (causal) -> last attended token -> score (CrossEncoder fine-tunes of Llama-3.2-1B, TinyLlama, SmolLM2)"""
    _hf_base = LlamaForSequenceClassification


class MistralReranker(_HipDecoderClassifierMixin, MistralForSequenceClassification):
    """MistralModel (causal, no sliding window) -> last attended token -> score"""
    _hf_base = MistralForSequenceClassification


_DECODER_RERANKERS = {"qwen2": Qwen2Reranker, "llama": LlamaReranker, "mistral": MistralReranker, QWEN3_TYPE: Qwen3Reranker}


class DecoderReranker:
    """``from_pretrained`` of the decoder rerankers by ``model_type`` (``qwen2`` / ``llama`` / ``mistral``), as ``DecoderE5Encoder`` dispatches the embedders;
    anything else is refused by name.  ``from_causal_lm`` folds a causal-LM "yes / no" reranker into a one-label one."""

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, **kwargs):
        model_type, _ = checkpoint_model_type(pretrained_model_name_or_path, kwargs, default=None)
        if model_type not in _DECODER_RERANKERS:
            check_decoder_reranker_config({"model_type": model_type})      # refuses by name (EuroBERT with the sentence about its head)
        return _DECODER_RERANKERS[model_type].from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)      # (checks config.json before a weight is read)

    @classmethod
    def from_causal_lm(cls, path, positive_token_id: int, negative_token_id: Optional[int] = None, **kwargs):
        """A one-label reranker from a causal-LM folder (``Qwen2ForCausalLM`` / ``LlamaForCausalLM`` / ``MistralForCausalLM`` / ``Qwen3ForCausalLM``): a "yes / no" reranker scores a
        pair by the difference of two LM-head logits at the last token, ``lm_head[pos] . x - lm_head[neg] . x``, which is the one-label score head
        ``score.weight = lm_head[pos] - lm_head[neg]`` (``lm_head[pos]`` alone when ``negative_token_id`` is None).  The LM-head rows are the
        ``embed_tokens`` rows when the embeddings are tied and the folder holds no ``lm_head.weight``.  The result is an ordinary twin:
        ``save_pretrained`` writes a ``...ForSequenceClassification`` folder that ``BGEReranker.from_pretrained`` loads.

        The prompt template, the instruction prefix and the yes / no token ids of a published LLM reranker are the caller's business: the scores mean what
        its authors say only on inputs built their way.  No such checkpoint was available to check this recipe against."""
        from transformers import AutoConfig, AutoModelForCausalLM
        attention = kwargs.pop("attention", None)
        config = AutoConfig.from_pretrained(path, **{k: v for k, v in kwargs.items() if k != "config"})
        d = config.to_dict()
        d["num_labels"] = 1
        d.pop("id2label", None); d.pop("label2id", None)
        check_decoder_reranker_config(d)                # from config.json alone, before a weight is read
        lm = AutoModelForCausalLM.from_pretrained(path, **kwargs)
        rows = lm.get_output_embeddings().weight.detach()       # lm_head.weight, or the tied embed_tokens.weight
        V = rows.shape[0]
        for t in (positive_token_id, negative_token_id):
            if t is not None and not 0 <= int(t) < V:
                raise ValueError(f"token id {t} outside the {V} rows of the LM head")
        score = rows[int(positive_token_id)].float().clone()
        if negative_token_id is not None:
            score -= rows[int(negative_token_id)].float()
        config.num_labels = 1
        config.architectures = None
        model = _DECODER_RERANKERS[config.model_type](config)
        res = model.model.load_state_dict(lm.model.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys, res
        with torch.no_grad():
            model.score.weight.copy_(score[None].to(model.score.weight.dtype))
        model.to(next(lm.parameters()).dtype)
        if attention is not None:
            model.set_attention(attention)
        return model.eval()


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
        if model_type in DECODER_RERANKER_TYPES + QWEN3_RERANKER_TYPES or model_type == EUROBERT_TYPE:      # (EuroBERT: refused there, with the sentence that says why)
            return DecoderReranker.from_pretrained(pretrained_model_name_or_path, *model_args, **kwargs)
        raise NotImplementedError(f"model_type={model_type!r}: cross-encoder rerankers run for 'bert', {MODERN_TYPE!r}, {DEBERTA_TYPE!r}, {ROBERTA_TYPES} and "
                                  f"{DECODER_RERANKER_TYPES} checkpoints (the classification heads of other families are other functions)")


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
