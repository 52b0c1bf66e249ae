"""Shared pieces of the RoBERTa-family tests (tests/test_xlmr_host.py, tests/test_gpu_xlmr.py): fairseq's position rule restated in numpy, synthetic XLM-R
weights, the HF fp32 reference with the encoders' pooling, and a toy fast tokenizer whose special ids are XLM-R's (<s> 0, <pad> 1, </s> 2, <unk> 3)."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import encoder_np as E

PAD = 1


def fairseq_positions(ids, P=PAD):
    """pos = P + cumsum(ids != P) * (ids != P), row by row over ALL columns (attended or not)"""
    m = (np.asarray(ids) != P).astype(np.int64)
    return P + np.cumsum(m, axis=1) * m


def differs_from_simple_rules(ids, mask, P=PAD):
    """True when, at some ATTENDED column of this row, fairseq's position is neither `column + P + 1` nor `P + rank among the attended columns`: a case that
    an implementation of either simpler rule cannot pass by accident"""
    ids, mask = np.asarray(ids), np.asarray(mask) != 0
    pos = fairseq_positions(ids[None], P)[0]
    by_column = np.arange(len(ids)) + P + 1
    by_mask = P + np.cumsum(mask)
    return bool((pos != by_column)[mask].any() and (pos != by_mask)[mask].any())


def cfg(H, L, heads, FF, vocab, max_pos, P=PAD):
    return SimpleNamespace(hidden_size=H, num_hidden_layers=L, num_attention_heads=heads, intermediate_size=FF, vocab_size=vocab, max_position_embeddings=max_pos,
                           type_vocab_size=1, layer_norm_eps=1e-5, hidden_act="gelu", model_type="xlm-roberta", pad_token_id=P)


def weights(H, L, FF, vocab, max_pos, wname="benign", seed=None):
    """oracle.encoder_np's synthetic BERT weights in XLM-R form: one token-type row, max_pos position rows"""
    if wname == "benign":
        w = E.synth_weights(H, L, FF, vocab, max_pos, seed=3 if seed is None else seed)
    else:
        w = E.synth_weights_outlier(H, L, FF, vocab, max_pos, seed=7 if seed is None else seed, gamma_lo=1.5, gamma_hi=3.0)    # out3 (tests/golden/g10_spec.py)
    w = dict(w)
    k = [n for n in w if n.endswith("token_type_embeddings.weight")][0]
    w[k] = np.ascontiguousarray(w[k][:1])
    return w


def hf_model(c, w, device="cuda"):
    from transformers import XLMRobertaConfig, XLMRobertaModel
    m = XLMRobertaModel(XLMRobertaConfig(hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                                         intermediate_size=c.intermediate_size, vocab_size=c.vocab_size, max_position_embeddings=c.max_position_embeddings,
                                         type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=c.pad_token_id, bos_token_id=0, eos_token_id=2),
                        add_pooling_layer=False)
    assert not m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False).missing_keys
    return m.float().eval().to(device)


@torch.no_grad()
def hf_encode(m, ids, mask, pool, chunk=16):
    """XLMRobertaModel fp32 -> masked mean (pool 0) / [:, 0] (pool 1) -> L2 normalise: the encoders' pooling.  HF derives the position ids from the input ids."""
    dev = next(m.parameters()).device
    outs = []
    for i in range(0, len(ids), chunk):
        a = torch.from_numpy(np.ascontiguousarray(ids[i:i + chunk])).to(dev); k = torch.from_numpy(np.ascontiguousarray(mask[i:i + chunk])).to(dev)
        lh = m(input_ids=a, attention_mask=k).last_hidden_state
        if pool == 0:
            lh = lh.masked_fill(~k[..., None].bool(), 0.0)
            v = lh.sum(1) / k.sum(1)[..., None]
        else:
            v = lh[:, 0]
        outs.append(torch.nn.functional.normalize(v, dim=-1).cpu().numpy())
    return np.concatenate(outs)


def toy_words(n=200):
    letters = "abcdefghijklmnopqrstuvwxyz"
    return [letters[i % 26] + letters[(i // 26) % 26] + letters[(i * 7) % 26] + str(i) for i in range(n)]


def toy_tokenizer(words=None, padding_side="right"):
    """A word-level fast tokenizer with XLM-R's special ids and its `<s> A </s>` template"""
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from tokenizers.processors import TemplateProcessing
    from transformers import PreTrainedTokenizerFast
    words = toy_words() if words is None else words
    vocab = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3}
    for extra in ("query", "passage", ":", ",", "title", "text"):
        vocab.setdefault(extra, len(vocab))
    for wd in words:
        vocab.setdefault(wd, len(vocab))
    t = Tokenizer(WordLevel(vocab, unk_token="<unk>"))
    t.pre_tokenizer = Whitespace()
    t.post_processor = TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    tok = PreTrainedTokenizerFast(tokenizer_object=t, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", cls_token="<s>", sep_token="</s>",
                                  padding_side=padding_side)
    assert tok.pad_token_id == 1 and tok.vocab_size == len(vocab)
    return tok
