#!/usr/bin/env python3
"""Encode-leg micro benchmark: passages/s of the HIP encoder (synthetic weights) at a BERT shape.

    python tools/enc_bench.py [n] [S] [ragged] [--shape e5-large|e5-small|minilm-l6|xlmr-base|xlmr-large|bge-m3|xlmr-base-8k|mpnet-base|mpnet-base-nobias|nomic-base|modernbert-base|modernbert-base-global|t5-base|t5-base-gated|deberta-v3-base ...] [--pool mean|cls] [--hf-fp16] [--expanded | --alternate-gqa (decoder shapes)]
                              [--first-forward] [--alternate-shapes] [--digest]

Several --shape values run one after the other in the same process (default: e5-large).  --hf-fp16 also times HF BertModel / XLMRobertaModel in fp16 under
torch on the same batch: a yardstick, not a product path.  --first-forward times, instead, the first eval forward of the MODULE (E5Encoder or its XLM-R
twin on the GPU: the weight sync, the word table included) and the first one after a train() / eval() round trip.  --alternate-shapes builds one handle
per --shape and times them in turns in this process (--reps rounds of 3 forwards: median, min, max).  --digest appends the first 16 hex digits of the sha256 of
the batch's embeddings (to compare two builds of the library, each in its own process under KIRAG_AMD_LIB)."""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from kirag_amd import bench_support as BS

PEAK_MFMA_DENSE_16BIT = 2.5e15   # MI355X_MICROARCH.md: bf16/f16 dense MFMA peak

# the RoBERTa-family shapes (fairseq position rule, padding index 1): xlm-roberta-base / -large (multilingual-e5-base / -large) and bge-m3 (xlmr-large with
# 8194 position rows = 8192 tokens)
XLMR_LARGE = dict(BS.E5_LARGE, vocab_size=250002, max_position_embeddings=514, type_vocab_size=1, layer_norm_eps=1e-5, model_type="xlm-roberta", pad_token_id=1)
XLMR_BASE = dict(XLMR_LARGE, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072)
BGE_M3 = dict(XLMR_LARGE, max_position_embeddings=8194)
XLMR_BASE_8K = dict(XLMR_BASE, max_position_embeddings=8194)     # xlmr-base with bge-m3's position rows: the yardstick of nomic-base beyond 512 tokens
# MPNet (all-mpnet-base-v2): the xlmr-base stack at vocab 30527 + the relative attention bias inside the attention kernels; mpnet-base-nobias is the same
# shape as a RoBERTa handle (identical GEMMs, attention without the bias): what the bias costs is the difference of the two
MPNET_BASE = dict(XLMR_BASE, vocab_size=30527, model_type="mpnet", relative_attention_num_buckets=32)
MPNET_BASE_NOBIAS = dict(XLMR_BASE, vocab_size=30527)
# NomicBert (nomic-embed-text-v1 / -v1.5): H and heads of xlmr-base, no position table (rotary q / k in the QKV epilogue), a gated MLP (gate | up as one
# projection of 2 FF columns + the SwiGLU epilogue): 32 H^2 projection FLOPs per token and layer against 24 H^2
NOMIC_BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=30528, max_position_embeddings=8192,
                  type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="silu", model_type="nomic_bert", head_dim=64,
                  rope_parameters={"rope_theta": 1000.0, "rope_type": "default"})
# ModernBERT-base (gte-modernbert-base, modernbert-embed-base, granite-embedding-english-r2): pre-LN, GeGLU with FF 1152 (2 FF = 2304 columns in one
# projection), two of every three layers under a sliding window of +-64 columns; modernbert-base-global: the same with every layer global (a handle-level
# setting: transformers' own config cannot say it) — what the window saves is the difference of the two
MODERNBERT_BASE = dict(hidden_size=768, num_hidden_layers=22, num_attention_heads=12, intermediate_size=1152, vocab_size=50368, max_position_embeddings=8192,
                       norm_eps=1e-5, hidden_activation="gelu", model_type="modernbert", local_attention=128, sliding_window=64,
                       layer_types=["sliding_attention" if i % 3 else "full_attention" for i in range(22)],
                       rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": 160000.0},
                                        "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}})
MODERNBERT_BASE_GLOBAL = dict(MODERNBERT_BASE, layer_types=["full_attention"] * 22)
# T5 encoders (gtr-t5-base, sentence-t5-base: t5-base, relu feed-forward; instructor-base / flan: t5-base-gated = v1.1, FF 2048 with wi_0 | wi_1 as one
# projection of 4096 columns).  t5-base has mpnet-base's H, heads, FF, bias table, 24 H^2 projection FLOPs per token and layer and launch count: what the
# separate residual stream of the pre-LN stack costs is the difference of the two.  The BERT-style fields serve the synthetic draws and the FLOP count.
T5_KEYS = ("d_model", "d_kv", "num_heads", "d_ff", "num_layers", "vocab_size", "feed_forward_proj", "layer_norm_epsilon", "relative_attention_num_buckets",
           "relative_attention_max_distance")
T5_BASE = dict(d_model=768, d_kv=64, num_heads=12, d_ff=3072, num_layers=12, vocab_size=32128, feed_forward_proj="relu", dense_act_fn="relu", is_gated_act=False,
               layer_norm_epsilon=1e-6, relative_attention_num_buckets=32, relative_attention_max_distance=128, n_positions=512, model_type="t5",
               hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=512, type_vocab_size=1,
               layer_norm_eps=1e-6)
T5_BASE_GATED = dict(T5_BASE, d_ff=2048, intermediate_size=2048, feed_forward_proj="gated-gelu", dense_act_fn="gelu_new", is_gated_act=True)
# DeBERTa-v3-base (mxbai-rerank-base-v1, nli-deberta-v3-base): xlmr-base's H, heads and FF on a DeBERTa handle — no position table, 256 log buckets over 512
# relative positions, the two position terms of every score from k_pos_scores + the AM_DISENT attention: what they cost is the difference to xlmr-base
DEBERTA_V3_BASE = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, vocab_size=128100, max_position_embeddings=512,
                       type_vocab_size=0, layer_norm_eps=1e-7, hidden_act="gelu", model_type="deberta-v2", relative_attention=True, position_buckets=256,
                       max_relative_positions=-1, norm_rel_ebd="layer_norm", share_att_key=True, pos_att_type=["p2c", "c2p"], position_biased_input=False)
# Decoder-LLM embedders (causal attention, last-token or mean pooling): the Qwen2 / Qwen2.5-0.5B shape (KaLM-embedding-multilingual-mini: 14 heads of 64 over 2
# KV heads, q / k / v biases) and Llama-3.2-1B's (32 heads of 64 over 8 KV heads, no bias).  The handle gets k_proj / v_proj with the checkpoint's KV heads
# ([A, H]: native grouped-query attention); --expanded builds it from the [H, H] tensors of expand_kv instead (the same bits; + 9.2 % / + 10.3 % projection MACs
# by the shapes), --alternate-gqa times one handle of each kind in turns in this process.  --bidirectional: config.decoder_attention = 0 on the same stack —
# the A/B partner of the causal mask
DECODER_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "num_key_value_heads", "intermediate_size", "vocab_size", "max_position_embeddings",
                "rms_norm_eps", "hidden_act", "rope_parameters", "tie_word_embeddings")
QWEN2_05B = dict(hidden_size=896, num_hidden_layers=24, num_attention_heads=14, num_key_value_heads=2, intermediate_size=4864, vocab_size=151936,
                 max_position_embeddings=32768, rms_norm_eps=1e-6, hidden_act="silu", rope_parameters={"rope_theta": 1000000.0, "rope_type": "default"},
                 tie_word_embeddings=True, model_type="qwen2", type_vocab_size=1, layer_norm_eps=1e-6)
LLAMA_1B = dict(hidden_size=2048, num_hidden_layers=16, num_attention_heads=32, num_key_value_heads=8, intermediate_size=8192, vocab_size=128256,
                max_position_embeddings=131072, rms_norm_eps=1e-5, hidden_act="silu", tie_word_embeddings=True, model_type="llama", type_vocab_size=1, layer_norm_eps=1e-5,
                rope_parameters={"rope_theta": 500000.0, "rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                 "original_max_position_embeddings": 8192})
# EuroBERT-210m: the decoders' stack (12 x 64 over 12 KV heads, no bias) under a bidirectional mask; --alternate times it against its causal twin
EUROBERT_210M = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, num_key_value_heads=12, intermediate_size=3072, vocab_size=128256,
                     max_position_embeddings=8192, rms_norm_eps=1e-5, hidden_act="silu", rope_parameters={"rope_theta": 250000.0, "rope_type": "default"},
                     tie_word_embeddings=False, model_type="eurobert", type_vocab_size=1, layer_norm_eps=1e-5)
# jina-embeddings-v3: xlmr-large's stack (biases everywhere, erf-GELU, post-LN) without a position table and with rotary q / k (EPI_QKV_ROTB): what the
# position scheme costs is the difference to xlmr-large
JINA_KEYS = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "vocab_size", "max_position_embeddings", "type_vocab_size",
             "layer_norm_eps", "hidden_act", "rope_parameters")
JINA_V3 = dict(BS.E5_LARGE, vocab_size=250002, max_position_embeddings=8194, type_vocab_size=1, layer_norm_eps=1e-5, hidden_act="gelu", model_type="jina_embeddings_v3",
               rope_parameters={"rope_theta": 20000.0, "rope_type": "default"})
# Qwen3-Embedding-0.6B / Qwen3-Reranker-0.6B: head_dim is a config field of its own — 16 heads of 128 over 8 KV heads on hidden 1024 (q and the attention output
# are 2048 wide), an RMS norm over every head of q and k in front of the rotation, no bias
QWEN3_06B = dict(hidden_size=1024, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8, head_dim=128, intermediate_size=3072, vocab_size=151936,
                 max_position_embeddings=32768, rms_norm_eps=1e-6, hidden_act="silu", tie_word_embeddings=True, model_type="qwen3", type_vocab_size=1, layer_norm_eps=1e-6,
                 rope_parameters={"rope_theta": 1000000.0, "rope_type": "default"})
DECODER_TYPES = ("qwen2", "llama", "mistral", "eurobert", "qwen3")
SHAPES = dict(BS.ENCODER_SHAPES, **{"qwen2-0.5b": QWEN2_05B, "qwen3-0.6b": QWEN3_06B, "llama-1b": LLAMA_1B, "eurobert-210m": EUROBERT_210M, "jina-v3": JINA_V3}, **{"deberta-v3-base": DEBERTA_V3_BASE, "t5-base": T5_BASE, "t5-base-gated": T5_BASE_GATED, "modernbert-base": MODERNBERT_BASE, "modernbert-base-global": MODERNBERT_BASE_GLOBAL, "xlmr-base": XLMR_BASE, "xlmr-large": XLMR_LARGE, "bge-m3": BGE_M3, "mpnet-base": MPNET_BASE,
                                    "mpnet-base-nobias": MPNET_BASE_NOBIAS, "nomic-base": NOMIC_BASE, "xlmr-base-8k": XLMR_BASE_8K})

ap = argparse.ArgumentParser()
ap.add_argument("n", type=int, nargs="?", default=1024)
ap.add_argument("S", type=int, nargs="?", default=128)
ap.add_argument("ragged", nargs="?", default="")
ap.add_argument("--shape", action="append", choices=sorted(SHAPES))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hf-fp16", action="store_true")
ap.add_argument("--pool", default="mean", choices=["mean", "cls", "last"])
ap.add_argument("--bidirectional", action="store_true", help="decoder shapes: config.decoder_attention = 0 (no causal mask) on the same stack")
ap.add_argument("--alternate", action="store_true", help="decoder shapes: a causal and a bidirectional handle in this process, timed in turns (--reps rounds)")
ap.add_argument("--expanded", action="store_true", help="decoder shapes: build the handle from k_proj / v_proj expanded to [H, H] (expand_kv) instead of the grouped tensors")
ap.add_argument("--alternate-gqa", action="store_true", help="decoder shapes: a native and an expanded handle of the same weights in this process, timed in turns (--reps rounds)")
ap.add_argument("--alternate-tail", action="store_true", help="BERT shapes: three handles of the same weights — the plain masked mean, config.normalize_output = 0 and "
                "config.pool_tokens = 1 (max) — timed in turns in this process (--reps rounds of 3)")
ap.add_argument("--first-forward", action="store_true")
ap.add_argument("--alternate-shapes", action="store_true", help="one handle per --shape, timed in turns in this process (--reps rounds of 3)")
ap.add_argument("--digest", action="store_true", help="append the sha256 (16 hex digits) of the batch's embeddings")
args = ap.parse_args() if __name__ == "__main__" else ap.parse_args([])      # imported (tools/one_shape.py): SHAPES and make_encoder only
n, S, ragged = args.n, args.S, args.ragged == "ragged"
dev = torch.device("cuda:0")


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def hf_classes(cfg):
    """(config class, model class, sentence-encoder module) of a shape: the RoBERTa family by its model_type"""
    import transformers as T
    from kirag_amd.retriever import encoders as ENC
    if cfg.get("model_type") == ENC.T5_TYPE:
        def T5Config(**kw):
            return T.T5Config(**{k: kw[k] for k in T5_KEYS}, dropout_rate=0.0)
        def T5EncoderModel(config, add_pooling_layer=False):
            return T.T5EncoderModel(config)
        return T5Config, T5EncoderModel, (ENC.T5E5Encoder if args.pool == "mean" else ENC.T5BGEEncoder)
    if cfg.get("model_type") == ENC.DEBERTA_TYPE:
        def DebertaV2Model(config, add_pooling_layer=False):
            return T.DebertaV2Model(config)
        return T.DebertaV2Config, DebertaV2Model, (ENC.DebertaV2E5Encoder if args.pool == "mean" else ENC.DebertaV2BGEEncoder)
    if cfg.get("model_type") == ENC.MODERN_TYPE:
        return T.ModernBertConfig, T.ModernBertModel, (ENC.ModernBertE5Encoder if args.pool == "mean" else ENC.ModernBertBGEEncoder)
    if cfg.get("model_type") == ENC.NOMIC_TYPE:
        return T.NomicBertConfig, T.NomicBertModel, (ENC.NomicBertE5Encoder if args.pool == "mean" else ENC.NomicBertBGEEncoder)
    if cfg.get("model_type") == ENC.MPNET_TYPE:
        return T.MPNetConfig, T.MPNetModel, (ENC.MPNetE5Encoder if args.pool == "mean" else ENC.MPNetBGEEncoder)
    if cfg.get("model_type") in ENC.ROBERTA_TYPES:
        return T.XLMRobertaConfig, T.XLMRobertaModel, (ENC.XLMRobertaE5Encoder if args.pool == "mean" else ENC.XLMRobertaBGEEncoder)
    return T.BertConfig, T.BertModel, (ENC.E5Encoder if args.pool == "mean" else ENC.BGEEncoder)


def make_encoder(cfg, extra_state=None):
    """the HIP encoder with synthetic weights; an MPNet shape also gets a bias table N(0, 1) (it has to arrive before the handle's first finalize), a NomicBert
    shape the same draws under NomicBert's names (no position table, no linear biases, up_proj = a second draw).  extra_state: tensors and settings that must
    arrive with the first load (a head: tools/rerank_bench.py), by library name"""
    if cfg.get("model_type") in DECODER_TYPES:
        return make_decoder(cfg, not args.bidirectional, args.expanded, extra_state)
    if cfg.get("model_type") not in ("mpnet", "nomic_bert", "modernbert", "t5", "deberta-v2", "jina_embeddings_v3"):
        assert extra_state is None
        return BS.make_hip_encoder(dev, cfg)
    from types import SimpleNamespace
    from kirag_amd.retriever.encoders import HipBertForward
    ns = SimpleNamespace(**cfg)
    if cfg["model_type"] == "jina_embeddings_v3":      # HF's own rotary module is built from HF's own config
        import transformers as T
        enc = HipBertForward(T.JinaEmbeddingsV3Config(**{k: cfg[k] for k in JINA_KEYS}), 0)
    else:
        enc = HipBertForward(ns, 0)
    if cfg["model_type"] == "modernbert":      # synthetic_state reads BERT's field names
        ns = SimpleNamespace(**dict(cfg, type_vocab_size=1, layer_norm_eps=cfg["norm_eps"]))
    if cfg["model_type"] == "deberta-v2":
        ns = SimpleNamespace(**dict(cfg, type_vocab_size=1))
    state = dict(BS.synthetic_state(ns, dev, 0))
    g = torch.Generator(device=dev); g.manual_seed(977)
    if cfg["model_type"] == "modernbert":
        # the same draws under ModernBert's names: Wqkv = q | k | v, mlp.Wi = the intermediate matrix | a second draw, LayerNorm weights in their pre-LN places
        L, b = cfg["num_hidden_layers"], "encoder.layer."
        st = {"embeddings.tok_embeddings.weight": state["embeddings.word_embeddings.weight"], "embeddings.norm.weight": state["embeddings.LayerNorm.weight"],
              "final_norm.weight": state[f"{b}{L - 1}.output.LayerNorm.weight"]}
        for l in range(L):
            if l:
                st[f"layers.{l}.attn_norm.weight"] = state[f"{b}{l - 1}.output.LayerNorm.weight"]
            st[f"layers.{l}.attn.Wqkv.weight"] = torch.cat([state[f"{b}{l}.attention.self.{n}.weight"] for n in ("query", "key", "value")])
            st[f"layers.{l}.attn.Wo.weight"] = state[f"{b}{l}.attention.output.dense.weight"]
            st[f"layers.{l}.mlp_norm.weight"] = state[f"{b}{l}.attention.output.LayerNorm.weight"]
            wi = state[f"{b}{l}.intermediate.dense.weight"]
            st[f"layers.{l}.mlp.Wi.weight"] = torch.cat([wi, 0.02 * torch.randn(wi.shape, generator=g, device=dev)])
            st[f"layers.{l}.mlp.Wo.weight"] = state[f"{b}{l}.output.dense.weight"]
        state = st
    elif cfg["model_type"] == "t5":
        # the same draws under T5EncoderModel's names: no biases, no position table, the norms in their pre-LN places, wi_1 = a second draw, a table N(0, 1)
        L, b = cfg["num_layers"], "encoder.layer."
        st = {"shared.weight": state["embeddings.word_embeddings.weight"], "encoder.final_layer_norm.weight": state[f"{b}{L - 1}.output.LayerNorm.weight"],
              "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": torch.randn(32, cfg["num_heads"], generator=g, device=dev)}
        for l in range(L):
            p = f"encoder.block.{l}.layer."
            for n, t in (("query", "q"), ("key", "k"), ("value", "v")):
                st[f"{p}0.SelfAttention.{t}.weight"] = state[f"{b}{l}.attention.self.{n}.weight"]
            st[f"{p}0.SelfAttention.o.weight"] = state[f"{b}{l}.attention.output.dense.weight"]
            st[f"{p}0.layer_norm.weight"] = state[f"{b}{l - 1}.output.LayerNorm.weight"] if l else state["embeddings.LayerNorm.weight"]
            st[f"{p}1.layer_norm.weight"] = state[f"{b}{l}.attention.output.LayerNorm.weight"]
            wi = state[f"{b}{l}.intermediate.dense.weight"]
            if cfg["is_gated_act"]:
                st[f"{p}1.DenseReluDense.wi_0.weight"] = wi
                st[f"{p}1.DenseReluDense.wi_1.weight"] = 0.02 * torch.randn(wi.shape, generator=g, device=dev)
            else:
                st[f"{p}1.DenseReluDense.wi.weight"] = wi
            st[f"{p}1.DenseReluDense.wo.weight"] = state[f"{b}{l}.output.dense.weight"]
        state = st
    elif cfg["model_type"] == "deberta-v2":
        # the same draws under DebertaV2Model's names: no position and token-type tables, a position table N(0, 1) behind a unit LayerNorm
        st = {}
        for k, v in state.items():
            if "position_embeddings" in k or "token_type_embeddings" in k:
                continue
            for nm in ("query", "key", "value"):
                k = k.replace(f"attention.self.{nm}.", f"attention.self.{nm}_proj.")
            st[k] = v
        st["encoder.rel_embeddings.weight"] = torch.randn(2 * cfg["position_buckets"], cfg["hidden_size"], generator=g, device=dev)
        st["encoder.LayerNorm.weight"] = torch.ones(cfg["hidden_size"], device=dev)
        st["encoder.LayerNorm.bias"] = torch.zeros(cfg["hidden_size"], device=dev)
        state = st
    elif cfg["model_type"] == "jina_embeddings_v3":
        # the same draws under JinaEmbeddingsV3Model's names: every bias kept, no position table
        names = (("attention.self.query.", "self_attn.q_proj."), ("attention.self.key.", "self_attn.k_proj."), ("attention.self.value.", "self_attn.v_proj."),
                 ("attention.output.dense.", "self_attn.o_proj."), ("attention.output.LayerNorm.", "post_attention_layernorm."),
                 ("intermediate.dense.", "mlp.fc1."), ("output.dense.", "mlp.fc2."), ("output.LayerNorm.", "post_mlp_layernorm."))
        renamed = {}
        for k, v in state.items():
            if "position_embeddings" in k:
                continue
            k = k.replace("encoder.layer.", "layers.")
            for a, b in names:
                k = k.replace(a, b)
            renamed[k] = v
        state = renamed
    elif cfg["model_type"] == "nomic_bert":
        names = (("attention.self.query.", "self_attn.q_proj."), ("attention.self.key.", "self_attn.k_proj."), ("attention.self.value.", "self_attn.v_proj."),
                 ("attention.output.dense.", "self_attn.o_proj."), ("attention.output.LayerNorm.", "post_attention_layernorm."),
                 ("intermediate.dense.", "mlp.gate_proj."), ("output.dense.", "mlp.down_proj."), ("output.LayerNorm.", "post_mlp_layernorm."))
        renamed = {}
        for k, v in state.items():
            if "position_embeddings" in k or (k.endswith(".bias") and "LayerNorm" not in k):
                continue
            k = k.replace("encoder.layer.", "layers.")
            for a, b in names:
                k = k.replace(a, b)
            renamed[k] = v
            if "gate_proj" in k:
                renamed[k.replace("gate_proj", "up_proj")] = 0.02 * torch.randn(v.shape, generator=g, device=dev)
        state = renamed
    else:
        state["encoder.relative_attention_bias.weight"] = torch.randn(32, cfg["num_attention_heads"], generator=g, device=dev)
    enc.load_state(dict(state, **(extra_state or {})))
    enc.cfg = ns
    return enc


def make_decoder(cfg, causal=True, expanded=False, extra_state=None):
    """a decoder handle with synthetic weights under HF's names: the BERT-shaped draws renamed (no position table, no token types, the norms in their pre-LN
    places, up_proj a second draw), k_proj / v_proj cut to the checkpoint's KV heads — loaded as they are, or with `expanded` repeated per query head first
    (expand_kv) —, q / k / v biases for qwen2; extra_state: a head's tensors by library name, loaded with the rest"""
    from types import SimpleNamespace
    import transformers as T
    from kirag_amd.retriever.encoders import HipBertForward, expand_kv

    qwen3 = cfg["model_type"] == "qwen3"
    conf = {"qwen2": T.Qwen2Config, "llama": T.LlamaConfig, "mistral": T.MistralConfig, "eurobert": T.EuroBertConfig, "qwen3": T.Qwen3Config}[cfg["model_type"]](
        **{k: cfg[k] for k in DECODER_KEYS + (("head_dim",) if qwen3 else ())})
    enc = HipBertForward(conf, 0, decoder_attention=1.0 if causal else 0.0)
    ns = SimpleNamespace(**dict(cfg, max_position_embeddings=8))      # synthetic_state draws a position table of this many rows; it is dropped below
    state = dict(BS.synthetic_state(ns, dev, 0))
    g = torch.Generator(device=dev); g.manual_seed(977)
    L, b, H = cfg["num_hidden_layers"], "encoder.layer.", cfg["hidden_size"]
    d_h = cfg.get("head_dim") or H // cfg["num_attention_heads"]
    kv_rows, q_rows = d_h * cfg["num_key_value_heads"], d_h * cfg["num_attention_heads"]
    # (a Qwen3 shape: q_proj [q_rows, H] and o_proj [H, q_rows] with q_rows != H — drawn here like the BERT-shaped ones, 0.02 N(0, 1))
    wide = lambda r, c: 0.02 * torch.randn((r, c), generator=g, device=dev)
    st = {"embed_tokens.weight": state["embeddings.word_embeddings.weight"], "norm.weight": state[f"{b}{L - 1}.output.LayerNorm.weight"]}
    for l in range(L):
        p = f"layers.{l}."
        st[p + "input_layernorm.weight"] = state[f"{b}{l - 1}.output.LayerNorm.weight"] if l else state["embeddings.LayerNorm.weight"]
        st[p + "post_attention_layernorm.weight"] = state[f"{b}{l}.attention.output.LayerNorm.weight"]
        for nm, t, rows in (("query", "q", q_rows), ("key", "k", kv_rows), ("value", "v", kv_rows)):
            st[p + f"self_attn.{t}_proj.weight"] = state[f"{b}{l}.attention.self.{nm}.weight"][:rows].contiguous() if rows <= H else wide(rows, H)
            if cfg["model_type"] == "qwen2":
                st[p + f"self_attn.{t}_proj.bias"] = state[f"{b}{l}.attention.self.{nm}.bias"][:rows].contiguous()
        st[p + "self_attn.o_proj.weight"] = state[f"{b}{l}.attention.output.dense.weight"] if q_rows == H else wide(H, q_rows)
        if qwen3:
            st[p + "self_attn.q_norm.weight"] = 1.0 + 0.1 * torch.randn(d_h, generator=g, device=dev)
            st[p + "self_attn.k_norm.weight"] = 1.0 + 0.1 * torch.randn(d_h, generator=g, device=dev)
        wi = state[f"{b}{l}.intermediate.dense.weight"]
        st[p + "mlp.gate_proj.weight"] = wi
        st[p + "mlp.up_proj.weight"] = 0.02 * torch.randn(wi.shape, generator=g, device=dev)
        st[p + "mlp.down_proj.weight"] = state[f"{b}{l}.output.dense.weight"]
    if expanded:
        st = {k: expand_kv(k, v, cfg["num_attention_heads"], cfg["num_key_value_heads"]) for k, v in st.items()}
    st.update(extra_state or {})      # a head ("score.weight": tools/rerank_bench.py)
    enc.load_state(st)
    enc.cfg = SimpleNamespace(**cfg)
    return enc


def decoder_flops(cfg, lens, causal):
    """8 H Dq (q, k, v, o with k / v expanded; Dq = H unless head_dim is the shape's own) + 6 H FF per token and layer, 4 s Dq of attention per token — half of it under the causal mask"""
    lens = lens.double()
    H, FF = cfg["hidden_size"], cfg["intermediate_size"]
    Dq = cfg["num_attention_heads"] * cfg["head_dim"] if cfg.get("head_dim") else H      # the width of q and of the attention output (a Qwen3 shape: not H)
    return float((cfg["num_hidden_layers"] * lens * (8.0 * H * Dq + 6.0 * H * FF + (2.0 if causal else 4.0) * lens * Dq)).sum())


def first_forward(shape, cfg, ids, mask):
    conf_cls, _, mod_cls = hf_classes(cfg)
    m = mod_cls(conf_cls(**{k: v for k, v in cfg.items() if k != "model_type" and (k != "hidden_act" or v != "gelu")}), add_pooling_layer=False).to(dev).eval()

    def once():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m(ids, mask)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    a, b = once(), once()
    m.train(); m.eval()
    c, d = once(), once()
    print(f"{shape} module {mod_cls.__name__} n={n} S={S}: first eval forward {a:.0f} ms (weight sync), next {b:.2f} ms; after train() / eval(): {c:.0f} ms, next {d:.2f} ms",
          flush=True)


def digest(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def shape_tokens(cfg):
    ids, mask = BS.synthetic_tokens(dev, n, S, seed=1, ragged=ragged)
    if "pad_token_id" in cfg:
        ids = torch.where(mask != 0, ids, torch.full_like(ids, cfg["pad_token_id"]))      # fairseq's rule counts every column that does not hold the pad id
    return ids, mask


pool = {"mean": 0, "cls": 1, "last": 5}[args.pool]
if __name__ == "__main__" and args.alternate_shapes:
    # one process, one handle per shape, timed in turns: what separates two shapes is the difference of their medians, the spread is min .. max
    made = {shape: (make_encoder(SHAPES[shape]),) + shape_tokens(SHAPES[shape]) for shape in args.shape}
    times = {shape: [] for shape in made}
    for _ in range(args.reps):
        for shape, (e, ids, mask) in made.items():
            times[shape].append(timed(lambda: e.forward(ids, mask, pool), 3) * 1e3)
    for shape in made:
        t = sorted(times[shape])
        print(f"{shape} pool={args.pool} n={n} S={S} ragged={ragged}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}, {len(t)} rounds of 3 in turns)", flush=True)
    sys.exit(0)
for shape in (args.shape or ["e5-large"]) if __name__ == "__main__" else ():
    cfg = SHAPES[shape]
    ids, mask = shape_tokens(cfg)
    if args.first_forward:
        first_forward(shape, cfg, ids, mask)
        torch.cuda.empty_cache()
        continue
    if args.alternate_tail:
        # one process, three handles of the same weights, timed in turns: what a tail costs over the plain mean is the difference of the medians
        from types import SimpleNamespace
        from kirag_amd.retriever.encoders import HipBertForward, StPipeline
        assert cfg.get("model_type", "bert") == "bert", "--alternate-tail builds BERT handles"
        ns = SimpleNamespace(**cfg)
        state = dict(BS.synthetic_state(ns, dev, 0))
        trio = {}
        for k, pipe in (("mean", None), ("unnormalised", StPipeline("mean", normalize=False)), ("max", StPipeline("max"))):
            trio[k] = HipBertForward(ns, 0, pipeline_settings=pipe.settings() if pipe else ())
            trio[k].load_state(state)
        times = {k: [] for k in trio}
        for _ in range(args.reps):
            for k, e in trio.items():
                times[k].append(timed(lambda: e.forward(ids, mask, 0), 3) * 1e3)
        for k in trio:
            t = sorted(times[k])
            print(f"{shape} tail={k} n={n} S={S} ragged={ragged}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}, {len(t)} rounds of 3 in turns)", flush=True)
        del trio, state
        torch.cuda.empty_cache()
        continue
    if cfg.get("model_type") in DECODER_TYPES and args.alternate:
        # one process, two handles of the same weights, timed in turns: what the causal mask saves is the difference
        pair = {"causal": make_decoder(cfg, True), "bidirectional": make_decoder(cfg, False)}
        times = {k: [] for k in pair}
        for _ in range(args.reps):
            for k, e in pair.items():
                times[k].append(timed(lambda: e.forward(ids, mask, pool), 3) * 1e3)
        for k in pair:
            t = sorted(times[k])
            print(f"{shape} {k} pool={args.pool} n={n} S={S} ragged={ragged}: median {t[len(t) // 2]:.2f} ms (min {t[0]:.2f}, max {t[-1]:.2f}, {len(t)} rounds of 3 in turns)  "
                  f"{decoder_flops(cfg, mask.sum(1), k == 'causal') / (t[len(t) // 2] * 1e-3) / 1e12:.0f} TFLOP/s", flush=True)
        del pair
        torch.cuda.empty_cache()
        continue
    if cfg.get("model_type") in DECODER_TYPES and args.alternate_gqa:
        # one process, two handles of the same weights, timed in turns: what the grouped k / v columns save is the difference; the outputs must be the same bits
        pair = {"native": make_decoder(cfg, not args.bidirectional, False), "expanded": make_decoder(cfg, not args.bidirectional, True)}
        outs = {k: e.forward(ids, mask, pool).clone() for k, e in pair.items()}
        same = bool(torch.equal(outs["native"].view(torch.int32), outs["expanded"].view(torch.int32)))
        times = {k: [] for k in pair}
        for _ in range(args.reps):
            for k, e in pair.items():
                times[k].append(timed(lambda: e.forward(ids, mask, pool), 3) * 1e3)
        for k in pair:
            t = sorted(times[k])
            print(f"{shape} {k} pool={args.pool} n={n} S={S} ragged={ragged}: median {t[len(t) // 2]:.3f} ms (min {t[0]:.3f}, max {t[-1]:.3f}, {len(t)} rounds of 3 in turns)  "
                  f"outputs bit-identical: {same}", flush=True)
        del pair, outs
        torch.cuda.empty_cache()
        continue
    enc = make_encoder(cfg)
    fl = BS.encoder_flops(enc.cfg, mask.sum(1))
    if cfg.get("model_type") in DECODER_TYPES:
        fl = decoder_flops(cfg, mask.sum(1), not args.bidirectional)
    if cfg.get("model_type") == "nomic_bert":      # the third intermediate matrix: + 8 H^2 per token and layer (FF = 4 H)
        fl += float(mask.sum()) * cfg["num_hidden_layers"] * 8.0 * cfg["hidden_size"] ** 2
    if cfg.get("model_type") == "modernbert":      # FF is not 4 H: 8 H^2 (q, k, v, o) + 6 H FF (input, gate, out) per token and layer; the attention FLOPs are
        lens = mask.sum(1).double()                # counted as global in both shapes (what the window saves shows as rate)
        fl = float((cfg["num_hidden_layers"] * lens * (8.0 * cfg["hidden_size"] ** 2 + 6.0 * cfg["hidden_size"] * cfg["intermediate_size"] + 4.0 * lens * cfg["hidden_size"])).sum())
    if cfg.get("model_type") == "t5" and cfg["is_gated_act"]:      # 8 H^2 (q, k, v, o) + 6 H FF (wi_0, wi_1, wo) per token and layer
        lens = mask.sum(1).double()
        fl = float((cfg["num_layers"] * lens * (8.0 * cfg["hidden_size"] ** 2 + 6.0 * cfg["hidden_size"] * cfg["d_ff"] + 4.0 * lens * cfg["hidden_size"])).sum())
    dt = timed(lambda: enc.forward(ids, mask, pool), args.reps)
    print(f"{shape} (H {cfg['hidden_size']}, {cfg['num_attention_heads']} heads of {cfg.get('head_dim') or cfg['hidden_size'] // cfg['num_attention_heads']}, L {cfg['num_hidden_layers']}) "
          f"tile={os.environ.get('KIRAG_AMD_PROJ_TILE','auto')} pool={args.pool} n={n} S={S} ragged={ragged}: {dt*1e3:.2f} ms  {n/dt:.0f} seq/s  {fl/dt/1e12:.0f} TFLOP/s  "
          f"{fl/dt/PEAK_MFMA_DENSE_16BIT:.3f} of MFMA peak  ({fl/n/1e9:.2f} GFLOP per sequence)" + (f"  sha256 {digest(enc.forward(ids, mask, pool))}" if args.digest else ""), flush=True)
    del enc
    if args.hf_fp16:
        conf_cls, model_cls, _ = hf_classes(cfg)
        m = model_cls(conf_cls(**{k: v for k, v in cfg.items() if k != "model_type" and (k != "hidden_act" or v != "gelu")}), add_pooling_layer=False).to(dev).half().eval()
        with torch.no_grad():
            dt = timed(lambda: m(input_ids=ids, attention_mask=mask).last_hidden_state, args.reps)
        print(f"{shape} HF {model_cls.__name__} fp16 (yardstick) n={n} S={S} ragged={ragged}: {dt*1e3:.2f} ms  {n/dt:.0f} seq/s  {fl/dt/1e12:.0f} TFLOP/s", flush=True)
        del m
    torch.cuda.empty_cache()
