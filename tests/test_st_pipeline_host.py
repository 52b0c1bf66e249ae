"""Host-side tests of the sentence-transformers tail (no GPU): the rules of the three reserved settings and of the head st_dense.* (kirag_amd/csrc/encoder_model.hpp
through the stand-alone program tests/capi/st_model_check.cpp), read_st_pipeline on folders written here, the ``pipeline="checkpoint"`` kwarg of the twins with its
save / load round trip and train()-mode forward, ContrieverEncoder, and the DistilBERT family's name map and refusals.  On a tree without the feature
"config.normalize_output" is an unknown setting, "st_dense.weight" an unknown tensor, ``read_st_pipeline`` does not exist and "distilbert" is no family."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import st_util as U  # noqa: E402
from oracle import encoder_np as E  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, L, HEADS, FF, VOCAB, MAX_POS = 128, 1, 2, 256, 100, 64
NORM, TOK, ACT = U.SETTINGS


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("st_model") / "st_model_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", "st_model_check.cpp"), "-o", exe])

    def run(lines, type_vocab=2, layers=L):
        text = ["config %d %d %d %d %d %d %d" % (H, layers, HEADS, FF, VOCAB, MAX_POS, type_vocab)]
        for ln in lines:
            text.append(" ".join([ln[0]] + ([ln[1]] if len(ln) > 1 else []) + ([" ".join("%r" % float(x) for x in ln[2])] if ln[0] == "setting" else [str(int(ln[2]))] if ln[0] == "tensor" else [])))
        p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = []
        for row in p.stdout.splitlines():
            head, tail = row.split(" rc=", 1)
            rc, _, msg = tail.partition(" ")
            out.append({"rc": int(rc), "msg": msg, "slot": head.split("slot=")[1].split()[0] if "slot=" in head else None})
        return out
    return run


def bert_tensors():
    return [("tensor", k, v.size) for k, v in E.synth_weights(H, L, FF, VOCAB, MAX_POS, seed=1).items()]


def plan_of(row):
    assert row["rc"] == 0 and row["msg"].startswith("plan "), row
    return dict(kv.split("=") for kv in row["msg"].split()[1:])


def test_setting_ranges_counts_and_the_known_list(run):
    for name, bad in ((NORM, [2]), (NORM, [-1]), (NORM, [0.5]), (TOK, [3]), (TOK, [-1]), (TOK, [1.5]), (ACT, [2]), (ACT, [-1])):
        r = run([("setting", name, bad)])[0]
        assert r["rc"] != 0 and name in r["msg"] and "expected" in r["msg"], r
    for name in U.SETTINGS:
        r = run([("setting", name, [0, 1])])[0]
        assert r["rc"] != 0 and "takes one value" in r["msg"], r
        assert run([("setting", name, [1])])[0]["rc"] == 0
    r = run([("setting", "config.no_such_thing", [1])])[0]
    assert r["rc"] != 0 and r["msg"].endswith("config.decoder_attention)") and all(n in r["msg"] for n in U.SETTINGS), r


def test_a_handle_without_any_of_it_finalizes_to_todays_plan(run):
    p = plan_of(run(bert_tensors() + [("finalize",)])[-1])
    assert p == {"family": "1", "heads": "00000000", "out_dim": str(H), "out_width": str(H), "normalize": "1", "pool_tokens": "0", "st_tanh": "0", "ws": "0", "zero_fill": str(L)}, p      # (zero_fill: the second half of a gated projection, which a BERT layer does not have)


def test_settings_and_the_head_reach_the_plan(run):
    rows = run(bert_tensors() + [("setting", NORM, [0]), ("setting", TOK, [1]), ("finalize",)])
    p = plan_of(rows[-1])
    assert (p["normalize"], p["pool_tokens"], p["out_dim"], p["heads"]) == ("0", "1", str(H), "00000000")
    rows = run(bert_tensors() + [("tensor", "st_dense.weight", 132 * H), ("tensor", "st_dense.bias", 132), ("setting", ACT, [1]), ("setting", TOK, [2]), ("finalize",)])
    p = plan_of(rows[-1])
    assert (p["out_dim"], p["out_width"], p["st_tanh"], p["pool_tokens"], p["normalize"], p["heads"], p["ws"]) == ("132", "132", "1", "2", "1", "00000001", "1"), p
    # a Dense without a bias is whole; its activation defaults to the identity
    p = plan_of(run(bert_tensors() + [("tensor", "st_dense.weight", 4 * H), ("finalize",)])[-1])
    assert (p["out_dim"], p["st_tanh"]) == ("4", "0")


def test_after_the_first_finalize(run):
    base = bert_tensors()
    rows = run(base + [("finalize",), ("setting", NORM, [1]), ("setting", TOK, [0]), ("setting", NORM, [0]), ("setting", TOK, [1]), ("setting", ACT, [0]),
                       ("tensor", "st_dense.weight", 8 * H)])
    n = len(base)
    assert rows[n]["rc"] == 0 and rows[n + 1]["rc"] == 0 and rows[n + 2]["rc"] == 0          # the defaults again: a no-op
    for r, name in ((rows[n + 3], NORM), (rows[n + 4], TOK)):
        assert r["rc"] != 0 and name in r["msg"] and "after kr_encoder_finalize" in r["msg"], r
    assert rows[n + 5]["rc"] != 0 and "after kr_encoder_finalize" in rows[n + 5]["msg"] and "Dense head" in rows[n + 5]["msg"], rows[n + 5]
    assert rows[n + 6]["rc"] != 0 and "after kr_encoder_finalize" in rows[n + 6]["msg"], rows[n + 6]
    # with the head: same shape reloads, another P is refused, the activation is known and fixed
    rows = run(base + [("tensor", "st_dense.weight", 8 * H), ("setting", ACT, [1]), ("finalize",), ("tensor", "st_dense.weight", 8 * H), ("tensor", "st_dense.bias", 8),
                       ("tensor", "st_dense.weight", 12 * H), ("setting", ACT, [1]), ("setting", ACT, [0])])
    assert [r["rc"] == 0 for r in rows[n + 2:]] == [True, True, True, False, True, False], rows[n + 2:]
    assert "P = 12" in rows[n + 5]["msg"] and "fixed" in rows[n + 5]["msg"]


def test_the_heads_shape_rule_and_a_bias_alone(run):
    for P in (0, 2, 2052, 6):
        r = run([("tensor", "st_dense.weight", P * H)])[0]
        assert r["rc"] != 0 and "st_dense.weight" in r["msg"] and "4 <= P <= 2048" in r["msg"] and "P % 4 == 0" in r["msg"], (P, r)
    r = run([("tensor", "st_dense.weight", 8 * H + 1)])[0]
    assert r["rc"] != 0
    rows = run([("tensor", "st_dense.weight", 8 * H), ("tensor", "st_dense.bias", 12)])
    assert rows[0]["rc"] == 0 and rows[1]["rc"] != 0 and "P = 12" in rows[1]["msg"]
    r = run(bert_tensors() + [("tensor", "st_dense.bias", 8), ("finalize",)])[-1]
    assert r["rc"] != 0 and "'st_dense.weight' was never loaded" in r["msg"], r
    r = run(bert_tensors() + [("setting", ACT, [1]), ("finalize",)])[-1]
    assert r["rc"] != 0 and ACT in r["msg"] and "st_dense.weight" in r["msg"], r


OTHER_HEADS = {
    "mlm": [("cls.predictions.transform.dense.weight", H * H), ("cls.predictions.transform.dense.bias", H), ("cls.predictions.transform.LayerNorm.weight", H),
            ("cls.predictions.transform.LayerNorm.bias", H), ("cls.predictions.decoder.weight", VOCAB * H), ("cls.predictions.decoder.bias", VOCAB)],
    "colbert": [("colbert_linear.weight", 128 * H), ("colbert_linear.bias", 128)],
    "sparse": [("sparse_linear.weight", H), ("sparse_linear.bias", 1)],
    "cls": [("classifier.dense.weight", H * H), ("classifier.dense.bias", H), ("classifier.out_proj.weight", 2 * H), ("classifier.out_proj.bias", 2)],
}


@pytest.mark.parametrize("other", sorted(OTHER_HEADS))
def test_never_next_to_another_head(run, other):
    head = [("tensor", n, k) for n, k in OTHER_HEADS[other]]
    first = OTHER_HEADS[other][0][0].split(".")[0]       # the library names a head by its first tensor, or by "classifier.*"
    for name in (NORM, TOK):
        r = run(bert_tensors() + head + [("setting", name, [0 if name == NORM else 1]), ("finalize",)])[-1]
        assert r["rc"] == -22 and name in r["msg"] and first in r["msg"], r
    r = run(bert_tensors() + head + [("tensor", "st_dense.weight", 8 * H), ("finalize",)])[-1]
    assert r["rc"] == -22 and "st_dense" in r["msg"] and first in r["msg"], r
    r = run(bert_tensors() + head + [("tensor", "st_dense.weight", 8 * H), ("setting", ACT, [1]), ("finalize",)])[-1]
    assert r["rc"] == -22 and "st_dense" in r["msg"] and first in r["msg"], r
    assert run(bert_tensors() + head + [("finalize",)])[-1]["rc"] == 0          # the other head alone is what it was


def _family_handles():
    """complete T5, ModernBert and decoder handles (settings + every tensor of the family) and the head each family alone takes: name -> (lines, head lines, the
    name the library calls the head by)"""
    import decoder_util as D
    import modernbert_util as MB
    import t5_util as T
    t = lambda w: [("tensor", k, np.asarray(v).size) for k, v in w.items()]
    t5 = [("setting", "config.t5_feed_forward", [0])] + t(T.weights(H, L, HEADS, FF, VOCAB))
    modern = ([("setting", "config.rotary_inv_freq", MB.inv_freq(H // HEADS, 10000.0)), ("setting", "config.local_attention_layers", [0] * L)] +
              t(MB.weights(H, L, FF, VOCAB)) + [("tensor", "embeddings.token_type_embeddings.weight", H)])
    dcfg = D.hf_config("llama-64", L=L, max_pos=MAX_POS)
    dw = {k: (np.zeros((VOCAB, H), np.float32) if k == "embed_tokens.weight" else v) for k, v in D.weights(dcfg).items()}
    dec = [("setting", "config.rotary_inv_freq", MB.inv_freq(H // HEADS, 100.0)), ("setting", "config.decoder_attention", [1])] + t(dw)
    return {"t5": (t5, [("tensor", "dense.weight", 8 * H)], "dense.weight"),
            "modern": (modern, [("tensor", "head.dense.weight", H * H), ("tensor", "head.norm.weight", H), ("tensor", "classifier.weight", 2 * H), ("tensor", "classifier.bias", 2)],
                       "head.dense.weight"),
            "decoder": (dec, [("tensor", "score.weight", 2 * H)], "score.weight")}


KR_EINVAL = -22


@pytest.mark.parametrize("family", ["t5", "modern", "decoder"])
def test_never_next_to_the_t5_dense_the_modern_or_the_score_head(run, family):
    """On COMPLETE handles: the family's own head alone finalizes, the new settings and the new head alone finalize, and either next to the family's head is KR_EINVAL
    naming both sides — so nothing but the coexistence rule of describe() can be what refuses."""
    base, head, first = _family_handles()[family]
    assert plan_of(run(base + [("finalize",)], type_vocab=1)[-1])["heads"] == "00000000"
    assert run(base + head + [("finalize",)], type_vocab=1)[-1]["rc"] == 0
    p = plan_of(run(base + [("setting", NORM, [0]), ("setting", TOK, [1]), ("tensor", "st_dense.weight", 8 * H), ("setting", ACT, [1]), ("finalize",)], type_vocab=1)[-1])
    assert (p["heads"], p["normalize"], p["pool_tokens"], p["st_tanh"], p["out_dim"]) == ("00000001", "0", "1", "1", "8")      # every family takes the tail
    for name, value in ((NORM, 0), (TOK, 1)):
        r = run(base + head + [("setting", name, [value]), ("finalize",)], type_vocab=1)[-1]
        assert r["rc"] == KR_EINVAL and name in r["msg"] and f"'{first}'" in r["msg"], r
    r = run(base + head + [("tensor", "st_dense.weight", 8 * H), ("finalize",)], type_vocab=1)[-1]
    assert r["rc"] == KR_EINVAL and "'st_dense.*'" in r["msg"] and f"'{first}'" in r["msg"], r
    r = run(base + head + [("tensor", "st_dense.weight", 8 * H), ("setting", ACT, [1]), ("finalize",)], type_vocab=1)[-1]
    assert r["rc"] == KR_EINVAL and "st_dense" in r["msg"] and f"'{first}'" in r["msg"], r


# ---- read_st_pipeline ----
def _folder(tmp_path, name, **kw):
    d = str(tmp_path / name)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"model_type": kw.pop("model_type", "bert"), "hidden_size": H}, f)
    U.write_pipeline(d, H, **kw)
    return d


def test_read_st_pipeline_accepts(tmp_path):
    from kirag_amd.retriever.encoders import read_st_pipeline
    assert read_st_pipeline(str(tmp_path), H) is None                      # no modules.json: as if the kwarg were absent
    W, b = U.dense_weights(H, 132)
    for pooling in ("cls", "mean", "max", "mean_sqrt_len"):
        for normalize in (True, False):
            p = read_st_pipeline(_folder(tmp_path, f"{pooling}{normalize}", pooling=(pooling,), normalize=normalize), H)
            assert (p.pooling, p.normalize, p.dense_weight, p.activation) == (pooling, normalize, None, "identity")
    p = read_st_pipeline(_folder(tmp_path, "last", pooling=("last",), model_type="qwen2"), H)
    assert p.pooling == "last"
    for act, bias, binfile in ((U.IDENTITY, True, False), (U.TANH, True, True), (U.TANH, False, False), (U.IDENTITY, False, True)):
        p = read_st_pipeline(_folder(tmp_path, f"d{act[-4:]}{bias}", pooling=("cls",), dense=(W, b if bias else None, act), torch_bin=binfile), H)
        assert p.activation == ("tanh" if act == U.TANH else "identity") and np.array_equal(p.dense_weight.numpy(), W)
        assert (p.dense_bias is None) == (not bias) and (not bias or np.array_equal(p.dense_bias.numpy(), b))
    s = dict((n, float(t[0])) for n, t in read_st_pipeline(_folder(tmp_path, "s", pooling=("max",), normalize=False, dense=(W, b, U.TANH)), H).settings())
    assert s == {NORM: 0.0, TOK: 1.0, ACT: 1.0}
    assert read_st_pipeline(_folder(tmp_path, "plain", pooling=("mean",)), H).settings() == ()


def test_read_st_pipeline_refuses_by_name(tmp_path, monkeypatch):
    import kirag_amd.retriever.encoders as ENC
    W, b = U.dense_weights(H, 8)
    cases = {
        "two_modes": (dict(pooling=("cls", "mean")), "pooling_mode_cls_token"),
        "weighted": (dict(pooling=("weightedmean",)), "pooling_mode_weightedmean_tokens"),
        "prompt": (dict(pooling=("mean",), include_prompt=False), "include_prompt"),
        "second_dense": (dict(pooling=("mean",), dense=(W, b, U.TANH), second_dense=True), "second Dense"),
        "in_features": (dict(pooling=("mean",), dense=(W[:, :64], b, U.TANH)), "in_features=64"),
        "out_features": (dict(pooling=("mean",), dense=(W[:6], b[:6], U.TANH)), "out_features=6"),
        "out_big": (dict(pooling=("mean",), dense=(W, b, U.TANH), dense_config={"out_features": 2052}), "out_features=2052"),
        "activation": (dict(pooling=("mean",), dense=(W, b, "torch.nn.modules.activation.ReLU")), "activation_function"),
        "norm_first": (dict(pooling=("mean",), dense=(W, b, U.TANH), normalize_before_dense=True), "Normalize in front of the Dense"),
        "layernorm": (dict(pooling=("mean",), extra_modules=(U.ST + "LayerNorm",)), "LayerNorm"),
        "wlp": (dict(pooling=("mean",), extra_modules=(U.ST + "WeightedLayerPooling",)), "WeightedLayerPooling"),
        "cnn": (dict(pooling=("mean",), extra_modules=(U.ST + "CNN",)), "CNN"),
        "router": (dict(pooling=("mean",), extra_modules=(U.ST + "Router",)), "Router"),
        "last_on_bert": (dict(pooling=("last",)), "pooling_mode_lasttoken"),
    }
    # a refusal comes before a weight is read
    monkeypatch.setattr(torch, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a weight was read")))
    import safetensors.torch
    monkeypatch.setattr(safetensors.torch, "load_file", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a weight was read")))
    for name, (kw, word) in cases.items():
        with pytest.raises(NotImplementedError) as ei:
            ENC.read_st_pipeline(_folder(tmp_path, name, **kw), H)
        assert word in str(ei.value), (name, str(ei.value))


def test_the_older_readers_are_what_they_were(tmp_path):
    from kirag_amd.retriever.encoders import read_st_dense, read_st_pooling
    W, b = U.dense_weights(H, 8)
    with pytest.raises(NotImplementedError, match="bias=True"):
        read_st_dense(_folder(tmp_path, "b", pooling=("mean",), dense=(W, b, U.IDENTITY)), H)
    with pytest.raises(NotImplementedError, match="pooling_mode_max_tokens"):
        read_st_pooling(_folder(tmp_path, "m", pooling=("max",)))


# ---- the kwarg on the twins, on the CPU ----
def _bert(tmp_path, name="bert"):
    from transformers import BertConfig, BertModel
    torch.manual_seed(3)
    m = BertModel(BertConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=2, intermediate_size=FF, vocab_size=VOCAB, max_position_embeddings=MAX_POS,
                             hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), add_pooling_layer=False)
    d = str(tmp_path / name)
    m.save_pretrained(d)
    return d, m.eval()


def _mpnet(tmp_path):
    from transformers import MPNetConfig, MPNetModel
    torch.manual_seed(4)
    m = MPNetModel(MPNetConfig(hidden_size=H, num_hidden_layers=1, num_attention_heads=2, intermediate_size=FF, vocab_size=VOCAB, max_position_embeddings=MAX_POS + 2,
                               hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), add_pooling_layer=False)
    d = str(tmp_path / "mpnet")
    m.save_pretrained(d)
    return d, m.eval()


def _qwen2(tmp_path):
    import decoder_util as D
    cfg = D.hf_config("llama-64", L=1, max_pos=MAX_POS)
    m = D.hf_model(cfg, D.weights(cfg))
    d = str(tmp_path / "llama")
    m.save_pretrained(d)
    return d, m


@pytest.mark.parametrize("family", ["bert", "mpnet", "decoder"])
def test_the_kwarg_on_a_twin_round_trip_and_train_mode(tmp_path, family):
    from kirag_amd.retriever.encoders import E5Encoder, BGEEncoder, LlamaE5Encoder, MPNetE5Encoder
    from kirag_amd.retriever.retrievers import BaseRetriever
    d, hf = {"bert": _bert, "mpnet": _mpnet, "decoder": _qwen2}[family](tmp_path)
    W, b = U.dense_weights(H, 132, seed=5)
    pooling = {"bert": "cls", "mpnet": "max", "decoder": "mean_sqrt_len"}[family]
    U.write_pipeline(d, H, pooling=(pooling,), dense=(W, b, U.TANH), normalize=False)
    ret = BaseRetriever("E5Retriever", d, retriever_kwargs={"pipeline": "checkpoint"})        # the registry class only selects the family twin
    m = ret.encoder
    assert type(m) is {"bert": E5Encoder, "mpnet": MPNetE5Encoder, "decoder": LlamaE5Encoder}[family]
    assert m._st.pooling == pooling and not m._st.normalize and m._st.activation == "tanh" and m.embedding_size == 132 and ret.hidden_size == 132
    assert m._pool == (U.POOL_CLS if pooling == "cls" else U.POOL_MEAN)
    names = dict(m.named_parameters())
    assert tuple(names["st_dense.weight"].shape) == (132, H) and tuple(names["st_dense.bias"].shape) == (132,)
    ids, mask = U.tokens(3, 12, "R", 1, vocab=VOCAB)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    m.train()
    with torch.no_grad():
        got = m(ti, tm)
        want = U.tail_torch(hf(input_ids=ti, attention_mask=tm).last_hidden_state, tm, pooling, W, b, "tanh", normalize=False)
    assert got.shape == (3, 132) and torch.allclose(got, want, atol=1e-6, rtol=0), float((got - want).abs().max())
    assert float((got.norm(dim=1) - 1).abs().min()) > 1e-2                  # not normalised
    # eval mode is the HIP path: a CPU model raises, it does not fall back
    with pytest.raises(RuntimeError, match="HIP path"):
        m.eval()(ti, tm)
    # round trip of the four files
    out = str(tmp_path / "saved")
    m.save_pretrained(out)
    for f in ("modules.json", "1_Pooling/config.json", "2_Dense/config.json", "2_Dense/model.safetensors"):
        assert os.path.exists(os.path.join(out, f)), f
    kinds = [x["type"].rsplit(".", 1)[1] for x in json.load(open(os.path.join(out, "modules.json")))]
    assert kinds == ["Transformer", "Pooling", "Dense"]                       # no Normalize was read, none is written
    from safetensors import safe_open
    main = [f for f in os.listdir(out) if f.endswith(".safetensors")]
    with safe_open(os.path.join(out, main[0]), "pt") as f:
        assert not any(k.startswith("st_dense") for k in f.keys())
    m2 = (BGEEncoder if family != "decoder" else LlamaE5Encoder).from_pretrained(out, pipeline="checkpoint").train()
    assert m2._st == m._st and m2._pool == m._pool
    with torch.no_grad():
        assert torch.equal(m2(ti, tm), got)
    # without the kwarg: the class's own tail, as ever
    if family == "decoder":       # the decoder twins read 1_Pooling on their own and go on refusing what they always refused
        with pytest.raises(NotImplementedError, match="pooling_mode_mean_sqrt_len_tokens"):
            type(m).from_pretrained(out)
        return
    m3 = type(m).from_pretrained(out).train()
    assert m3._st is None and getattr(m3, "st_dense", None) is None and m3.embedding_size == H
    with torch.no_grad():
        own = m3(ti, tm)
        lh = hf(input_ids=ti, attention_mask=tm).last_hidden_state
        assert torch.allclose(own, U.tail_torch(lh, tm, "mean"), atol=1e-6, rtol=0)


def test_a_folder_without_modules_json_and_a_bad_kwarg(tmp_path):
    from kirag_amd.retriever.encoders import E5Encoder
    d, _ = _bert(tmp_path)
    m = E5Encoder.from_pretrained(d, pipeline="checkpoint")
    assert m._st is None and "_pool" not in m.__dict__
    with pytest.raises(ValueError, match="pipeline="):
        E5Encoder.from_pretrained(d, pipeline="folder")


def test_t5_keeps_its_own_dense_path_for_a_bias_free_identity_dense(tmp_path):
    from transformers import T5Config, T5EncoderModel
    from kirag_amd.retriever.encoders import T5E5Encoder
    torch.manual_seed(1)
    hf = T5EncoderModel(T5Config(d_model=H, d_kv=64, num_heads=2, d_ff=FF, num_layers=1, vocab_size=VOCAB, dropout_rate=0.0))
    d = str(tmp_path / "t5")
    hf.save_pretrained(d)
    W, b = U.dense_weights(H, 8)
    U.write_pipeline(d, H, pooling=("mean",), dense=(W, None, U.IDENTITY))
    m = T5E5Encoder.from_pretrained(d, pipeline="checkpoint")
    assert m._st is None and m.dense is not None and getattr(m, "st_dense", None) is None      # dense.weight, bit for bit
    U.write_pipeline(d, H, pooling=("mean",), dense=(W, b, U.TANH))
    m = T5E5Encoder.from_pretrained(d, pipeline="checkpoint")
    assert m._st is not None and m.dense is None and m.st_dense.bias is not None


def test_contriever_encoder(tmp_path):
    from kirag_amd.retriever.encoders import ContrieverEncoder
    from kirag_amd.retriever.retrievers import RETRIEVER_MAP
    assert ContrieverEncoder not in RETRIEVER_MAP.values() and sorted(RETRIEVER_MAP) == ["BGERetriever", "E5Retriever"]
    d, hf = _bert(tmp_path)
    m = ContrieverEncoder.from_pretrained(d).train()
    assert dict((n, float(t[0])) for n, t in m._st.settings()) == {NORM: 0.0}
    ids, mask = U.tokens(3, 12, "R", 2, vocab=VOCAB)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    with torch.no_grad():
        got = m(ti, tm)
        lh = hf(input_ids=ti, attention_mask=tm).last_hidden_state
        # the reference's arithmetic (retriever/encoders.py:93-95)
        want = lh.masked_fill(~tm[..., None].bool(), 0.0).sum(dim=1) / tm.sum(dim=1)[..., None]
    assert torch.equal(got, want)
    out = str(tmp_path / "c")
    m.save_pretrained(out)
    assert not os.path.exists(os.path.join(out, "modules.json"))            # the reference's class writes HF's files only


# ---- DistilBERT ----
def test_distilbert_every_key_is_consumed_exactly_once(run):
    from kirag_amd.retriever.encoders import FAMILIES, DistilBertBGEEncoder, DistilBertE5Encoder, describe_distilbert, distilbert_rename, family_of
    cfg = U.distil_config(H, 2, HEADS, FF, VOCAB, MAX_POS)
    fam = family_of("distilbert")
    assert fam is FAMILIES["distilbert"] and fam.twins == (DistilBertE5Encoder, DistilBertBGEEncoder) and not fam.token_types
    spec = describe_distilbert(cfg)
    assert spec.cfg == (H, 2, HEADS, FF, VOCAB, MAX_POS, 1, 1e-12) and spec.settings == ()
    m = DistilBertE5Encoder(cfg)
    state = m.state_dict()
    assert sorted(state) == sorted(n for n, _ in m.named_parameters())       # nothing but parameters: the weight sync sees every key
    lines = [("tensor", distilbert_rename(k), v.numel()) for k, v in state.items()]
    rows = run(lines + [("tensor", "embeddings.token_type_embeddings.weight", H), ("finalize",)], type_vocab=1, layers=2)
    slots = [r["slot"] for r in rows[:len(state)]]
    assert all(r["rc"] == 0 for r in rows), [r for r in rows if r["rc"]]
    assert len(set(slots)) == len(slots) and all(int(s) >= 0 for s in slots)  # every key a slot of its own, none ignored
    p = plan_of(rows[-1])
    assert p["family"] == "1" and p["zero_fill"] == "2"                      # a complete BERT handle: nothing to fill but the gated half a BERT layer does not have
    with pytest.raises(KeyError):
        distilbert_rename("pooler.dense.weight")


def test_distilbert_refusals_name_the_field(tmp_path):
    from kirag_amd.retriever.encoders import BGEEncoder, check_distilbert_config
    ok = dict(dim=H, n_layers=1, n_heads=2, hidden_dim=FF, vocab_size=VOCAB, max_position_embeddings=MAX_POS, model_type="distilbert")
    check_distilbert_config(ok)
    for field, value, word in (("activation", "relu", "activation='relu'"), ("dim", 96, "dim=96"), ("dim", 2176, "dim=2176"), ("n_heads", 8, "n_heads=8"),
                               ("hidden_dim", 200, "hidden_dim=200")):
        with pytest.raises(NotImplementedError) as ei:
            check_distilbert_config({**ok, field: value})
        assert str(ei.value).startswith("model_type='distilbert':") and word in str(ei.value), str(ei.value)
    # from config.json alone, through the registry class, before a weight is read
    d = str(tmp_path / "relu")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({**ok, "activation": "relu"}, f)
    with pytest.raises(NotImplementedError, match="activation='relu'"):
        BGEEncoder.from_pretrained(d)


def test_distilbert_twin_train_mode_and_dispatch(tmp_path):
    from kirag_amd.retriever.encoders import DistilBertBGEEncoder, DistilBertE5Encoder, E5Encoder, BGEEncoder
    cfg = U.distil_config(H, 1, HEADS, FF, VOCAB, MAX_POS, sinusoidal_pos_embds=True)
    w = U.to_distil_names(E.synth_weights(H, 1, FF, VOCAB, MAX_POS, seed=2))
    hf = U.distil_model(cfg, w)
    d = str(tmp_path / "distil")
    hf.save_pretrained(d)
    e5, bge = E5Encoder.from_pretrained(d), BGEEncoder.from_pretrained(d)
    assert type(e5) is DistilBertE5Encoder and type(bge) is DistilBertBGEEncoder
    ids, mask = U.tokens(3, 12, "R", 3, vocab=VOCAB)
    ti, tm = torch.from_numpy(ids), torch.from_numpy(mask)
    with torch.no_grad():
        lh = hf(input_ids=ti, attention_mask=tm).last_hidden_state
        assert torch.allclose(e5.train()(ti, tm), U.tail_torch(lh, tm, "mean"), atol=1e-6, rtol=0)
        assert torch.allclose(bge.train()(ti, tm), U.tail_torch(lh, tm, "cls"), atol=1e-6, rtol=0)
    # the position table travels as it stands in the state dict
    assert "embeddings.position_embeddings.weight" in dict(e5.named_parameters())


def test_splade_still_refuses_distilbert(tmp_path):
    from transformers import DistilBertConfig
    from kirag_amd.retriever.splade import SpladeModel
    d = str(tmp_path / "sp")
    DistilBertConfig(dim=128, n_layers=1, n_heads=2, hidden_dim=256, vocab_size=64).save_pretrained(d)
    with pytest.raises(NotImplementedError, match="model_type='distilbert'") as ei:
        SpladeModel.from_pretrained(d)
    assert "DistilBERT- and RoBERTa-based MLM heads" in str(ei.value)
