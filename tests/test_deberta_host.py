"""Host-side tests of the DeBERTa-v2 / v3 family (no GPU): the model table through tests/capi/encoder_model_check.cpp — every state-dict key of DebertaV2Model /
DebertaV2ForSequenceClassification resolves, the plan shows family 6 with AM_DISENT in every layer and HEAD_CLS as the classifier, every refusal of the table
fires — the bucket rule of the library (tests/capi/deberta_bucket_check.cpp, a program of its own) against HF's make_log_bucket_position + clamp, the refusals
the Python layer reads from config.json alone, the dispatch of the registry classes, and the ABI that stays what it was."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deberta_util as D  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_EINVAL, KR_ESTATE = -22, -1
H, L, FF, V, MAX_POS = 128, 2, 256, 120, 512
DEBERTA, POS_DISENT, AM_DISENT, HEAD_CLS, FF_GELU = 6, 4, 3, 4, 0
BK, MAXREL = D.SETTINGS


def _cxx(src, exe):
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-O1", os.path.join(REPO, "tests", "capi", src), "-o", exe])


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("deberta_model") / "encoder_model_check")
    _cxx("encoder_model_check.cpp", exe)

    def run(lines, heads=2, type_vocab=1, layers=L, max_pos=MAX_POS):
        text = ["config %d %d %d %d %d %d %d" % (H, layers, heads, FF, V, max_pos, type_vocab)]
        for ln in lines:
            text.append(" ".join([ln[0]] + ([ln[1]] if len(ln) > 1 else []) + ([" ".join("%r" % float(x) for x in ln[2])] if ln[0] == "setting" else [str(int(ln[2]))] if ln[0] == "tensor" else [])))
        p = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, (p.returncode, p.stderr)
        out = []
        for row in p.stdout.splitlines():
            head, tail = row.split(" rc=", 1)
            rc, _, msg = tail.partition(" ")
            d = {"rc": int(rc), "msg": msg, "cmd": head.split()[0]}
            d.update(kv.split("=", 1) for kv in head.split()[1:] + (msg.split()[1:] if msg.startswith("plan ") else []) if "=" in kv)
            out.append(d)
        assert len(out) == len(lines), p.stdout
        return out
    return run


def refused(check, lines, code, *fragments, **kw):
    """the LAST line of the script is refused with `code` and a message holding every fragment; every line before it succeeds"""
    out = check(lines, **kw)
    for ln, d in zip(lines[:-1], out[:-1]):
        assert d["rc"] == 0, (ln, d)
    assert out[-1]["rc"] == code and all(f in out[-1]["msg"] for f in fragments), (lines[-1], out[-1])
    return out[-1]["msg"]


def script(heads=2, Bk=32, M=128, classifier=False, labels=3, drop=(), norm="layer_norm", settings=True):
    """the lines the Python layer sends for a tiny model: the two settings, then every state-dict key (the task model's under the reranker's names)"""
    from kirag_amd.retriever.rerankers import deberta_rename
    c = D.cfg(H, L, heads, FF, Bk, M, MAX_POS, V, labels=labels if classifier else None, norm=norm)
    lines = [("setting", BK, (Bk,)), ("setting", MAXREL, (M,))] if settings else []
    for k, shape in D.state_dict_keys(c, classifier).items():
        name = deberta_rename(k) if classifier else k
        if name not in drop:
            lines.append(("tensor", name, int(np.prod(shape))))
    return lines


@pytest.mark.parametrize("heads", [2, 4])
@pytest.mark.parametrize("Bk,M", [(32, 128), (256, 512)])
def test_every_state_dict_key_resolves_and_the_plan_is_debertas(check, heads, Bk, M):
    lines = script(heads, Bk, M) + [("finalize",)]
    out = check(lines, heads=heads)
    named = 0
    for ln, d in zip(lines[:-1], out[:-1]):
        assert d["rc"] == 0, (ln, d)
        if ln[0] == "tensor" and "position_ids" not in ln[1]:
            assert int(d["slot"]) != -1, (ln, d)                              # nothing of the backbone is ignored
            if int(d["slot"]) >= 0:
                assert int(d["expect"]) == ln[2], (ln, d)
            named += ".attention.self." in ln[1] or "rel_embeddings" in ln[1] or ln[1].startswith("encoder.LayerNorm")
            if ".attention.self." in ln[1] or "rel_embeddings" in ln[1] or ln[1].startswith("encoder.LayerNorm"):
                assert int(d["family"]) == DEBERTA, (ln, d)
    assert named == 6 * L + 3
    p = out[-1]
    assert p["rc"] == 0, p
    assert (int(p["family"]), int(p["pre_ln"]), int(p["rms"]), int(p["pos"]), int(p["ff"]), int(p["ff_gated"])) == (DEBERTA, 0, 0, POS_DISENT, FF_GELU, 0), p
    assert p["qkv"] == "00" and p["attn"] == str(AM_DISENT) * L and p["heads"] == "000000" and int(p["classifier"]) == -1 and int(p["out_dim"]) == H, p


def test_the_task_models_keys_resolve_and_hold_the_classifier(check):
    lines = script(classifier=True, labels=3) + [("finalize",)]
    out = check(lines)
    for ln, d in zip(lines[:-1], out[:-1]):
        assert d["rc"] == 0, (ln, d)
    heads = [d for ln, d in zip(lines, out) if ln[1:2] and ln[1] in D.HEAD]
    assert len(heads) == 4 and all(int(d["head"]) == HEAD_CLS for d in heads)
    p = out[-1]
    assert p["rc"] == 0 and p["heads"] == "000010" and int(p["classifier"]) == HEAD_CLS and int(p["family"]) == DEBERTA and int(p["out_width"]) == H, p
    # the table without its norm (norm_rel_ebd none): still a DeBERTa handle
    lines = script(norm="none") + [("finalize",)]
    assert not any(ln[1].startswith("encoder.LayerNorm") for ln in lines[:-1])
    assert check(lines)[-1]["rc"] == 0


def test_refusals_of_the_table(check):
    base = script()
    rel = ("tensor", D.REL_NAME, 64 * H)
    # the settings: range, evenness, one without the other, M - 1 > Bk / 2, next to another position scheme, fixed at the first finalize
    for bad in (0, 1, 3, 31, 258, 2.5):
        refused(check, [("setting", BK, (bad,))], KR_EINVAL, BK)
    refused(check, [("setting", MAXREL, (1,))], KR_EINVAL, MAXREL)
    refused(check, [("setting", BK, (32, 32))], KR_EINVAL, "one value")
    refused(check, [ln for ln in base if ln[1] != MAXREL] + [("finalize",)], KR_EINVAL, BK, MAXREL)
    refused(check, [ln for ln in base if ln[1] != BK] + [("finalize",)], KR_EINVAL, BK, MAXREL)
    refused(check, [("setting", BK, (32,)), ("setting", MAXREL, (17,))] + base[2:] + [("finalize",)], KR_EINVAL, "M - 1 >")
    for name, vals in (("config.position_padding_idx", (1,)), ("config.rotary_inv_freq", [0.5] * 32), ("config.t5_feed_forward", (0,)),
                       ("config.attention_half_window", (8,)), ("config.local_attention_layers", (0, 1))):
        refused(check, [("setting", name, vals)] + base + [("finalize",)], KR_EINVAL, "one position scheme")
    refused(check, base + [("tensor", "encoder.relative_attention_bias.weight", 32 * 2), ("finalize",)], KR_EINVAL, "one position scheme")
    done = base + [("finalize",)]
    assert check(done + [("setting", BK, (32,)), ("setting", MAXREL, (128,))])[-1]["rc"] == 0                   # the same values later: a no-op
    refused(check, done + [("setting", BK, (64,))], KR_EINVAL, "fixed at the handle's first finalize")
    refused(check, done + [("setting", MAXREL, (512,))], KR_EINVAL, "fixed at the handle's first finalize")
    bert = [("tensor", "embeddings.word_embeddings.weight", V * H), ("finalize",)]
    assert check(bert)[-1]["rc"] == KR_ESTATE                                  # (an unfinished BERT handle; what follows needs a finalized one)
    # the position table: its shape, missing, against the setting, fixed with the handle; its norm whole or absent
    for n in (0, H, 3 * H, 64 * H + 1, 514 * H):
        refused(check, [("tensor", D.REL_NAME, n)], KR_EINVAL, D.REL_NAME)
    refused(check, [ln for ln in base if ln[1] != D.REL_NAME] + [("finalize",)], KR_ESTATE, D.REL_NAME, "never loaded")
    refused(check, [ln for ln in base if ln[1] != D.REL_NAME] + [("tensor", D.REL_NAME, 128 * H), ("finalize",)], KR_EINVAL, D.REL_NAME, "64")
    refused(check, done + [("tensor", D.REL_NAME, 128 * H)], KR_EINVAL, "fixed")
    assert check(done + [rel, ("finalize",)])[-1]["rc"] == 0                   # new values of the same shape: the weight sync
    for keep, lost in ((0, 1), (1, 0)):
        refused(check, [ln for ln in base if ln[1] != D.REL_LN[lost]] + [("finalize",)], KR_ESTATE, D.REL_LN[lost], "never loaded")
    refused(check, [ln for ln in base if ln[1] not in D.REL_LN] + [("finalize",), ("tensor", D.REL_LN[0], H)], KR_EINVAL, "finalized without")
    refused(check, base + [("tensor", D.REL_LN[0], H + 1)], KR_EINVAL, D.REL_LN[0])
    # DeBERTa's names on a handle of another kind: refused at finalize, naming the tensor (and after a finalize at once)
    plain = [ln for ln in base if ln[0] == "tensor"]
    refused(check, plain + [("finalize",)], KR_EINVAL, BK, "never loaded")
    q0 = "encoder.layer.0.attention.self.query_proj.weight"
    only = [ln for ln in plain if ln[1] == q0]
    refused(check, only + [("finalize",)], KR_EINVAL, q0, BK)
    refused(check, [ln for ln in plain if ln[1] == D.REL_NAME] + [("finalize",)], KR_EINVAL, D.REL_NAME, BK)
    refused(check, [ln for ln in plain if ln[1] == D.REL_LN[1]] + [("finalize",)], KR_EINVAL, D.REL_LN[1], BK)
    # other families' names on a DeBERTa handle, naming the tensor
    for other in ("encoder.layer.0.attention.self.query.weight", "encoder.layer.1.attention.attn.k.weight", "encoder.layer.0.attention.self.value.bias"):
        refused(check, base + [("tensor", other, H * H if other.endswith("weight") else H), ("finalize",)], KR_EINVAL, other, "DeBERTa handle")
    refused(check, base + [("tensor", "embeddings.position_embeddings.weight", MAX_POS * H), ("finalize",)], KR_EINVAL, "position_embeddings", "position_biased_input")
    refused(check, base + [("tensor", "layers.0.self_attn.q_proj.weight", H * H), ("finalize",)], KR_EINVAL, "q_proj")
    # the heads a DeBERTa handle refuses: bge-m3's, the MLM head, the Dense head; and a partial classifier
    for name, n in (("colbert_linear.weight", 128 * H), ("sparse_linear.weight", H), ("cls.predictions.transform.dense.weight", H * H), ("dense.weight", 8 * H)):
        refused(check, base + [("tensor", name, n), ("finalize",)], KR_EINVAL, name.split(".")[0], "DeBERTa")
    full = script(classifier=True)
    for drop in D.HEAD:
        refused(check, [ln for ln in full if ln[1] != drop] + [("finalize",)], KR_ESTATE, drop, "never loaded")
    refused(check, base + [("tensor", "head.dense.weight", H * H), ("finalize",)], KR_EINVAL, "head.dense", "DeBERTa")


@pytest.mark.parametrize("Bk,M", [(256, 512), (32, 128), (64, 512)])
def test_bucket_rule_is_hfs(tmp_path, Bk, M):
    """p for every r in -(M - 1) .. M - 1 and 40 values beyond on both sides, from the library's inline function in a program of its own, against HF's tensor code"""
    exe = str(tmp_path / "deberta_bucket_check")
    _cxx("deberta_bucket_check.cpp", exe)
    rows = np.array(subprocess.check_output([exe, str(Bk), str(M), "40"], timeout=60).decode().split(), dtype=np.int64).reshape(-1, 2)
    r = np.arange(-(M - 1 + 40), M + 40)
    assert np.array_equal(rows[:, 0], r)
    ref = D.hf_buckets(r, Bk, M)
    assert np.array_equal(rows[:, 1], ref), r[rows[:, 1] != ref]
    assert rows[:, 1].min() == 0 and rows[:, 1].max() == 2 * Bk - 1 and rows[r == 0, 1] == Bk       # the clamp is reached on both sides
    mid = Bk // 2
    assert np.array_equal(rows[np.abs(r) <= mid, 1], r[np.abs(r) <= mid] + Bk)                        # the identity up to mid


def _config_json(tmp_path, **over):
    c = D.hf_config(D.cfg(H, 1, 2, FF, 32, 128, MAX_POS, V, labels=1)).to_dict()
    c.update(over)
    d = tmp_path / ("cfg_" + "_".join(over) if over else "cfg")
    d.mkdir(exist_ok=True)
    with open(d / "config.json", "w") as f:
        json.dump(c, f)
    return str(d), c


REFUSALS = [("relative_attention", False), ("position_biased_input", True), ("pos_att_type", ["c2p"]), ("pos_att_type", "c2p|p2c|p2p"), ("share_att_key", False),
            ("position_buckets", -1), ("position_buckets", 0), ("position_buckets", 33), ("position_buckets", 512), ("conv_kernel_size", 3),
            ("embedding_size", 64), ("type_vocab_size", 2), ("hidden_act", "relu"), ("pooler_hidden_act", "tanh"), ("pooler_hidden_size", 64),
            ("attention_head_size", 16), ("norm_rel_ebd", "layer_norm|scale"), ("id2label", {str(i): str(i) for i in range(65)}), ("hidden_size", 192),
            ("num_attention_heads", 8), ("intermediate_size", 200), ("max_relative_positions", 16), ("model_type", "deberta")]


@pytest.mark.parametrize("field,value", REFUSALS, ids=[f"{k}={v if not isinstance(v, dict) else len(v)}" for k, v in REFUSALS])
def test_refusals_from_config_json_alone(tmp_path, monkeypatch, field, value):
    """every unsupported field is a NotImplementedError that begins model_type='deberta-v2': and names the field — from a folder that holds config.json and
    nothing else (no weight can have been read), with the library unloadable"""
    from kirag_amd import _lib
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever import rerankers as RR
    monkeypatch.setattr(_lib, "load", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    d, c = _config_json(tmp_path, **{field: value})
    names = {"id2label": "num_labels"}
    head_only = field in ("pooler_hidden_act", "pooler_hidden_size", "id2label")
    with pytest.raises(NotImplementedError, match=r"^model_type='deberta-v2': .*" + re.escape(names.get(field, field))):
        RR.BGEReranker.from_pretrained(d)
    with pytest.raises(NotImplementedError, match=r"^model_type='deberta-v2': "):
        ENC.check_deberta_config(c, head=True)
    if not head_only:
        for cls in (ENC.E5Encoder, ENC.BGEEncoder):
            with pytest.raises(NotImplementedError, match=r"^model_type='deberta-v2': .*" + re.escape(field)):
                cls.from_pretrained(d)
    else:
        assert ENC.check_deberta_config(c) == {"buckets": 32, "max_rel": 128}


def test_config_defaults_and_dispatch(tmp_path):
    """max_relative_positions < 1 means max_position_embeddings; a good config passes as a dict and as a DebertaV2Config; the registry classes reach the twins"""
    from kirag_amd.retriever import encoders as ENC
    from kirag_amd.retriever import rerankers as RR
    import transformers as tr
    d, c = _config_json(tmp_path)
    assert ENC.check_deberta_config(c, head=True) == {"buckets": 32, "max_rel": 128}
    assert ENC.check_deberta_config(dict(c, max_relative_positions=-1)) == {"buckets": 32, "max_rel": MAX_POS}
    assert ENC.check_deberta_config(D.hf_config(D.cfg(H, 1, 2, FF, 256, 512)), head=True) == {"buckets": 256, "max_rel": 512}
    assert issubclass(ENC.DebertaV2E5Encoder, tr.DebertaV2Model) and issubclass(ENC.DebertaV2BGEEncoder, tr.DebertaV2Model)
    assert issubclass(RR.DebertaV2Reranker, tr.DebertaV2ForSequenceClassification)
    assert ENC.FAMILIES["deberta-v2"].twin(ENC.E5Encoder._pool) is ENC.DebertaV2E5Encoder and ENC.FAMILIES["deberta-v2"].twin(ENC.BGEEncoder._pool) is ENC.DebertaV2BGEEncoder
    assert (ENC.DebertaV2E5Encoder._pool, ENC.DebertaV2BGEEncoder._pool) == (ENC.POOL_MEAN, ENC.POOL_CLS)
    # the reranker's names: the backbone loses its prefix, pooler.dense / classifier are the library's head; the pooler half travels as `extra`
    cfg = D.hf_config(D.cfg(H, 1, 2, FF, 32, 128, MAX_POS, V, labels=3))
    m = RR.DebertaV2Reranker(cfg)
    sent = {RR.deberta_rename(n) for n, _ in m.named_parameters() if not n.startswith("pooler.")} | {n for n, _ in RR.DebertaV2Reranker._hip_extra(m)}
    assert set(D.HEAD) <= sent and D.REL_NAME in sent and "embeddings.word_embeddings.weight" in sent and not any(n.startswith("deberta.") for n in sent)
    m.save_pretrained(str(tmp_path / "rr"))
    assert type(RR.BGEReranker.from_pretrained(str(tmp_path / "rr"))) is RR.DebertaV2Reranker
    e = ENC.DebertaV2E5Encoder(D.hf_config(D.cfg(H, 1, 2, FF, 32, 128, MAX_POS, V)))
    e.save_pretrained(str(tmp_path / "enc"))
    assert type(ENC.E5Encoder.from_pretrained(str(tmp_path / "enc"))) is ENC.DebertaV2E5Encoder
    assert type(ENC.BGEEncoder.from_pretrained(str(tmp_path / "enc"))) is ENC.DebertaV2BGEEncoder
    with pytest.raises(RuntimeError, match="HIP path only"):
        e.eval()(**{k: __import__("torch").from_numpy(v) for k, v in zip(("input_ids", "attention_mask"), D.tokens(2, 8))})


MUTATION_CASES = [((256, 512), 40, 2), ((256, 512), 150, 4), ((32, 128), 150, 2)]      # S = 150 > mid at Bk 256 (the log zone); the clamp at (32, 128)


def test_each_part_of_the_disentangled_attention_decides_the_output():
    """The teeth of the 3e-2 bar of tests/test_gpu_deberta.py, on the CPU: the float64 restatement of the forward (deberta_util.by_hand) agrees with HF fp32
    on the test weights, and each mutation of it — c2p dropped, p2c dropped, p of (j - i), sqrt(d) or sqrt(2 d) for sqrt(3 d), R without its LayerNorm, PQ / PK
    without the projection biases, linear clamped distances for the log buckets, no clamp — moves some attended row by more than 10 x the bar."""
    bar = 3e-2
    moves = {mu: 0.0 for mu in D.MUTATIONS}
    for (Bk, M), S, heads in MUTATION_CASES:
        c = D.cfg(heads=heads, Bk=Bk, M=M)
        w = D.weights(c)
        ids, mask = D.tokens(3, S, seed=1)
        att = mask.astype(bool)
        good = D.by_hand(c, w, ids, mask)
        assert np.abs(good - D.hf_hidden(D.hf_model(c, w), ids, mask))[att].max() < 1e-4
        for mu in D.MUTATIONS:
            moves[mu] = max(moves[mu], float(np.abs(D.by_hand(c, w, ids, mask, mu) - good)[att].max()))
    print("teeth: " + ", ".join(f"{k} {v:.2f}" for k, v in moves.items()))
    assert min(moves.values()) > 10 * bar, moves
    # init-range weights would show none of it: the position terms move the output by about 1e-3
    c = D.cfg(Bk=32, M=128)
    w = D.weights(c, qk=1.0, qk_bias=1.0, gamma=1.0, vo=1.0)
    ids, mask = D.tokens(3, 40, seed=1)
    assert np.abs(D.by_hand(c, w, ids, mask, "no_c2p") - D.by_hand(c, w, ids, mask))[mask.astype(bool)].max() < bar


def test_abi_is_unchanged():
    """no new C function: KR_ABI_VERSION 9, 50 exported kr_ symbols"""
    from kirag_amd import _lib
    lib = _lib.load()
    assert lib.kr_abi_version() == 9 == _lib.ABI_VERSION
    with open(os.path.join(REPO, "include", "kirag_amd.h")) as f:
        header = f.read()
    assert "#define KR_ABI_VERSION 9" in header
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(REPO, "kirag_amd", "libkirag_amd.so")], text=True)
    syms = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("kr_")})
    assert len(syms) == 50, syms
    for name in ("kr_encoder_load_weight", "kr_encoder_finalize", "kr_encoder_forward", "kr_encoder_forward_packed", "kr_encoder_last_hidden"):
        assert name in syms and hasattr(lib, name)
    assert C.sizeof(_lib.BertCfg) == 32
