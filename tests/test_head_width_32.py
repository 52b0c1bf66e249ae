"""CPU checks of the 32-wide attention heads (e5-small / bge-small / MiniLM: hidden 384, 12 heads of 32): kr_encoder_create accepts head widths 32 and
64 and still refuses every other one; the checkpoint precision tool runs on a 384-wide model (torch emulation of the rounding points, no GPU needed)."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

from kirag_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(hidden, heads, ff=1536):
    lib = _lib.load()
    cfg = _lib.BertCfg(hidden, 2, heads, ff, 1000, 64, 2, 1e-12)
    h = C.c_void_p()
    rc = lib.kr_encoder_create(C.byref(cfg), 0, C.byref(h))
    if rc == 0:
        lib.kr_encoder_destroy(h)
    return rc, lib.kr_last_error()


@pytest.mark.parametrize("hidden,heads,ff", [(384, 12, 1536), (128, 4, 512)])
def test_head_width_32_is_accepted(hidden, heads, ff):
    rc, msg = _create(hidden, heads, ff)
    # without a GPU: KR_ENODEV (the config passed validation), with one: a handle
    assert rc == (-19 if not torch.cuda.is_available() else 0), (rc, msg)


@pytest.mark.parametrize("hidden,heads", [(384, 8), (768, 6), (384, 24), (1024, 8)])
def test_other_head_widths_are_refused(hidden, heads):
    rc, msg = _create(hidden, heads)
    assert rc == -22 and b"32 or 64" in msg, (rc, msg)


def test_head_width_64_configs_are_unchanged():
    for hidden, heads in ((128, 2), (384, 6), (1024, 16)):
        rc, msg = _create(hidden, heads)
        assert rc == (-19 if not torch.cuda.is_available() else 0), (hidden, heads, rc, msg)


def test_checkpoint_check_runs_on_a_384_wide_model():
    from transformers import BertConfig, BertModel
    sp = importlib.util.spec_from_file_location("checkpoint_check", os.path.join(REPO, "tools", "checkpoint_check.py"))
    cc = importlib.util.module_from_spec(sp); sp.loader.exec_module(cc)
    torch.manual_seed(0)
    m = BertModel(BertConfig(hidden_size=384, num_hidden_layers=2, num_attention_heads=12, intermediate_size=1536, vocab_size=3000,
                             max_position_embeddings=128), add_pooling_layer=False)
    out = cc.check_model(m, cc.parse(["(384 wide)", "--n", "6", "--max-length", "32", "--random-tokens", "--emulate"]))
    assert out["tested_path"] == "emulation" and len(out["layers"]) == 2 and len(out["modes"]) == 4
    assert all(r["finite"] for r in out["modes"]) and out["modes"][0]["worst_score_error"] <= 1e-3
