"""Synthetic-weight encoder construction for bench.py / smoke (BERT-large shape, N(0,0.02) weights,
LayerNorm gamma=1 beta=0; throughput does not depend on the weight values).  Weights are generated on the device."""
from __future__ import annotations

from types import SimpleNamespace

import torch

from .retriever.encoders import HipBertForward

E5_LARGE = dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096, vocab_size=30522,
                max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu")
# the small siblings (e5-small-v2, bge-small-en-v1.5, gte-small: 12 layers; all-MiniLM-L6-v2: 6): 12 heads of 32
E5_SMALL = dict(E5_LARGE, hidden_size=384, num_hidden_layers=12, num_attention_heads=12, intermediate_size=1536)
MINILM_L6 = dict(E5_SMALL, num_hidden_layers=6)
ENCODER_SHAPES = {"e5-large": E5_LARGE, "e5-small": E5_SMALL, "minilm-l6": MINILM_L6}


def synthetic_state(cfg: SimpleNamespace, device, seed: int = 0):
    g = torch.Generator(device=device); g.manual_seed(seed)
    H, FF = cfg.hidden_size, cfg.intermediate_size

    def n(*shape):
        return 0.02 * torch.randn(*shape, generator=g, device=device)

    yield "embeddings.word_embeddings.weight", n(cfg.vocab_size, H)
    yield "embeddings.position_embeddings.weight", n(cfg.max_position_embeddings, H)
    yield "embeddings.token_type_embeddings.weight", n(cfg.type_vocab_size, H)
    yield "embeddings.LayerNorm.weight", torch.ones(H, device=device)
    yield "embeddings.LayerNorm.bias", torch.zeros(H, device=device)
    for l in range(cfg.num_hidden_layers):
        p = f"encoder.layer.{l}."
        for nm in ("query", "key", "value"):
            yield p + f"attention.self.{nm}.weight", n(H, H)
            yield p + f"attention.self.{nm}.bias", torch.zeros(H, device=device)
        yield p + "attention.output.dense.weight", n(H, H)
        yield p + "attention.output.dense.bias", torch.zeros(H, device=device)
        yield p + "attention.output.LayerNorm.weight", torch.ones(H, device=device)
        yield p + "attention.output.LayerNorm.bias", torch.zeros(H, device=device)
        yield p + "intermediate.dense.weight", n(FF, H)
        yield p + "intermediate.dense.bias", torch.zeros(FF, device=device)
        yield p + "output.dense.weight", n(H, FF)
        yield p + "output.dense.bias", torch.zeros(H, device=device)
        yield p + "output.LayerNorm.weight", torch.ones(H, device=device)
        yield p + "output.LayerNorm.bias", torch.zeros(H, device=device)


def make_hip_encoder(device, cfg_dict=None, seed: int = 0, operand_dtype=None, residual_lo=None) -> HipBertForward:
    cfg = SimpleNamespace(**(cfg_dict or E5_LARGE))
    idx = device.index if device.index is not None else torch.cuda.current_device()
    enc = HipBertForward(cfg, idx, operand_dtype=operand_dtype, residual_lo=residual_lo)
    enc.load_state(dict(synthetic_state(cfg, device, seed)))
    enc.cfg = cfg
    return enc


def synthetic_tokens(device, n: int, S: int, seed: int, ragged: bool = False):
    """ids uniform in [1000, 30000), ids[:,0]=101, last real token 102, right padded."""
    g = torch.Generator(device=device); g.manual_seed(seed)
    ids = torch.randint(1000, 30000, (n, S), generator=g, device=device, dtype=torch.int64)
    if ragged:
        lens = torch.clamp(torch.round(torch.randn(n, generator=g, device=device) * 0.2 * S + 0.86 * S), min(16, S), S).to(torch.int64)
    else:
        lens = torch.full((n,), S, device=device, dtype=torch.int64)
    mask = (torch.arange(S, device=device)[None, :] < lens[:, None]).to(torch.int64)
    ids[:, 0] = 101
    ids[torch.arange(n, device=device), lens - 1] = 102
    return ids * mask, mask


class CorpusDist:
    """Synthetic corpus-embedding generators (rows are unit vectors, generated on the device chunk by chunk).

    ``gaussian``  iid Gaussian directions: pairwise cosines ~ N(0, 1/d) — the easy case for a low-precision scan.
    ``mixed``     e5like with a 2 % cluster of near-duplicates of one passage and 3 % of the queries aiming at it: the realistic case for pass 2.
    ``neardup``   a corpus of near-duplicates (rows within 3e-5 of one direction): nothing certifies in the 16-bit pass; measures pass 2.
    ``e5like``    what real e5 / bge embeddings look like to the scan: every row shares a mean direction (pairwise cosines centred at
                  ``mean_cos`` = 0.75) and the remainder is anisotropic (spectrum lambda_i ~ 1/i over randomly permuted axes: effective
                  dimension (sum lambda)^2 / sum lambda^2 ~ 34 at d = 1024), so query-passage scores sit in a narrow band, sigma ~ 0.04: at 5M
                  rows the rank-100 score gaps are ~1e-4, far below the bf16 scan's worst-case error bound (~5e-3).
    """

    def __init__(self, kind: str, d: int, device, seed: int = 3, mean_cos: float = 0.75):
        assert kind in ("gaussian", "e5like", "neardup", "mixed"), kind
        self.kind, self.d, self.device, self.mean_cos = kind, d, device, mean_cos
        g = torch.Generator(device=device); g.manual_seed(seed * 7919 + 11)
        if kind in ("e5like", "neardup", "mixed"):
            mu = torch.randn(d, generator=g, device=device)
            self.mu = mu / mu.norm()
            lam = 1.0 / torch.arange(1, d + 1, device=device, dtype=torch.float32)
            self.scale = lam.sqrt()[torch.randperm(d, generator=g, device=device)]
            b = torch.randn(d, generator=g, device=device) * self.scale
            b = torch.nn.functional.normalize(b - (b @ self.mu) * self.mu, dim=0)
            self.boiler = torch.nn.functional.normalize((mean_cos ** 0.5) * self.mu + ((1.0 - mean_cos) ** 0.5) * b, dim=0)   # the duplicated passage of "mixed"

    def rows(self, m: int, gen) -> torch.Tensor:
        """m unit-norm fp32 rows [m, d] drawn with the caller's generator."""
        z = torch.randn(m, self.d, generator=gen, device=self.device)
        if self.kind == "gaussian":
            return torch.nn.functional.normalize(z, dim=1)
        if self.kind == "mixed":
            # e5like, except that 2 % of the rows are near-duplicates of one passage (a boilerplate cluster): the queries that aim at it (3 % of a batch,
            # queries_near) cannot be certified by the 16-bit pass and share one fp64 pass 2; everything else certifies in pass 1
            u = z * self.scale
            u = torch.nn.functional.normalize(u - (u @ self.mu)[:, None] * self.mu, dim=1)
            x = torch.nn.functional.normalize((self.mean_cos ** 0.5) * self.mu + ((1.0 - self.mean_cos) ** 0.5) * u, dim=1)
            dup = torch.rand(m, generator=gen, device=self.device) < 0.02
            x[dup] = torch.nn.functional.normalize(self.boiler + 3e-5 * z[dup], dim=1)
            return x
        if self.kind == "neardup":
            # adversarial for a 16-bit scan: every row within ~3e-5 of one direction, so ALL scores of a query fall inside the bf16 error bound and
            # pass 1 can certify nothing (the data the fp64 pass 2 exists for; round 1 answered it with one full fp32 scan PER QUERY)
            return torch.nn.functional.normalize(self.mu + 3e-5 * z, dim=1)
        u = z * self.scale
        u = u - (u @ self.mu)[:, None] * self.mu                     # remainder orthogonal to the mean direction
        u = torch.nn.functional.normalize(u, dim=1)
        return torch.nn.functional.normalize((self.mean_cos ** 0.5) * self.mu + ((1.0 - self.mean_cos) ** 0.5) * u, dim=1)

    def queries_near(self, head: torch.Tensor, gen, noise: float = 0.05) -> torch.Tensor:
        """Queries = corpus rows + noise, re-normalised (known near neighbours; the background scores follow the corpus distribution).
        gaussian: q = normalize(x + noise * N(0, I)).  e5like: a query is a sample of the passages' own distribution whose
        anisotropic remainder is the picked row's remainder perturbed by 10 x noise (cos(q, picked row) ~ 0.97, background mean_cos +- 0.04)."""
        z = torch.randn(head.shape, generator=gen, device=self.device)
        if self.kind == "gaussian":
            return torch.nn.functional.normalize(head + noise * z, dim=1)
        if self.kind == "neardup":
            return torch.nn.functional.normalize(self.mu + 0.3 * torch.nn.functional.normalize(z, dim=1), dim=1)
        if self.kind == "mixed":
            kind, self.kind = self.kind, "e5like"
            q = self.queries_near(head, gen, noise)
            self.kind = kind
            n_aim = max(1, int(0.03 * len(q)))                      # 3 % of the batch asks for the boilerplate passage
            w = torch.nn.functional.normalize(z[:n_aim] * self.scale, dim=1)
            q[:n_aim] = torch.nn.functional.normalize(self.boiler + 0.2 * w, dim=1)
            return q
        u = torch.nn.functional.normalize(head - (head @ self.mu)[:, None] * self.mu, dim=1)
        w = z * self.scale
        w = torch.nn.functional.normalize(w - (w @ self.mu)[:, None] * self.mu, dim=1)
        uq = torch.nn.functional.normalize(u + 10.0 * noise * w, dim=1)
        return torch.nn.functional.normalize((self.mean_cos ** 0.5) * self.mu + ((1.0 - self.mean_cos) ** 0.5) * uq, dim=1)


def encoder_flops(cfg, lens) -> float:
    """Algorithmic FLOPs: per sequence of length s: L * s * (24 H^2 + 4 s H)."""
    H, L = cfg.hidden_size, cfg.num_hidden_layers
    lens = lens.double()
    return float((L * lens * (24.0 * H * H + 4.0 * lens * H)).sum().item())


def wordpiece_tokenizer(vocab_file: str, do_lower_case: bool = True):
    """``BertTokenizerFast`` over a plain ``vocab.txt`` (synthetic vocabularies of the tests / feed benchmark; real checkpoints go through
    ``AutoTokenizer.from_pretrained`` exactly as in the reference).  transformers >= 5 takes the vocabulary as ``vocab=`` and silently IGNORES the
    ``vocab_file=`` keyword of 4.x — every word then tokenises to [UNK] (rounds 1-2 of this repo tested the collators that way without noticing);
    this helper uses whichever spelling yields the file's vocabulary and fails loudly otherwise."""
    from transformers import BertTokenizerFast
    with open(vocab_file) as f:
        n_lines = sum(1 for line in f if line.rstrip("\n"))
    tok = BertTokenizerFast(vocab_file=vocab_file, do_lower_case=do_lower_case)
    if tok.vocab_size != n_lines:
        tok = BertTokenizerFast(vocab=vocab_file, do_lower_case=do_lower_case)
    if tok.vocab_size != n_lines:
        raise RuntimeError(f"BertTokenizerFast loaded {tok.vocab_size} of the {n_lines} entries of {vocab_file}")
    return tok


def synthetic_text_corpus(n: int, folder: str, seed: int = 0):
    """``n`` synthetic passages as TEXT in the reference's passage format (``dataset/corpus.py:117-120``: "title:  T, text:  ...") over a synthetic 30522-entry
    WordPiece vocabulary written to ``folder/vocab.txt`` (5 special tokens, 20000 words, 10517 "##" suffix pieces; 30 % of the words carry a suffix piece so the
    tokenizer does real WordPiece work) — 60-99 words, ~111 tokens per passage with the "passage: " prefix.  Returns ``(vocab_file, texts)``.  Used by
    bench.py's ``encode.entry_point`` block and tools/feed_bench.py: what ``cal_doc_embeddings`` is fed when a user runs it."""
    import os
    import numpy as np
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))

    def rand_words(k, lo, hi):
        out = set()
        while len(out) < k:
            lens = rng.integers(lo, hi, 2 * k)
            flat = rng.choice(letters, int(lens.sum()))
            cuts = np.concatenate([[0], np.cumsum(lens)])
            out.update("".join(flat[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
        return sorted(out)[:k]
    words, pieces = rand_words(20000, 3, 9), rand_words(10517, 2, 5)
    vocab_file = os.path.join(folder, "vocab.txt")
    with open(vocab_file, "w") as f:
        f.write("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + words + ["##" + p for p in pieces]) + "\n")
    k = rng.integers(60, 100, n)
    total = int(k.sum())
    wi = rng.integers(0, len(words), total); pi = rng.integers(0, len(pieces), total); glue = rng.random(total) < 0.3
    toks = [words[a] + pieces[b] if g else words[a] for a, b, g in zip(wi.tolist(), pi.tolist(), glue.tolist())]
    cuts = np.concatenate([[0], np.cumsum(k)]).tolist()
    texts = ["title:  " + toks[a] + ", text:  " + " ".join(toks[a + 1:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    return vocab_file, texts
