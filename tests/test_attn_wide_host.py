"""The reference of the 128-wide attention probe has teeth (no GPU): at d_h = 128 the data of tests/attn_probe_util.py still makes every visited 64-key step of
every 32-query tile decisive, admits no decoy and names the KV head that was read — on the shapes, lengths and modes tests/test_gpu_attn_wide.py launches.
MOVE = 0.3 is attn_probe_util's own margin: 75 times the f16 bound and 17 times the bf16 one at these lengths."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_probe_util as U  # noqa: E402

DH, MOVE = 128, 0.3
SHAPES = ((2, 1), (4, 2))
LENS = [1, 31, 32, 33, 63, 64, 65, 129, 300]


@pytest.mark.parametrize("mode", ["plain", "causal", "window"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_hiding_any_visited_step_moves_the_reference(shape, mode):
    for n, kind in U.list_kinds(LENS, mode):
        s = U.make_seq(n, kind, shape[0], shape[1], DH, mode, "needles")
        assert s.q.shape == (s.nq, shape[0], DH) and s.k.shape == (s.nk, shape[1], DH) and np.abs(s.v).max() <= U.VMAX
        ref, moved = U.reference(s, sens=True)
        assert np.isfinite(ref).all() and not [k for k in moved if k[0] == "unvisited"], (n, kind)
        weak = {k: v for k, v in moved.items() if 0 <= v < MOVE}
        assert not weak, (mode, n, kind, weak)
        assert U.error_bound("bf16", s.nk) * 17 < MOVE


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_a_decoy_or_another_kv_head_moves_the_reference(shape):
    heads, kv = shape
    for n in (33, 129, 300):
        s = U.make_seq(n, "right", heads, kv, DH, "causal", "needles")
        ref = U.reference(s)
        assert np.abs(U.reference(s, win=None) - ref).max() >= MOVE, n            # no mask at all: the decoys above the diagonal win
        assert np.abs(U.reference(s, win=(U.MAX_POS, 1)) - ref).max() >= MOVE, n  # one column too many
        if kv > 1:
            wrong = (np.arange(heads) // s.group + 1) % kv
            assert np.abs(U.reference(s, kv_of=wrong) - ref).max() >= MOVE, n
        d = U.make_seq(n, "right", heads, kv, DH, "causal", "diffuse")
        assert np.isfinite(U.reference(d)).all()
