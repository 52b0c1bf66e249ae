"""Static checks of the BUILT libkirag_late.so (no GPU), from the notes of its gfx950 code object as tools/kernel_notes.py reads them: no kernel uses scratch
memory or spills a vector register (a scratch reload is a VMEM operation in the queue the document fragments travel in, and hipcc drains that queue behind
it), and the MaxSim kernel keeps four waves per SIMD (128 registers), which is what makes it faster at narrow rows."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
LIB = os.path.join(REPO, "kirag_amd", "libkirag_late.so")


@pytest.fixture(scope="module")
def notes():
    import kernel_notes
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    # no skip: the library is built by the hipcc of the ROCm tree that ships llvm-readelf, so where the library exists the tool does, and a missing tool
    # must not make the no-scratch guarantee vanish quietly
    assert os.path.exists(kernel_notes.READELF), kernel_notes.READELF + " is missing: the kernels' notes cannot be read"
    ks = kernel_notes.kernels(LIB)
    assert {n for k in ks for n in ("k_maxsim", "k_gather_f16") if n in k["name"]} == {"k_maxsim", "k_gather_f16"}, [k["name"] for k in ks]
    return ks


def test_no_late_kernel_uses_scratch_or_spills(notes):
    bad = [(k["name"], k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0), k.get("private_segment_fixed_size", 0)) for k in notes
           if k.get("vgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0)]
    assert not bad, "kernels with scratch memory: %r" % bad


def test_maxsim_keeps_four_waves_per_simd(notes):
    for k in notes:
        if "k_maxsim" in k["name"]:
            assert k["vgpr_count"] + k.get("agpr_count", 0) <= 128, k
