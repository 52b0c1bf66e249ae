"""Static checks of the BUILT libkirag_pairs.so (no GPU), from the notes of its gfx950 code object as tools/kernel_notes.py reads them: k_pair_dot is present,
uses no scratch memory, spills no register and declares no LDS (one wave per pair, everything in registers)."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
LIB = os.path.join(REPO, "kirag_amd", "libkirag_pairs.so")
KERNELS = {"k_pair_dot"}


@pytest.fixture(scope="module")
def notes():
    import kernel_notes
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    # no skip: the library is built by the hipcc of the ROCm tree that ships llvm-readelf, so where the library exists the tool does
    assert os.path.exists(kernel_notes.READELF), kernel_notes.READELF + " is missing: the kernels' notes cannot be read"
    ks = kernel_notes.kernels(LIB)
    assert {n for k in ks for n in KERNELS if n in k["name"]} == KERNELS, [k["name"] for k in ks]
    assert len(ks) == len(KERNELS), [k["name"] for k in ks]
    return ks


def test_no_pairs_kernel_uses_scratch_or_spills(notes):
    bad = [(k["name"], k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0), k.get("private_segment_fixed_size", 0)) for k in notes
           if k.get("vgpr_spill_count", 0) or k.get("sgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0)]
    assert not bad, "kernels with scratch memory or spilled registers: %r" % bad


def test_pair_dot_declares_no_lds_and_is_launched_with_256_threads(notes):
    for k in notes:
        assert k["group_segment_fixed_size"] == 0, k
        assert k.get("max_flat_workgroup_size", 256) == 256, k
