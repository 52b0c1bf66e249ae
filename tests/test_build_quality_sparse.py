"""Static checks of the BUILT libkirag_sparse.so (no GPU), from the notes of its gfx950 code object as tools/kernel_notes.py reads them: no kernel uses scratch
memory or spills a vector register, and the scan kernel's static LDS (the block's R fp32 accumulators, the segment table / histogram and the select's few
words) fits the 160 KiB a single workgroup may declare on this chip."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
LIB = os.path.join(REPO, "kirag_amd", "libkirag_sparse.so")
KERNELS = {"k_sparse_scan", "k_sparse_merge", "k_sparse_count", "k_sparse_compact"}


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
    return ks


def test_no_sparse_kernel_uses_scratch_or_spills(notes):
    bad = [(k["name"], k.get("vgpr_spill_count", 0), k.get("sgpr_spill_count", 0), k.get("private_segment_fixed_size", 0)) for k in notes
           if k.get("vgpr_spill_count", 0) or k.get("private_segment_fixed_size", 0)]
    assert not bad, "kernels with scratch memory: %r" % bad


def test_scan_lds_holds_the_accumulators_and_fits_one_workgroups_160_kib(notes):
    from kirag_amd import _sparse_lib
    for k in notes:
        if "k_sparse_scan" in k["name"]:
            assert 4 * _sparse_lib.block_rows() <= k["group_segment_fixed_size"] <= 163840, k
