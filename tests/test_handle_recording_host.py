"""``HipBertForward`` against a recording stand-in for the library, on the CPU: for every model family the ordered calls of handle creation + ``sync`` /
``load_state`` (``kr_bert_cfg`` fields, reserved-name settings, every tensor's name, element count and sha256), the handle's attributes afterwards and the
silence of a second ``sync`` equal ``tests/golden/handle_recordings.json``, recorded by ``tests/golden/make_handle_recordings.py`` before the Python side was
reorganised into one table of families."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_handle_recordings", os.path.join(GOLDEN, "make_handle_recordings.py"))
REC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REC)

with open(REC.OUT) as _f:
    RECORDED = json.load(_f)


def test_every_case_is_recorded():
    assert sorted(RECORDED) == sorted(REC.CASES)


@pytest.mark.parametrize("name", sorted(REC.CASES))
def test_handle_talks_to_the_library_as_recorded(name):
    got, want = REC.record(name), RECORDED[name]
    assert [c[:3] for c in got["calls"]] == [c[:3] for c in want["calls"]]      # first without the hashes: a readable difference
    assert got["calls"] == want["calls"]
    assert got["attributes"] == want["attributes"]
    assert got["flags"] == want["flags"]
    assert got["second_sync"] == want["second_sync"]
    if want["second_sync"] is not None:
        assert want["second_sync"] == []        # the fast path makes no call at all
    assert want["calls"][0][0] == "create" and want["calls"][-1] == ["finalize"]
