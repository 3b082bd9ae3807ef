"""The Node binding's host side against tests/golden/napi_binding.json: the seeded corpus
of tools/gen_napi_binding_golden.py replayed through lodestar_amd/napi/index.js (over a
stand-in addon object) and through bgv_addon.c linked against the recording stand-in
library tools/bgv_record_stub.c, and every recorded digest, library call, result object,
refusal and metrics object compared with the file.  No real library, no GPU."""
import json

import pytest

from tools import gen_napi_binding_golden as G

pytestmark = pytest.mark.skipif(not G.available(), reason="node or node_api.h not found")

SECTIONS = ["encoders", "refusals", "verifiers", "addon"]


@pytest.fixture(scope="module")
def replay():
    with open(G.OUT) as f:
        return G.record(), json.load(f)


def test_the_generator_reproduces_the_file_byte_for_byte(replay):
    with open(G.OUT) as f:
        assert G.dumps(replay[0]) == f.read()


@pytest.mark.parametrize("section", SECTIONS)
def test_replayed_corpus_equals_the_golden_file(replay, section):
    got, want = replay[0][section], replay[1][section]
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], f"{section}: {case}"


def test_no_section_is_left_out_and_the_export_lists_stand(replay):
    assert sorted(replay[0]) == sorted(replay[1]) == sorted(["generator", "exports"] + SECTIONS)
    assert replay[0]["generator"] == replay[1]["generator"]
    assert replay[0]["exports"] == replay[1]["exports"]
    assert len(replay[1]["addon"]["exports"]) == 33
