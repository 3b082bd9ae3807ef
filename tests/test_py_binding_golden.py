"""The Python binding's host side against tests/golden/py_binding.json: the seeded
corpus of tools/gen_py_binding_golden.py replayed through the public functions of
lodestar_amd/verifier.py and lodestar_amd/native.py, and every recorded digest,
struct field, refusal and metrics dict compared with the file.  No library, no GPU."""
import json

import pytest

from tools import gen_py_binding_golden as G


@pytest.fixture(scope="module")
def replay():
    with open(G.OUT) as f:
        return G.record(), json.load(f)


def test_the_generator_reproduces_the_file_byte_for_byte(replay):
    with open(G.OUT) as f:
        assert G.dumps(replay[0]) == f.read()


@pytest.mark.parametrize("section", ["encoders", "merging", "refusals", "structs", "runners", "verifiers"])
def test_replayed_corpus_equals_the_golden_file(replay, section):
    got = json.loads(json.dumps(replay[0][section]))  # tuples and numpy-free, as the file holds them
    want = replay[1][section]
    assert sorted(got) == sorted(want)
    for case in want:
        assert got[case] == want[case], f"{section}: {case}"


def test_no_section_is_left_out(replay):
    assert sorted(replay[0]) == sorted(replay[1]) == sorted(
        ["generator", "encoders", "merging", "refusals", "structs", "runners", "verifiers"])
    assert replay[0]["generator"] == replay[1]["generator"]
