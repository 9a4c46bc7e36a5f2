"""The forward / data-gradient block-matrix kernels (csrc/hc_conv_fwd.hip, hc_conv_vec.hip, hc_conv_smallk.hip and what they
share, csrc/hc_conv_tile.h) on the MI355X, bit for bit on seeded randn inputs: every launch of
tests/golden/hc_conv_bits_cases.py has the SHA-256 that the library before the shared tile origin, K range, epilogue and
statistics flush wrote (tests/golden/hc_conv_bits.json, make_golden_hc_conv_bits.py).  An output element meets its K steps
in one fixed order and its bias, addend and old value in that order; statistics are digested only where each replica row
receives one workgroup's contribution per channel (digests_stats), so nothing compared here depends on the order of
atomics.  Every case first asserts the labels the library reports under its environment."""
import functools
import json
import os

import pytest
import torch

from tests.golden import hc_conv_bits_cases as C
from tests.helpers import pkg
from tests.test_hc_exact_host import library_labels, set_case_env

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hc_conv_bits.json")


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("case", C.CASES, ids=C.NAMES)
def test_bits_are_the_recorded_ones(case, seld_env):
    P = pkg()
    set_case_env(case, seld_env)
    assert library_labels(P, case) == case["labels"], case["name"]
    want = _fixture()["cases"][case["name"]]
    assert want["labels"] == {str(w): v for w, v in case["labels"].items() if w < 2}
    got = {n: C.digest(v) for n, v in C.run_case(P, case, DEV).items()}
    for n in got:
        print(case["name"], n, got[n], want["sha256"].get(n))
    assert set(got) == set(want["sha256"]), "the launches of the case are the recorded ones"
    wrong = [n for n in got if got[n] != want["sha256"][n]]
    assert not wrong, (case["name"], wrong, case["why"])


def test_statistics_are_digested_only_where_a_replica_row_has_one_writer():
    assert pkg().hip_ops.STATS_REPLICAS == C.STATS_REPLICAS
    for case in C.CASES:
        has = any(n.endswith(" stats") for n in _fixture()["cases"][case["name"]]["sha256"])
        assert has == C.digests_stats(case), case["name"]
        if has:
            assert C.position_tiles(case, 0) <= C.STATS_REPLICAS


def test_fixture_names_its_writer_and_covers_the_cases():
    doc = _fixture()
    assert doc["written_by"].startswith("the library of commit ")
    assert set(doc["cases"]) == set(C.NAMES)
    assert C.REQUIRED <= set().union(*(C.traits(c) for c in C.CASES))
