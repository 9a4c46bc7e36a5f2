"""The stride-phase / forward implicit GEMM shared by the 2-D transposed and the 3-D convolutions (csrc/hc_phase_gemm.h)
on the MI355X, bit for bit: a 2-D transposed forward equals the same problem at depth 1 on the 3-D transposed forward,
and every launch of tests/golden/phase_gemm_cases.py has the SHA-256 the library before the shared body wrote
(tests/golden/phase_gemm_bits.json, make_golden_phase_gemm.py).  The kernels use no atomics and a given output element
meets its K steps in one fixed order (tap w fastest, then h, then d, then the channel block), so the comparisons are
torch.equal on seeded floats, every element of every case."""
import functools
import json
import os

import pytest
import torch

from tests.golden import phase_gemm_cases as C
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phase_gemm_bits.json")
TWIN = {c["name"]: c for c in C.TWIN_CASES}
C3 = {c["name"]: c for c in C.C3_CASES}


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _twin(name):
    """Each case runs once: (label, 2-D output equals the depth-1 output, digest of the 2-D output)."""
    label, y2, y3 = C.run_twin(pkg().hip_ops, TWIN[name], DEV)
    torch.cuda.synchronize()
    assert tuple(y3.shape) == tuple(y2.shape[:2]) + (1,) * (5 - y2.dim()) + tuple(y2.shape[2:])
    return label, torch.equal(y2, y3.view(y2.shape)), C.digest(y2)


@functools.lru_cache(maxsize=None)
def _c3(name):
    label, y = C.run_c3(pkg().hip_ops, C3[name], DEV)
    torch.cuda.synchronize()
    return label, C.digest(y)


@pytest.mark.parametrize("name", list(TWIN))
def test_transposed_2d_equals_3d_at_depth_1(name):
    label, equal, _ = _twin(name)
    print(name, label, "equal" if equal else "DIFFERENT")
    assert equal, (name, label, TWIN[name]["what"])


def test_twin_cases_reach_the_three_2d_tiles():
    assert {_twin(name)[0] for name in TWIN} >= C.TWIN_TILES
    assert _twin("tile_12x1")[0] == "hc_tconv_kernel<12, 1>" and _twin("tile_4x4")[0] == "hc_tconv_kernel<4, 4>"


@pytest.mark.parametrize("name", list(TWIN))
def test_transposed_2d_bits_are_the_recorded_ones(name):
    label, _, sha = _twin(name)
    want = _fixture()["twin"][name]
    print(name, label, sha, want["sha256"])
    assert label == want["label"]
    assert sha == want["sha256"], (name, label, TWIN[name]["what"])


@pytest.mark.parametrize("name", list(C3))
def test_3d_bits_are_the_recorded_ones(name):
    label, sha = _c3(name)
    want = _fixture()["c3"][name]
    print(name, label, sha, want["sha256"])
    assert label == want["label"]
    assert C3[name]["label"] in (None, label), "the case no longer reaches the kernel form it was made for"
    assert sha == want["sha256"], (name, label, C3[name]["what"])


def test_fixture_names_its_writer_and_covers_the_cases():
    doc = _fixture()
    assert doc["written_by"].startswith("the library of commit ")
    assert set(doc["twin"]) == set(TWIN) and set(doc["c3"]) == set(C3)
    assert all(v["equals_depth_1"] for v in doc["twin"].values()), "the recorded kernels agreed at depth 1"
