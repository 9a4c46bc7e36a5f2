"""The block-matrix convolution family's dispatch, host side (no GPU): the built library must answer the host-only
queries -- output shape, kernel labels, pair support, data-gradient workspace, transposed-convolution labels -- exactly as
the fixture records them, for every descriptor of the grid and under every recorded environment.  The fixture was written
by the library that preceded the one-plan-per-family launch code (tests/golden/make_golden_conv_dispatch.py), so a row that
differs is a changed kernel choice, or a label that no longer names what is launched."""
import json
import os

import pytest

from tests.golden import make_golden_conv_dispatch as G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch.json")


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return G.decode(json.load(f))


def test_fixture_matches_the_grid(recorded):
    rows = list(G.descriptors())
    assert len(rows) == len(G.ALGEBRAS) * len(G.CHANNELS) * len(G.KERNELS) * len(G.STRIDES) * len(G.DILATIONS) * \
        len(G.SPATIAL) * len(G.BATCHES) + len(G.EXTRA)
    assert list(recorded) == [name for name, _ in G.ENVS]
    assert all(len(col) == len(rows) for col in recorded.values())
    # the grid is worth its size: every kernel family and every tile of both plans is named somewhere in it
    text = " ".join(sorted({v[1] for col in recorded.values() for a in col for v in a if isinstance(v, list)}))
    for stem in ("hc_conv_kernel<", "hc_conv_vec_kernel<", "hc_conv_smallk_kernel<", "hc_wgrad_kernel<",
                 "hc_wgrad32_kernel<", "hc_wgrad_row_kernel<"):
        assert stem in text, stem
    for tile in ("2, 4, 4", "4, 3, 5", "2, 2, 2", "2, 3, 4", "4, 1, 5", "4, 1, 10"):
        assert "hc_wgrad_row_kernel<" + tile in text or "hc_wgrad32_kernel<" + tile in text \
            or "hc_wgrad_kernel<" + tile in text, tile
    for ct, pt in ((12, 1), (12, 2), (6, 1), (4, 4), (2, 4), (1, 4)):
        assert f"hc_conv_kernel<{ct}, {pt}, " in text, (ct, pt)


def test_library_answers_as_recorded(recorded, seld_env):
    def setenv(name, value):
        seld_env.unset(name) if value is None else seld_env.set(name, value)
    got = G.walk(setenv)
    rows = list(G.descriptors())
    for name, _ in G.ENVS:
        for row, w, g in zip(rows, recorded[name], got[name]):
            assert g == w, (name, row)
