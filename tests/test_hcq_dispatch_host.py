"""The fast-product ("hcq") convolution family's dispatch, host side (no GPU): the built library must answer the host-only
queries -- packed-weight size, kernel label and launch shape (grid, LDS bytes, ring offset, slot kind, rows per workgroup)
for every mode and pair count, weight-gradient support and label, grouped weight-gradient family -- exactly as the fixture
records them, for every descriptor and under every recorded environment.  The fixture was written by the library that
preceded the one-table, one-plan launch code (tests/golden/make_golden_hcq_dispatch.py), so a row that differs is a changed
kernel choice, a changed launch, or a label that no longer names what is launched."""
import json
import os
import re

import pytest

from tests.golden import make_golden_hcq_dispatch as G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hcq_dispatch.json")

# the instantiation table of csrc/hcq_conv.hip: KH, KW, IBC, XI of the dual-quaternion / quaternion kernels (0: none) ...
INST = ((1, 3, 8, 5, 3), (1, 3, 8, 7, 5), (1, 3, 8, 9, 0), (1, 3, 4, 6, 3), (1, 1, 16, 8, 4), (1, 1, 24, 12, 6),
        (1, 1, 8, 4, 2), (3, 3, 4, 7, 4), (3, 3, 2, 4, 2), (3, 3, 1, 2, 1))
# ... and its tile programs: NT1, NT2, NR, MX
TILEV = ((1, 2, 2, "false"), (1, 1, 2, "true"), (1, 1, 2, "false"), (2, 0, 1, "false"), (1, 0, 1, "false"))


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return G.decode(json.load(f))


def test_fixture_matches_the_grid(recorded):
    rows = list(G.descriptors())
    assert len(rows) == len(list(G.G.descriptors())) + len(G.EXTRA)
    assert list(recorded) == [name for name, _ in G.ENVS]
    assert all(len(col) == len(rows) for col in recorded.values())
    launches = {(v[1][1], tuple(v[2][1:])) for col in recorded.values() for a in col for v in a[1:1 + len(G.COMBOS)]
                if v[1][0] == 0}
    labels = {l for l, _ in launches}
    # every row of the table in every tile program it is instantiated for
    for kh, kw, ibc, xi8, xi4 in INST:
        for nt1, nt2, nr, mx in TILEV:
            xi = xi8 if nr == 2 else xi4
            if xi:
                stem = f"hcq_conv_kernel<{kh}, {kw}, {ibc}, {nt1}, {nt2}, {nr}, {xi}, {mx}, "
                assert any(l.startswith(stem) for l in labels), stem
    # every state of the plan's flags: mixed-tile workgroups or not, ring or per-wave global loads (dual quaternion too),
    # both slot kinds of the ring
    for mx in ("true", "false"):
        for gf in ("true", "false"):
            if (mx, gf) != ("true", "true"):      # (a mixed-tile launch takes whole-pair slots at two workgroups per CU)
                assert any(re.fullmatch(rf"hcq_conv_kernel<.*, 2, \d+, {mx}, {gf}>", l) for l in labels), (mx, gf)
    ring = {s[4] for l, s in launches if l.endswith("false>")}
    assert ring == {0, 1}
    assert all(s[3:5] == (0, 0) for l, s in launches if not l.endswith("false>")), "no ring: no offset, no slot kind"
    # the first-layer kernels, plain and pooling: one and two block channels in both algebras, every tile count
    for stem in ("hcq_first_kernel", "hcq_first_pool_kernel"):
        for ibc in (1, 2):
            for nt1, nt2, nr, mx in TILEV:
                if mx == "false":
                    assert f"{stem}<{ibc}, {nt1}, {nt2}, {nr}, 8>" in labels
    assert all((s[5] == 8) == l.startswith("hcq_first_") for l, s in launches)
    # the weight gradient: every tap shape, both XI buckets, and the grouped kernel's four families
    wl = {v[1] for col in recorded.values() for a in col for v in a[9:11] if v[0] == 0}
    for kh, kw in ((1, 1), (1, 3), (3, 3)):
        for xi in (4, 8):
            assert any(re.fullmatch(rf"hcq_wgrad_kernel<{kh}, {kw}, \d, \d, {xi}>", l) for l in wl), (kh, kw, xi)
    assert {a[11] for a in recorded["default"] if len(a) > 1} == {-1, 0, 1, 2, 3}
    # SELD_CONV_NO_HCQ: nothing is packed, no weight gradient is taken
    assert all(v[0] == 0 for a in recorded["SELD_CONV_NO_HCQ=1"] for v in a[1:1 + len(G.COMBOS)])
    assert all(a[7] == 0 and a[8] == 0 for a in recorded["SELD_CONV_NO_HCQ=1"] if len(a) > 1)
    # SELD_CONV_NO_SMALLK: the 8-channel first layer comes over at the benchmark's size
    row = rows.index(G._c1(8, (32, 8, 128, 512), 192, (3, 3), 1, 1))
    assert recorded["default"][row][1][0] == 0
    assert recorded["SELD_CONV_NO_SMALLK=1"][row][1][1] == [0, "hcq_first_kernel<1, 1, 2, 2, 8>"]


def test_library_answers_as_recorded(recorded, seld_env):
    def setenv(name, value):
        seld_env.unset(name) if value is None else seld_env.set(name, value)
    got = G.walk(setenv)
    rows = list(G.descriptors())
    for name, _ in G.ENVS:
        for row, w, g in zip(rows, recorded[name], got[name]):
            assert g == w, (name, row)
