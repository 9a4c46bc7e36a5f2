"""Host side of the exact tests of the first stage without its convolution output (no GPU): the plan restated in
tests/first_stage_exact.py against the byte queries of the built library (seld_first_stage_gram_workspace,
seld_first_stage_bwd_workspace) on every case and on a grid that crosses each constant; what every case of
tests/golden/first_stage_exact_cases.py claims to reach (blocks per workgroup, ragged or not, chunk lengths, the
fs_wgrad_kernel form); the exactness conditions from the references' own numbers; and that the comparisons of the GPU
tests notice the defects they are there for."""
import ctypes

import pytest
import torch

from tests import first_stage_exact as FX
from tests.helpers import pkg

IDS = [c["name"] for c in FX.CASES]


def _queries(x, cout, algebra):
    P = pkg()
    lib = P._lib.lib()
    d = P.hip_ops.make_conv_desc(tuple(x), cout, algebra, (3, 3), 1, 1, 1)
    return int(lib.seld_first_stage_gram_workspace(ctypes.byref(d))), int(lib.seld_first_stage_bwd_workspace(ctypes.byref(d)))


@pytest.mark.parametrize("case", FX.CASES, ids=IDS)
def test_case_reaches_what_it_lists(case):
    pl = FX.plan(case)
    assert len(case["why"]) > 8 and set(case["sections"]) <= set("ABC")
    assert case["x"][1] == 8 and case["x"][2] % 8 == 0 and case["x"][3] % 64 == 0
    assert pl["blocks"] == case["blocks"]
    assert pl["gram"] == case["gram"] and pl["wgrad"] == case["wgrad"]
    assert pl["chunks"] == case["chunks"] and sum(pl["chunks"]) == pl["total"] and all(n % 4 == 0 and n > 0 for n in pl["chunks"])
    assert pl["form"] == case["form"]
    gram_bytes, bwd_bytes = _queries(case["x"], case["cout"], case["algebra"])
    assert gram_bytes == pl["gram_bytes"] and bwd_bytes == pl["bwd_bytes"]
    assert FX.bwd_supported(case["algebra"], case["cout"])


def test_the_table_holds_the_hazards_of_the_kernels():
    by, pl = FX.BY_NAME, lambda n: FX.plan(FX.BY_NAME[n])
    ragged = lambda walk: walk[0] != walk[1]
    # one block; the three block tables on it
    assert {by[n]["algebra"] for n in ("one_block_q64", "one_block_dq64", "one_block_r64")} == {1, 4, 8}
    assert all(pl(n)["blocks"] == 1 for n in ("one_block_q64", "one_block_dq64", "one_block_r64"))
    # interior halos both ways and an image boundary between blocks
    N, _, H, Wd = by["halos_dq128"]["x"]
    assert N > 1 and H // 8 > 1 and Wd // 64 > 1
    # every fs_wgrad_kernel instantiation
    assert {c["form"] for c in FX.CASES if "C" in c["sections"]} == {"<2, false>", "<2, true>", "<4, true>", "<6, true>"}
    assert by["one_block_r64"]["form"] == by["one_block_q64"]["form"] == "<2, false>"
    # fs_wgrad_kernel: a second block in some workgroups (cross-block prefetch), then a third (the buffer toggle returns)
    assert pl("ragged_wgrad_q64")["wgrad"] == (1, 2) and not ragged(pl("ragged_wgrad_q64")["gram"])
    assert pl("ragged_gram_q64")["wgrad"] == (2, 3) and pl("ragged_gram_dq192")["wgrad"] == (2, 3)
    # fs_gram_kernel: a second block in some workgroups, then a third
    assert pl("ragged_gram_q64")["gram"] == (1, 2) and pl("three_gram_blocks")["gram"] == (2, 3)
    # fs_reduce_kernel: several chunks, the last one short
    ch = pl("ragged_wgrad_dq64")["chunks"]
    assert len(ch) == 3 and ch[-1] < ch[0] and ch == (8536, 8536, 8528)
    assert len(pl("ragged_gram_q64")["chunks"]) == 4
    # no bias, Dropout on one quaternion and one dual-quaternion case
    assert [c["name"] for c in FX.CASES if not c["bias"]] == ["one_block_dq64"]
    assert sorted(c["algebra"] for c in FX.CASES if c["drop"]) == [4, 8]
    assert [c["name"] for c in FX.CASES if c["sections"] == "A"] == ["three_gram_blocks"]


def test_plan_restated_on_a_grid():
    """Both byte queries on shapes either side of every constant of the plan: 256 and 512 workgroups, 8192 elements per
    reduction chunk, the clamp to 64 chunks, each supported (algebra, Cout)."""
    n = 0
    seen = set()
    shapes = [(1, 8, 64), (1, 8, 128), (3, 16, 64), (1, 8, 64 * 255), (1, 8, 64 * 256), (1, 8, 64 * 257), (2, 8, 64 * 256),
              (1, 8, 64 * 511), (1, 16, 64 * 256), (1, 8, 64 * 513), (1, 8, 8128), (1, 8, 8192), (1, 8, 16320), (1, 8, 16384),
              (2, 8, 8192 * 3 + 64), (8, 64, 8192), (8, 64, 8128), (8, 72, 8192), (5, 8, 5120), (3, 24, 3712)]
    for (N, H, Wd) in shapes:
        for algebra, cout in ((1, 64), (4, 64), (8, 64), (8, 128), (8, 192)):
            c = dict(x=(N, 8, H, Wd), cout=cout, algebra=algebra)
            pl = FX.plan(c)
            assert _queries(c["x"], cout, algebra) == (pl["gram_bytes"], pl["bwd_bytes"]), (c, pl)
            seen.add((pl["gram_wgs"] == FX.GRAM_WGS, pl["wgrad_wgs"] == FX.WGRAD_WGS, min(pl["nchunk"], 3), pl["nchunk"] == FX.RED_MAX))
            n += 1
    chunks = {FX.plan(dict(x=(N, 8, H, Wd), cout=64, algebra=4))["nchunk"] for N, H, Wd in shapes}
    assert {1, 2, 3, 63, 64} <= chunks, chunks
    print(f"{n} descriptors, {len(seen)} regimes")
    # (256 blocks hold 16384 elements of a channel: below 256 workgroups there are fewer than three chunks)
    assert seen == {(False, False, 1, False), (False, True, 2, False), (False, True, 3, False), (True, True, 3, False),
                    (True, True, 3, True)}


def test_shapes_the_path_does_not_take():
    assert _queries((1, 8, 8, 64), 256, 8) [1] == 0 and _queries((1, 8, 8, 64), 256, 8)[0] > 0       # Cout 256: no backward
    assert _queries((1, 8, 8, 64), 128, 4)[1] == 0 and _queries((1, 8, 8, 64), 128, 1)[1] == 0      # wider quaternion / real
    assert _queries((1, 8, 8, 96), 64, 4) == (0, 0) and _queries((1, 8, 12, 64), 64, 4) == (0, 0)   # W % 64, H % 8
    assert not FX.bwd_supported(8, 256) and not FX.bwd_supported(4, 128) and FX.bwd_supported(8, 128)
    for algebra, cout, form in ((8, 192, "<6, true>"), (8, 128, "<4, true>"), (8, 64, "<2, true>"), (4, 64, "<2, false>"),
                                (1, 64, "<2, false>")):
        assert FX.wgrad_form(algebra, cout) == form


@pytest.mark.parametrize("case", FX.CASES, ids=IDS)
def test_exactness_conditions_and_integer_references(case):
    """reference() asserts the conditions itself (|G|, |s|, |W G| < 2^24; per-chunk sum |dz xhat| and per-workgroup
    sum |a dz xcol| < 2^22); here: the inputs are what the module says, and the identity the device relies on holds in
    float64 against the statistics of y itself."""
    t = FX.inputs(case)
    for n, lim in (("x", 2), ("dout", 2), ("beta", 2), ("mean", 2), ("gamma", 2)):
        assert t[n].dtype == torch.float32 and bool((t[n] == t[n].round()).all()) and float(t[n].abs().max()) <= lim, n
    assert all(set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and tuple(w.shape) == FX.weight_shape(case) for w in t["ws"])
    assert set(t["invstd"].unique().tolist()) <= {0.5, 1.0, 2.0}
    assert (t["bias"] is None) == (not case["bias"])
    g = t["gamma"].view(-1, 8)
    assert bool(((g > 0).any(1) & (g < 0).any(1) & (g == 0).any(1)).all()), "a positive, a negative, a zero channel per group"
    r = FX.reference(case)
    assert float(r["gram"][72, 72]) == r["P"] == case["x"][0] * case["x"][2] * case["x"][3]
    assert torch.equal(r["gram"], r["gram"].t()) and float(r["gram"][73:].abs().max()) == 0.0
    print(f"{case['name']}: max G {float(r['G'].abs().max()):.3g}")
    if case["sections"] == "A":
        return
    assert r["identity_gap"] < 1e-9, r["identity_gap"]
    assert r["ties"] > 0, "integer inputs: windows with several maximal rows"
    print(f"  max |W G| {float(r['WG'].abs().max()):.3g}, max |y| {r['ymax']:.0f}, identity gap {r['identity_gap']:.1e}")
    for p, b in r["bwd"].items():
        for k, dw in enumerate(b["dw"]):
            bound = FX.dw_bound([m[k] for m in b["mag"]], b["count"][k], FX.slot_fill(k))
            print(f"  drop_p {p}: component {k}: max |dw| {float(dw.abs().max()):.4g}, largest bound {float(bound.max()):.3g}")
        opened = float((b["out"] != 0).double().mean())
        assert 0.05 < opened < 0.95, opened
    assert sorted(r["bwd"]) == ([0.0, 0.5] if case["drop"] else [0.0])


# ---- sensitivity: what the comparisons of the GPU tests would see -----------------------------------------------------------
def test_a_transposed_gram_tile_and_a_dropped_border_tap_are_visible():
    r = FX.reference(FX.case("one_block_q64"))
    E = r["gram"]
    bad = E.clone()
    bad[0:16, 16:32] = E[0:16, 16:32].t()
    bad[16:32, 0:16] = bad[0:16, 16:32].t()
    assert not torch.equal(bad, E) and torch.equal(bad, bad.t()), "a transposed off-diagonal tile keeps the symmetry"
    x = r["x"].clone()
    assert float(x[0, :, :, 0].abs().sum()) > 0
    x[0, :, :, 0] = 0.0                                   # the column a tap dropped at the left image border would lose
    G2, s2, _ = FX.gram_reference(x)
    assert not torch.equal(G2, r["G"]) and not torch.equal(s2, r["s"])


def test_a_window_row_matched_one_off_moves_dw_past_its_bound():
    """The backward reference with every window row r replaced by r ^ 1, on a one-block and on a multi-block case: some
    component gradient moves by more than its bound (by 0.5 at least: a dz is a multiple of 0.5)."""
    for name in ("one_block_q64", "halos_dq128"):
        c = FX.case(name)
        r = FX.reference(c)
        b = r["bwd"][0.0]
        N, _, H, Wd = c["x"]
        C = c["cout"]
        a = (r["gamma"] * r["invstd"]).double()
        moved = torch.zeros(C, FX.FS_K, dtype=torch.float64)
        for n in range(N):
            xc = torch.nn.functional.unfold(r["x"][n:n + 1].double(), 3, padding=1)[0]
            for flip in (0, 1):
                dzf = torch.zeros(C, H // 8, 8, Wd, dtype=torch.float64)
                dzf.scatter_(2, (r["idx"][n].long() ^ flip).unsqueeze(2), b["dz"][n].unsqueeze(2))
                moved += (1 - 2 * flip) * ((a.view(C, 1) * dzf.view(C, H * Wd)) @ xc.t())
        delta, _ = FX.fold_components(moved, c["algebra"])
        worst = max(float((d.abs() / FX.dw_bound([m[k] for m in b["mag"]], b["count"][k], FX.slot_fill(k))).max())
                    for k, d in enumerate(delta))
        assert max(float(d.abs().max()) for d in delta) >= 0.5 and worst > 100, (name, worst)


# ---- D: the closed-form float64 reference is torch autograd of conv -> batch_norm -> relu -> max_pool ------------------------
@pytest.mark.parametrize("name,kind", [("one_block_q64", "randn"), ("halos_dq128", "feature")])
def test_end_to_end_reference_is_float64_autograd(name, kind):
    import torch.nn.functional as F
    from oracle import seld_oracle as O
    c = FX.case(name)
    ref = FX.E2E(c, kind)
    assert ref.excusable <= FX.ROW_CAP
    t = ref.t
    w64 = [w.double().requires_grad_(True) for w in t["ws"]]
    b64 = t["bias"].double() if t["bias"] is not None else None
    g64, be64 = t["gamma"].double().requires_grad_(True), t["beta"].double().requires_grad_(True)
    y = O.hypercomplex_conv(t["x"].double(), w64, b64, 1, 1, 1, 1, mode="explicit")
    z = F.batch_norm(y, None, None, g64, be64, training=True, eps=float(torch.tensor(FX.EPS, dtype=torch.float32)))
    pooled, where = F.max_pool2d(F.relu(z), (FX.POOL, 1), return_indices=True)
    (pooled * t["cot"].double()).sum().backward()
    _, _, pre, e_z = ref.forward(ref.rows)
    assert float((torch.relu(pre) - pooled.detach()).abs().max()) < 1e-11
    b = ref.backward(ref.rows, pre > 0)
    assert float((b["dgamma"] - g64.grad).abs().max()) < 1e-9 * float(g64.grad.abs().max())
    assert float((b["dbeta"] - be64.grad).abs().max()) < 1e-9 * float(be64.grad.abs().max())
    for k, w in enumerate(w64):
        assert float((b["dw"][k] - w.grad).abs().max()) < 1e-9 * float(w.grad.abs().max()), k
    # every bound is positive and finite, and a window row moved to its neighbour is refused
    assert all(bool((e > 0).all()) and bool(torch.isfinite(e).all()) for e in b["e_dw"] + [b["e_dgamma"], b["e_dbeta"], e_z])
    with pytest.raises(AssertionError, match="window rows differ"):
        ref.check_rows((ref.rows + 1) % FX.POOL)


def test_rows_of_the_end_to_end_test():
    """Every row but the last is run end to end, is not served by the pooling convolution, or is named as left out."""
    P = pkg()
    lib = P._lib.lib()
    served = {c["name"]: int(lib.seld_hcq_pack_floats(ctypes.byref(FX.desc(P.hip_ops, c)), 2, 1)) > 0 for c in FX.CASES}
    assert all(served[n] for n in FX.D_NAMES + FX.D_TOO_SLOW) and not any(served[n] for n in FX.D_NOT_SERVED)
    assert sorted(FX.D_NAMES + FX.D_NOT_SERVED + FX.D_TOO_SLOW) == sorted(c["name"] for c in FX.CASES if "C" in c["sections"])
    assert {FX.plan(FX.case(n))["wgrad"] for n in FX.D_NAMES} == {(1, 1), (1, 2), (2, 3)}
    assert {FX.plan(FX.case(n))["gram"] for n in FX.D_NAMES} == {(1, 1), (1, 2)}
