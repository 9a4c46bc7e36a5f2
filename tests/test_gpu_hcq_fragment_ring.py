"""hcq_conv_kernel's weight-fragment ring (csrc/hcq_conv.hip): a workgroup copies each unit of packed fragments into one
of two LDS slots and its four waves read them there.  The shapes are the smallest that reach each way the ring can go
wrong (pairs of k-groups per chunk = ranges x ceil(ceil(chunk x taps / 4) / 2)); values against the fp64 oracle at the
tolerance of every convolution test (1e-4 of max|ref|), and every plain launch three times with bitwise equal results:
a race on a ring slot or an input buffer shows as a run-to-run difference."""
import pytest
import torch

from oracle import seld_oracle as O

pytestmark = pytest.mark.gpu
REL = 1e-4
DEV = "cuda:0"

RING_CASES = {
    # algebra, x shape, cout, k, pad, dil
    "one_chunk_one_pair": (4, (1, 32, 64), 64, 1, 0, 1),                 # prologue only, nothing to prefetch (forward:
                                                                         # 8 block channels of x are no channel tile)
    "odd_pairs_two_chunks": (4, (2, 64, 128), 128, 3, 2, 2),             # 3 pairs per chunk: slot parity flips per chunk
    "odd_pairs_six_chunks": (4, (1, 192, 64), 64, 3, 1, 1),
    "odd_pairs_3x3_four_chunks": (4, (1, 64, 3, 64), 64, (3, 3), 1, 1),  # 5 pairs per chunk (the quaternion 1-D layers
                                                                         # above keep per-wave global loads: hcq_plan)
    "half_filled_last_pair": (8, (3, 192, 64), 384, 3, 55, 55),          # 3 k-groups, chunk 4, halo wider than the tile
    "c3x3_mixed_tiles": (8, (1, 192, 4, 128), 192, (3, 3), 1, 1),        # 10 pairs per chunk, narrower range-1 units,
                                                                         # mixed-tile workgroups, halo rows at the edge
    "c3x3_three_tiles": (8, (9, 192, 8, 512), 192, (3, 3), 1, 1),        # 12 KB slots (the cnn.1 layout)
    "k1_one_pair_per_range": (8, (2, 192, 128), 128, 1, 0, 1),
    "k1_chunk_16_24": (8, (2, 384, 128), 192, 1, 0, 1),
}


def _err(got, ref):
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max()), max(float(ref.abs().max()), 1e-6)


def _close(got, ref, rel=REL):
    err, scale = _err(got, ref)
    assert err <= rel * scale, f"max err {err:.3e} vs scale {scale:.3e}"


FORWARD_ONLY = ("one_chunk_one_pair",)


def _setup(name, seed=91):
    import seld_amd
    H = seld_amd.hip_ops
    algebra, shape, cout, k, pad, dil = RING_CASES[name]
    kk = (k,) if isinstance(k, int) else k
    desc = H.make_conv_desc(tuple(shape), cout, algebra, kk, 1, pad, dil)
    for mode in ((0,) if name in FORWARD_ONLY else (0, 1)):
        assert H.hcq_label(desc, mode).startswith("hcq_conv_kernel<"), H.hcq_label(desc, mode)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen)
    wshape = (cout // algebra, shape[1] // algebra) + tuple(kk)
    ws = [torch.randn(wshape, generator=gen) * 0.2 for _ in range(algebra)]
    yshape = (shape[0], cout) + tuple(shape[2:])
    dy = torch.randn(yshape, generator=gen)
    return H, desc, x, ws, dy, (pad, dil, cout)


def _three_times(H, desc, mode, src, wp, shape):
    outs = []
    for _ in range(3):
        out = torch.full(shape, float("nan"), device=DEV)
        H.hcq_conv(desc, mode, src, wp, (out,))
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "run-to-run difference"
    return outs[0]


@pytest.mark.parametrize("name", [n for n in RING_CASES if n != "k1_chunk_16_24"])
def test_ring_forward_and_data_gradient_vs_oracle(name):
    H, desc, x, ws, dy, (pad, dil, _) = _setup(name)
    xd, dyd, wd = x.to(DEV), dy.to(DEV), [w.to(DEV) for w in ws]
    y = _three_times(H, desc, 0, xd, H.hcq_pack(desc, 0, wd), tuple(dy.shape))
    x64 = x.double().requires_grad_(True)
    yr = O.hypercomplex_conv(x64, [w.double() for w in ws], None, 1, pad, 1, dil, mode="explicit")
    _close(y, yr)
    if name in FORWARD_ONLY:
        return
    dx = _three_times(H, desc, 1, dyd, H.hcq_pack(desc, 1, wd), tuple(x.shape))
    (yr * dy.double()).sum().backward()
    _close(dx, x64.grad)


def test_ring_k1_chunk_16_and_24_vs_block_matrix_kernels(seld_env):
    """384 input channels (chunk 16 forward, 24 in the data gradient): the oracle is slow here, the reference is the
    block-matrix kernels (pinned by the oracle tests), 1e-5 of the maximum."""
    H, desc, x, ws, dy, _ = _setup("k1_chunk_16_24")
    xd, dyd, wd = x.to(DEV), dy.to(DEV), [w.to(DEV) for w in ws]
    y = _three_times(H, desc, 0, xd, H.hcq_pack(desc, 0, wd), tuple(dy.shape))
    dx = _three_times(H, desc, 1, dyd, H.hcq_pack(desc, 1, wd), tuple(x.shape))
    seld_env.set("SELD_CONV_NO_HCQ", "1")
    y_ref = H.conv_fwd(desc, xd, wd)
    dx_ref = H.conv_bwd_data(desc, dyd, wd, tuple(x.shape))
    torch.cuda.synchronize()
    seld_env.unset("SELD_CONV_NO_HCQ")
    _close(y, y_ref, 1e-5)
    _close(dx, dx_ref, 1e-5)


@pytest.mark.parametrize("name", ["half_filled_last_pair", "k1_chunk_16_24"])
def test_ring_pair_launches_match_two_single_calls(name):
    """Two weight sets in one launch (forward) and two sources along K (data gradient: the source switches at chunk
    nch) against the two single calls."""
    H, desc, x, wsA, dy, (pad, dil, cout) = _setup(name)
    assert H._hcq_ok(desc, 0, 2) and H._hcq_ok(desc, 1, 2)
    assert H.hcq_label(desc, 0, 2).startswith("hcq_conv_kernel<") and H.hcq_label(desc, 1, 2).startswith("hcq_conv_kernel<")
    gen = torch.Generator().manual_seed(92)
    wsB = [torch.randn(w.shape, generator=gen) * 0.2 for w in wsA]
    dyB = torch.randn(dy.shape, generator=gen)
    wl = [[w.to(DEV).requires_grad_(True) for w in wsA], [w.to(DEV).requires_grad_(True) for w in wsB]]
    cots = [dy.to(DEV), dyB.to(DEV)]

    def run(pair):
        xs = x.to(DEV).requires_grad_(True)
        if pair:
            ya, yb = H.hyper_conv_pair(xs, wl[0], None, wl[1], None, 1, pad, dil)
        else:
            ya = H.hyper_conv(xs, wl[0], None, 1, pad, dil)
            yb = H.hyper_conv(xs, wl[1], None, 1, pad, dil)
        ((ya * cots[0]).sum() + (yb * cots[1]).sum()).backward()
        return ya.detach(), yb.detach(), xs.grad

    got, ref = run(True), run(False)
    for a, b in zip(got, ref):
        _close(a, b)
    # the pair launches themselves, three times each
    xd = x.to(DEV)
    wd = [[w.detach() for w in s] for s in wl]
    wp = H.hcq_pack(desc, 0, wd[0], wd[1])
    outs = []
    for _ in range(3):
        o1, o2 = torch.empty_like(cots[0]), torch.empty_like(cots[0])
        H.hcq_conv(desc, 0, xd, wp, (o1, o2))
        outs.append((o1, o2))
    wpd = H.hcq_pack(desc, 1, wd[0], wd[1])
    douts = []
    for _ in range(3):
        od = torch.empty_like(xd)
        H.hcq_conv(desc, 1, cots[0], wpd, (od,), x2=cots[1])
        douts.append(od)
    torch.cuda.synchronize()
    for i in (1, 2):
        assert torch.equal(outs[0][0], outs[i][0]) and torch.equal(outs[0][1], outs[i][1]) and torch.equal(douts[0], douts[i])
    _close(outs[0][0], ref[0])
    _close(outs[0][1], ref[1])
    _close(douts[0], ref[2])


@pytest.mark.parametrize("name", ["odd_pairs_two_chunks", "c3x3_mixed_tiles"])
def test_ring_epilogues_that_overlay_the_staging_area(name):
    """ADD + STATS (the statistics scratch overlays LDS after the K loop) and ACCUMULATE, against the oracle; the
    statistics as in test_hcq_conv_vs_oracle (not bitwise: the replicas are filled with atomics)."""
    import seld_amd
    L = seld_amd._lib
    H, desc, x, ws, dy, (pad, dil, cout) = _setup(name)
    gen = torch.Generator().manual_seed(93)
    bias = torch.randn(cout, generator=gen)
    addend = torch.randn(dy.shape, generator=gen)
    xd, wd, bd, ad = x.to(DEV), [w.to(DEV) for w in ws], bias.to(DEV), addend.to(DEV)
    yr = O.hypercomplex_conv(x.double(), [w.double() for w in ws], bias.double(), 1, pad, 1, dil, mode="explicit")
    stats_rep = H.new_stats(cout, torch.device(DEV))
    y2 = H.conv_fwd(desc, xd, wd, bd, epilogue=L.SELD_EPI_ADD | L.SELD_EPI_STATS, addend=ad, stats=stats_rep)
    ref2 = yr + addend.double()
    _close(y2, ref2)
    stats = stats_rep.view(H.STATS_REPLICAS, 2 * cout).sum(0).double().cpu()
    red = tuple(i for i in range(ref2.dim()) if i != 1)
    assert torch.allclose(stats[:cout], ref2.sum(dim=red), rtol=1e-4, atol=2e-3)
    assert torch.allclose(stats[cout:], (ref2 ** 2).sum(dim=red), rtol=1e-4, atol=2e-3)
    y3 = y2.clone()
    H.conv_fwd(desc, xd, wd, None, out=y3, epilogue=L.SELD_EPI_ACCUMULATE)
    _close(y3, ref2 + (yr - bias.double().view(1, -1, *([1] * (yr.dim() - 2)))))
