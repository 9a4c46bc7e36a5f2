"""Every dropout mask of the HIP path against the host Philox reference (tests/philox_ref.py, itself held to published
known answers by tests/test_philox_host.py).  A mask is a pure function of the seed (torch.initial_seed() mixed with
hip_ops.philox.stream_id), the counter (host offset + the device base, word 0 of the step state) and float32(p), so
there is nothing to tolerate: the mask comparisons are np.array_equal / torch.equal.  The model-level test at the end
feeds the same masks to the fp64 oracle and compares a two-step training trajectory with Dropout ON.

Inputs are finite everywhere: the consumers differ on a non-finite activation at a dropped position (some multiply by
0, some select 0), which is not what these tests are about."""
import math

import numpy as np
import pytest
import torch

from oracle import seld_oracle as O
from tests import philox_ref as R
from tests.golden.cases import MODEL_CASES, model_kwargs, train_target
from tests.helpers import build_model, fill_weights, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20240607
BIG_N = 4 * 256 * 8192 + 5          # one group past grid_for's cap of 8192 blocks x 256 threads: the grid-stride loop runs


def _H():
    return pkg().hip_ops


@pytest.fixture
def philox():
    """hip_ops.philox with its seed set and its position at 0; stream_id, offset and device base restored afterwards."""
    H = _H()
    sid = H.philox.stream_id
    torch.manual_seed(SEED)
    H.philox.set_offset(0)
    try:
        yield H.philox
    finally:
        H.philox.stream_id = sid
        H.philox.set_offset(0)


def _mixed(f, n):
    """A comparison against an all-kept or all-dropped mask would show nothing."""
    if n > 2:
        assert (f > 0).any() and (f == 0).any(), "host mask is not mixed: pick another offset"


def _values(n, salt):
    gen = torch.Generator().manual_seed(salt)
    return torch.randn(n, generator=gen)            # both signs, finite


_big = {}


def _inputs(n):
    """(x, cot) for a size; the 34 MB pair is made once for its three rates."""
    if n != BIG_N:
        return _values(n, 100 + n), _values(n, 200 + n)
    if not _big:
        _big["x"], _big["cot"] = _values(n, 1), _values(n, 2)
    return _big["x"], _big["cot"]


# the first offset at which, under SEED, every (n, p) below with n in {3, 4, 5} has a kept AND a dropped element (found
# by a host search over the reference; _mixed asserts it in every case)
_OFFSET = 18


@pytest.mark.parametrize("p", [0.3, 0.5, 0.9])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, BIG_N])
def test_dropout_forward_and_backward_masks(n, p, philox):
    H = _H()
    x, cot = _inputs(n)
    philox.set_offset(_OFFSET)
    f = R.factors(torch.initial_seed(), _OFFSET, n, p)
    _mixed(f, n)
    xd = x.to(DEV).requires_grad_(True)
    y = H.dropout(xd, p, True)
    y.backward(cot.to(DEV))
    torch.cuda.synchronize()
    assert philox.offset == _OFFSET + (n + 3) // 4
    assert set(np.unique(f).tolist()) <= {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    assert np.array_equal(y.detach().cpu().numpy(), x.numpy() * f)
    assert np.array_equal(xd.grad.cpu().numpy(), cot.numpy() * f)


def test_dropout_entry_point_p_zero_is_identity_and_bad_p_is_refused(philox):
    L = pkg()._lib
    x = _values(1023, 5).to(DEV)
    y = torch.full_like(x, 7.0)
    st = philox.state(DEV)
    call = lambda p: L.lib().seld_dropout_fwd(L.ptr(x), x.numel(), p, philox.seed(), 3, L.ptr(st), L.ptr(y), L.current_stream())
    assert call(0.0) == L.SELD_OK
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), x.view(torch.int32))          # the identity, bit for bit
    einval = next(k for k, v in L._ERRORS.items() if v == "SELD_EINVAL")
    y.fill_(7.0)
    assert call(1.0) == einval
    assert call(-0.25) == einval
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                          # a refused call launches nothing


@pytest.mark.parametrize("p", [0.5, 0.25])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 8192])
def test_channel_dropout_mask(rows, p, philox):
    H = _H()
    philox.set_offset(_OFFSET)
    f = R.factors(torch.initial_seed(), _OFFSET, rows, p)
    _mixed(f, rows)
    N, C = (rows, 1) if rows % 2 else (2, rows // 2)
    mask = H.channel_dropout_mask(N, C, p, torch.device(DEV))
    assert mask.shape == (rows,) and philox.offset == _OFFSET + (rows + 3) // 4
    assert np.array_equal(mask.cpu().numpy(), f)


def test_stacked_channel_masks_are_the_blocks_consecutive_draws(philox):
    """model.TC_Block._dropout_masks: one launch over (N * blocks, G) rows, N * G % 4 == 0; block i's rows are what the
    i-th of `blocks` consecutive draws of N * G rows gives."""
    H = _H()
    N, blocks, G, p = 2, 10, 32, 0.5
    philox.set_offset(_OFFSET)
    host = R.Stream(torch.initial_seed(), offset=_OFFSET)
    masks = H.channel_dropout_mask(N * blocks, G, p, torch.device(DEV)).view(blocks, N * G).cpu().numpy()
    for i in range(blocks):
        f = host.draw(N * G, p)
        _mixed(f, N * G)
        assert np.array_equal(masks[i], f), i
    assert philox.offset == host.offset
    # and through the model's own method
    M = pkg().model
    tcn = M.TC_Block(in_channels=16, domain="R", G=G, U=16, V=[16, 16], D=[blocks], spatial_dropout_rate=p).to(DEV).train()
    philox.set_offset(_OFFSET)
    got = tcn._dropout_masks(torch.zeros(N, 16, 8, device=DEV))
    assert got is not None and np.array_equal(got.cpu().numpy(), masks)
    assert philox.offset == host.offset


def _draw16(H, p=0.5):
    """16 factors through H.dropout on ones (4 groups)."""
    return H.dropout(torch.ones(16, device=DEV), p, True).cpu().numpy()


def test_counter_carries_into_the_high_word(philox):
    H = _H()
    first = 2 ** 32 - 2                        # groups 2^32 - 2 .. 2^32 + 1: c1 goes 0 -> 1 inside the tensor
    philox.set_offset(first)
    f = R.factors(torch.initial_seed(), first, 16, 0.5)
    _mixed(f, 16)
    assert np.array_equal(_draw16(H), f)
    assert not np.array_equal(f[8:], R.factors(torch.initial_seed(), 0, 8, 0.5))       # c1 matters on the host side
    assert philox.offset == first + 4 == philox.get_offset()


def test_seed_above_2_32_reaches_the_high_key_word(philox):
    H = _H()
    seed = 2 ** 40 + 12345
    torch.manual_seed(seed)
    assert torch.initial_seed() == seed and philox.seed() == seed
    f = R.factors(seed, 0, 16, 0.5)
    _mixed(f, 16)
    assert np.array_equal(_draw16(H), f)
    assert not np.array_equal(f, R.factors(seed & 0xFFFFFFFF, 0, 16, 0.5))


def test_stream_id_mixes_into_the_seed_mod_2_64(philox):
    H = _H()
    philox.stream_id = 3
    host = R.Stream(torch.initial_seed(), stream_id=3)
    assert philox.seed() == host.seed() and 3 * R.GOLDEN64 >= 2 ** 64
    f3 = host.draw(16, 0.5)
    _mixed(f3, 16)
    assert np.array_equal(_draw16(H), f3)
    philox.stream_id = 0
    philox.set_offset(0)
    f0 = _draw16(H)
    assert np.array_equal(f0, R.Stream(torch.initial_seed()).draw(16, 0.5))
    assert not np.array_equal(f0, f3)


def test_device_base_is_added_to_the_host_offset(philox):
    H = _H()
    base, off = 2 ** 32 - 3 - _OFFSET, _OFFSET         # the sum carries too
    philox.set_offset(off)                              # (zeroes the base: write it afterwards)
    philox.state(DEV)[0] = base
    assert philox.get_offset() == base + off
    f = R.factors(torch.initial_seed(), base + off, 16, 0.5)
    _mixed(f, 16)
    assert np.array_equal(_draw16(H), f)
    assert not np.array_equal(f, R.factors(torch.initial_seed(), off, 16, 0.5))
    assert philox.offset == off + 4 and philox.get_offset() == base + off + 4
    mask = H.channel_dropout_mask(1, 6, 0.5, torch.device(DEV))
    assert np.array_equal(mask.cpu().numpy(), R.factors(torch.initial_seed(), base + off + 4, 6, 0.5))
    philox.set_offset(0)
    assert philox.get_offset() == 0 and int(philox.state(DEV)[0].item()) == 0


def test_consecutive_draws_are_consecutive_slices_of_one_stream(philox):
    H = _H()
    host = R.Stream(torch.initial_seed())
    dev = torch.device(DEV)
    got = [H.dropout(torch.ones(5, device=DEV), 0.5, True),
           H.channel_dropout_mask(1, 4, 0.5, dev),
           H.dropout(torch.ones(1, device=DEV), 0.5, True),
           H.channel_dropout_mask(3, 341, 0.5, dev)]
    whole = R.factors(torch.initial_seed(), 0, 4 * 260, 0.5)
    at = 0
    for g, n in zip(got, (5, 4, 1, 1023)):
        f = host.draw(n, 0.5)
        assert np.array_equal(f, whole[4 * at:4 * at + n])
        assert np.array_equal(g.cpu().numpy(), f), n
        at += (n + 3) // 4
    assert philox.offset == host.offset == 260


# ------------------------------------------------------------------------------------------
# the fused consumers of the mask
# ------------------------------------------------------------------------------------------
def _close(got, ref, rel, what):
    got, ref = got.double(), ref.double()
    scale = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


# the shapes of test_gpu_ops.py::test_bn_relu_pool_with_the_stage_dropout_inside (all taken by the fused kernels) and one
# that seld_bn_relu_pool_drop_ok refuses (W % 4 != 0: the dropout launch follows the pass)
@pytest.mark.parametrize("shape,ph,fused", [((2, 192, 16, 64), 8, True), ((3, 16, 4, 40), 2, True), ((2, 8, 12, 32), 3, True),
                                            ((2, 8, 12, 30), 3, False)])
def test_bn_relu_pool_dropout_is_the_host_mask(shape, ph, fused, philox):
    """out(drop_p = 0.3) == out(drop_p = 0) * host factors, bit for bit, and the backward pass with the cotangent `cot` is
    the undropped backward pass with the cotangent cot * factors (tolerances of the test named above)."""
    P = pkg()
    H, L = P.hip_ops, P._lib
    assert bool(L.lib().seld_bn_relu_pool_drop_ok(shape[2], shape[3], ph, 1)) == fused
    gen = torch.Generator().manual_seed(41)
    y0 = torch.randn(*shape, generator=gen)
    C = shape[1]
    g0, b0 = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1
    cot = torch.randn(shape[0], C, shape[2] // ph, shape[3], generator=gen)
    f = torch.from_numpy(R.factors(torch.initial_seed(), 5000, cot.numel(), 0.3)).view(cot.shape)

    def run(drop_p, cot_):
        bn = P.hip_nn.BatchNorm2d(C).to(DEV).train()           # a fresh module: the same running buffers for both calls
        with torch.no_grad():
            bn.weight.copy_(g0.to(DEV)); bn.bias.copy_(b0.to(DEV))
        y = y0.to(DEV).requires_grad_(True)
        philox.set_offset(5000)
        out = H.bn_relu_pool(y, bn, ph, 1, None, drop_p)
        (out * cot_.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        return out.detach().cpu(), y.grad.cpu(), bn.weight.grad.cpu(), bn.bias.grad.cpu(), philox.offset - 5000

    z = run(0.0, cot * f)
    got = run(0.3, cot)
    assert z[4] == 0 and got[4] == (cot.numel() + 3) // 4
    assert (f == 0).any() and (f > 0).any() and bool(((z[0] > 0) & (f == 0)).any())      # the mask bites on open ReLUs
    assert torch.equal(got[0], z[0] * f)
    _close(got[1], z[1], 1e-5, "dy")
    _close(got[2], z[2], 1e-4, "dgamma")
    _close(got[3], z[3], 1e-4, "dbeta")


# which entry point applies the stage's Dropout, per route: at hw = (16, 64) (the shape of
# test_gpu_ops.py::test_first_stage_dropout_in_the_pooled_pass) the pooling convolution is not taken -- it wants one channel
# tile per position tile, which 192 output channels get from N * H * W >= 512 * 64 on -- so the fused function launches
# seld_dropout_fwd itself; at hw = (128, 128) (a tiny model's first stage) the three routes are the three consumers
_FIRST_STAGE_ROUTES = {
    ((16, 64), "default"): "seld_dropout_fwd", ((16, 64), "SELD_FIRST_STAGE_STORE_Y"): "seld_dropout_fwd",
    ((16, 64), "SELD_NO_FUSED_STAGE0"): "seld_bn_relu_pool_fwd_drop",
    ((128, 128), "default"): "seld_hcq_first_pool_bn", ((128, 128), "SELD_FIRST_STAGE_STORE_Y"): "seld_bn_pool_finish",
    ((128, 128), "SELD_NO_FUSED_STAGE0"): "seld_bn_relu_pool_fwd_drop",
}


@pytest.mark.parametrize("hw", [(16, 64), (128, 128)], ids=["16x64", "128x128"])
@pytest.mark.parametrize("route", ["default", "SELD_FIRST_STAGE_STORE_Y", "SELD_NO_FUSED_STAGE0"])
def test_first_stage_dropout_is_the_host_mask(route, hw, philox, seld_env, monkeypatch):
    """conv_bn_relu_pool(..., drop_p = 0.3) on its three routes (no stored convolution output: the mask in the pooling
    convolution's epilogue; stored output: seld_bn_pool_finish; not fused: bn_relu_pool): the output is the undropped
    output z times the host factors, bit for bit; the weight and BatchNorm gradients are those of the undropped stage
    under the cotangent cot * factors (tolerances of test_gpu_ops.py::test_first_stage_dropout_in_the_pooled_pass).

    z is the output of the same call with drop_p = 0 from the same BatchNorm state wherever the two calls see the same
    batch statistics bit for bit: at 16 x 64 (32 position tiles, fewer than the 64 replica rows of a statistics buffer:
    one addend per slot) and on the route without the convolution output (statistics from the input's second moments,
    no atomics).  The other two routes at 128 x 128 sum their statistics with float atomics over 512 workgroups, which
    two calls need not repeat to the last bit: there z is the undropped `pooled` tensor that the very call under test
    keeps for its backward pass (the same kernel writes both), and the drop_p = 0 call must agree with it to 1e-6."""
    P = pkg()
    H, T, L = P.hip_ops, P.train, P._lib
    if route != "default":
        seld_env.set(route, "1")
    called = []
    check = L.check
    monkeypatch.setattr(L, "check", lambda rc, what: (called.append(what), check(rc, what))[1])
    cin, cout, ph = 8, 192, 8
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(2, cin, *hw, generator=gen)
    ws0 = [torch.randn(cout // 8, cin // 8, 3, 3, generator=gen) * 0.3 for _ in range(8)]
    g0 = torch.rand(cout, generator=gen) - 0.4
    g0[7] = 0.0
    cot = torch.randn(2, cout, hw[0] // ph, hw[1], generator=gen)
    f = torch.from_numpy(R.factors(torch.initial_seed(), 1000, cot.numel(), 0.3)).view(cot.shape)
    same_call = hw == (128, 128) and route != "default"

    def run(drop_p, cot_):
        ws = [torch.nn.Parameter(w.clone().to(DEV)) for w in ws0]
        bn = P.hip_nn.BatchNorm2d(cout).to(DEV).train()          # a fresh module: the same running buffers for both calls
        with torch.no_grad():
            bn.weight.copy_(g0.to(DEV))
        opt = T.FlatAdam(ws + list(bn.parameters()), lr=1e-3)
        opt.zero_grad()
        philox.set_offset(1000)
        del called[:]
        y = H.conv_bn_relu_pool(x.to(DEV), ws, None, bn, ph, 1, 1, 1, 1, drop_p=drop_p)
        fwd = list(called)
        kept = None
        if same_call and drop_p > 0:
            kept = [t for t in y.grad_fn.saved_tensors if t.shape == y.shape and t.dtype == torch.float32]
            assert len(kept) == 1
            kept = kept[0].detach().cpu().clone()
        (y * cot_.to(DEV)).sum().backward()
        H.join_side_stream()
        torch.cuda.synchronize()
        return (y.detach().cpu(), [w.grad.detach().cpu().clone() for w in ws], bn.weight.grad.cpu().clone(),
                philox.offset - 1000, bn.running_mean.cpu().clone(), bn.running_var.cpu().clone(), fwd, kept)

    z = run(0.0, cot * f)
    got = run(0.3, cot)
    assert _FIRST_STAGE_ROUTES[hw, route] in got[6], got[6]
    assert z[3] == 0 and got[3] == (cot.numel() + 3) // 4
    assert bool(((z[0] > 0) & (f == 0)).any()) and bool(((z[0] > 0) & (f > 0)).any())
    if same_call:
        _close(z[0], got[7], 1e-6, "undropped output of the two calls")
        assert torch.equal(got[0], got[7] * f)
        _close(got[4], z[4], 1e-6, "running mean"); _close(got[5], z[5], 1e-6, "running var")
    else:
        assert torch.equal(got[0], z[0] * f)
        assert torch.equal(got[4], z[4]) and torch.equal(got[5], z[5])          # dropout does not touch the statistics
    for a, b in zip(got[1], z[1]):
        _close(a, b, 2e-4, "dw")
    _close(got[2], z[2], 1e-5, "dgamma")


# ------------------------------------------------------------------------------------------
# the whole model, Dropout on, against the oracle with the same masks
# ------------------------------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().double().numpy()


def _mask_source(stream):
    """The oracle's draw(shape, p, kind) from the host stream.  The oracle visits the sites in the order model.py draws on
    the device (offsets are handed out at Python call time, side streams do not reorder them): per branch the three CNN
    stages, then the residual blocks' channel masks (one stacked launch = the blocks' consecutive draws when
    N * G % 4 == 0, a draw per block otherwise), branch A before B, then the sed head, then the doa head.  An element
    site draws numel factors in the tensor's contiguous order; a channel site draws N * C rows, broadcast over time."""
    def draw(shape, p, kind):
        n = int(np.prod(shape))
        return torch.from_numpy(stream.draw(n, p)).double().reshape(shape)
    return draw


def _dropout_case(name, **over):
    case = next(c for c in MODEL_CASES if c["name"] == name)
    return dict(case, dropout_perc=0.3, spatial_dropout_rate=0.5, **over)      # as tests/test_gpu_deterministic.py::_case(name, True)


_TRAIN_DROPOUT_CASES = [
    _dropout_case("tiny_DQ"), _dropout_case("tiny_Q"), _dropout_case("tiny_R"), _dropout_case("tiny_2stream"),
    _dropout_case("tiny_Qcls"),                                     # fc_dropout = "all" (and ReLU heads, conv biases)
    # N * G = 3 * 30 = 90 rows, 90 % 4 == 2: the residual blocks draw one by one, each draw ends in a partial group
    dict(_dropout_case("tiny_R", G=30, B=3), name="tiny_R_G30_B3"),
]


@pytest.mark.parametrize("case", _TRAIN_DROPOUT_CASES, ids=lambda c: c["name"])
def test_train_step_with_dropout_matches_oracle(case, philox):
    """Two consecutive training steps (zero_grad, forward, seld_loss_fn, backward, FlatAdam.step) with dropout_perc = 0.3
    and spatial_dropout_rate = 0.5 against the fp64 oracle under torch.optim.Adam, the oracle's masks drawn from the
    host Philox stream in the device's order.  Compared: each step's loss at 2e-4 relative
    (test_six_step_trajectory_matches_oracle); the first step's gradients at the tolerances of
    test_gpu_model.py::test_train_step_matches_reference (per-parameter sum and sum of squares, the case's full
    gradients at 1e-3 of their maximum); the running statistics after both steps (that test's checksum tolerance, and
    1e-3 of the maximum element by element, the module-wide bound of test_gpu_model.py); and the Philox position, which
    must equal the host stream's: step 2 continues the stream.  A wrong or misplaced mask is an error of order 1.

    tiny_R_G30_B3 is the case with N * G % 4 != 0 (the stock tiny models all have N * G = 64): its blocks draw one by
    one, 23 groups for 90 rows each."""
    T, H = pkg().train, _H()
    m = build_model(case)
    fill_weights(m.state_dict().items(), case)
    m = m.to(DEV).train()
    torch.manual_seed(2 ** 33 + 77)                      # after build_model, which seeds for its initialisation
    philox.set_offset(0)
    H.hcq_weights.reset()
    host = R.Stream(torch.initial_seed())
    draw = _mask_source(host)
    sd64 = {k: v.detach().cpu().double().clone() for k, v in m.state_dict().items()}
    names = [n for n, _ in m.named_parameters()]
    leaves = [sd64[n].requires_grad_(True) for n in names]
    cfg = O.SeldConfig(**model_kwargs(case))
    lr = 1e-3
    opt = T.FlatAdam(m.parameters(), lr=lr)
    ropt = torch.optim.Adam(leaves, lr=lr)
    n_sed = int(case["output_classes"] * 3)
    shape = (case["B"], case["input_channels"], case["freq_dim"], case["time_dim"])
    xs = [O.closed_form_input(shape), O.closed_form_input(shape).flip(3) * 0.7]
    tg = [train_target(case), train_target(case).flip(1)]
    params = dict(m.named_parameters())
    rows = case["B"] * case["G"]
    per_step = None
    for step in range(2):
        x, t = xs[step], tg[step]
        opt.zero_grad()
        sed, doa = m(x.to(DEV))
        loss = T.seld_loss_fn(sed, doa, t.to(DEV), n_sed, 1.0, 5.0)
        loss.backward()
        H.join_side_stream()
        torch.cuda.synchronize()
        if step == 0:
            grads = {n: (None if p.grad is None else p.grad.detach().cpu().double().clone()) for n, p in params.items()}
        opt.step()
        ropt.zero_grad()
        stats = {}
        rsed, rdoa = O.seld_forward(sd64, cfg, x.double(), train=True, mode="explicit", stats_out=stats, dropout=draw)
        rloss = O.seld_loss(rsed, rdoa, t.double(), n_sed)
        rloss.backward()
        if step == 0:
            rgrads = {n: (None if l.grad is None else l.grad.detach().clone()) for n, l in zip(names, leaves)}
            per_step = host.offset
        ropt.step()
        with torch.no_grad():
            for k, v in stats.items():
                sd64[k].copy_(v)
        print(f"{case['name']} step {step}: loss {loss.item():.7f} oracle {rloss.item():.7f} "
              f"rel {abs(loss.item() - rloss.item()) / abs(rloss.item()):.2e}; philox {philox.offset} host {host.offset}")
        assert philox.offset == host.offset, (step, philox.offset, host.offset)
        assert abs(loss.item() - rloss.item()) <= 2e-4 * abs(rloss.item()), (step, loss.item(), rloss.item())
    assert per_step > 0 and host.offset == 2 * per_step == philox.get_offset()
    assert (rows % 4 != 0) == (case["name"] == "tiny_R_G30_B3")
    # --- the first step's gradients
    numel = np.array([params[n].numel() for n in names], dtype=np.float64)
    ref_sq = np.array([0.0 if rgrads[n] is None else float((rgrads[n] ** 2).sum()) for n in names])
    ref_rms = np.sqrt(ref_sq / numel)
    floor = 1e-4 * ref_rms.max()
    gtol = case.get("grad_tol", 1e-3) / 1e-3
    worst = [0.0, 0.0]
    for i, n in enumerate(names):
        g, r = grads[n], rgrads[n]
        if r is None:                                # allocated, never used (batch_gate1; the last block's conv2_residual)
            assert g is None or float(g.abs().max()) == 0.0, n
            continue
        assert g is not None, n
        rms = max(ref_rms[i], floor)
        d1 = abs(float((g ** 2).sum()) - ref_sq[i]) / (gtol * 4e-3 * rms * rms * numel[i])
        d0 = abs(float(g.sum()) - float(r.sum())) / (gtol * 2e-3 * rms * numel[i])
        worst = [max(worst[0], d0), max(worst[1], d1)]
        assert d1 <= 1.0 and d0 <= 1.0, (n, d0, d1)
    print(f"{case['name']}: gradient checksums, worst fraction of the tolerance: sum {worst[0]:.3f}, sum of squares {worst[1]:.3f}")
    for n in case.get("full_grads", []):
        ref = _np(rgrads[n])
        scale = max(float(np.abs(ref).max()), 10 * floor)
        err = float(np.abs(_np(grads[n]) - ref).max())
        print(f"{case['name']}: grad {n}: max err {err:.3e} of {scale:.3e}")
        assert err <= gtol * 1e-3 * scale, (n, err, scale)
    # --- the running statistics after two steps
    sd = m.state_dict()
    for k, ref in sd64.items():
        if "running" not in k:
            continue
        got, ref = sd[k].detach().cpu().double(), ref.detach()
        ck_got = np.array([got.sum().item(), (got ** 2).sum().item()])
        ck_ref = np.array([ref.sum().item(), (ref ** 2).sum().item()])
        assert np.allclose(ck_got, ck_ref, rtol=1e-4, atol=1e-6 + 1e-4 * math.sqrt(ck_ref[1])), (k, ck_got, ck_ref)
        assert float((got - ref).abs().max()) <= 1e-3 * max(float(ref.abs().max()), 1e-6), k
