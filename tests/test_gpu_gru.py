"""The GRU kernels (csrc/gru.hip), hip_ops.gru, hip_nn.GRU and the recurrent back end of SELD_Model (use_tcn=False) on the
device, against tests/gru_ref.py in fp64.

Bound of every fp64 comparison of a layer: torch.nn.GRU runs in fp32 on the CPU on the same inputs, its error against the
same fp64 reference is e32, and the kernel's error must stay within max(16 * e32, 2e-6) per tensor, errors taken as the
largest difference relative to the reference tensor's largest entry.  The factor 16 covers another summation order (MFMA
k-chunks of 4, products folded in splits) and __expf / rcp gates against libm; the floor only keeps a lucky e32 from
making the bound meaningless.  err / bound is printed per tensor."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import gru_ref as R
from tests.golden.cases import MODEL_CASES, model_kwargs, train_target
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1234.5
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
CASE = {c["name"]: c for c in MODEL_CASES}
NAMES = list(R.CASES)


# ======================================================================================================================
# plumbing
# ======================================================================================================================
@functools.lru_cache(maxsize=None)
def _case(name):
    """The case, its fp64 results and torch's fp32 errors, computed once and never modified."""
    c = R.make_case(name)
    ref_layer, ref_rec = R.layer(c), R.recurrence(c)
    t32, t32_rec = R.torch_gru(c, torch.float32), R.torch_gru(c, torch.float32, identity_input=True)
    e32 = {k: R.rel_err(v, ref_layer[k]) for k, v in t32.items()}
    e32_rec = {k: R.rel_err(v, ref_rec[k]) for k, v in t32_rec.items()}
    e32_rec["dgh"] = e32_rec["dgx"]         # dgx with the n part times r <= 1: torch has no such tensor
    return c, ref_layer, ref_rec, e32, e32_rec


def _bound(e32):
    return max(16.0 * e32, 2e-6)


def _dev(t):
    return None if t is None else t.float().contiguous().to(DEV)


def _out(*shape):
    """An output tensor holding NaN with sentinel floats around it: (view, whole buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 16,), SENTINEL)
    buf[8:8 + n] = float("nan")
    buf = buf.to(DEV)
    return buf[8:8 + n].view(*shape), buf


def _intact(buf):
    b = buf.cpu()
    return bool((b[:8] == SENTINEL).all() and (b[-8:] == SENTINEL).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pack(params, H):
    L = pkg()._lib
    lib = L.lib()
    dirs = len(params)
    ws = [_dev(p[1]) for p in params]
    bs = [_dev(p[3]) for p in params]
    wpack = torch.empty(int(lib.seld_gru_pack_floats(dirs, H)), device=DEV)
    L.check(lib.seld_gru_pack(dirs, H, L.ptr(ws[0]), L.ptr(ws[-1] if dirs == 2 else None), L.ptr(bs[0]),
                              L.ptr(bs[-1] if dirs == 2 else None), L.ptr(wpack), L.current_stream()), "seld_gru_pack")
    return wpack


def _recurrence(gx, params, h0, dy, dh_n):
    """seld_gru_fwd + seld_gru_bwd on float64 / float32 host tensors: outputs (device) and their sentinel buffers."""
    L = pkg()._lib
    lib = L.lib()
    dirs, B, T, G = gx.shape
    H = G // 3
    wpack = _pack(params, H)
    gx, h0, dy, dh_n = _dev(gx), _dev(h0), _dev(dy), _dev(dh_n)
    out, bufs = {}, {}
    for k, shape in (("y", (B, T, dirs * H)), ("h_n", (dirs, B, H)), ("dgx", (dirs, B, T, G)), ("dgh", (dirs, B, T, G)),
                     ("dh0", (dirs, B, H))):
        out[k], bufs[k] = _out(*shape)
    n = int(lib.seld_gru_saved_floats(dirs, B, T, H))
    assert n == 5 * dirs * B * T * H
    saved, bufs["saved"] = _out(n)
    st = L.current_stream()
    L.check(lib.seld_gru_fwd(dirs, B, T, H, L.ptr(gx), L.ptr(wpack), L.ptr(h0), L.ptr(out["y"]), L.ptr(out["h_n"]),
                             L.ptr(saved), n, st), "seld_gru_fwd")
    L.check(lib.seld_gru_bwd(dirs, B, T, H, L.ptr(dy), L.ptr(dh_n), L.ptr(wpack), L.ptr(saved), n, L.ptr(out["dgx"]),
                             L.ptr(out["dgh"]), L.ptr(out["dh0"]), st), "seld_gru_bwd")
    torch.cuda.synchronize()
    out["saved"] = saved
    return out, bufs


def _layer(c):
    """hip_ops.gru (one layer) forward and backward of sum(y dy) + sum(h_n dh_n): the dict of gru_ref.layer, without dgx."""
    H = pkg().hip_ops
    leaf = lambda t: None if t is None else _dev(t).requires_grad_(True)
    x, h0 = leaf(c["x"]), leaf(c["h0"])
    params = [tuple(leaf(p) for p in group) for group in c["params"]]
    y, h_n = H.gru(x, [params], c["H"], 1, c["dirs"], h0)
    ((y * _dev(c["dy"])).sum() + (h_n * _dev(c["dh_n"])).sum()).backward()
    torch.cuda.synchronize()
    out = dict(y=y.detach(), h_n=h_n.detach(), dx=x.grad)
    if h0 is not None:
        out["dh0"] = h0.grad
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(params):
        out[f"dW_ih{d}"], out[f"dW_hh{d}"] = w_ih.grad, w_hh.grad
        if b_ih is not None:
            out[f"db_ih{d}"], out[f"db_hh{d}"] = b_ih.grad, b_hh.grad
    return out


def _hold(got, ref, e32, what):
    worst = 0.0
    for k, v in got.items():
        err, bound = R.rel_err(v, ref[k]), _bound(e32[k])
        print(f"{what} {k}: err {err:.3e} e32 {e32[k]:.3e} err/bound {err / bound:.3f}")
        worst = max(worst, err / bound)
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
        assert R.rel_err(v, ref[k]) <= _bound(e32[k]), (what, k, R.rel_err(v, ref[k]), _bound(e32[k]))
    return worst


# ======================================================================================================================
# the kernels and hip_ops.gru against fp64
# ======================================================================================================================
@pytest.mark.parametrize("name", NAMES)
def test_recurrence_matches_fp64(name):
    """seld_gru_fwd / seld_gru_bwd from gx rounded to fp32: y, h_n, dgx, dgh, dh0; the sentinels around every output and
    around the saved tensors are intact."""
    c, _, ref, _, e32 = _case(name)
    out, bufs = _recurrence(c["gx32"], c["params"], c["h0"], c["dy"], c["dh_n"])
    for k, b in bufs.items():
        assert _intact(b), k
    saved = out.pop("saved")
    assert torch.isfinite(saved).all()
    _hold(out, ref, e32, f"recurrence {name}")


@pytest.mark.parametrize("name", NAMES)
def test_layer_matches_fp64(name):
    """hip_ops.gru, one layer, through autograd: y, h_n, dh0, dx, dW_ih, dW_hh, db_ih, db_hh of every direction."""
    c, ref, _, e32, _ = _case(name)
    got = _layer(c)
    assert {"y", "h_n", "dx", "dW_ih0", "dW_hh0"} <= set(got)
    _hold(got, ref, e32, f"layer {name}")


# ======================================================================================================================
# exact properties
# ======================================================================================================================
def test_backward_direction_is_the_forward_one_on_flipped_time():
    """Both directions with the same weights, direction 1 fed the time-flipped gx and dy of direction 0: its y and dgx are
    direction 0's, flipped back, bit for bit."""
    c = _case("odd_T_masked_columns")[0]
    H = c["H"]
    params = [c["params"][0], c["params"][0]]
    gx = torch.stack((c["gx32"][0], c["gx32"][0].flip(1)))
    h0 = torch.stack((c["h0"][0], c["h0"][0]))
    dh_n = torch.stack((c["dh_n"][0], c["dh_n"][0]))
    dy = torch.cat((c["dy"][:, :, :H], c["dy"][:, :, :H].flip(1)), 2)
    out, _ = _recurrence(gx, params, h0, dy, dh_n)
    assert torch.equal(_bits(out["y"][:, :, H:]), _bits(out["y"][:, :, :H].flip(1)))
    assert torch.equal(_bits(out["dgx"][1]), _bits(out["dgx"][0].flip(1)))
    assert torch.equal(_bits(out["h_n"][1]), _bits(out["h_n"][0])) and torch.equal(_bits(out["dh0"][1]), _bits(out["dh0"][0]))


def test_a_sample_alone_gives_the_bits_it_gives_in_the_batch():
    """Samples 0 (column 0 of the first tile) and 16 (the one live column of the second tile) of the batch of 17, each run
    alone: the same bits."""
    c = _case("second_tile_no_bias")[0]
    H = c["H"]
    full, _ = _recurrence(c["gx32"], c["params"], c["h0"], c["dy"], c["dh_n"])
    for b in (0, 16):
        one, _ = _recurrence(c["gx32"][:, b:b + 1], c["params"], c["h0"][:, b:b + 1], c["dy"][b:b + 1], c["dh_n"][:, b:b + 1])
        assert torch.equal(_bits(one["y"]), _bits(full["y"][b:b + 1])), b
        for k in ("h_n", "dgx", "dgh", "dh0"):
            assert torch.equal(_bits(one[k]), _bits(full[k][:, b:b + 1])), (b, k)


@pytest.mark.parametrize("name", ["second_tile_no_bias", "largest_resident"])
def test_two_calls_give_the_same_bits(name):
    c = _case(name)[0]
    a, _ = _recurrence(c["gx32"], c["params"], c["h0"], c["dy"], c["dh_n"])
    b, _ = _recurrence(c["gx32"], c["params"], c["h0"], c["dy"], c["dh_n"])
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    la, lb = _layer(c), _layer(c)
    for k in la:
        assert torch.equal(_bits(la[k]), _bits(lb[k])), k


def test_a_refused_call_writes_nothing():
    L = pkg()._lib
    lib = L.lib()
    dirs, B, T, H = 2, 3, 5, 32
    wpack = torch.zeros(int(lib.seld_gru_pack_floats(dirs, H)), device=DEV)
    gx = torch.zeros(dirs, B, T, 3 * H, device=DEV)
    n = int(lib.seld_gru_saved_floats(dirs, B, T, H))
    outs = {k: _out(*s) for k, s in (("y", (B, T, dirs * H)), ("h_n", (dirs, B, H)), ("saved", (n,)),
                                     ("dgx", (dirs, B, T, 3 * H)), ("dgh", (dirs, B, T, 3 * H)), ("dh0", (dirs, B, H)))}
    before = {k: b.clone() for k, (_, b) in outs.items()}
    p = {k: L.ptr(v) for k, (v, _) in outs.items()}
    st = L.current_stream()
    fwd = lambda dirs_, H_, n_: lib.seld_gru_fwd(dirs_, B, T, H_, L.ptr(gx), L.ptr(wpack), None, p["y"], p["h_n"], p["saved"], n_, st)
    bwd = lambda dirs_, H_, n_: lib.seld_gru_bwd(dirs_, B, T, H_, L.ptr(gx), None, L.ptr(wpack), p["saved"], n_, p["dgx"],
                                                 p["dgh"], p["dh0"], st)
    for call in (fwd, bwd):
        assert call(3, H, n) == EINVAL
        assert call(dirs, 129, n) == EUNSUPPORTED
        assert call(dirs, H, n - 1) == EWORKSPACE
    assert lib.seld_gru_fwd(dirs, B, T, H, None, L.ptr(wpack), None, p["y"], p["h_n"], p["saved"], n, st) == EINVAL
    assert lib.seld_gru_pack(dirs, 129, L.ptr(gx), L.ptr(gx), None, None, p["saved"], st) == EUNSUPPORTED
    torch.cuda.synchronize()
    for k, (_, b) in outs.items():
        assert torch.equal(_bits(b), _bits(before[k])), k


# ======================================================================================================================
# hip_nn.GRU
# ======================================================================================================================
def _stack_inputs(batch_first, seed=11):
    g = torch.Generator().manual_seed(seed)
    B, T, I, H = 5, 19, 12, 24
    x = torch.randn((B, T, I) if batch_first else (T, B, I), generator=g)
    h0 = 0.5 * torch.randn(4, B, H, generator=g)
    dy = torch.randn((B, T, 2 * H) if batch_first else (T, B, 2 * H), generator=g)
    dh = torch.randn(4, B, H, generator=g)
    return x, h0, dy, dh, I, H


def _torch_stack(sd, batch_first, dtype, x, h0, dy, dh, I, H):
    m = torch.nn.GRU(I, H, 2, batch_first=batch_first, bidirectional=True).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    x, h0 = x.to(dtype).clone().requires_grad_(True), h0.to(dtype).clone().requires_grad_(True)
    y, h_n = m(x, h0)
    ((y * dy.to(dtype)).sum() + (h_n * dh.to(dtype)).sum()).backward()
    return dict(y=y.detach(), h_n=h_n.detach(), dx=x.grad, dh0=h0.grad, **{k: p.grad for k, p in m.named_parameters()})


@pytest.mark.parametrize("batch_first", [True, False], ids=["batch_first", "time_first"])
def test_two_layer_bidirectional_module_matches_torch_fp64(batch_first):
    """hip_nn.GRU(12, 24, 2 layers, both directions) against torch.nn.GRU in fp64 with the bound above, (y, h_n) and every
    gradient; under FlatAdam the gradients are in the optimiser's flat buffer."""
    P = pkg()
    x, h0, dy, dh, I, H = _stack_inputs(batch_first)
    torch.manual_seed(3)
    m = P.hip_nn.GRU(I, H, 2, batch_first=batch_first, bidirectional=True)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ref = _torch_stack(sd, batch_first, torch.float64, x, h0, dy, dh, I, H)
    t32 = _torch_stack(sd, batch_first, torch.float32, x, h0, dy, dh, I, H)
    e32 = {k: R.rel_err(v, ref[k]) for k, v in t32.items()}
    m = m.to(DEV)
    opt = P.train.FlatAdam(m.parameters(), lr=1e-3)
    opt.zero_grad()
    xd, hd = x.to(DEV).requires_grad_(True), h0.to(DEV).requires_grad_(True)
    y, h_n = m(xd, hd)
    assert y.shape == dy.shape and h_n.shape == (4, x.shape[0 if batch_first else 1], H)
    ((y * dy.to(DEV)).sum() + (h_n * dh.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    got = dict(y=y.detach(), h_n=h_n.detach(), dx=xd.grad, dh0=hd.grad, **{k: p.grad for k, p in m.named_parameters()})
    _hold(got, ref, e32, f"module batch_first={batch_first}")
    lo, hi = opt.flat_grad.data_ptr(), opt.flat_grad.data_ptr() + 4 * opt.flat_grad.numel()
    for k, p in m.named_parameters():
        assert lo <= p.grad.data_ptr() < hi, k
    at = 0
    for k, p in m.named_parameters():       # the flat buffer itself holds them, in registration order
        assert R.rel_err(opt.flat_grad[at:at + p.numel()].view(p.shape), ref[k]) <= _bound(e32[k]), k
        at += p.numel()


def test_dropout_between_the_layers():
    """dropout=0.5: eval mode equals dropout=0 bit for bit; in training the tensor between the layers (seen through a hook
    on the project's dropout op) keeps about half its entries, each scaled by 1 / (1 - p) = 2 exactly, and the last
    layer's output is not dropped."""
    P = pkg()
    H = P.hip_ops
    x, h0, _, _, I, Hd = _stack_inputs(True, seed=12)
    torch.manual_seed(4)
    m0 = P.hip_nn.GRU(I, Hd, 2, batch_first=True, bidirectional=True, dropout=0.0).to(DEV)
    m5 = P.hip_nn.GRU(I, Hd, 2, batch_first=True, bidirectional=True, dropout=0.5).to(DEV)
    m5.load_state_dict(m0.state_dict())
    xd = x.to(DEV)
    with torch.no_grad():
        y0 = m0.eval()(xd)[0]
        assert torch.equal(_bits(m5.eval()(xd)[0]), _bits(y0))
    seen = []
    inner = H.DropoutFn.apply

    class Spy:
        @staticmethod
        def apply(t, p):
            out = inner(t, p)
            seen.append((t.detach().clone(), out.detach().clone(), p))
            return out
    H.philox.set_offset(0)
    real = H.norm_act.DropoutFn
    H.norm_act.DropoutFn = Spy
    try:
        with torch.no_grad():
            y5 = m5.train()(xd)[0]
    finally:
        H.norm_act.DropoutFn = real
    torch.cuda.synchronize()
    assert len(seen) == 1 and seen[0][2] == 0.5
    before, after, _ = seen[0]
    assert before.shape == (x.shape[0], x.shape[1], 2 * Hd)
    kept = after != 0
    assert torch.equal(_bits(after[kept]), _bits(2.0 * before[kept]))
    n = before.numel()
    share = float(kept.float().mean())
    assert abs(share - 0.5) <= 5.0 * 0.5 / n ** 0.5, share      # five standard deviations of a fair coin over n draws
    assert not torch.equal(_bits(y5), _bits(y0)) and float((y5 == 0).float().mean()) < 0.01


# ======================================================================================================================
# the model
# ======================================================================================================================
RNN_KW = dict(use_tcn=False, pool_time="CNN", rnn_size=32, rnn_layers=2)


def _forward_fp64(sd, cfg, x):
    """SELD_Model(use_tcn=False).forward in fp64: the oracle's CNN stages and heads around gru_ref's recurrence (plain
    torch operations, so autograd gives the reference gradients)."""
    import torch.nn.functional as F
    from oracle import seld_oracle as O
    p = "seld_block"
    for i, pool in enumerate(cfg.pool_size[:len(cfg.cnn_filters)]):
        x = O._conv_layer(sd, f"{p}.cnn.{i}.0", cfg.algebra, x, 1, 1, 1, "explicit")
        x = O._bn(sd, f"{p}.cnn.{i}.1", x, True, None)
        x = F.max_pool2d(torch.relu(x), [pool[0], pool[1]])
    B = x.shape[0]
    x = x.permute(0, 3, 1, 2).reshape(B, x.shape[3], -1)        # (B, T', C F')
    for layer in range(RNN_KW["rnn_layers"]):
        params = [tuple(sd[f"{p}.rnn.{n}_l{layer}{sfx}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                  for sfx in ("", "_reverse")]
        x = R.recurrence_forward(R.input_gates(x, params), params, None)[0]
    return torch.sigmoid(O._head(sd, "sed", cfg, x, "explicit")), torch.tanh(O._head(sd, "doa", cfg, x, "explicit"))


@pytest.mark.parametrize("name", ["tiny_DQ", "tiny_Q"])
def test_model_with_gru_back_end_matches_fp64(name, seld_env):
    """Forward and one backward of the tiny models with use_tcn=False, pool_time='CNN', rnn_size=32, rnn_layers=2 (closed-form
    weights in the CNN and the heads, the GRU's own initialisation) against the same walk in fp64, the way and with the
    tolerance of tests/test_gpu_squeeze_excite.py::test_model_with_se_matches_fp64: 1e-3 on the outputs, every gradient to
    1e-3 of its largest entry with that test's floor."""
    seld_env.set("SELD_DETERMINISTIC", "1")
    from oracle import seld_oracle as O
    P = pkg()
    H = P.hip_ops
    case = CASE[name]
    x = O.closed_form_input((case["B"], case["input_channels"], case["freq_dim"], case["time_dim"]))
    target = train_target(case)
    np.random.seed(1)
    torch.manual_seed(1)
    m = P.model.SELD_Model(**dict(model_kwargs(case), **RNN_KW))
    assert m.model_name.startswith({"tiny_DQ": "DualQ", "tiny_Q": "Q"}[name] + "SELDnet-GRU2x32_BN_pooltCNN")
    O.closed_form_fill_([(k, v) for k, v in m.state_dict().items() if ".rnn." not in k])
    sd64 = {k: v.detach().double().clone() for k, v in m.state_dict().items()}
    for v in sd64.values():
        v.requires_grad_(v.is_floating_point())
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    m = m.to(DEV).train()
    opt = P.train.FlatAdam(m.parameters(), lr=1e-4)
    opt.zero_grad()
    sed, doa = m(x.to(DEV))
    loss = P.train.seld_loss_fn(sed, doa, target.to(DEV), 42, 1.0, 5.0)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters()}
    cfg = O.SeldConfig(**dict(model_kwargs(case), pool_time="CNN"))
    rsed, rdoa = _forward_fp64(sd64, cfg, x.double())
    assert rsed.shape == sed.shape and rdoa.shape == doa.shape
    O.seld_loss(rsed, rdoa, target.double(), 42).backward()
    err = max(float((sed.detach().cpu().double() - rsed.detach()).abs().max()),
              float((doa.detach().cpu().double() - rdoa.detach()).abs().max()))
    print("GRU model", name, "max |out - fp64|", err)
    assert err <= 1e-3
    rms = [float(v.grad.pow(2).mean().sqrt()) for v in sd64.values() if v.grad is not None]
    floor = 1e-4 * max(rms)
    worst = 0.0
    assert any(".rnn." in k for k in grads)
    for k, gr in grads.items():
        ref = sd64[k].grad
        assert ref is not None, k
        rel = float((gr.cpu().double() - ref).abs().max()) / max(float(ref.abs().max()), 10 * floor)
        worst = max(worst, rel)
        assert rel <= 1e-3, (k, rel)
    print("GRU model", name, "worst gradient", worst)


TRAIN_FLAGS = dict(use_cuda="True", gpu_id=0, patience=1, test_step=0, checkpoint_step=0, num_frames=8,
                   dataset_normalization="UnitNorm", n_mics=2, domain="DQ", domain_classifier="DQ", phase="False",
                   input_channels=8, time_dim=64, freq_dim=128, output_classes=14, class_overlaps=3,
                   cnn_filters="[16, 16, 16]", pool_size="[[8, 2], [8, 2], [2, 2]]", pool_time="CNN", D="[10]",
                   dilation_mode="fibonacci", G=32, U=16, V="[16, 16]", V_kernel_size=3, fc_layers="[16]",
                   fc_activations="linear", fc_dropout="Last", use_bias_conv="False", use_bias_linear="True", batch_norm="BN",
                   dropout_perc=0.0, spatial_dropout_rate=0.0, lr=1e-3, use_lr_scheduler="False", min_lr=1e-6, TextArgs="none",
                   use_tcn="False", rnn_size=32, rnn_layers=2, batch_size=2, epochs=2, min_n_epochs=2)


def _train_main(paths, out, **extra):
    T, H = pkg().train, pkg().hip_ops
    H.philox.set_offset(0)
    H.hcq_weights.reset()
    flags = dict(TRAIN_FLAGS, **paths, results_path=os.path.join(out, "res"), checkpoint_dir=os.path.join(out, "ck"), **extra)
    history = []
    state = T.main(T.parse_args([f"--{k}={v}" for k, v in flags.items()]), history=history)
    torch.cuda.synchronize()
    assert state["epochs"] == 2 and state["step"] == 4
    ck_root = os.path.join(out, "ck")
    assert "SELDnet-GRU2x32" in os.listdir(ck_root)[0]
    path = os.path.join(ck_root, os.listdir(ck_root)[0], "checkpoint")
    return history, torch.load(path, map_location="cpu", weights_only=False), path


def test_train_main_eager_and_recorded_steps_agree_and_the_checkpoint_round_trips(seld_env, tmp_path):
    """train.main on 4 synthetic pickled samples (tests/test_gpu_train_loader.py's), batch 2, 2 epochs = 4 full steps of the
    tiny DQ model with the GRU back end: eager against --resident_loader=True --graph_step=True.  Every loss is finite, the
    weights are bit-identical, and the checkpoint loads into a fresh model and optimiser with every tensor equal."""
    from tests.test_gpu_train_loader import write_pickles
    seld_env.set("SELD_DETERMINISTIC", "1")
    P = pkg()
    paths = write_pickles(tmp_path, 4)
    h_e, ck_e, _ = _train_main(paths, str(tmp_path / "eager"))
    h_g, ck_g, path = _train_main(paths, str(tmp_path / "graph"), resident_loader="True", graph_step="True")
    for h in (h_e, h_g):
        assert len(h) == 2 and all(np.isfinite(v) for row in h for v in row[1:]), h
    a, b = ck_e["model_state_dict"], ck_g["model_state_dict"]
    assert a.keys() == b.keys() and any(".rnn." in k for k in a)
    diff = {k: float((a[k].double() - b[k].double()).abs().max()) for k in a if not torch.equal(a[k], b[k])}
    print("eager vs recorded, tensors that differ:", diff)
    assert not diff
    args = P.train.parse_args([f"--{k}={v}" for k, v in dict(TRAIN_FLAGS, **paths).items()])
    m = P.cli.model_from_args(args).to(DEV)
    opt = P.train.FlatAdam(m.parameters(), lr=1e-3)
    P.checkpoint.load_model(m, opt, path, True, torch.device(DEV))
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), b[k]), k
    assert opt.step_count == 4
