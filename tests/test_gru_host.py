"""Host-side checks of the GRU layer: the fp64 reference of tests/gru_ref.py against torch.nn.GRU, the refusals of the C
calls (pointers that are never dereferenced), the label strings, hip_nn.GRU's state dict, and the refusals and the
untouched defaults of SELD_Model / cli.rnn_from_args.  No device is touched."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from tests import gru_ref as R
from tests.helpers import pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
P = ctypes.c_void_p(4096)       # a non-NULL pointer no refused call may read or write


# ======================================================================================================================
# the reference
# ======================================================================================================================
@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_matches_torch_gru_in_fp64(name):
    """Output, h_n and every gradient, to 1e-12 of the tensor's largest entry; the recurrence alone, fed gx through an
    identity W_ih, gives dgx as well."""
    c = R.make_case(name)
    ref, t64 = R.layer(c), R.torch_gru(c, torch.float64)
    assert {"y", "h_n", "dh0", "dx", "dW_ih0", "dW_hh0"} <= set(t64)
    assert ("db_hh0" in t64) == (R.CASES[name][6])
    for k, v in t64.items():
        assert R.rel_err(v, ref[k]) <= 1e-12, (k, R.rel_err(v, ref[k]))
    rec, i64 = R.recurrence(c), R.torch_gru(c, torch.float64, identity_input=True)
    assert set(i64) == {"y", "h_n", "dh0", "dgx"}
    for k, v in i64.items():
        assert R.rel_err(v, rec[k]) <= 1e-12, (k, R.rel_err(v, rec[k]))


def test_case_list():
    assert [v[:5] for v in R.CASES.values()] == [(1, 1, 8, 16, 1), (3, 37, 24, 32, 2), (3, 37, 24, 32, 2), (17, 33, 40, 48, 2),
                                                 (2, 9, 8, 20, 2), (2, 64, 128, 128, 2), (2, 600, 16, 16, 1)]
    c = R.make_case("H_padded")
    assert c["x"].dtype == torch.float64 and torch.equal(c["x"], c["x"].float().double())
    assert float(c["params"][0][1].abs().max()) <= 1 / 20 ** 0.5
    assert torch.equal(R.make_case("H_padded")["gx32"], c["gx32"])


# ======================================================================================================================
# the C calls
# ======================================================================================================================
def _fwd(lib, dirs=2, B=3, T=5, H=32, gx=P, wpack=P, y=P, h_n=P, saved=P, n=None):
    n = 5 * dirs * B * T * H if n is None else n
    return lib.seld_gru_fwd(dirs, B, T, H, gx, wpack, None, y, h_n, saved, n, None)


def _bwd(lib, dirs=2, B=3, T=5, H=32, dy=P, wpack=P, saved=P, dgx=P, dgh=P, n=None):
    n = 5 * dirs * B * T * H if n is None else n
    return lib.seld_gru_bwd(dirs, B, T, H, dy, None, wpack, saved, n, dgx, dgh, None, None)


def test_the_calls_refuse_before_anything_is_read():
    lib = pkg()._lib.lib()
    for call in (_fwd, _bwd):
        for bad in (dict(dirs=3), dict(dirs=0), dict(B=0), dict(T=0), dict(H=0), dict(wpack=None)):
            assert call(lib, **bad) == EINVAL, (call.__name__, bad)
        assert call(lib, H=129) == EUNSUPPORTED
        assert call(lib, B=1 << 20, T=1 << 10, H=16) == EUNSUPPORTED        # 2^31 elements and more
        assert call(lib, n=5 * 2 * 3 * 5 * 32 - 1) == EWORKSPACE
    for bad in (dict(gx=None), dict(y=None), dict(h_n=None)):
        assert _fwd(lib, **bad) == EINVAL, bad
    for bad in (dict(dy=None), dict(saved=None), dict(dgx=None), dict(dgh=None)):
        assert _bwd(lib, **bad) == EINVAL, bad
    pack = lambda dirs, H, w0=P, w1=P, b0=None, b1=None, out=P: lib.seld_gru_pack(dirs, H, w0, w1, b0, b1, out, None)
    assert pack(3, 16) == EINVAL and pack(2, 0) == EINVAL and pack(2, 16, w1=None) == EINVAL and pack(1, 16, out=None) == EINVAL
    assert pack(2, 16, b0=P) == EINVAL and pack(2, 129) == EUNSUPPORTED
    assert lib.seld_gru_saved_floats(2, 3, 37, 32) == 5 * 2 * 3 * 37 * 32
    assert lib.seld_gru_saved_floats(3, 3, 37, 32) == 0 and lib.seld_gru_saved_floats(2, 3, 37, 129) == 0
    # both weight forms and the bias, padded to 32 hidden units
    assert lib.seld_gru_pack_floats(2, 20) == 2 * (2 * 3 * 32 * 32 + 3 * 32) and lib.seld_gru_pack_floats(1, 129) == 0


def test_kernel_labels():
    H = pkg().hip_ops
    lib = pkg()._lib.lib()
    assert H.gru_kernel_label(H.GRU_FWD, 128) == "gru_fwd_kernel<8>"
    assert H.gru_kernel_label(H.GRU_BWD, 128) == "gru_bwd_kernel<8>"
    assert H.gru_kernel_label(H.GRU_FWD, 20) == "gru_fwd_kernel<2>" and H.gru_kernel_label(H.GRU_BWD, 1) == "gru_bwd_kernel<1>"
    buf = ctypes.create_string_buffer(64)
    assert lib.seld_gru_kernel_label(2, 16, buf, 64) == EINVAL and lib.seld_gru_kernel_label(0, 16, buf, 8) == EINVAL
    assert lib.seld_gru_kernel_label(0, 16, None, 64) == EINVAL and lib.seld_gru_kernel_label(0, 0, buf, 64) == EINVAL
    assert lib.seld_gru_kernel_label(1, 129, buf, 64) == EUNSUPPORTED
    assert H.GRU_MAX_HIDDEN == 128 == pkg().model.RNN_MAX_SIZE


# ======================================================================================================================
# the layer
# ======================================================================================================================
@pytest.mark.parametrize("kw", [dict(), dict(num_layers=2, bidirectional=True), dict(bias=False, batch_first=True),
                                dict(num_layers=3, bidirectional=True, dropout=0.25, batch_first=True)])
def test_module_has_torchs_state_dict(kw):
    hnn = pkg().hip_nn
    torch.manual_seed(7)
    ours = hnn.GRU(12, 20, **kw)
    torch.manual_seed(7)
    theirs = torch.nn.GRU(12, 20, **kw)
    a, b = ours.state_dict(), theirs.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k        # the same draws, too
    torch.manual_seed(8)
    other = torch.nn.GRU(12, 20, **kw)
    ours.load_state_dict(other.state_dict())
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in ours.state_dict().items())
    assert isinstance(ours, torch.nn.GRU) and (ours.batch_first, ours.dropout) == (theirs.batch_first, theirs.dropout)


def test_module_refusals():
    hnn = pkg().hip_nn
    with pytest.raises(ValueError, match="hidden_size 129"):
        hnn.GRU(8, 129)
    hnn.GRU(8, 128)
    m = hnn.GRU(4, 8)
    packed = torch.nn.utils.rnn.pack_padded_sequence(torch.zeros(3, 2, 4), [3, 2])
    with pytest.raises(ValueError, match="PackedSequence"):
        m(packed)
    with pytest.raises(pkg()._lib.SeldHipError):       # no CPU path
        m(torch.zeros(3, 2, 4))


# ======================================================================================================================
# the model and the flags
# ======================================================================================================================
KW = dict(time_dim=64, freq_dim=128, input_channels=8, output_classes=14, domain='DQ', domain_classifier='DQ',
          cnn_filters=[16, 16, 16], pool_size=[[8, 2], [8, 2], [2, 2]], D=[3], G=32, U=16, V=[16, 16], fc_layers=[16])


def _model(**kw):
    np.random.seed(1)
    torch.manual_seed(1)
    return pkg().model.SELD_Model(**dict(KW, **kw))


@pytest.mark.parametrize("bad, match", [
    (dict(pool_time='TCN'), "pool_time='CNN'"), (dict(rnn_size=129), "rnn_size"), (dict(rnn_size=0), "rnn_size"),
    (dict(rnn_size=True), "rnn_size"), (dict(rnn_layers=0), "rnn_layers"), (dict(rnn_layers=1.5), "rnn_layers"),
    (dict(se_mode='tcn'), "se_mode"), (dict(at_key_size=8), "at_key_size"), (dict(use_tcn="no"), "use_tcn")])
def test_model_refusals(bad, match):
    with pytest.raises(ValueError, match=match):
        _model(**dict(dict(use_tcn=False, pool_time='CNN'), **bad))
    M = pkg().model
    if "use_tcn" not in bad:
        with pytest.raises(ValueError, match=match):
            M.ConvTC_Block(64, 128, 8, cnn_filters=[16, 16, 16], **dict(dict(use_tcn=False, pool_time='CNN'), **bad))


def test_defaults_build_the_model_they_always_built():
    """No rnn key, and under fixed seeds the weights of a model built without the new arguments; the rnn arguments are not
    read with use_tcn=True."""
    a = _model(pool_time='TCN')
    b = _model(pool_time='TCN', use_tcn=True, rnn_size=1000, rnn_layers=0)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and not any("rnn" in k for k in sa) and any(".tcn." in k for k in sa)
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert a.model_name == b.model_name == "DualQSELD-TCN-PHI-S1_BN_RF9_3RB"


def test_recurrent_model_layout():
    m = _model(use_tcn=False, pool_time='CNN', rnn_size=32, rnn_layers=2)
    keys = list(m.state_dict())
    assert not any(".tcn." in k for k in keys)
    rnn = [k for k in keys if ".rnn." in k]
    assert len(rnn) == 16 and rnn[0] == "seld_block.rnn.weight_ih_l0" and rnn[-1] == "seld_block.rnn.bias_hh_l1_reverse"
    assert isinstance(m.seld_block.rnn, pkg().hip_nn.GRU) and m.seld_block.rnn.batch_first and m.seld_block.rnn.bidirectional
    assert m.seld_block.rnn.input_size == 16 and m.seld_block.rnn.hidden_size == 32
    assert m.sed[0].in_features == 64 // 8          # the dual-quaternion head counts per component
    assert m.model_name == "DualQSELDnet-GRU2x32_BN_pooltCNN"
    two = _model(use_tcn=False, pool_time='CNN', rnn_size=16, rnn_layers=1, input_channels=16, parallel_ConvTC_block='2Parallel')
    assert two.sed[0].in_features == 64 // 8 and two.model_name == "DualQSELDnet-GRU1x16_2Parallel_BN_pooltCNN"
    assert "branch_A.rnn.weight_hh_l0_reverse" in two.state_dict()
    q = _model(use_tcn=False, pool_time='CNN', domain='Q', domain_classifier='R', rnn_size=8, rnn_layers=3)
    assert q.model_name.startswith("QSELDnet-GRU3x8_") and q.sed[0].in_features == 16


def test_rnn_from_args():
    cli = pkg().cli
    ns = lambda **kw: argparse.Namespace(**kw)
    assert cli.rnn_from_args(ns()) == dict(use_tcn=True, rnn_size=128, rnn_layers=2)
    assert cli.rnn_from_args(ns(use_tcn=True, pool_time='TCN', rnn_size=999)) == dict(use_tcn=True, rnn_size=999, rnn_layers=2)
    ok = ns(use_tcn=False, pool_time='CNN', rnn_size=64, rnn_layers=1, se_mode='cnn', at_key_size=0)
    assert cli.rnn_from_args(ok) == dict(use_tcn=False, rnn_size=64, rnn_layers=1)
    for bad, match in ((dict(pool_time='TCN'), "--use_tcn=False needs pool_time"), (dict(rnn_size=129), "--rnn_size"),
                       (dict(rnn_layers=0), "--rnn_layers"), (dict(se_mode='tcn'), "--se_mode"), (dict(at_key_size=4), "--at_key_size")):
        with pytest.raises(ValueError, match=match):
            cli.rnn_from_args(ns(**dict(vars(ok), **bad)))
    args = cli.parse_args(["--TextArgs=none", "--use_tcn=False", "--pool_time=CNN", "--rnn_size=48", "--rnn_layers=3"])
    assert cli.rnn_from_args(args) == dict(use_tcn=False, rnn_size=48, rnn_layers=3)
    assert cli.parse_args(["--TextArgs=none"]).rnn_size == 128
    with pytest.raises(ValueError, match="pool_time"):      # train.main refuses before the device is touched
        pkg().train.main(cli.parse_args(["--TextArgs=none", "--use_tcn=False", "--pool_time=TCN", "--use_cuda=False"]))


def test_benchmark_config_builds_the_recurrent_model():
    import os
    cli = pkg().cli
    path = os.path.join(os.path.dirname(cli.__file__), "config", "BENCH_c6_DQSELDnet-GRU_8ch_F128.txt")
    args = cli.parse_args(["--TextArgs", path])
    assert cli.rnn_from_args(args) == dict(use_tcn=False, rnn_size=128, rnn_layers=2) and args.pool_time == "CNN"
    c3 = cli.parse_args(["--TextArgs", path.replace("c6_DQSELDnet-GRU", "c3_DQSELD-TCN")])
    differ = {k for k in vars(args) if getattr(args, k) != getattr(c3, k)}
    assert differ == {"TextArgs", "use_tcn", "pool_time", "architecture"}
