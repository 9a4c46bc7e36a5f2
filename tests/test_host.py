"""CPU-only checks: the C ABI library exports what include/seld_hip.h declares, the host-side mirror has the
reference's state-dict layout and initialisation, config handling, and the product path refuses to run
without the HIP device (no fallback)."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from tests.golden.cases import MODEL_CASES, model_kwargs
from tests.helpers import PKG, build_model, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    lib_path = os.path.join(ROOT, PKG, "csrc", "libseld_hip.so")
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(lib_path)
    header = open(os.path.join(ROOT, "include", "seld_hip.h")).read()
    names = sorted(set(re.findall(r"\b(seld_\w+)\s*\(", header)))
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    lib.seld_build_arch.restype = ctypes.c_char_p
    assert lib.seld_build_arch() == b"gfx950"
    assert lib.seld_abi_version() >= 1


def _declared():
    """[(name, parameter count)] of every seld_* prototype in the header, counted independently of the binding's parser."""
    text = open(os.path.join(ROOT, "include", "seld_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))
    found = re.findall(r"\b(seld_\w+)\s*\(([^()]*)\)", text)
    return [(name, 0 if params.strip() == "void" else params.count(",") + 1) for name, params in found]


def test_every_declared_entry_point_is_typed():
    lib = pkg()._lib.lib()
    declared = _declared()
    assert len(declared) == len(set(n for n, _ in declared)) >= 148
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seld_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(seld_\w+)\s*\(", text)) == set(n for n, _ in declared)
    for name, nparams in declared:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert len(fn.argtypes) == nparams, (name, nparams, fn.argtypes)


def test_parser_agrees_with_prototypes_written_by_hand():
    from ctypes import c_char_p, c_double, c_float, c_int, c_int32 as i32, c_int64 as i64, c_size_t, c_void_p as vp
    lib = pkg()._lib.lib()
    by_hand = {
        "seld_decode_workspace": (c_size_t, [i64, i32, i32, i32]),
        "seld_decode_count": (c_int, [vp, i32, i64, i32, i32, i32, vp, c_size_t, vp]),
        "seld_decode_write": (c_int, [vp, i32, i64, i32, i32, i32, c_double, vp, c_size_t, vp, vp, i64, vp, vp]),
        "seld_bn_finalize_ex": (c_int, [vp, i32, i64, c_float, c_float, vp, vp, vp, vp, vp, i32, vp]),
        "seld_hc_conv_transpose_out_shape": (c_int, [vp, vp, vp]),
        "seld_build_arch": (c_char_p, []),
    }
    for name, (restype, argtypes) in by_hand.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, (name, fn.restype)
        assert list(fn.argtypes) == argtypes, (name, fn.argtypes)
    assert lib.seld_build_arch() == b"gfx950"


def test_parser_refuses_what_it_cannot_type():
    L = pkg()._lib
    good = "int seld_a(const float* x /* nullable, (C) */, int64_t n, void* stream);\nsize_t seld_b(void);\n"
    assert L.prototypes(good) == {"seld_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]),
                                  "seld_b": (ctypes.c_size_t, [])}
    with pytest.raises(L.SeldHipError, match="seld_half_scale"):
        L.prototypes(good + "int seld_half_scale(float* x, _Float16 s, void* stream);\n")
    with pytest.raises(L.SeldHipError, match="seld_norm"):
        L.prototypes(good + "float seld_norm(const float* x, int64_t n);\n")
    with pytest.raises(L.SeldHipError, match="seld_split"):
        L.prototypes(good + "int\nseld_split(const float* x);\n")
    with pytest.raises(L.SeldHipError, match="seld_each"):
        L.prototypes(good + "int seld_each(void (*fn)(int32_t), void* stream);\n")


def test_wide_arguments_keep_their_width_without_a_wrapper():
    """Plain Python ints reach an int64_t / size_t parameter whole: 2 recordings give a positive size, (1 << 32) + 2 must
    not be taken for 2 (tests/test_decode_host.py fixes both halves: 2 is accepted, 1 << 22 recordings are refused)."""
    lib = pkg()._lib.lib()
    p = ctypes.c_void_p(64)
    assert lib.seld_decode_workspace(2, 600, 14, 3) > 0
    assert lib.seld_decode_workspace((1 << 32) + 2, 600, 14, 3) == 0
    need = lib.seld_decode_workspace(2, 600, 14, 3)
    assert lib.seld_decode_count(p, 0, 2, 600, 14, 3, p, need - 1, None) == -2         # R = 2: the workspace is checked
    assert lib.seld_decode_count(p, 0, (1 << 32) + 2, 600, 14, 3, p, (1 << 32) + need, None) == -4    # SELD_EUNSUPPORTED


def test_descriptor_validation_without_gpu():
    """Pure host-side argument checking of the ABI (no kernel is launched)."""
    L = pkg()._lib
    H = pkg().hip_ops
    d = H.make_conv_desc((2, 16, 40), 32, 8, (3,), 1, 1, 1)
    assert H.conv_out_shape(d) == (1, 40)
    d2 = H.make_conv_desc((2, 8, 12, 20), 16, 4, (3, 3), 1, 1, 1)
    assert H.conv_out_shape(d2) == (12, 20)
    bad = H.make_conv_desc((2, 12, 40), 32, 8, (3,), 1, 1, 1)      # 12 channels: not a multiple of 8
    out = (ctypes.c_int32 * 2)()
    assert L.lib().seld_hc_conv_out_shape(ctypes.byref(bad), out) == -1
    assert L.lib().seld_stft_frames(6400, 512, 112) == 16
    assert L.lib().seld_stft_frames(32000 * 60, 512, 112) == 4800


@pytest.mark.parametrize("case", MODEL_CASES, ids=[c["name"] for c in MODEL_CASES])
def test_state_dict_layout_matches_reference(case, golden):
    g = golden("model_" + case["name"])
    m = build_model(case)
    sd = m.state_dict()
    assert list(sd.keys()) == str(g["sd_names"]).split("\n")
    shapes = [",".join(str(d) for d in v.shape) for v in sd.values()]
    assert shapes == str(g["sd_shapes"]).split("\n")


@pytest.mark.parametrize("case", [c for c in MODEL_CASES if c.get("train")], ids=lambda c: c["name"])
def test_default_initialisation_matches_reference(case, golden):
    """Same seeds -> same weights: the initialisers reproduce the reference's random draws."""
    g = golden("init")
    M = importlib.import_module(PKG + ".model")
    np.random.seed(1)
    torch.manual_seed(1)
    m = M.SELD_Model(**model_kwargs(case))
    names = str(g[case["name"] + ".names"]).split("\n")
    cks = g[case["name"] + ".checksums"]
    params = dict(m.named_parameters())
    assert list(params.keys()) == names
    for i, n in enumerate(names):
        d = params[n].detach().double()
        got = np.array([d.sum().item(), (d ** 2).sum().item(), d.flatten()[0].item(), d.flatten()[-1].item()])
        assert np.allclose(got, cks[i], rtol=1e-6, atol=1e-7), (n, got, cks[i])


def test_model_names_and_receptive_field():
    m = build_model(MODEL_CASES[3])
    assert m.model_name == "DualQSELD-TCN-PHI-S1_BN_RF287_10RB"
    assert (m.receptive_field, m.total_n_resblocks) == (287, 10)
    M = importlib.import_module(PKG + ".model")
    assert M.TC_Block.dilation_schedule([10], "fibonacci") == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55]
    assert M.TC_Block.dilation_schedule([4], "pow2") == [1, 2, 4, 8]
    assert M.TC_Block.dilation_schedule([[1, 7], 2], "fibonacci") == [1, 7, 1, 1]


def test_no_cpu_fallback():
    L = pkg()._lib
    m = build_model(MODEL_CASES[3]).eval()
    x = torch.zeros(1, 8, 128, 64)
    with pytest.raises(L.SeldHipError):
        m(x)
    with pytest.raises(L.SeldHipError):
        pkg().hip_ops.stft_magphase(torch.zeros(2, 4096))


def test_readfile_and_configs(tmp_path):
    T = pkg().train
    p = tmp_path / "a.txt"
    p.write_text("--domain=DQ\n--use_bias_conv=False\n--fixed_seed=True\n--D=[10]\n#comment\n--lr=0.001\n")
    toks = T.readFile(str(p))
    assert toks == ['--domain', 'DQ', '--use_bias_conv', 0, '--fixed_seed', '1', '--D', '[10]', '--lr', '0.001']
    args = T.parse_args(["--TextArgs=" + str(p)])
    assert args.domain == "DQ" and args.use_bias_conv == 0 and args.fixed_seed == 1 and args.D == [10] and args.lr == 1e-3
    cfg_dir = os.path.join(ROOT, PKG, "config")
    for f in sorted(os.listdir(cfg_dir)):
        a = T.parse_args(["--TextArgs=" + os.path.join(cfg_dir, f)])
        m = T.model_from_args(a)
        n_params = sum(p.numel() for p in m.parameters())
        assert n_params > 0
        if "DQSELD-TCN-S1-PHI_8ch" in f and f.startswith("SERVER"):
            assert a.U == 384 and a.domain == "DQ" and m.model_name.startswith("DualQSELD-TCN-PHI-S1_BN_RF287_10RB")
        if "QSELD-TCN-S1-PHI_parallel" in f and f.startswith("SERVER"):
            # `--parallel_ConvTC_block=True` becomes '1', which is NOT a two-stream mode
            assert a.parallel_ConvTC_block == '1' and hasattr(m, "seld_block") and "_1_" in m.model_name


def test_flat_adam_aliases_parameters():
    """Host-side bookkeeping of the flat optimiser (the update itself is a HIP kernel, tested on the GPU)."""
    T = pkg().train
    lin = torch.nn.Linear(5, 3)
    w0 = lin.weight.detach().clone()
    opt = T.FlatAdam(lin.parameters(), lr=1e-3)
    assert opt.flat_param.numel() == 18
    assert torch.equal(lin.weight.detach(), w0)
    assert lin.weight.data_ptr() == opt.flat_param.data_ptr()
    assert lin.bias.data_ptr() == opt.flat_param.data_ptr() + 15 * 4
    lin(torch.ones(2, 5)).sum().backward()
    assert lin.weight.grad.data_ptr() == opt.flat_grad.data_ptr()      # autograd accumulated in place
    assert float(opt.flat_grad[:15].abs().sum()) > 0
    opt.zero_grad()
    assert float(opt.flat_grad.abs().sum()) == 0.0
    s = T.StepLR(opt, 2, 0.5)
    for _ in range(4):
        s.step()
    assert abs(opt.param_groups[0]["lr"] - 0.25e-3) < 1e-12


def test_shapes_beyond_32bit_offsets_are_not_given_to_the_fast_kernels():
    """The fast-product kernels index a tensor with 32-bit byte offsets (csrc/hcq_conv.hip, hcq_wgrad_grp.hip): the host must
    refuse them a tensor of 4 GB or more -- e.g. the first layer at batch 64, F = 256 (6.4 GB of output; /root/reference
    model.py:273-283 at twice the benchmark batch) -- so that such a call runs on the 64-bit-indexed generic kernels instead.
    Host-side queries only: nothing is launched."""
    pkg = importlib.import_module(PKG)
    H, L = pkg.hip_ops, pkg._lib
    big = H.make_conv_desc((64, 8, 256, 512), 192, 8, (3, 3), 1, 1, 1)           # y: 64*192*256*512*4 B = 6.4 GB
    ok = H.make_conv_desc((32, 8, 128, 512), 192, 8, (3, 3), 1, 1, 1)            # the benchmark's first layer: 1.6 GB
    assert H.hcq_pack_floats(ok, 2) > 0 and H.hcq_pack_floats(big, 2) == 0       # mode 2: the pooling first-layer kernel
    ok1 = H.make_conv_desc((32, 192, 16, 512), 192, 8, (3, 3), 1, 1, 1)
    big1_2d = H.make_conv_desc((256, 192, 32, 512), 192, 8, (3, 3), 1, 1, 1)     # 3.2 GB each way ... x2 batch: 6.4 GB
    big2_2d = H.make_conv_desc((512, 192, 32, 512), 192, 8, (3, 3), 1, 1, 1)
    for mode in (0, 1):
        assert H.hcq_pack_floats(ok1, mode) > 0
        assert H.hcq_pack_floats(big2_2d, mode) == 0
    del big1_2d
    big1 = H.make_conv_desc((32, 192, 16384), 384, 8, (3,), 1, 1, 1)             # 1-D: y = 32*384*16384*4 B = 805 MB per ... ok
    assert H.hcq_pack_floats(big1, 0) > 0
    huge1 = H.make_conv_desc((256, 192, 16384), 384, 8, (3,), 1, 1, 1)           # y = 6.4 GB
    assert H.hcq_pack_floats(huge1, 0) == 0 and H.hcq_pack_floats(huge1, 1) == 0
    # grouped weight gradient: one image of either operand stays below 2 GB, the step space below 2^30
    fam = L.lib().seld_hcq_wgrad_group_family
    assert fam(ctypes.byref(H.make_conv_desc((32, 192, 512), 384, 8, (3,), 1, 1, 1))) == 0
    assert fam(ctypes.byref(H.make_conv_desc((32, 192, 16, 512), 192, 8, (3, 3), 1, 1, 1))) == 2
    assert fam(ctypes.byref(H.make_conv_desc((1, 192, 4096, 1024), 192, 8, (3, 3), 1, 1, 1))) == -1      # 3.2 GB per image
