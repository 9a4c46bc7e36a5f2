// Environment switches of libseld_hip.so, read ONCE (first use) into a validated table; seld_env_reload() re-reads
// them (the tests switch kernel generations inside one process).
//
// Selection switches -- every setting computes the same results, they only choose which kernel generation runs
// (the test suite uses them to cover every generation):
//   SELD_CONV_CFG=ct,pt   force the convolution tile (one of the candidates of pick_cfg, anything else is ignored)
//   SELD_CONV_NO_SMALLK   short reductions on the tiled kernels instead of hc_conv_smallk_kernel
//   SELD_CONV_NO_HCQ      block-matrix (16/48-product) kernels instead of the fast-product ones of hcq_conv.hip
//   SELD_MHA_NO_MFMA      attention without the MFMA kernels
//   SELD_DETERMINISTIC    run-to-run reproducible results: reductions that are normally split over workgroups and folded
//                         with float atomics (BatchNorm statistics, weight-gradient splits, bias / loss sums) run as ONE
//                         ordered chain per output element -- same values up to summation order, slower
#pragma once

namespace seld {

struct SeldEnv {
    int conv_cfg_ct = 0, conv_cfg_pt = 0;          // 0 = not forced
    bool conv_no_smallk = false;                    // SELD_CONV_NO_SMALLK
    bool conv_no_hcq = false;                       // SELD_CONV_NO_HCQ: 16/48-product kernels instead of hcq_conv.hip
    bool mha_no_mfma = false;                       // SELD_MHA_NO_MFMA
    bool deterministic = false;                     // SELD_DETERMINISTIC: every reduction in a fixed order (no multi-contributor float atomics)
};

const SeldEnv& env();      // abi.hip

}  // namespace seld
