"""Cases of the exact forward / data-gradient tests of the fast-product convolution (tests/hcq_exact.py,
test_hcq_exact_host.py, test_gpu_hcq_exact.py).  Data only: the fields make_conv_desc takes under a name, and per
(mode, npair) -- mode 0 forward, 1 data gradient; npair 2: two weight sets (forward) or two sources (gradient) in one
launch -- the kernel label and the ring slot kind (0: whole pairs of k-groups or no ring, 1: half pairs) the library is
expected to answer for the shape.  A combination that is absent is one the fast-product kernels do not take.

KEY_CASES: one case per launch key (mode, npair, label, slot kind) that the `default` column of
tests/golden/hcq_dispatch.json records for modes 0 and 1, at the smallest shape that still produces the key among
N = 2, W = 128 for the 1-D layers, (N, H, W) = (2, 3, 64) and (1, 8, 64) for the 3x3 layers, and, for the three-tile keys
alone (24 output block channels and at least 512 position tiles, 256 for a forward pair), 16384 or 32768 positions.
The shapes were found on the CPU with the host-only queries, as make_golden_hcq_dispatch.py asks them; one case usually
serves several keys.  EDGE_CASES: shapes beside them (`edge` says which).

thin: the launches that gather BatchNorm statistics run on a weight set of their own in which one weight in `thin` is
non-zero (default: the dense set A itself), chosen so that the oracle's per-channel sum |o| and sum o^2 stay below 2^24
and the statistics of the epilogue are exact (tests/hcq_exact.py); stats_exact records whether they do.
test_hcq_exact_host.py recomputes every recorded answer from the built library and the oracle."""
FWD, FWD_PAIR, DGRAD, DGRAD_PAIR = (0, 1), (0, 2), (1, 1), (1, 2)


def _c(name, algebra, x, cout, k, padding, dilation, launch, thin=1, stats_exact=True, edge=None):
    return dict(name=name, algebra=algebra, x=tuple(x), cout=cout, k=tuple(k), stride=1, padding=padding,
                dilation=dilation, launch=launch, thin=thin, stats_exact=stats_exact, edge=edge)


KEY_CASES = [
    _c("q_1x1_ib8_ob16_d1_n2_w128", 4, (2, 32, 128), 64, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 8, 1, 0, 1, 2, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 0, 1, 2, false, true>", 0)}),
    _c("q_1x1_ib16_ob16_d1_n2_w128", 4, (2, 64, 128), 64, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0)}),
    _c("q_1x1_ib8_ob32_d1_n2_w128", 4, (2, 32, 128), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 8, 2, 0, 1, 2, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 8, 2, 0, 1, 2, false, true>", 0)}),
    _c("q_1x1_ib24_ob16_d1_n2_w128", 4, (2, 96, 128), 64, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 24, 1, 0, 1, 6, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 24, 1, 0, 1, 6, false, true>", 0)}),
    _c("q_1x1_ib16_ob32_d1_n2_w128", 4, (2, 64, 128), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 2, 0, 1, 4, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 2, 0, 1, 4, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0)}),
    _c("q_1x1_ib32_ob16_d1_n2_w128", 4, (2, 128, 128), 64, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 16, 2, 0, 1, 4, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 16, 2, 0, 1, 4, false, true>", 0)}),
    _c("q_1x1_ib24_ob32_d1_n2_w128", 4, (2, 96, 128), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 24, 2, 0, 1, 6, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 24, 2, 0, 1, 6, false, true>", 0)}),
    _c("q_1x3_ib4_ob16_d1_n2_w128", 4, (2, 16, 128), 64, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 0, 1, 3, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 0, 1, 3, false, true>", 0)}),
    _c("q_1x3_ib8_ob16_d1_n2_w128", 4, (2, 32, 128), 64, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0)}),
    _c("q_1x3_ib8_ob16_d17_n2_w128", 4, (2, 32, 128), 64, (3,), 17, 17, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0)}),
    _c("q_1x3_ib16_ob8_d1_n2_w128", 4, (2, 64, 128), 32, (3,), 1, 1, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0)}),
    _c("q_1x3_ib16_ob8_d17_n2_w128", 4, (2, 64, 128), 32, (3,), 17, 17, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0)}),
    _c("q_1x3_ib4_ob32_d1_n2_w128", 4, (2, 16, 128), 128, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 2, 0, 1, 3, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 2, 0, 1, 3, false, true>", 0)}),
    _c("q_1x3_ib8_ob32_d1_n2_w128", 4, (2, 32, 128), 128, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 3, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 3, false, true>", 0)}),
    _c("q_1x3_ib8_ob32_d17_n2_w128", 4, (2, 32, 128), 128, (3,), 17, 17, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 5, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 5, false, true>", 0)}),
    _c("q_1x3_ib32_ob8_d1_n2_w128", 4, (2, 128, 128), 32, (3,), 1, 1, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 3, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 3, false, true>", 0)}),
    _c("q_3x3_ib1_ob16_d1_n2_h3_w64", 4, (2, 4, 3, 64), 64, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 1, 1, 0, 1, 1, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 1, 0, 1, 1, false, false>", 0)}),
    _c("q_3x3_ib2_ob16_d1_n2_h3_w64", 4, (2, 8, 3, 64), 64, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 2, 1, 0, 1, 2, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 1, 0, 1, 2, false, false>", 0)}),
    _c("q_3x3_ib4_ob16_d1_n2_h3_w64", 4, (2, 16, 3, 64), 64, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0)}),
    _c("q_3x3_ib16_ob4_d1_n2_h3_w64", 4, (2, 64, 3, 64), 16, (3, 3), 1, 1, {
        DGRAD: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0)}),
    _c("q_3x3_ib1_ob16_d1_n1_h8_w64", 4, (1, 4, 8, 64), 64, (3, 3), 1, 1, {
        FWD: ("hcq_first_kernel<1, 1, 0, 1, 8>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 1, 0, 1, 1, false, false>", 0)}),
    _c("q_3x3_ib2_ob16_d1_n1_h8_w64", 4, (1, 8, 8, 64), 64, (3, 3), 1, 1, {
        FWD: ("hcq_first_kernel<2, 1, 0, 1, 8>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 1, 0, 1, 2, false, false>", 0)}),
    _c("q_3x3_ib1_ob32_d1_n2_h3_w64", 4, (2, 4, 3, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 1, 2, 0, 1, 1, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 2, 0, 1, 1, false, false>", 0)}),
    _c("q_3x3_ib2_ob32_d1_n2_h3_w64", 4, (2, 8, 3, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 2, 2, 0, 1, 2, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 2, 0, 1, 2, false, false>", 0)}),
    _c("q_3x3_ib4_ob32_d1_n2_h3_w64", 4, (2, 16, 3, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 2, 0, 1, 4, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 2, 0, 1, 4, false, false>", 0)}),
    _c("q_3x3_ib32_ob4_d1_n2_h3_w64", 4, (2, 128, 3, 64), 16, (3, 3), 1, 1, {
        DGRAD: ("hcq_conv_kernel<3, 3, 4, 2, 0, 1, 4, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<3, 3, 4, 2, 0, 1, 4, false, false>", 0)}),
    _c("q_3x3_ib1_ob32_d1_n1_h8_w64", 4, (1, 4, 8, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_first_kernel<1, 2, 0, 1, 8>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 2, 0, 1, 1, false, false>", 0)}),
    _c("q_3x3_ib2_ob32_d1_n1_h8_w64", 4, (1, 8, 8, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_first_kernel<2, 2, 0, 1, 8>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 2, 0, 1, 2, false, false>", 0)}),
    _c("dq_1x1_ib8_ob16_d1_n2_w128", 8, (2, 64, 128), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, false, false>", 0)}),
    _c("dq_1x1_ib16_ob8_d1_n2_w128", 8, (2, 128, 128), 64, (1,), 0, 1, {
        DGRAD: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, false, false>", 0)}),
    _c("dq_1x1_ib16_ob16_d1_n2_w128", 8, (2, 128, 128), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, false, false>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, false, false>", 0)}),
    _c("dq_1x1_ib24_ob8_d1_n2_w128", 8, (2, 192, 128), 64, (1,), 0, 1, {
        DGRAD: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, true, false>", 0)}),
    _c("dq_1x1_ib16_ob24_d1_n2_w128", 8, (2, 128, 128), 192, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, true, false>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, false, false>", 0)}),
    _c("dq_1x1_ib24_ob16_d1_n2_w128", 8, (2, 192, 128), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, true, false>", 0)}),
    _c("dq_1x1_ib24_ob24_d1_n2_w128", 8, (2, 192, 128), 192, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, true, false>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, true, false>", 0)}),
    _c("dq_1x1_ib16_ob24_d1_n2_w8192", 8, (2, 128, 8192), 192, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 1, 1, 2, 8, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 2, 2, 8, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, false, false>", 0)}),
    _c("dq_1x1_ib24_ob24_d1_n2_w8192", 8, (2, 192, 8192), 192, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 24, 1, 2, 2, 12, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, true, false>", 0)}),
    _c("dq_1x1_ib24_ob8_d1_n2_w16384", 8, (2, 192, 16384), 64, (1,), 0, 1, {
        DGRAD: ("hcq_conv_kernel<1, 1, 8, 1, 2, 2, 4, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 2, 2, 4, false, false>", 1)}),
    _c("dq_1x1_ib16_ob24_d1_n2_w16384", 8, (2, 128, 16384), 192, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 1, 2, 2, 8, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 2, 2, 8, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 1, 2, 4, false, false>", 0)}),
    _c("dq_1x1_ib24_ob16_d1_n2_w16384", 8, (2, 192, 16384), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 24, 1, 1, 2, 12, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 16, 1, 2, 2, 8, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 2, 2, 8, false, false>", 1)}),
    _c("dq_1x1_ib24_ob24_d1_n2_w16384", 8, (2, 192, 16384), 192, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 24, 1, 2, 2, 12, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 24, 1, 2, 2, 12, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 24, 1, 2, 2, 12, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 2, 2, 4, false, false>", 1)}),
    _c("dq_1x3_ib4_ob16_d1_n2_w128", 8, (2, 32, 128), 128, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 0)}),
    _c("dq_1x3_ib8_ob16_d1_n2_w128", 8, (2, 64, 128), 128, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0)}),
    _c("dq_1x3_ib8_ob16_d9_n2_w128", 8, (2, 64, 128), 128, (3,), 9, 9, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 0)}),
    _c("dq_1x3_ib16_ob8_d1_n2_w128", 8, (2, 128, 128), 64, (3,), 1, 1, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0)}),
    _c("dq_1x3_ib12_ob16_d41_n2_w128", 8, (2, 96, 128), 128, (3,), 41, 41, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 1)}),
    _c("dq_1x3_ib12_ob16_d57_n2_w128", 8, (2, 96, 128), 128, (3,), 57, 57, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0)}),
    _c("dq_1x3_ib24_ob4_d1_n2_w128", 8, (2, 192, 128), 32, (3,), 1, 1, {
        DGRAD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, true, false>", 0)}),
    _c("dq_1x3_ib8_ob24_d1_n2_w128", 8, (2, 64, 128), 192, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0)}),
    _c("dq_1x3_ib16_ob16_d5_n2_w128", 8, (2, 128, 128), 128, (3,), 5, 5, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1)}),
    _c("dq_1x3_ib16_ob16_d13_n2_w128", 8, (2, 128, 128), 128, (3,), 13, 13, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, true>", 0)}),
    _c("dq_1x3_ib16_ob16_d33_n2_w128", 8, (2, 128, 128), 128, (3,), 33, 33, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1)}),
    _c("dq_1x3_ib24_ob8_d1_n2_w128", 8, (2, 192, 128), 64, (3,), 1, 1, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0)}),
    _c("dq_1x3_ib24_ob8_d9_n2_w128", 8, (2, 192, 128), 64, (3,), 9, 9, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, true, false>", 0)}),
    _c("dq_1x3_ib24_ob8_d33_n2_w128", 8, (2, 192, 128), 64, (3,), 33, 33, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, true, false>", 1)}),
    _c("dq_1x3_ib24_ob16_d33_n2_w128", 8, (2, 192, 128), 128, (3,), 33, 33, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, true, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, true, false>", 1)}),
    _c("dq_1x3_ib4_ob24_d1_n2_w8192", 8, (2, 32, 8192), 192, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 2, 2, 6, false, false>", 0)}),
    _c("dq_1x3_ib16_ob24_d1_n2_w8192", 8, (2, 128, 8192), 192, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 5, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0)}),
    _c("dq_1x3_ib4_ob24_d1_n2_w16384", 8, (2, 32, 16384), 192, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 2, 2, 6, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 2, 2, 6, false, false>", 0)}),
    _c("dq_1x3_ib24_ob4_d49_n2_w16384", 8, (2, 192, 16384), 32, (3,), 49, 49, {
        DGRAD: ("hcq_conv_kernel<1, 3, 4, 1, 2, 2, 6, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 2, 2, 6, false, true>", 0)}, thin=4),
    _c("dq_1x3_ib24_ob8_d1_n2_w16384", 8, (2, 192, 16384), 64, (3,), 1, 1, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 5, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 5, false, false>", 1)}, thin=4),
    _c("dq_1x3_ib24_ob8_d9_n2_w16384", 8, (2, 192, 16384), 64, (3,), 9, 9, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 7, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 7, false, true>", 0)}, thin=4),
    _c("dq_1x3_ib24_ob8_d21_n2_w16384", 8, (2, 192, 16384), 64, (3,), 21, 21, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 7, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 7, false, false>", 0)}, thin=4),
    _c("dq_1x3_ib24_ob8_d25_n2_w16384", 8, (2, 192, 16384), 64, (3,), 25, 25, {
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 9, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 9, false, false>", 1)}, thin=4),
    _c("dq_1x3_ib24_ob12_d49_n2_w16384", 8, (2, 192, 16384), 96, (3,), 49, 49, {
        DGRAD: ("hcq_conv_kernel<1, 3, 4, 1, 2, 2, 6, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 2, 2, 6, false, true>", 0)}, thin=4),
    _c("dq_1x3_ib16_ob24_d1_n2_w16384", 8, (2, 128, 16384), 192, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 5, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 5, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0)}, thin=4),
    _c("dq_1x3_ib24_ob16_d1_n2_w16384", 8, (2, 192, 16384), 128, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 5, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 5, false, false>", 1)}, thin=4),
    _c("dq_1x3_ib24_ob16_d9_n2_w16384", 8, (2, 192, 16384), 128, (3,), 9, 9, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 7, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 2, 2, 7, false, true>", 0)}, thin=4),
    _c("dq_3x3_ib1_ob16_d1_n2_h3_w64", 8, (2, 8, 3, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 1, 1, 1, 2, 2, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 1, 1, 2, 2, false, false>", 0)}),
    _c("dq_3x3_ib2_ob16_d1_n2_h3_w64", 8, (2, 16, 3, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 2, 1, 1, 2, 4, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 1, 1, 2, 4, false, false>", 0)}),
    _c("dq_3x3_ib4_ob16_d1_n2_h3_w64", 8, (2, 32, 3, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0)}),
    _c("dq_3x3_ib16_ob4_d1_n2_h3_w64", 8, (2, 128, 3, 64), 32, (3, 3), 1, 1, {
        DGRAD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0)}),
    _c("dq_3x3_ib1_ob16_d1_n1_h8_w64", 8, (1, 8, 8, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_first_kernel<1, 1, 1, 2, 8>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 1, 1, 2, 2, false, false>", 0)}),
    _c("dq_3x3_ib2_ob16_d1_n1_h8_w64", 8, (1, 16, 8, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_first_kernel<2, 1, 1, 2, 8>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 1, 1, 2, 4, false, false>", 0)}),
    _c("dq_3x3_ib1_ob24_d1_n2_h3_w64", 8, (2, 8, 3, 64), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 1, 1, 1, 2, 2, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 1, 1, 2, 2, true, false>", 0)}),
    _c("dq_3x3_ib2_ob24_d1_n2_h3_w64", 8, (2, 16, 3, 64), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 2, 1, 1, 2, 4, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 1, 1, 2, 4, true, false>", 0)}),
    _c("dq_3x3_ib4_ob24_d1_n2_h3_w64", 8, (2, 32, 3, 64), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0)}),
    _c("dq_3x3_ib24_ob4_d1_n2_h3_w64", 8, (2, 192, 3, 64), 32, (3, 3), 1, 1, {
        DGRAD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0)}),
    _c("dq_3x3_ib1_ob24_d1_n2_h4_w2048", 8, (2, 8, 4, 2048), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 1, 1, 1, 2, 2, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 1, 1, 2, 2, 2, false, false>", 0)}),
    _c("dq_3x3_ib2_ob24_d1_n2_h4_w2048", 8, (2, 16, 4, 2048), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 2, 1, 1, 2, 4, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 1, 2, 2, 4, false, false>", 0)}),
    _c("dq_3x3_ib4_ob24_d1_n2_h4_w2048", 8, (2, 32, 4, 2048), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 2, 2, 7, false, false>", 0)}),
    _c("dq_3x3_ib2_ob24_d1_n2_h16_w1024", 8, (2, 16, 16, 1024), 192, (3, 3), 1, 1, {
        FWD: ("hcq_first_kernel<2, 1, 2, 2, 8>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 2, 1, 2, 2, 4, false, false>", 0)}),
    _c("dq_3x3_ib4_ob24_d1_n4_h4_w2048", 8, (4, 32, 4, 2048), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 2, 2, 7, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 2, 2, 7, false, false>", 0)}),
    _c("dq_3x3_ib24_ob4_d1_n4_h4_w2048", 8, (4, 192, 4, 2048), 32, (3, 3), 1, 1, {
        DGRAD: ("hcq_conv_kernel<3, 3, 4, 1, 2, 2, 7, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 2, 2, 7, false, false>", 0)}, thin=16),
]

EDGE_CASES = [
    _c("dq_1x3_ib8_ob16_d1_n1_w64", 8, (1, 64, 64), 128, (3,), 1, 1, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 0)}, edge="one_tile"),
    _c("q_1x1_ib8_ob16_d1_n1_w64", 4, (1, 32, 64), 64, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 8, 1, 0, 1, 2, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 8, 1, 0, 1, 2, false, true>", 0)}, edge="one_tile"),
    _c("dq_3x3_ib4_ob16_d1_n1_h1_w64", 8, (1, 32, 1, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0)}, edge="one_tile"),
    _c("dq_1x3_ib8_ob24_d5_n1_w128", 8, (1, 64, 128), 192, (3,), 5, 5, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0)}, edge="n1"),
    _c("dq_1x3_ib8_ob24_d5_n3_w128", 8, (3, 64, 128), 192, (3,), 5, 5, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, true, false>", 0)}, edge="n3"),
    _c("q_1x1_ib16_ob32_d1_n3_w64", 4, (3, 64, 64), 128, (1,), 0, 1, {
        FWD: ("hcq_conv_kernel<1, 1, 16, 2, 0, 1, 4, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 1, 16, 2, 0, 1, 4, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 1, 16, 1, 0, 1, 4, false, true>", 0)}, edge="n3"),
    _c("q_3x3_ib8_ob16_d1_n3_h3_w64", 4, (3, 32, 3, 64), 64, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0)}, edge="n3"),
    _c("dq_3x3_ib4_ob24_d1_n2_h1_w64", 8, (2, 32, 1, 64), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0)}, edge="h1"),
    _c("dq_3x3_ib4_ob24_d1_n2_h2_w64", 8, (2, 32, 2, 64), 192, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, true, false>", 0)}, edge="h2"),
    _c("q_3x3_ib4_ob16_d1_n2_h1_w128", 4, (2, 16, 1, 128), 64, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 0, 1, 4, false, false>", 0)}, edge="h1"),
    _c("q_3x3_ib4_ob32_d1_n2_h2_w128", 4, (2, 16, 2, 128), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 2, 0, 1, 4, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 2, 0, 1, 4, false, false>", 0)}, edge="h2"),
    _c("dq_1x3_ib16_ob16_d64_n2_w64_side_taps_in_padding", 8, (2, 128, 64), 128, (3,), 64, 64, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0)}, edge="side_taps_in_padding"),
    _c("q_1x3_ib12_ob16_d64_n2_w64_side_taps_in_padding", 4, (2, 48, 64), 64, (3,), 64, 64, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 0, 1, 3, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 0, 1, 3, false, true>", 0)}, edge="side_taps_in_padding"),
    _c("dq_1x3_ib16_ob24_d64_n2_w64_side_taps_in_padding", 8, (2, 128, 64), 192, (3,), 64, 64, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, true, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, true, false>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0)}, edge="side_taps_in_padding"),
    _c("dq_3x3_ib16_ob16_d1_n2_h3_w64_route", 8, (2, 128, 3, 64), 128, (3, 3), 1, 1, {
        FWD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0),
        DGRAD: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<3, 3, 4, 1, 1, 2, 7, false, false>", 0)}, edge="route"),
    _c("q_1x3_ib16_ob32_d2_n2_w128_route", 4, (2, 64, 128), 128, (3,), 2, 2, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 3, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 2, 0, 1, 3, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0)}, edge="route"),
    _c("dq_1x3_ib16_ob16_d8_n2_w128_last_dilation_of_row", 8, (2, 128, 128), 128, (3,), 8, 8, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 5, false, false>", 1)}, edge="last_dilation_of_row"),
    _c("dq_1x3_ib16_ob16_d9_n2_w128_first_dilation_of_row", 8, (2, 128, 128), 128, (3,), 9, 9, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 1)}, edge="first_dilation_of_row"),
    _c("dq_1x3_ib16_ob16_d24_n2_w128_last_dilation_of_row", 8, (2, 128, 128), 128, (3,), 24, 24, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 7, false, false>", 0)}, edge="last_dilation_of_row"),
    _c("dq_1x3_ib16_ob16_d25_n2_w128_first_dilation_of_row", 8, (2, 128, 128), 128, (3,), 25, 25, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 0)}, edge="first_dilation_of_row"),
    _c("dq_1x3_ib16_ob16_d40_n2_w128_last_dilation_of_row", 8, (2, 128, 128), 128, (3,), 40, 40, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 1, 2, 9, false, false>", 1)}, edge="last_dilation_of_row"),
    _c("dq_1x3_ib16_ob16_d45_n2_w128_first_dilation_of_row", 8, (2, 128, 128), 128, (3,), 45, 45, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 1),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 1),
        DGRAD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 1),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, false>", 1)}, edge="first_dilation_of_row"),
    _c("dq_1x3_ib16_ob16_d64_n2_w128_last_dilation_of_row", 8, (2, 128, 128), 128, (3,), 64, 64, {
        FWD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 4, 1, 1, 2, 6, false, true>", 0)}, edge="last_dilation_of_row"),
    _c("q_1x3_ib16_ob16_d16_n2_w128_last_dilation_of_row", 4, (2, 64, 128), 64, (3,), 16, 16, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 3, false, true>", 0)}, edge="last_dilation_of_row"),
    _c("q_1x3_ib16_ob16_d17_n2_w128_first_dilation_of_row", 4, (2, 64, 128), 64, (3,), 17, 17, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0)}, edge="first_dilation_of_row"),
    _c("q_1x3_ib16_ob16_d48_n2_w128_last_dilation_of_row", 4, (2, 64, 128), 64, (3,), 48, 48, {
        FWD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        FWD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        DGRAD: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0),
        DGRAD_PAIR: ("hcq_conv_kernel<1, 3, 8, 1, 0, 1, 5, false, true>", 0)}, edge="last_dilation_of_row"),
]

ALL_CASES = KEY_CASES + EDGE_CASES
BY_NAME = {c["name"]: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES), "case names are unique"

# Launch keys of the fixture that no case reaches, by name, each with its reason (at most 5 % of the keys): none.
LEFT_OUT = {}

# ---- C. guard bands: one case per tile program (three-tile, mixed, two-tile dual quaternion, two and one quaternion
# tiles, the first-layer kernel in both algebras), the dilation-64 cases on a 64-wide row, an image of height 1
GUARD = ["dq_1x3_ib4_ob24_d1_n2_w16384", "dq_1x3_ib8_ob24_d1_n2_w128", "dq_1x3_ib16_ob16_d13_n2_w128",
         "q_3x3_ib4_ob32_d1_n2_h3_w64", "q_1x3_ib8_ob16_d17_n2_w128", "dq_3x3_ib2_ob16_d1_n1_h8_w64",
         "q_3x3_ib1_ob32_d1_n1_h8_w64", "dq_1x3_ib16_ob24_d64_n2_w64_side_taps_in_padding",
         "q_1x3_ib12_ob16_d64_n2_w64_side_taps_in_padding", "dq_3x3_ib4_ob24_d1_n2_h1_w64"]

# ---- D. the autograd routes: dual-quaternion 1x3, 1x1 and 3x3, quaternion 1x3
# (shapes the fast-product kernels take in all four launches)
ROUTES = ["dq_1x3_ib16_ob16_d5_n2_w128", "dq_1x1_ib16_ob24_d1_n2_w128", "dq_3x3_ib16_ob16_d1_n2_h3_w64_route",
          "q_1x3_ib16_ob32_d2_n2_w128_route"]
assert all(n in BY_NAME for n in GUARD + ROUTES)
