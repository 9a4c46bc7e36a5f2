"""Exact tests of the first stage without its convolution output (no GPU in this module): inputs, float64 references, the
host plan of csrc/first_stage.hip restated, and the bounds of tests/test_gpu_first_stage_exact.py.

INPUTS.  x integers in [-2, 2], component weights in {-1, 0, 1}, bias integers in [-2, 2] (or none), gamma in {-2 .. 2},
beta and mean integers in [-2, 2], invstd in {0.5, 1, 2}, dout integers in [-2, 2], drop_p in {0, 0.5} (scale 1 or 2).
The weights of block-channel ZERO_OB are zero in every component, so the output channels po * OB + ZERO_OB have an all-zero
row of the real matrix: variance 0, the `var < 0` clamp and 1 / sqrt(eps).

REFERENCES never use the Gram identity.  xcol = unfold(x, 3, padding 1) in float64; G = xcol xcol^T, s = sum xcol,
P = N H W;  y = W xcol + bias with W the oracle's assembled real matrix (oracle.seld_oracle.assemble_conv_weight);
mean and biased variance are those of y itself;  the window row is tests/pool_window_ref.window_rows;  the backward
reference forms dy = a (dz - k1 - xhat k2) at every position of y, takes dWf = sum_pos dy xcol^T and folds it onto the
components with the oracle's block table.

WHY THE DEVICE MUST AGREE EXACTLY.  Every entry of xcol is an integer of magnitude <= 2, so every product of the Gram
pass is an integer of magnitude <= 4 and every partial sum of them an integer bounded by the largest diagonal entry of G
(|sum x_i x_j| <= sum |x_i x_j| <= max(G_ii, G_jj)).  While that stays below 2^24 -- asserted on the reference's G -- every
float32 MFMA step, wave add and the double fold are exact IN ANY ORDER.  The same for |s| and, in double, for W G
(|W G| < 2^24 makes the float32 copy `wg` exact).  In the backward pass dz = dout * scale is an integer of magnitude <= 4,
xhat = (raw - mean) invstd a multiple of 0.5, a dz a multiple of 0.5 of magnitude <= 16: the per-chunk sums of
fs_reduce_kernel are exact while sum |dz xhat| of a chunk stays below 2^22, the weight-gradient partial of a workgroup
while sum |a dz xcol| over its blocks does (asserted from the reference, per chunk and per workgroup, never branched on).

PLAN.  blocks = N (H / 8) (W / 64);  fs_gram_kernel runs min(blocks, 512) workgroups, fs_wgrad_kernel min(blocks, 256),
workgroup g walks blocks g, g + grid, ...;  fs_reduce_kernel splits the N (H / 8) W elements of a channel into
clamp(elements / 8192, 1, 64) chunks of 4 * ceil(elements / 4 / chunks).  Bytes:
  gram   80 * 80 * 8  +  15 * 256 * 8  +  workgroups * 15 * 256 * 4
  bwd    C * chunks * 2 * 4  +  3 C * 4  +  72 C * 4  +  (C / 16) * 5 * 256 * 8  +  workgroups * (C / 16) * 5 * 256 * 4  +  64"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import seld_oracle as O
from tests import hcq_exact as X
from tests import philox_ref as R
from tests import pool_window_ref as PW
from tests.golden.first_stage_exact_cases import BY_NAME, CASES

assert_exact, sentinel_output, assert_band_intact, mismatch_report = \
    X.assert_exact, X.sentinel_output, X.assert_band_intact, X.mismatch_report

FS_K, FS_KP, FS_NTILE = 72, 80, 15
POOL = 8
GRAM_WGS, WGRAD_WGS = 512, 256
RED_CHUNK, RED_MAX = 8192, 64
EXACT24, EXACT22 = 2.0 ** 24, 2.0 ** 22
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
EPS = 1e-5
MOMENTUM = 0.1
ZERO_OB = 1                                   # block channel whose weights are zero in every component
FILL_STEP = 0.25
SEED, OFFSET = 0x5E1D2024, 977                # the Dropout of the drop_p = 0.5 runs


def case(name):
    return BY_NAME[name]


def desc(H, c):
    return H.make_conv_desc(tuple(c["x"]), c["cout"], c["algebra"], c["k"], c["stride"], c["padding"], c["dilation"])


def weight_shape(c):
    return (c["cout"] // c["algebra"], 8 // c["algebra"], 3, 3)


def pooled_shape(c):
    N, _, H, Wd = c["x"]
    return (N, c["cout"], H // POOL, Wd)


# ---- the host plan, restated ----------------------------------------------------------------------------------------------
def _walk(nblocks, nwg):
    """(fewest, most) blocks a workgroup of a grid-stride walk takes."""
    return nblocks // nwg, (nblocks + nwg - 1) // nwg


def wgrad_form(algebra, cout):
    if cout == 192:
        return "<6, true>"
    if cout == 128:
        return "<4, true>"
    return "<2, true>" if algebra == 8 else "<2, false>"


def plan(c):
    N, _, H, Wd = c["x"]
    C = c["cout"]
    nblocks = N * (H // 8) * (Wd // 64)
    gram_wgs, wgrad_wgs = min(nblocks, GRAM_WGS), min(nblocks, WGRAD_WGS)
    total = N * (H // 8) * Wd
    nchunk = max(1, min(RED_MAX, total // RED_CHUNK))
    per = ((total // 4 + nchunk - 1) // nchunk) * 4
    chunks = tuple(max(0, min(total, (k + 1) * per) - k * per) for k in range(nchunk))
    gram_bytes = FS_KP * FS_KP * 8 + FS_NTILE * 256 * 8 + gram_wgs * FS_NTILE * 256 * 4
    bwd_bytes = C * nchunk * 2 * 4 + 3 * C * 4 + C * FS_K * 4 + (C // 16) * 5 * 256 * 8 + wgrad_wgs * (C // 16) * 5 * 256 * 4 + 64
    return dict(blocks=nblocks, gram_wgs=gram_wgs, wgrad_wgs=wgrad_wgs, gram=_walk(nblocks, gram_wgs),
                wgrad=_walk(nblocks, wgrad_wgs), nchunk=nchunk, per=per, chunks=chunks, total=total,
                gram_bytes=gram_bytes, bwd_bytes=bwd_bytes, form=wgrad_form(c["algebra"], C))


def bwd_supported(algebra, cout):
    return cout % 64 == 0 and cout <= 192 and (algebra == 8 or cout == 64)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def inputs(c):
    """float32 tensors: x, ws (component list), bias (None where the case has none), dout, and the BatchNorm inputs of
    the backward test (gamma, beta, mean, invstd: tests/pool_window_ref.bn_inputs)."""
    gen = torch.Generator().manual_seed(X.W._seed(c, None) ^ 0xF57A)
    draw = lambda s: torch.randint(-2, 3, s, generator=gen).float()
    t = {"x": draw(tuple(c["x"]))}
    t["ws"] = [torch.randint(-1, 2, weight_shape(c), generator=gen).float() for _ in range(c["algebra"])]
    for w in t["ws"]:
        w[ZERO_OB] = 0.0
    b = draw((c["cout"],))
    t["bias"] = b if c["bias"] else None
    t["dout"] = draw(pooled_shape(c))
    t.update(PW.bn_inputs(c["cout"], gen))
    return t


def zero_channels(c):
    OB = c["cout"] // c["algebra"]
    return [po * OB + ZERO_OB for po in range(c["algebra"])]


def real_matrix(ws):
    """(C, 72) float64: row c of the real matrix, column = input channel * 9 + tap (the oracle's assembly)."""
    w = O.assemble_conv_weight([w.double() for w in ws])
    return w.reshape(w.shape[0], FS_K)


def fold_components(dwf, algebra, absolute=False):
    """(component gradients, blocks per component) of a real-matrix gradient dwf (C, 72) by the oracle's block table;
    absolute: the signs dropped (dwf holds magnitudes)."""
    C = dwf.shape[0]
    OB, IB = C // algebra, 8 // algebra
    blocks = dwf.view(algebra, OB, algebra, IB, 9)
    out = [torch.zeros(OB, IB, 9, dtype=torch.float64) for _ in range(algebra)]
    count = [0] * algebra
    for po, row in enumerate(O.block_table(algebra)):
        for qi, e in enumerate(row):
            if e is not None:
                out[e[0]] += (1 if absolute else e[1]) * blocks[po, :, qi]
                count[e[0]] += 1
    return [o.view(OB, IB, 3, 3) for o in out], count


def dropout_mask(c, p):
    """float64 factors (0 or 1 / (1 - p)) of the stage's Dropout on the pooled tensor, from tests/philox_ref.py."""
    shape = pooled_shape(c)
    if p == 0.0:
        return torch.ones(shape, dtype=torch.float64)
    n = int(np.prod(shape))
    return torch.from_numpy(R.factors(SEED, OFFSET, n, p)).view(shape).double()


# ---- references -------------------------------------------------------------------------------------------------------------
def gram_reference(x):
    """(G (72, 72), s (72), P) of x (N, 8, H, W) in float64, image by image."""
    G = torch.zeros(FS_K, FS_K, dtype=torch.float64)
    s = torch.zeros(FS_K, dtype=torch.float64)
    for n in range(x.shape[0]):
        xc = F.unfold(x[n:n + 1].double(), 3, padding=1)[0]
        G += xc @ xc.t()
        s += xc.sum(1)
    return G, s, float(x.shape[0] * x.shape[2] * x.shape[3])


def gram_expected(G, s, P):
    """The 80 x 80 doubles seld_first_stage_gram documents."""
    E = torch.zeros(FS_KP, FS_KP, dtype=torch.float64)
    E[:FS_K, :FS_K] = G
    E[FS_K, :FS_K] = s
    E[:FS_K, FS_K] = s
    E[FS_K, FS_K] = P
    return E


def assert_gram_exactness(G, s):
    assert bool((G == G.round()).all()) and bool((s == s.round()).all())
    assert float(G.diagonal().max()) == float(G.abs().max()) < EXACT24 and float(s.abs().max()) < EXACT24


_refs = {}


def reference(c):
    """Everything the tests of a case compare with (cached per case name, left unchanged by its users)."""
    if c["name"] not in _refs:
        _refs[c["name"]] = _reference(c)
    return _refs[c["name"]]


def _reference(c):
    t = inputs(c)
    G, s, P = gram_reference(t["x"])
    assert_gram_exactness(G, s)
    r = dict(t, G=G, s=s, P=P, gram=gram_expected(G, s, P))
    if c["sections"] == "A":
        return r
    N, _, H, Wd = c["x"]
    C, A = c["cout"], c["algebra"]
    Wf = real_matrix(t["ws"])
    bias = t["bias"].double() if t["bias"] is not None else torch.zeros(C, dtype=torch.float64)
    WG = Wf @ G
    assert bool((WG == WG.round()).all()) and float(WG.abs().max()) < EXACT24
    xcol = [F.unfold(t["x"][n:n + 1].double(), 3, padding=1)[0] for n in range(N)]            # N x (72, H W)
    y = torch.stack([(Wf @ xc).view(C, H, Wd) for xc in xcol]) + bias.view(1, C, 1, 1)
    assert bool((y == y.round()).all())
    # ---- B: the statistics of y itself
    mean = y.mean(dim=(0, 2, 3))
    var = ((y - mean.view(1, C, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    ey2 = ((y - bias.view(1, C, 1, 1)) ** 2).mean(dim=(0, 2, 3))                             # what w^T G w / P evaluates
    zc = zero_channels(c)
    assert all(float(var[k]) == 0.0 and float(mean[k]) == float(bias[k]) for k in zc)
    assert int((var == 0).sum()) == len(zc)
    # (the identity the device relies on, to the accuracy of float64: recorded by the host test)
    t1 = (Wf @ s) / P
    r["identity_gap"] = float((((Wf @ G) * Wf).sum(1) / P - t1 * t1 - var).abs().max())
    r.update(Wf=Wf, WG=WG, mean_y=mean, var_y=var, ey2=ey2, ymax=float(y.abs().max()))
    # ---- C: windows chosen by the test's gamma, the stage's output and the backward pass at the test's mean / invstd
    raw, idx, ties = PW.window_rows(y, t["gamma"], POOL)
    z = PW.bn_relu(raw, t["gamma"], t["beta"], t["mean"], t["invstd"])
    r.update(raw=raw.float(), idx=idx.to(torch.uint8), ties=ties, bwd={})
    pl = plan(c)
    a = (t["gamma"] * t["invstd"]).double()
    mu, istd = t["mean"].double(), t["invstd"].double()
    xhat_p = (raw - mu.view(1, C, 1, 1)) * istd.view(1, C, 1, 1)
    for p in ((0.0, 0.5) if c["drop"] else (0.0,)):
        scale = 1.0 / (1.0 - p)
        out = z * dropout_mask(c, p)
        dz = t["dout"].double() * scale * (out != 0)
        term = dz * xhat_p
        v0, v1 = term.sum(dim=(0, 2, 3)), dz.sum(dim=(0, 2, 3))
        # exactness of fs_reduce_kernel: per chunk, from these values
        flat = term.abs().permute(1, 0, 2, 3).reshape(C, -1)
        worst_chunk = max(float(flat[:, k * pl["per"]:(k + 1) * pl["per"]].sum(1).max()) for k in range(pl["nchunk"]))
        assert worst_chunk < EXACT22, (c["name"], worst_chunk)
        # ... and of a workgroup's weight-gradient partial: sum |a dz| over its blocks times the largest |xcol| = 2
        az = (a.abs().view(1, C, 1, 1) * dz.abs()).view(N, C, H // 8, Wd // 64, 64).sum(-1).permute(1, 0, 2, 3).reshape(C, -1)
        nwg = pl["wgrad_wgs"]
        pad = (-az.shape[1]) % nwg
        per_wg = F.pad(az, (0, pad)).view(C, -1, nwg).sum(1)
        assert 2.0 * float(per_wg.max()) < EXACT22, (c["name"], float(per_wg.max()))
        M = float(N * H * Wd)
        k1, k2 = v1 / M, v0 / M
        dwf = torch.zeros(C, FS_K, dtype=torch.float64)
        part = torch.zeros(C, FS_K, dtype=torch.float64)
        for n in range(N):
            dzf = torch.zeros(C, H // 8, POOL, Wd, dtype=torch.float64)
            dzf.scatter_(2, idx[n].unsqueeze(2), dz[n].unsqueeze(2))
            dzf = dzf.view(C, H * Wd)
            xh = (y[n].reshape(C, H * Wd) - mu.view(C, 1)) * istd.view(C, 1)
            dy = a.view(C, 1) * (dzf - k1.view(C, 1) - xh * k2.view(C, 1))
            dwf += dy @ xcol[n].t()
            part += (a.view(C, 1) * dzf) @ xcol[n].t()
        dw, count = fold_components(dwf, A)
        # magnitudes the bound charges (no credit for cancellation): |c1 (W G + bias s)| + |a| (|mu is k2| + |k1|) |s| + |partial|
        c1 = a * istd * k2
        mag1 = c1.abs().view(C, 1) * (WG + bias.view(C, 1) * s.view(1, FS_K)).abs()
        mag0 = (a.abs() * ((mu * istd * k2).abs() + k1.abs())).view(C, 1) * s.abs().view(1, FS_K)
        mag_c = [fold_components(m_, A, absolute=True)[0] for m_ in (mag1, mag0, part.abs())]
        r["bwd"][p] = dict(out=out.float(), dz=dz, v0=v0, v1=v1, dw=dw, mag=mag_c, count=count)
        assert bool((out == out.float().double()).all())
    return r


# ---- bounds -----------------------------------------------------------------------------------------------------------------
# float32 roundings between the exact inputs and a component of dw, counted from fs_coef_kernel, fs_wsum_kernel and
# fs_wfold_kernel, each term charged with its own (an FMA contraction only removes some):
#   T1 = |c1 (W G + bias s)|:  c1 = -a * is * k2: a = gamma * is, a * is, k2 = (float)(s0 / count), the product with k2   4
#                              wg = (float)(W G)                                                                           1
#   T0 = |a| (|mu is k2| + |k1|) |s| (no credit for the cancellation inside c0 = a * (mu * is * k2 - k1)):
#                              a, mu * is, k2, the product, k1, the difference, the product with a                        7
#   Tp = |partial|:            exact under the conditions above                                                            0
#   every term and the slot:   dwf = (float)(double sum); fs_wfold_kernel: one add per block that holds the component
#                              (`count`); the `+=` into the slot                                                           1 + count + 1
C1_ROUNDINGS, C0_ROUNDINGS = 5, 7


def dw_bound(mag, count, slot):
    """Componentwise bound on |dw - reference| for a component held by `count` blocks with the slot's old value `slot`;
    mag = (T1, T0, Tp) summed over those blocks."""
    t1, t0, tp = mag
    common = count + 2
    return U * SLACK * ((C1_ROUNDINGS + common) * t1 + (C0_ROUNDINGS + common) * t0 + common * (tp + abs(slot))) + 2.0 ** -126


def slot_fill(k):
    return FILL_STEP * (k + 1)


def bn_tolerances(r):
    """(mean, invstd) tolerances of seld_first_stage_bn against the statistics of y itself: one float32 rounding of the
    double result, the float64 evaluation noise of both sides on the mean (2^-45 max |y|), and the double evaluation of
    w^T G w / P - (w.s / P)^2 on invstd: relative 2^-50 E[(y - bias)^2] / var."""
    var = r["var_y"]
    inv = 1.0 / torch.sqrt(var + float(np.float32(EPS)))
    safe = torch.where(var > 0, var, torch.ones_like(var))
    tol_mean = U * SLACK * r["mean_y"].abs() + 2.0 ** -45 * r["ymax"]
    exact = r["mean_y"].float().double() == r["mean_y"]                 # a float32 number: the single rounding has nothing to do
    tol_mean = torch.where(exact, torch.zeros_like(tol_mean), tol_mean)
    tol_inv = inv * (U * SLACK + 2.0 ** -50 * r["ey2"] / safe)
    return tol_mean, tol_inv, inv


# ---- real-valued inputs: the float32 Gram under a bound ---------------------------------------------------------------------
# A term x_i x_j of a workgroup's partial meets at most gram_depth() float32 roundings: its product, the adds of its wave's
# MFMA chain -- 8 rows x 4 column groups = 32 steps of 4 products a block, every product charged as an add of its own, times
# the most blocks a workgroup walks -- and the 3 adds of the other waves' tiles.  The partials are summed in double.
#   |G_dev - G|   <= depth u (1 + 2^-10) Gabs + 2^-30 Gabs =: E_G     Gabs = |xcol| |xcol|^T  (no credit for cancellation;
#                                                                     2^-30: the float64 sums of both sides)
#   |t1_dev - t1| <= |w| . E_s / P =: e1           t1 = w . s / P, the mean without the bias
#   |m2_dev - m2| <= |w|^T E_G |w| / P =: e2       m2 = w^T G w / P
#   |var_dev - var| <= e2 + 2 |t1| e1 + e1^2 + 2^-40 m2 =: e_var       (the double evaluation of m2 - t1^2)
#   |invstd_dev - invstd| <= invstd (d / 2 / (1 - d)^1.5 + u (1 + 2^-10)),  d = e_var / (var + eps) < 1/2 asserted
#   |mean_dev - mean| <= e1 + u (1 + 2^-10) |mean| + 2^-40 max |y|
REAL_KINDS = ("randn", "feature")


def gram_depth(c):
    return 4 * 32 * plan(c)["gram"][1] + 3 + 1


def real_inputs(c, kind):
    """x drawn from randn, or feature-like: channel ch = m_ch + s_ch * randn with m_ch in [-4, 4], s_ch in [0.25, 4];
    weights 0.3 * randn, bias 0.1 * randn (None where the case has none)."""
    gen = torch.Generator().manual_seed(X.W._seed(c, None) ^ (0x11AA if kind == "randn" else 0x22BB))
    x = torch.randn(tuple(c["x"]), generator=gen)
    if kind == "feature":
        m = torch.rand(8, generator=gen) * 8.0 - 4.0
        sd = torch.rand(8, generator=gen) * 3.75 + 0.25
        x = m.view(1, 8, 1, 1) + sd.view(1, 8, 1, 1) * x
    ws = [torch.randn(weight_shape(c), generator=gen) * 0.3 for _ in range(c["algebra"])]
    bias = torch.randn(c["cout"], generator=gen) * 0.1 if c["bias"] else None
    return {"x": x, "ws": ws, "bias": bias}


def real_reference(c, kind):
    """float64: the 80 x 80 Gram layout and its magnitude twin, the statistics of y = W xcol + bias itself, and the
    bounds above."""
    t = real_inputs(c, kind)
    N, _, H, Wd = c["x"]
    C = c["cout"]
    P = float(N * H * Wd)
    G, Ga = torch.zeros(FS_K, FS_K, dtype=torch.float64), torch.zeros(FS_K, FS_K, dtype=torch.float64)
    s, sa = torch.zeros(FS_K, dtype=torch.float64), torch.zeros(FS_K, dtype=torch.float64)
    Wf = real_matrix(t["ws"])
    bias = t["bias"].double() if t["bias"] is not None else torch.zeros(C, dtype=torch.float64)
    ys = []
    for n in range(N):
        xc = F.unfold(t["x"][n:n + 1].double(), 3, padding=1)[0]
        G += xc @ xc.t()
        Ga += xc.abs() @ xc.abs().t()
        s += xc.sum(1)
        sa += xc.abs().sum(1)
        ys.append(Wf @ xc)
    y = torch.stack(ys) + bias.view(1, C, 1)                                    # (N, C, H W)
    mean = y.mean(dim=(0, 2))
    var = ((y - mean.view(1, C, 1)) ** 2).mean(dim=(0, 2))
    m2 = ((y - bias.view(1, C, 1)) ** 2).mean(dim=(0, 2))
    factor = gram_depth(c) * U * SLACK + 2.0 ** -30
    gram, mag = gram_expected(G, s, P), gram_expected(Ga, sa, P)
    E = factor * mag
    E[FS_K, FS_K] = 0.0                                                         # the count: a sum of ones, exact below 2^24
    assert plan(c)["gram"][1] * 8 * 64 < EXACT24
    Wa = Wf.abs()
    e1 = Wa @ E[FS_K, :FS_K] / P
    e2 = ((Wa @ E[:FS_K, :FS_K]) * Wa).sum(1) / P
    t1 = mean - bias
    e_var = e2 + 2.0 * t1.abs() * e1 + e1 * e1 + 2.0 ** -40 * m2
    eps = float(np.float32(EPS))
    d = e_var / (var + eps)
    assert float(d.max()) < 0.5, (c["name"], kind, float(d.max()))
    inv = 1.0 / torch.sqrt(var + eps)
    return dict(t, gram=gram, E=E, mean=mean, var=var, invstd=inv,
                tol_mean=e1 + U * SLACK * mean.abs() + 2.0 ** -40 * float(y.abs().max()),
                tol_inv=inv * (d / 2.0 / (1.0 - d) ** 1.5 + U * SLACK), cancel=float((m2 / var).max()))


# ---- D: H.conv_bn_relu_pool on real-valued inputs, element by element ---------------------------------------------------------
# Every bound componentwise, u = 2^-24, times 1 + 2^-10, no credit for cancellation; (v, e) pairs multiply as
# P(|v| + e) - P|v|.  The reference is float64 and never uses the Gram identity: y = W xcol + bias, its own mean and
# variance, dy = a (dz - k1 - xhat k2) at every position, dWf = sum_pos dy xcol^T.  It is FED the device's window rows and
# ReLU pattern (which elements of the output are non-zero), after those are held to the oracle's (below).
#  forward, the pooling convolution (csrc/hcq_first.hip, fast product of csrc/hcq_forms.h): an output component is
#      c_q = sum_m R2[q][m] / 2 * P_m,  P_m = sum_k F_m(w_k) G_m(x_k) over k = (block channel, tap, range), at most 18 terms
#      (2 block channels x 9 taps in the quaternion, 1 x 9 x 2 ranges in the dual half of the dual quaternion).
#      F_m, G_m: one rounding each; the product and the MFMA chain: at most 18; hcq_recombine: 3; the bias: 1.  So
#      e_y = 24 u (A_q + |bias|),  A_q = sum_m |R2[q][m]| / 2 * sum_k (|w_c1| + |w_c2|)(|x_c1| + |x_c2|)    (fwd_magnitude)
#  statistics: e_mean, e_inv of real_reference (the Gram depth through w^T E_G w / P)
#      a = fl(gamma invstd): e_a = |gamma| e_inv + u |a|;   b = fl(beta - fl(mean a)):
#      e_b = (|mean| + e_mean)(|a| + e_a) - |mean a| + u (2 |mean a| + |beta|)
#  output z = max(v a + b, 0) at the device's row, v = y there:  e_z = (|v| + e_y)(|a| + e_a) - |v a| + e_b + 2u (|v a| + |b|)
#      (max(., 0) does not expand an error; the bound is on the value in front of it, which is what xhat is rebuilt from)
#  rows: the device's row may differ from the oracle's only where key(oracle row) - key(device row) <= e_y + e_y', key =
#      sign(gamma) y; the windows whose two best keys lie that close are counted on the reference BEFORE the device runs:
#      at most 0.1 %.
#  fs_reduce_kernel: xhat = (z - beta) fl(1 / gamma): e_xhat = (e_z + 3u (|z| + |beta| + e_z)) / |gamma|;  for gamma == 0,
#      xhat = (v - mean) invstd: e_xhat = (|v - mean| + e_y + e_mean)(invstd + e_inv) - |v - mean| invstd + 2u |xhat|
#      v0 = sum dz xhat, v1 = sum dz in float32: depth c_r = 4 ceil(chunk / 1024) + 6 + 2 + 1, chunks added in double, one cast
#      e_v0 = sum |dz| e_xhat + (c_r + 1) u sum |dz xhat|,  e_v1 = (c_r + 1) u sum |dz|      = the bounds of dgamma, dbeta
#  fs_coef_kernel: k = fl(v / M): e_k = e_v / M + u |k|;   c1 = -a is k2: three pairs + 2u |c1|;
#      t = mu is k2: three pairs + 2u |t|;  c0 = a (t - k1): magnitude m0 = |a| (|t| + |k1|),
#      e_c0 = (|a| + e_a)(|t| + |k1| + e_t + e_k1 + u (|t| + |k1|)) - m0 + u m0
#  fs_wgrad_kernel: operand fl(fl(a scale) dout): e_a + 2u |a| on a;  a term meets 4 * 32 adds a block times the most blocks a
#      workgroup walks + 3 quarter adds + the product:  e_part = (e_a + (depth_w + 2) u |a|) sum |dz| |xcol|
#  fs_wsum_kernel (double): wg = fl(W G_dev): e_wg = |W| E_G + u |W G|;  s: E_s;  one cast
#      e_dwf = e_part + (|c1| + e_c1)(|W G| + e_wg + |bias| (|s| + E_s)) - |c1| (|W G| + |bias| |s|)
#              + (m0 + e_c0)(|s| + E_s) - m0 |s| + u D,   D = |c1| (|W G| + |bias s|) + m0 |s| + |a| sum |dz| |xcol|
#  fs_wfold_kernel: e_dw = sum over the component's blocks of e_dwf + count u sum D      (the slot holds 0: the add is exact)
FWD_ROUNDINGS = 2 + 18 + 3 + 1
ROW_CAP = 1e-3
# The rows of the case table the route takes: the pooling convolution (seld_hcq_pack_floats(desc, 2, 1) > 0) serves the
# quaternion at 64 channels and the dual quaternion from 128; at 192 channels only from 512 position tiles, which of the
# table only ragged_gram_dq192 has -- left out for its 5 s of float64 reference per draw.  D_NOT_SERVED fall to the path that
# writes y (tests/test_first_stage_exact_host.py holds both lists to the library).
D_NAMES = ("one_block_q64", "halos_dq128", "ragged_wgrad_q64", "ragged_gram_q64")
D_NOT_SERVED = ("one_block_dq64", "one_block_r64", "halos_dq192", "ragged_wgrad_dq64")
D_TOO_SLOW = ("ragged_gram_dq192",)


def _pairs(v, e):
    """P(|v_i| + e_i) - P|v_i| for (value, error) pairs."""
    hi, lo = None, None
    for a, b in zip(v, e):
        hi = (a.abs() + b) if hi is None else hi * (a.abs() + b)
        lo = a.abs() if lo is None else lo * a.abs()
    return hi - lo, lo


def fwd_magnitude(c, t):
    """A (N, C, H, W): what the fast product's roundings are charged on (without the bias)."""
    from tests.hcq_forms_ref import HCQ_F, HCQ_G, HCQ_R2
    A, C = c["algebra"], c["cout"]
    N, _, H, Wd = c["x"]
    OB, IB = C // A, 8 // A
    xa = t["x"].double().abs().view(N, A, IB, H, Wd)
    wa = [w.double().abs() for w in t["ws"]]
    out = torch.zeros(N, A, OB, H, Wd, dtype=torch.float64)
    ranges = [(0, 0, 0)] if A == 4 else [(0, 0, 0), (4, 0, 4), (0, 4, 4)]          # (first weight, first input part, first output part)
    for w0, x0, o0 in ranges:
        P = []
        for m in range(8):
            fa = wa[w0 + HCQ_F[m][0]] + wa[w0 + HCQ_F[m][1]]
            ga = xa[:, x0 + HCQ_G[m][0]] + xa[:, x0 + HCQ_G[m][1]]
            P.append(F.conv2d(ga, fa, padding=1))
        for q in range(4):
            out[:, o0 + q] += sum(abs(HCQ_R2[q][m]) / 2.0 * P[m] for m in range(8))
    return out.view(N, C, H, Wd)


def e2e_inputs(c, kind):
    t = real_inputs(c, kind)
    C = c["cout"]
    gen = torch.Generator().manual_seed(X.W._seed(c, None) ^ 0x33CC)
    gamma = torch.rand(C, generator=gen) + 0.5
    gamma[1::3] *= -1.0
    gamma[5] = 0.0
    t.update(gamma=gamma, beta=torch.randn(C, generator=gen) * 0.2, cot=torch.randn(pooled_shape(c), generator=gen))
    return t


class E2E:
    """The float64 side of section D for one (case, draw)."""

    def __init__(self, c, kind):
        self.c, self.kind = c, kind
        t = self.t = e2e_inputs(c, kind)
        st = self.st = real_reference(c, kind)
        assert torch.equal(st["x"], t["x"])
        N, _, H, Wd = c["x"]
        C = c["cout"]
        self.Wf = real_matrix(t["ws"])
        self.bias = t["bias"].double() if t["bias"] is not None else torch.zeros(C, dtype=torch.float64)
        self.xcol = [F.unfold(t["x"][n:n + 1].double(), 3, padding=1)[0] for n in range(N)]
        self.y = torch.stack([(self.Wf @ xc).view(C, H, Wd) for xc in self.xcol]) + self.bias.view(1, C, 1, 1)
        self.e_y = FWD_ROUNDINGS * U * SLACK * (fwd_magnitude(c, t) + self.bias.abs().view(1, C, 1, 1))
        self.gamma, self.beta = t["gamma"].double(), t["beta"].double()
        self.mean, self.inv = st["mean"], st["invstd"]
        self.e_mean, self.e_inv = st["tol_mean"], st["tol_inv"]
        self.a = self.gamma * self.inv
        self.e_a = self.gamma.abs() * self.e_inv + U * SLACK * self.a.abs()
        ma = (self.mean * self.a).abs()
        self.b = self.beta - self.mean * self.a
        self.e_b = (self.mean.abs() + self.e_mean) * (self.a.abs() + self.e_a) - ma + U * SLACK * (2 * ma + self.beta.abs())
        # the oracle's rows, and how many windows could go either way
        win = lambda v: v.view(N, C, H // POOL, POOL, Wd)
        key = torch.sign(self.gamma).view(1, C, 1, 1, 1) * win(self.y)
        _, self.rows, _ = PW.window_rows(self.y, t["gamma"], POOL)
        top = key.topk(2, dim=3).values
        live = (self.gamma != 0).view(1, C, 1, 1)
        self.close = ((top[:, :, :, 0] - top[:, :, :, 1]) <= 2.0 * win(self.e_y).max(dim=3).values) & live
        self.excusable = float(self.close.double().mean())
        assert self.excusable <= ROW_CAP, (c["name"], kind, self.excusable)

    def at(self, v, rows):
        N, C, H, Wd = v.shape
        return v.view(N, C, H // POOL, POOL, Wd).gather(3, rows.long().unsqueeze(3)).squeeze(3)

    def check_rows(self, rows):
        """Rows of the device: the oracle's, or inside the forward bound of the oracle's key."""
        N, C = self.y.shape[:2]
        sg = torch.sign(self.gamma).view(1, C, 1, 1)
        gap = sg * (self.at(self.y, self.rows) - self.at(self.y, rows))
        room = self.at(self.e_y, self.rows) + self.at(self.e_y, rows)
        differ = rows.long() != self.rows
        bad = differ & ((gap > room) | (self.gamma == 0).view(1, C, 1, 1))
        assert int(bad.sum()) == 0, f"{int(bad.sum())} window rows differ from the oracle's beyond the forward bound"
        assert float(differ.double().mean()) <= ROW_CAP
        return int(differ.sum())

    def forward(self, rows):
        """(value in front of the ReLU, its bound) at the given rows."""
        C = self.y.shape[1]
        v, e_y = self.at(self.y, rows), self.at(self.e_y, rows)
        pc = lambda u_: u_.view(1, C, 1, 1)
        va = (v * pc(self.a)).abs()
        pre = v * pc(self.a) + pc(self.b)
        e_z = (v.abs() + e_y) * pc(self.a.abs() + self.e_a) - va + pc(self.e_b) + 2 * U * SLACK * (va + pc(self.b.abs()))
        return v, e_y, pre, e_z

    def backward(self, rows, opened):
        """Reference dgamma, dbeta, dw (component list) and their bounds for the device's rows and ReLU pattern."""
        c = self.c
        N, _, H, Wd = c["x"]
        C, A = c["cout"], c["algebra"]
        pl = plan(c)
        pc = lambda u_: u_.view(1, C, 1, 1)
        v, e_y, pre, e_z = self.forward(rows)
        dz = self.t["cot"].double() * opened
        xhat = (v - pc(self.mean)) * pc(self.inv)
        g = pc(self.gamma)
        safe = torch.where(g == 0, torch.ones_like(g), g).abs()
        e_x = (e_z + 3 * U * SLACK * (pre.abs() + pc(self.beta.abs()) + e_z)) / safe
        dm = (v - pc(self.mean)).abs()
        e_x0 = (dm + e_y + pc(self.e_mean)) * pc(self.inv + self.e_inv) - dm * pc(self.inv) + 2 * U * SLACK * xhat.abs()
        e_x = torch.where(g == 0, e_x0, e_x)
        c_r = 4 * ((pl["per"] + 1023) // 1024) + 6 + 2 + 1 + 1
        red = (0, 2, 3)
        v0, v1 = (dz * xhat).sum(red), dz.sum(red)
        e_v0 = (dz.abs() * e_x).sum(red) + c_r * U * SLACK * (dz * xhat).abs().sum(red)
        e_v1 = c_r * U * SLACK * dz.abs().sum(red)
        M = float(N * H * Wd)
        k1, k2 = v1 / M, v0 / M
        e_k1, e_k2 = e_v1 / M + U * SLACK * k1.abs(), e_v0 / M + U * SLACK * k2.abs()
        a, e_a, inv, e_inv, mu, e_mu = self.a, self.e_a, self.inv, self.e_inv, self.mean, self.e_mean
        d_c1, c1 = _pairs((a, inv, k2), (e_a, e_inv, e_k2))
        e_c1 = d_c1 + 2 * U * SLACK * c1
        d_t, tt = _pairs((mu, inv, k2), (e_mu, e_inv, e_k2))
        e_t = d_t + 2 * U * SLACK * tt
        inner = tt + k1.abs()
        m0 = a.abs() * inner
        e_c0 = (a.abs() + e_a) * (inner + e_t + e_k1 + U * SLACK * inner) - m0 + U * SLACK * m0
        depth_w = 4 * 32 * pl["wgrad"][1] + 3 + 1
        dwf = torch.zeros(C, FS_K, dtype=torch.float64)
        sabs = torch.zeros(C, FS_K, dtype=torch.float64)
        for n in range(N):
            dzf = torch.zeros(C, H // 8, POOL, Wd, dtype=torch.float64)
            dzf.scatter_(2, rows[n].long().unsqueeze(2), dz[n].unsqueeze(2))
            dzf = dzf.view(C, H * Wd)
            xh = (self.y[n].reshape(C, H * Wd) - mu.view(C, 1)) * inv.view(C, 1)
            dy = a.view(C, 1) * (dzf - k1.view(C, 1) - xh * k2.view(C, 1))
            dwf += dy @ self.xcol[n].t()
            sabs += dzf.abs() @ self.xcol[n].abs().t()
        col = lambda u_: u_.view(C, 1)
        E = self.st["E"]
        G, s = self.st["gram"][:FS_K, :FS_K], self.st["gram"][FS_K, :FS_K]
        WG = (self.Wf @ G).abs()
        e_wg = self.Wf.abs() @ E[:FS_K, :FS_K] + U * SLACK * WG
        sa, E_s = s.abs().view(1, FS_K), E[FS_K, :FS_K].view(1, FS_K)
        ba = col(self.bias.abs())
        e_part = col(e_a + (depth_w + 2) * U * SLACK * a.abs()) * sabs
        D = col(c1) * (WG + ba * sa) + col(m0) * sa + col(a.abs()) * sabs
        e_dwf = e_part + col(c1 + e_c1) * (WG + e_wg + ba * (sa + E_s)) - col(c1) * (WG + ba * sa) + \
            col(m0 + e_c0) * (sa + E_s) - col(m0) * sa + (U * SLACK + 2.0 ** -40) * D
        dw, count = fold_components(dwf, A)
        e_f, _ = fold_components(e_dwf, A, absolute=True)
        D_f, _ = fold_components(D, A, absolute=True)
        e_dw = [e + count[k] * U * SLACK * d_ for k, (e, d_) in enumerate(zip(e_f, D_f))]
        return dict(dgamma=v0, dbeta=v1, e_dgamma=e_v0 + U * SLACK * v0.abs() + 2.0 ** -126,
                    e_dbeta=e_v1 + U * SLACK * v1.abs() + 2.0 ** -126, dw=dw, e_dw=e_dw)
