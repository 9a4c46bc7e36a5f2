// Shared by the attention kernels of mha.hip (VALU) and mha_mfma.hip (fp32 MFMA): the optional keep-mask.
#pragma once
#include <math.h>
#include <stdint.h>

namespace seld {

// uint8 keep-mask over the (N, H, Tq, Tk) energy: score (n, h, q, k) takes part iff p[n*sn + h*sh + q*sq + k*sk] != 0.
// Strides are in elements and 0 on a broadcast dim, so a (N, 1, 1, Tk) key-padding mask is read as it is.  A masked
// score becomes -1e9 * scale (masked_fill(mask == 0, -1e9) before the division by sqrt(hd), model.py:42-46): every
// masked score of a row takes the same finite value, so a fully masked row attends uniformly to all Tk keys.
struct MhaMask {
    const uint8_t* p = nullptr;
    long long sn = 0, sh = 0, sq = 0, sk = 0;
    __device__ __forceinline__ const uint8_t* row(int n, int h, int q) const { return p + n * sn + h * sh + q * sq; }
    __device__ __forceinline__ const uint8_t* col(int n, int h, int k) const { return p + n * sn + h * sh + k * sk; }
};

// lse saved for a row whose every key is masked.  Its true value, -1e9 * scale + log(Tk), rounds to -1e9 * scale in
// fp32, which would give exp(s - lse) = 1 instead of 1 / Tk in backward; the masked backward kernels give every key of
// such a row the weight 1 / Tk and no score gradient instead.
#define MHA_LSE_ALL_MASKED INFINITY

}  // namespace seld
