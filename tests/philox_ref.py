"""Host reference of the dropout random numbers: Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as
easy as 1, 2, 3", SC'11) in numpy, written from the published algorithm, and the mapping from its words to dropout
factors that include/seld_hip.h documents.  No torch, no GPU.

One round of Philox-4x32 on the counter (c0, c1, c2, c3) with the round key (k0, k1):

    hi0, lo0 = mulhilo(M0, c0)        M0 = 0xD2511F53
    hi1, lo1 = mulhilo(M1, c2)        M1 = 0xCD9E8D57
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)

Ten rounds; the key is bumped by the Weyl constants (W0, W1) = (0x9E3779B9, 0xBB67AE85) between rounds (not after the
last one, which would change nothing).

Everything that reaches a comparison with a kernel is computed in float32, so the factors are bit-comparable."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
GOLDEN64 = 0x9E3779B97F4A7C15       # the stream_id mix of hip_ops.norm_act._Philox.seed
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


def _u64(v):
    return np.atleast_1d(np.asarray(v, dtype=np.uint64))


def philox4x32_10_general(counter, key):
    """counter: (..., 4) words, key: (..., 2) words (anything that fits uint32) -> (..., 4) uint32."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(MASK32)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(MASK32)
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    lo, sh = np.uint64(MASK32), np.uint64(32)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & lo
            k1 = (k1 + np.uint64(W1)) & lo
        p0 = np.uint64(M0) * c0            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo, (p0 >> sh) ^ c3 ^ k1, p0 & lo
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def split_u64(v):
    """(low word, high word) of uint64 values."""
    v = _u64(v)
    return v & np.uint64(MASK32), v >> np.uint64(32)


def philox4x32_10(counter_u64, key_u64):
    """The form the device uses: counter = (low, high, 0, 0) of a 64-bit group number, key = (low, high) of the 64-bit
    seed.  Arrays (or scalars) of uint64 -> (n, 4) uint32."""
    c_lo, c_hi = split_u64(counter_u64)
    k_lo, k_hi = split_u64(key_u64)
    c_lo, c_hi, k_lo, k_hi = np.broadcast_arrays(c_lo, c_hi, k_lo, k_hi)
    zero = np.zeros_like(c_lo)
    return philox4x32_10_general(np.stack([c_lo, c_hi, zero, zero], -1), np.stack([k_lo, k_hi], -1))


def u01(words):
    """The top 24 bits of each word as a float32 in [0, 1): exact, 2^-24 granularity."""
    return (np.asarray(words, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def scale_of(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


def factors(seed, first_group, n, p, chunk=1 << 20):
    """float32[n]: element i is float32(1) / (float32(1) - float32(p)) if word i % 4 of group first_group + i // 4 gives
    u01 >= float32(p), else 0.  `first_group` is taken mod 2^64."""
    n = int(n)
    out = np.empty(n, dtype=np.float32)
    groups = (n + 3) // 4
    p32, s = np.float32(p), scale_of(p)
    seed = int(seed) & MASK64
    for g0 in range(0, groups, chunk):
        g1 = min(groups, g0 + chunk)
        first = (int(first_group) + g0) & MASK64
        # uint64 addition wraps mod 2^64 like the device's
        ctr = np.uint64(first) + np.arange(g1 - g0, dtype=np.uint64)
        keep = u01(philox4x32_10(ctr, np.uint64(seed))).reshape(-1) >= p32
        lo, hi = 4 * g0, min(n, 4 * g1)
        out[lo:hi] = np.where(keep[:hi - lo], s, np.float32(0))
    return out


class Stream:
    """The bookkeeping of hip_ops.norm_act._Philox on the host: a draw of n elements takes ceil(n / 4) groups."""

    def __init__(self, seed, stream_id=0, offset=0):
        self.base_seed, self.stream_id, self.offset = int(seed), int(stream_id), int(offset)

    def seed(self):
        return (self.base_seed + GOLDEN64 * self.stream_id) & MASK64

    def draw(self, n, p):
        out = factors(self.seed(), self.offset, n, p)
        self.offset += (int(n) + 3) // 4
        return out
