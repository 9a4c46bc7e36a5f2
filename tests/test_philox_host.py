"""The host Philox reference (tests/philox_ref.py) against published known answers, and its own bookkeeping.  The GPU
tests (tests/test_gpu_dropout.py) hold every dropout kernel to this reference bit for bit, so it has to be right by
something other than agreement with the kernels."""
import numpy as np
import pytest

from tests import philox_ref as R

# known-answer vectors of philox4x32_10 (Random123's kat_vectors): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,out", KAT, ids=["zeros", "ones", "pi"])
def test_general_form_known_answers(counter, key, out):
    got = R.philox4x32_10_general(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert [int(v) for v in got] == list(out)


def test_general_form_is_elementwise_over_arrays():
    c = np.array([k[0] for k in KAT], dtype=np.uint64)
    k = np.array([k[1] for k in KAT], dtype=np.uint64)
    got = R.philox4x32_10_general(c, k)
    assert np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint32))


def test_u64_form_splits_counter_and_key_low_high():
    """counter -> (low, high, 0, 0), key -> (low, high): with a counter >= 2^32 and a key >= 2^32, against the general
    form called with the words written out."""
    cases = [(0, 0), (5, 7), (2 ** 32, 3), (2 ** 32 + 9, 2 ** 32 + 1), (0xFEDCBA9876543210, 0x0123456789ABCDEF),
             (2 ** 64 - 1, 2 ** 64 - 1)]
    for ctr, key in cases:
        words = R.philox4x32_10(np.uint64(ctr), np.uint64(key))
        assert words.shape == (1, 4) and words.dtype == np.uint32
        want = R.philox4x32_10_general(np.array([ctr & 0xFFFFFFFF, ctr >> 32, 0, 0], dtype=np.uint64),
                                       np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint64))
        assert np.array_equal(words[0], want), (hex(ctr), hex(key))
    # the first known answer is the u64 form at (0, 0); the high words matter
    assert [int(v) for v in R.philox4x32_10(np.uint64(0), np.uint64(0))[0]] == list(KAT[0][2])
    assert not np.array_equal(R.philox4x32_10(np.uint64(2 ** 32), np.uint64(0)), R.philox4x32_10(np.uint64(0), np.uint64(0)))
    assert not np.array_equal(R.philox4x32_10(np.uint64(0), np.uint64(2 ** 32)), R.philox4x32_10(np.uint64(0), np.uint64(0)))
    # an array of counters is the stack of the scalar calls
    ctrs = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1], dtype=np.uint64)
    stacked = R.philox4x32_10(ctrs, np.uint64(2 ** 40 + 17))
    for i, c in enumerate(ctrs):
        assert np.array_equal(stacked[i], R.philox4x32_10(c, np.uint64(2 ** 40 + 17))[0])


def test_u01_is_the_top_24_bits():
    w = np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFFFF], dtype=np.uint32)
    u = R.u01(w)
    assert u.dtype == np.float32
    assert u.tolist() == [0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]


def test_factors_follow_the_words():
    seed, first, n, p = 2 ** 40 + 3, 2 ** 32 - 1, 11, 0.3
    f = R.factors(seed, first, n, p)
    assert f.dtype == np.float32 and f.shape == (n,)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    for i in range(n):
        word = R.philox4x32_10(np.uint64(first + i // 4), np.uint64(seed))[0, i % 4]
        keep = np.float32(int(word) >> 8) * np.float32(2.0 ** -24) >= np.float32(p)
        assert f[i] == (scale if keep else np.float32(0)), i
    # the chunked evaluation is the unchunked one
    assert np.array_equal(R.factors(seed, first, 1023, p, chunk=7), R.factors(seed, first, 1023, p))
    # the tail group has words of its own: not those of group 0
    assert np.array_equal(R.factors(seed, 0, 5, p)[4:], R.factors(seed, 1, 1, p))


def test_stream_bookkeeping():
    s = R.Stream(1234)
    t = R.Stream(1234)
    whole = R.factors(1234, 0, 4 * 260, 0.5)
    at = 0
    for n, adv in ((5, 2), (4, 1), (1, 1), (1023, 256)):
        before = s.offset
        f = s.draw(n, 0.5)
        assert s.offset - before == adv
        assert np.array_equal(f, whole[4 * at:4 * at + n])       # consecutive slices of one stream, group-aligned
        at += adv
    assert s.offset == 260 and t.offset == 0
    assert R.Stream(7, offset=12).draw(3, 0.5).tolist() == R.factors(7, 12, 3, 0.5).tolist()


def test_stream_seed_mix_wraps_mod_2_64():
    assert R.Stream(5).seed() == 5
    assert R.Stream(5, stream_id=1).seed() == 5 + 0x9E3779B97F4A7C15
    assert R.Stream(5, stream_id=3).seed() == (5 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64
    assert 3 * 0x9E3779B97F4A7C15 >= 2 ** 64                      # the case above really wraps
    a, b = R.Stream(5).draw(64, 0.5), R.Stream(5, stream_id=3).draw(64, 0.5)
    assert not np.array_equal(a, b)
