"""Host model, in plain integers, of what k_digit_gemm_mfma computes: the two-piece int8 split of a key-switch digit, the signed byte digits of a weight
(pack_gemm_mfma), the P + 1 diagonals of their products and the fold back to S = sum_k w_k dig_k - and the bounds the plan relies on (cn_gemm_plan.h)."""
import numpy as np
import pytest


def split(dg):
    """dg = lo + 256 hi with lo in -128..127: the kernel's bytes of t = dg + 128, byte 0 flipped in its top bit and read as int8"""
    t = dg + 128
    lo = np.uint8((t & 255) ^ 0x80).astype(np.int8).astype(np.int64) if isinstance(t, np.ndarray) else int(np.int8(np.uint8((t & 255) ^ 0x80)))
    return lo, t >> 8


def planes(w, P):
    """signed base-256 digits of a weight, as pack_gemm_mfma recodes them"""
    rec = ((w + 0x808080) & 0xFFFFFFFF) ^ 0x808080
    return [int(np.int8(np.uint8((rec >> (8 * p)) & 255))) for p in range(P)]


@pytest.mark.parametrize("dbc", range(1, 15))
def test_every_digit_splits_into_two_int8_pieces(dbc):
    dg = np.arange(1 << dbc, dtype=np.int64)
    lo, hi = split(dg)
    assert np.array_equal(lo + 256 * hi, dg)
    assert lo.min() >= -128 and lo.max() <= 127 and hi.min() >= 0 and hi.max() <= 64


def test_fifteen_bits_do_not_fit():
    assert split(np.array([(1 << 15) - 1], dtype=np.int64))[1].max() > 127


@pytest.mark.parametrize("P,wmax", [(1, 127), (2, 32639), (3, (1 << 20) - 1)])
def test_diagonals_fold_to_the_weighted_digit_sum(P, wmax):
    rng = np.random.default_rng(P)
    for dbc in (7, 10, 14):
        K = 64
        w = [int(x) for x in rng.integers(-wmax, wmax + 1, size=K)]
        w[:4] = [wmax, -wmax, min(wmax, 128), -min(wmax, 128)]
        dg = [int(x) for x in rng.integers(0, 1 << dbc, size=K)]
        dg[:2] = [(1 << dbc) - 1, 0]
        acc = [0] * (P + 1)
        for wk, dk in zip(w, dg):
            wp = planes(wk, P)
            assert sum(d << (8 * p) for p, d in enumerate(wp)) == wk and all(-128 <= d <= 127 for d in wp)
            lo, hi = split(dk)
            for p in range(P):
                acc[p] += lo * wp[p]
                acc[p + 1] += hi * wp[p]
        assert sum(a << (8 * j) for j, a in enumerate(acc)) == sum(wk * dk for wk, dk in zip(w, dg))


def test_accumulator_and_fold_bounds():
    """i32 diagonals at the largest K (3 K < 2^17) and exact FP64 partial sums of the fold for any such diagonals"""
    K = ((1 << 17) - 1) // 3
    assert 3 * K < 1 << 17 <= 3 * (K + 1)
    per_term = 128 * 128 + 64 * 128                  # one lo x w_p and one hi x w_(p-1) product share a diagonal
    assert K * per_term < 1 << 31
    top = K * 64 * 128                               # the top diagonal holds hi x w_(P-1) products only
    i32 = (1 << 31) - 1
    assert i32 * (1 + 256 + 65536) < 1 << 53         # P <= 2: three diagonals of any i32 values
    assert i32 * (1 + 256 + 65536) + (top << 24) < 1 << 53      # P = 3
