"""CPU: the packed row codecs of cryptonets_amd.serialization (pack_rows / unpack_rows) against the big-integer statement of the format
(tests/packed_model.py), and the word count formula of cn_packed_words for the suite's parameter sets."""
import numpy as np
import pytest

import packed_model as pm
from conftest import PARAMS
from cryptonets_amd import serialization as ser

WIDTHS = (2, 30, 36, 37, 43, 44, 48, 49, 59, 60)


def rows(bits, n, rng):
    """random rows, and rows that hold 0 and 2^bits - 1 in the first and last coefficient"""
    top = (1 << bits) - 1
    v = rng.integers(0, top + 1, size=(5, n), dtype=np.uint64)
    v[1, 0], v[1, -1] = 0, top
    v[2, 0], v[2, -1] = top, 0
    v[3, :] = top
    v[4, :] = 0
    return v


@pytest.mark.parametrize("n", [64, 1024])
@pytest.mark.parametrize("bits", WIDTHS)
def test_pack_and_unpack_rows_against_the_big_integer_statement(bits, n, rng):
    v = rows(bits, n, rng)
    p = ser.pack_rows(v, bits)
    assert p.shape == (5, n * bits // 64) and p.dtype == np.uint64
    for r in range(v.shape[0]):
        assert np.array_equal(p[r], pm.pack_row_big(v[r], bits)), (bits, n, r)
        assert np.array_equal(ser.unpack_rows(p[r], bits, n), pm.unpack_row_big(p[r], bits, n)), (bits, n, r)
    assert np.array_equal(ser.unpack_rows(p, bits, n), v)                      # round trip, batched
    assert np.array_equal(ser.pack_rows(v.reshape(5, 1, n), bits), p.reshape(5, 1, -1))


def test_unpack_rows_of_arbitrary_words(rng):
    """every word pattern is a row: the unpacked values are those of the statement (they may exceed a modulus - the device reduces and reports)"""
    for bits in (36, 43, 60):
        p = rng.integers(0, 1 << 64, size=(2, 1024 * bits // 64), dtype=np.uint64)
        p[1, :] = pm.MASK64
        got = ser.unpack_rows(p, bits, 1024)
        for r in range(2):
            assert np.array_equal(got[r], pm.unpack_row_big(p[r], bits, 1024))
        assert np.array_equal(ser.pack_rows(got, bits), p)


def test_codecs_refuse_what_is_not_a_row():
    with pytest.raises(ValueError):
        ser.pack_rows(np.array([[4] + [0] * 63], dtype=np.uint64), 2)          # 4 does not fit 2 bits
    with pytest.raises(ValueError):
        ser.pack_rows(np.zeros((1, 64), dtype=np.uint64), 61)
    with pytest.raises(ValueError):
        ser.pack_rows(np.zeros((1, 33), dtype=np.uint64), 36)                  # not whole words
    with pytest.raises(ValueError):
        ser.unpack_rows(np.zeros((1, 35), dtype=np.uint64), 36, 64)


def resolved_q(name):
    q = PARAMS[name]["q"]
    if q is None:                      # CoeffModulus128(8192) of SEAL 3.2: 43, 43, 44, 44, 44 bits (218 of 320)
        assert name == "c3"
        q = [0x7fffffd8001, 0x7fffffc8001, 0xfffffffc001, 0xffffff6c001, 0xfffffebc001]
    return q


@pytest.mark.parametrize("name,bits,words", [("tiny", [36, 36, 37], 1744), ("c3", [43, 43, 44, 44, 44], 27904), ("c5", [48, 48, 48, 49, 49, 49, 49, 49], 99584)])
def test_packed_words_formula(name, bits, words):
    """words of one packed polynomial, as literals: 16 * 109, 128 * 218, 256 * 389"""
    n, q = PARAMS[name]["n"], resolved_q(name)
    assert ser.packed_bits(q) == bits
    for polys in (1, 2, 3):
        assert pm.packed_words(n, q, polys) == polys * words
    w = np.zeros((2, 2 * len(q) * n), dtype=np.uint64)
    assert ser.pack_ciphertexts(w, q, n).shape == (2, pm.packed_words(n, q, 2))


def test_pack_ciphertexts_row_order(rng):
    """[poly][limb] rows, each the statement's row"""
    q, n = PARAMS["tiny"]["q"], 1024
    w = pm.random_words(rng, q, n, 2, 3)
    p = ser.pack_ciphertexts(w, q, n)
    off = 0
    for poly in range(3):
        for j, qj in enumerate(q):
            b = qj.bit_length()
            for c in range(2):
                assert np.array_equal(p[c, off:off + n * b // 64], pm.pack_row_big(w[c].reshape(3, 3, n)[poly, j], b))
            off += n * b // 64
    assert off == p.shape[1]
    assert np.array_equal(ser.unpack_ciphertexts(p, q, n, 3), w)
