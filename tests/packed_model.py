"""Big-integer statement of the packed row format (include/cnhip.h: cn_packed_words): the row of the residues v_0 .. v_(n-1) in `bits` bits each is the
integer sum_i v_i 2^(i bits), cut into little-endian 64-bit words.  Plain Python integers - the model the vectorised codecs and the kernels are
tested against."""
import numpy as np

MASK64 = (1 << 64) - 1


def pack_row_big(values, bits):
    n = len(values)
    assert (n * bits) % 64 == 0
    big = 0
    for i, v in enumerate(values):
        assert 0 <= int(v) < 1 << bits
        big |= int(v) << (i * bits)
    return np.array([(big >> (64 * w)) & MASK64 for w in range(n * bits // 64)], dtype=np.uint64)


def unpack_row_big(words, bits, n):
    big = 0
    for w, x in enumerate(words):
        big |= int(x) << (64 * w)
    return np.array([(big >> (i * bits)) & ((1 << bits) - 1) for i in range(n)], dtype=np.uint64)


def packed_words(n, q, polys):
    """cn_packed_words: polys * (n / 64) * sum_j bit_length(q_j)"""
    return polys * (n // 64) * sum(int(x).bit_length() for x in q)


def random_words(rng, q, n, count, polys):
    """uint64 [count, polys * k * n]: canonical residues, limb j below q_j, with 0 and q_j - 1 at the ends of the rows of the first two ciphertexts"""
    w = np.stack([rng.integers(0, qj, size=(count, polys, n), dtype=np.uint64) for qj in q], axis=2)
    for j, qj in enumerate(q):
        w[0, :, j, 0], w[0, :, j, -1] = 0, qj - 1
        if count > 1:
            w[1, :, j, 0], w[1, :, j, -1] = qj - 1, 0
    return w.reshape(count, -1)
