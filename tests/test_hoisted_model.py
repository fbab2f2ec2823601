"""The word contract of the hoisted rotations, proved without a GPU (tests/hoisted_model.py): the permutation identity the kernels rely on, against the oracle's
transform; the model's output decrypts under the oracle to the plaintext of Oracle.apply_galois; its noise stays below the decryption bound.
N = 1024, k = 2 and 3, digit widths 60 and 10, both key-switch conventions; a row step, a negative step and the column swap."""
import numpy as np
import pytest

from hoisted_model import automorphism, hoisted, perm_index
from modswitch_model import crt_compose
from oracle.cno import Oracle
from size_policy_sets import Q, T

N = 1024
STEPS = (4, -2, 0)                                          # 0: the column swap (element 2N - 1)


def make(k, width, xi):
    o = Oracle(N, T, q=Q["f64"][:k], dbc=width, gdbc=width, ks_xi=xi)
    o.keygen(41 + k, galois=True)
    return o


@pytest.mark.parametrize("g", [3, 5, 2 * N - 1, 3 ** 7 % (2 * N), pow(3, -5, 2 * N)])
def test_automorphism_permutes_the_transform_without_a_sign(g):
    """NTT_j(s_g(a)) = P_g(NTT_j(a)) for random polynomials, every limb of a three-prime set (one of 60 bits)"""
    rng = np.random.default_rng(g)
    o = Oracle(N, T, q=[Q["u64"][0], Q["f64"][0], Q["f64l"][2]], dbc=60, gdbc=60)
    src = perm_index(N, g)
    assert sorted(src) == list(range(N))
    for j, m in enumerate(o.q):
        a = rng.integers(0, m, size=N, dtype=np.uint64)
        assert np.array_equal(o.ntt_fwd(j, automorphism(a, g, m)), o.ntt_fwd(j, a)[src])
    # neighbours stay neighbours (swapped or not): what lets a kernel gather 16 bytes at a time
    assert all(src[p + 1] == src[p] ^ 1 for p in range(0, N, 2))


@pytest.mark.parametrize("xi", [False, True])
@pytest.mark.parametrize("width", [60, 10])
@pytest.mark.parametrize("k", [2, 3])
def test_model_decrypts_to_the_rotation_with_noise_below_the_bound(k, width, xi):
    o = make(k, width, xi)
    rng = np.random.default_rng(100 * k + width + xi)
    ct = o.encrypt(o.encode(rng.integers(0, T, size=N, dtype=np.uint64)))
    have = o.galois_elts()
    Qp = 1
    for m in o.q:
        Qp *= m
    for s in STEPS:
        g = o.galois_elt_from_step(s)
        ref = o.apply_galois(ct, g)
        got = hoisted(o, ct, g, o.galois_key(have.index(g)), ks_xi=xi)
        assert np.array_equal(o.decrypt(got), o.decrypt(ref)), (k, width, xi, s)
        # invariant noise t (c0 + c1 s) mod q, centred: decryption is right while it stays below q / 2; the hoisted sum runs over the same digits and key errors as
        # SEAL's, so it may take no more than a bit beyond it
        norm = []
        for words in (got, ref):
            x = o.dot_with_secret(words).reshape(o.k, N)
            v = [crt_compose([int(x[j, i]) * T % o.q[j] for j in range(o.k)], o.q) for i in range(N)]
            norm.append(max(min(c, Qp - c) for c in v))
        assert norm[0] < Qp // 2 and norm[0].bit_length() <= norm[1].bit_length() + 1, (k, width, xi, s, norm)
    assert np.array_equal(hoisted(o, ct, 1, None), ct)       # element 1: the ciphertext itself


def test_dense_path_counts_with_hoisted_baby_steps():
    """diagonal.dense_path_counts(..., hoisted=True) at the LoLa-CIFAR layer (N = 16384, k = 8, one digit per limb, B = 128): the 127 baby steps cost
    64 + 127 x 16 = 2 096 limb transforms instead of 127 x (64 + 16) = 10 160; nothing else of the count moves, and the default (hoisted=False) is unchanged"""
    from cryptonets_amd import diagonal
    args = (5488, 16268, 16384, 8, 8)
    plain, hoist = diagonal.dense_path_counts(*args, B=128), diagonal.dense_path_counts(*args, B=128, hoisted=True)
    assert plain == diagonal.dense_path_counts(*args, B=128, hoisted=False) and plain["babies"] == 128
    assert plain["diagonal"] - hoist["diagonal"] == 10160 - 2096
    assert {k: v for k, v in plain.items() if k != "diagonal" and k != "choice"} == {k: v for k, v in hoist.items() if k != "diagonal" and k != "choice"}
    # a layer with one baby step has nothing to hoist
    one = (3, 1000, 1024, 3, 6)
    assert diagonal.dense_path_counts(*one, B=1, hoisted=True) == diagonal.dense_path_counts(*one, B=1)
