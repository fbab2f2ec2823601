"""Parameter sets of the sampler known-answer tests (tests/test_gpu_sampler_kat.py; the collision test of tests/test_sampler_model.py uses the largest): the
smallest that reach every path of device key generation and encryption.

  A  N = 1024,  36/36/37 bit   FP64 with 22-bit limbs (POL_F64L), three limbs, four relinearisation digits per limb, Galois keys, a level context
  B  N = 2048,  2 x 48 bit     FP64 (POL_F64), three relinearisation digits per limb
  C  N = 4096,  2 x 55 bit     the integer policy (no FP64 form at 50 bits and more); also run with "f64" = 0 forced
  D  N = 8192,  2 x 40 bit     "ks_xi" = 1: the message factor (q / q_l) 2^(dbc d), two digits per limb
  E  N = 16384, 2 x 48 bit     the largest block indices (2048 blocks per limb), one 1024-thread workgroup per transform, Galois keys

The plain modulus is a batching prime of the ring (1 mod 2N)."""
from test_oracle_math import is_prime


def ntt_primes(bits, n, count, avoid=()):
    """the `count` largest primes below 2^bits that are 1 mod 2n and not in `avoid`, decreasing (as in tests/test_gpu_wide_moduli.py)"""
    out, x = [], ((1 << bits) - 1) // (2 * n) * (2 * n) + 1
    while len(out) < count:
        if x not in avoid and is_prime(x):
            out.append(x)
        x -= 2 * n
    for p in out:
        assert is_prime(p) and p.bit_length() == bits and p % (2 * n) == 1, hex(p)
    return out


TINY_Q = [0xffffee001, 0xffffc4001, 0x1ffffe0001]

CASES = {
    "A": dict(n=1024, t=12289, q=TINY_Q, dbc=10, gdbc=20, galois=True, ks_xi=0),
    "B": dict(n=2048, t=12289, q=ntt_primes(48, 2048, 2), dbc=20, gdbc=60, galois=False, ks_xi=0),
    "C": dict(n=4096, t=40961, q=ntt_primes(55, 4096, 2), dbc=60, gdbc=60, galois=False, ks_xi=0),
    "D": dict(n=8192, t=557057, q=ntt_primes(40, 8192, 2), dbc=30, gdbc=60, galois=False, ks_xi=1),
    "E": dict(n=16384, t=957181001729, q=ntt_primes(48, 16384, 2), dbc=60, gdbc=60, galois=True, ks_xi=0),
}
for _c in CASES.values():
    assert is_prime(_c["t"]) and _c["t"] % (2 * _c["n"]) == 1


def make_oracle(case, limbs=None):
    from oracle.cno import Oracle
    return Oracle(case["n"], case["t"], q=case["q"][:limbs] if limbs else case["q"], dbc=case["dbc"], gdbc=case["gdbc"], ks_xi=bool(case["ks_xi"]))
