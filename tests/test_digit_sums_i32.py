"""Digit sums as int32 words ("digit_i32"): cn_square_gemm and cn_mul_relin_sum hand their key switch S[output][digit][N] as 32-bit words where the plan's digit
bound max_o sum_k |w_ok| (2^dbc - 1) is at most 2^31 - 1, as doubles otherwise.  The ciphertext words must not move: every case is compared word for word with the
CPU oracle (Multiply + Relinearize per input, then the scalar GEMM) and with the same call under "digit_i32" = 0; "ks_digits_i32" reads back which form the key
switch took, "square_gemm_fused" / "mul_sum_fused" that the one-key-switch-per-output form ran at all.

Shapes - the smallest at which these kernels can go wrong:
  * N = 1024 and 4096 with k = 2 and 3 limbs of 37, (37,) 36 bits at dbc 9: the last limb has 4 digits, the others 5.  K = 1, 3, 33 inputs (33: one past a 32-wide K
    step of the matrix-core digit GEMM, more than two sets of four of the FP64 one), M = 1, 16, 33 outputs (1: the two-output tile of k_digit_gemm; 16 and 33: the
    matrix-core form, one tile and a second one with a single row).  Every case runs the fused key switch and both two-launch forms ("ks_wide" 0, 1, 2).
  * signs: rows (+w, -w, -v) that gather the inputs (A, A, B) make S = -v dig(B) - never positive, zero where the digit is zero - and a row of the opposite sign; the test
    checks on the oracle's product that both negative and zero words occur.
  * the bound itself at dbc = 1, the only digit width at which sum |w| (2^dbc - 1) takes both 2^31 - 1 and 2^31 (2^31 - 1 is prime): 2048 weights of 2^20 - 1 and
    one of 2047 (2048) over three inputs; a coefficient whose bit is set in all three products makes |S| the bound itself, with either sign.
  * cn_mul_relin_sum (k_product_sum) at N = 1024 with K = 2 and 9.
  * the two-launch forms with 1 and 10 outputs and one case of 8 inputs and 4 outputs at the workload's ring (N = 8192, k = 5, dbc 10).
The references (oracle squarings) are computed once per parameter set and shared.
"""
import numpy as np
import pytest

from conftest import PARAMS
from test_gpu_mul_relin_sum import expected as sum_expected, operands, upload
from test_oracle_math import is_prime
from test_square_gemm import fresh_context, inputs, res

pytestmark = pytest.mark.gpu

P36 = 0xffffee001                                                    # 36 bits, 1 mod 8192 (the "tiny" set)


def plain_prime():
    """the smallest prime above 2^21 that is 1 mod 8192: weights up to 2^20 - 1 in magnitude are residues below t / 2, and t is below every modulus"""
    p = (1 << 21) + 1
    while not is_prime(p):
        p += 8192
    return p


T22 = plain_prime()


def primes_37():
    """the two largest 37-bit primes that are 1 mod 8192"""
    out, p = [], (1 << 37) - 8192 + 1
    while len(out) < 2:
        if is_prime(p):
            out.append(p)
        p -= 8192
    return out


P37 = primes_37()
assert all(p.bit_length() == 37 for p in P37) and P36.bit_length() == 36
SETS = {(n, k): dict(n=n, t=T22, q=P37[:k - 1] + [P36], dbc=9, gdbc=20) for n in (1024, 4096) for k in (2, 3)}
SETS["bound"] = dict(n=1024, t=T22, q=[P37[0], P36], dbc=1, gdbc=20)


class Case:
    """oracle, device context, `count` uploaded inputs and their oracle squarings (relinearised) of one parameter set"""

    def __init__(self, p, count, seed, shared=None):
        from cryptonets_amd._native import Context
        from oracle.cno import Oracle
        if shared is None:
            self.o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
            self.o.keygen(11, galois=False)
            self.g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
            self.g.set_relin_key(self.o.relin_key())
        else:
            self.o, self.g = shared
        self.X = inputs(self.o, count, seed)
        self.sq = self.o.mul_relin_batch(self.X, self.X)
        self.h = self.g.ct_alloc(count)
        self.g.ct_upload(self.h, 0, self.X)

    def close(self):
        self.g.close()

    def run(self, W, idx=None, i32=1, ks_wide=-1):
        """cn_square_gemm of the plan (W, idx) over the inputs -> (words, what the counters say)"""
        g, O = self.g, W.shape[0]
        g.set_option("digit_i32", i32)
        g.set_option("ks_wide", ks_wide)
        plan, out = g.gemm_plan(W, idx=idx), g.ct_alloc(O)
        before = {c: g.get_option(c) for c in ("square_gemm_fused", "ks_digits_i32", "digit_gemm_mfma")}
        g.stats(reset=True)
        g.square_gemm(plan, self.h, 0, out, 0)
        launches = g.stats()["kernel_launches"]
        words = g.ct_download(out, 0, O)
        info = {c: g.get_option(c) - v for c, v in before.items()}
        info["launches"] = launches
        g.free(plan)
        g.free(out)
        g.set_option("digit_i32", 1)
        g.set_option("ks_wide", -1)
        return words, info

    def expected(self, W, idx=None):
        return self.o.scalar_gemm(self.sq, W, idx)


@pytest.fixture(scope="module", params=sorted(k for k in SETS if k != "bound"), ids=lambda k: "n%d-k%d" % k)
def ring(request):
    c = Case(SETS[request.param], 33, 0x132)
    yield c
    c.close()


# ------------------------------------------------------------------ 1. the shape matrix
@pytest.mark.parametrize("K", [1, 3, 33])
@pytest.mark.parametrize("M", [1, 16, 33])
def test_shape_matrix_gives_the_oracles_words_in_every_key_switch_form(ring, K, M):
    c = ring
    assert [int(x) for x in (c.g.get_option("digit_i32"), c.g.get_option("ks_wide"))] == [1, -1]
    rng = np.random.default_rng(0xD132 + 64 * K + M)
    # int32 bound at dbc 9: sum |w| 511 <= 2^31 - 1, sum |w| <= 4 202 495
    wmax = (1 << 20) - 1 if K <= 3 else 127000
    assert K * wmax * 511 <= 2 ** 31 - 1
    W = rng.integers(-wmax, wmax + 1, size=(M, K))
    W[W == 0] = 1
    W[0, :] = wmax                                                   # the largest row sum, and its negative
    W[-1, :] = -wmax
    idx = np.tile(rng.permutation(33)[:K].astype(np.int32), (M, 1))  # K of the 33 inputs
    Wr = res(W, c.o.t)
    exp = c.expected(Wr, idx)
    ref, info0 = c.run(Wr, idx, i32=0, ks_wide=0)
    assert info0["square_gemm_fused"] == 1 and info0["ks_digits_i32"] == 0
    assert np.array_equal(ref, exp)
    for ks_wide in (0, 1, 2):
        got, info = c.run(Wr, idx, i32=1, ks_wide=ks_wide)
        assert info["square_gemm_fused"] == 1 and info["ks_digits_i32"] == 1, (ks_wide, info)
        assert info["digit_gemm_mfma"] == (1 if M >= 16 else 0), info
        assert info["launches"] == info0["launches"] + (1 if ks_wide else 0), (ks_wide, info, info0)      # a two-launch key switch is one launch more
        assert np.array_equal(got, exp), "ks_wide %d" % ks_wide
        assert np.array_equal(got, ref)


# ------------------------------------------------------------------ 2. signs and zeros
@pytest.fixture(scope="module")
def signs():
    c = Case(SETS[(1024, 3)], 6, 0x51A)                              # (inputs 0 .. 2 hold edge residues, 3 .. 5 are uniform)
    yield c
    c.close()


def digit_words(o, d2):
    """digits [tot][N] of component 2 of a product, limbs in order"""
    out, mask = [], (1 << o.dbc) - 1
    for j, qj in enumerate(o.q):
        for d in range(-(-qj.bit_length() // o.dbc)):
            out.append(((d2[j] >> np.uint64(o.dbc * d)) & np.uint64(mask)).astype(np.int64))
    return np.stack(out)


@pytest.mark.parametrize("ks_wide", [0, 1, 2])
def test_negative_and_zero_digit_sums(signs, ks_wide):
    c = signs
    o = c.o
    w, v = 1000003, 1048573                                          # sum |w| 511 = 1.56e9 <= 2^31 - 1; |S| up to 5.4e8
    W = np.array([[w, -w, -v], [-w, w, v], [3, 5, -7]], dtype=np.int64)
    src = [3, 3, 5]                                                  # every row gathers (A, A, B)
    idx = np.tile(np.array(src, dtype=np.int32), (3, 1))
    D = [digit_words(o, o.multiply(c.X[i], c.X[i]).reshape(3, o.k, o.n)[2]) for i in src]
    S = [sum(int(W[r, i]) * D[i] for i in range(3)) for r in range(3)]
    assert np.array_equal(S[0], -v * D[2]) and (S[0] < 0).any() and (S[0] == 0).any() and not (S[0] > 0).any()
    assert (S[1] > 0).any() and (S[2] < 0).any() and (S[2] > 0).any()
    assert max(int(np.abs(s).max()) for s in S) <= 2 ** 31 - 1
    Wr = res(W, c.o.t)
    exp = c.expected(Wr, idx)
    got, info = c.run(Wr, idx, i32=1, ks_wide=ks_wide)
    ref, info0 = c.run(Wr, idx, i32=0, ks_wide=ks_wide)
    assert (info["square_gemm_fused"], info["ks_digits_i32"], info0["square_gemm_fused"], info0["ks_digits_i32"]) == (1, 1, 1, 0)
    assert np.array_equal(got, exp) and np.array_equal(ref, exp)


# ------------------------------------------------------------------ 3. the bound itself
@pytest.fixture(scope="module")
def bound():
    c = Case(SETS["bound"], 6, 0xB0D)                                # (inputs 0 .. 2 hold edge residues, 3 .. 5 are uniform)
    yield c
    c.close()


@pytest.mark.parametrize("last,i32", [(2047, 1), (2048, 0)])
def test_a_plan_at_2_31_minus_1_takes_int32_and_one_at_2_31_takes_doubles(bound, last, i32):
    c = bound
    o = c.o
    K, big = 2049, (1 << 20) - 1
    row = np.full(K, big, dtype=np.int64)
    row[-1] = last
    assert int(row.sum()) * (2 ** o.dbc - 1) == (2 ** 31 - 1 if i32 else 2 ** 31)
    W = np.stack([row, -row])
    idx = np.tile(3 + np.arange(K, dtype=np.int32) % 3, (2, 1))
    # a coefficient whose bit is set in all three products: |S| is the bound itself there
    D = [digit_words(o, o.multiply(c.X[i], c.X[i]).reshape(3, o.k, o.n)[2]) for i in (3, 4, 5)]
    assert (D[0] & D[1] & D[2]).any()
    Wr = res(W, c.o.t)
    exp = c.expected(Wr, idx)
    got, info = c.run(Wr, idx, i32=1, ks_wide=0)
    assert info["square_gemm_fused"] == 1 and info["ks_digits_i32"] == i32, info
    assert np.array_equal(got, exp)
    ref, info0 = c.run(Wr, idx, i32=0, ks_wide=0)
    assert info0["square_gemm_fused"] == 1 and info0["ks_digits_i32"] == 0
    assert np.array_equal(ref, exp)


# ------------------------------------------------------------------ 4. cn_mul_relin_sum (k_product_sum)
@pytest.fixture(scope="module")
def tiny():
    o, g = fresh_context("tiny")
    yield o, g
    g.close()


@pytest.mark.parametrize("K,count,b_stride", [(2, 1, 0), (9, 2, 1)])
def test_mul_relin_sum_words(tiny, K, count, b_stride):
    o, g = tiny
    A, B = operands(o, K, count, b_stride, 0x932 + K)
    exp = sum_expected(o, A, B, b_stride)
    ha, hb = [upload(g, A[k]) for k in range(K)], [upload(g, B[k]) for k in range(K)]
    out = g.ct_alloc(count)
    try:
        for i32 in (1, 0):
            g.set_option("digit_i32", i32)
            before = (g.get_option("mul_sum_fused"), g.get_option("ks_digits_i32"))
            g.mul_relin_sum(ha, None, hb, None, b_stride, out, 0, count)
            step = (g.get_option("mul_sum_fused") - before[0], g.get_option("ks_digits_i32") - before[1])
            assert step == (1, i32), step
            assert np.array_equal(g.ct_download(out, 0, count), exp), "digit_i32 %d" % i32
    finally:
        g.set_option("digit_i32", 1)
        for h in ha + hb + [out]:
            g.free(h)


# ------------------------------------------------------------------ 5. the workload's ring
@pytest.fixture(scope="module")
def c3():
    o, g = fresh_context("c3")
    c = Case(PARAMS["c3"], 8, 0xC32, shared=(o, g))
    yield c
    c.close()


def c3_weights(O, seed, t=PARAMS["c3"]["t"]):
    rng = np.random.default_rng(seed)
    W = rng.integers(-200000, 200001, size=(O, 8))                   # sum |w| 1023 <= 8 x 200 000 x 1023 < 2^31
    W[W == 0] = 1
    W[0, :] = 200000
    return res(W, t)


def test_workload_ring_eight_inputs_four_outputs(c3):
    c = c3
    assert (c.o.n, c.o.k, c.o.dbc) == (8192, 5, 10)
    W = c3_weights(4, 0xC34)
    exp = c.expected(W)
    ref, info0 = c.run(W, i32=0, ks_wide=0)
    assert info0["square_gemm_fused"] == 1 and info0["ks_digits_i32"] == 0 and np.array_equal(ref, exp)
    for ks_wide in (0, -1):                                          # the fused kernel of the 100-output layer; what the library picks for 4 outputs
        got, info = c.run(W, i32=1, ks_wide=ks_wide)
        assert info["square_gemm_fused"] == 1 and info["ks_digits_i32"] == 1
        assert np.array_equal(got, exp)


@pytest.mark.parametrize("O", [1, 10])
@pytest.mark.parametrize("ks_wide,form", [(1, "k_ks_digit_mac"), (2, "k_ks_limb_mac")])
def test_two_launch_forms_with_1_and_10_outputs(c3, O, ks_wide, form):
    """the form is the one "ks_wide" names unless the partial products do not fit the scratch limit - then it is the fused kernel, one launch less: read from
    "kernel_launches" against the same call under "ks_wide" = 0"""
    c = c3
    W = c3_weights(O, 0xC30 + O)
    exp = c.expected(W)
    fused, info0 = c.run(W, i32=1, ks_wide=0)
    got, info = c.run(W, i32=1, ks_wide=ks_wide)
    assert info["launches"] == info0["launches"] + 1, (form, info, info0)
    assert info["square_gemm_fused"] == 1 and info["ks_digits_i32"] == 1
    assert np.array_equal(got, exp) and np.array_equal(fused, exp)
    ref, info1 = c.run(W, i32=0, ks_wide=ks_wide)
    assert info1["launches"] == info["launches"] and info1["ks_digits_i32"] == 0
    assert np.array_equal(ref, exp)
