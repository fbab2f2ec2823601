"""cn_mul_plain_sum - out[g] = sum_e MultiplyPlain(ct[ct_idx[e]], pt[e]) over the terms of group g, in one call - word for word against the CPU oracle.

Modular arithmetic is exact and the results are canonical, so the call must write the words of the oracle's multiply_plain per term followed by add, in any
order.  The evaluator is a function of words: the ciphertexts are uniform residues with the edge words q - 1, 0 and q / 2 in the first three.

Shapes: the smallest register-radix ring (N = 1024) with 2 and 3 limbs under each arithmetic policy - 60/60/50-bit moduli (integer), 49/49/47-bit (FP64: the
accumulators recentre every other term) and 36/36/37-bit (FP64-light) - in G = 3 groups of 1, 5 and 17 terms that share ciphertexts, one plaintext with a single
non-zero coefficient, every handle used at an offset; 2 x 3 terms at N = 8192 and N = 16384 (the other two transform plans), at N = 16384 under the integer
policy and at N = 512 (no kernel: the composed calls); a level context; a recorded graph; the refusals.
"""
import numpy as np
import pytest

from conftest import PARAMS
from test_gpu_wide_moduli import TINY_Q, ntt_primes
from test_square_gemm import inputs

pytestmark = pytest.mark.gpu

T = 12289
Q_POLICY = {
    "u64": ntt_primes(60, 1024, 2) + ntt_primes(50, 1024, 1),
    "f64": ntt_primes(49, 1024, 2) + ntt_primes(47, 1024, 1),
    "f64l": TINY_Q,
}
CN_ERR_ARG, CN_ERR_ZERO = -1, -4


def pair(n, t, q, **opt):
    """(oracle, library context) over q: no keys - products with plaintexts and additions need none"""
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    o = Oracle(n, t, q=q, dbc=60, gdbc=60)
    g = Context(n, t, q=q, dbc=60, gdbc=60, device=0)
    for name, v in opt.items():
        g.set_option(name, v)
    return o, g


def plaintexts(o, rng, count):
    """dense plaintexts with every coefficient drawn from [0, t), the values t - 1 and t / 2 among them; the second has ONE non-zero coefficient"""
    P = rng.integers(0, o.t, size=(count, o.n), dtype=np.uint64)
    P[0, :3] = (o.t - 1, o.t // 2, o.t // 2 + 1)
    if count > 1:
        P[1] = 0
        P[1, 5] = o.t - 1
    return P


def expected(o, cts, pts, grp_off, ct_idx):
    out = []
    for g in range(len(grp_off) - 1):
        acc = None
        for e in range(grp_off[g], grp_off[g + 1]):
            p = o.multiply_plain(cts[ct_idx[e]], pts[e])
            acc = p if acc is None else o.add(acc, p)
        out.append(acc)
    return np.stack(out)


def run(o, g, grp_off, ct_idx, ncts, seed, ci=1, pi=2, oi=1):
    """one call with every handle used at an offset; asserts the oracle's words and that the neighbours of the outputs keep theirs"""
    rng = np.random.default_rng(seed)
    G, E = len(grp_off) - 1, grp_off[-1]
    cts, pts = inputs(o, ncts, seed), plaintexts(o, rng, E)
    sentinel = inputs(o, G + 2, seed + 1)
    hc, hp, ho = g.ct_alloc(ci + ncts), g.pt_alloc(pi + E), g.ct_alloc(oi + G + 1)
    try:
        g.ct_upload(hc, ci, cts)
        g.pt_upload(hp, pi, pts)
        g.ct_upload(ho, 0, sentinel[:oi + G + 1])
        g.mul_plain_sum(hc, ci, hp, pi, grp_off, ct_idx, ho, oi)
        got = g.ct_download(ho, 0, oi + G + 1)
        assert np.array_equal(got[oi:oi + G], expected(o, cts, pts, grp_off, ct_idx))
        assert np.array_equal(got[:oi], sentinel[:oi]) and np.array_equal(got[oi + G:], sentinel[oi + G:oi + G + 1])
        assert np.array_equal(g.ct_download(hc, ci, ncts), cts)
    finally:
        for h in (hc, ho, hp):
            g.free(h)


def main_lists(seed):
    """G = 3 groups of 1, 5 and 17 terms over 6 ciphertexts: every ciphertext is named, inside and across groups more than once"""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([[3], [0, 3, 3, 5, 1], rng.permutation(np.arange(17) % 6)]).astype(np.uint32)
    return [0, 1, 6, 23], idx


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("policy", ["u64", "f64", "f64l"])
def test_words_under_each_policy(policy, k):
    o, g = pair(1024, T, Q_POLICY[policy][:k])
    try:
        grp_off, idx = main_lists(7 + k)
        run(o, g, grp_off, idx, 6, 0xD1A0 + k)
    finally:
        g.close()


def test_integer_policy_by_option_on_small_moduli():
    """"f64" = 0: the integer kernel on moduli the FP64 kernels would take"""
    o, g = pair(1024, T, TINY_Q, f64=0)
    try:
        grp_off, idx = main_lists(3)
        run(o, g, grp_off, idx, 6, 0xD1A9)
    finally:
        g.close()


@pytest.mark.parametrize("name,opt", [("c3", {}), ("c5", {}), ("c5", {"f64": 0})], ids=["n8192", "n16384", "n16384-integer-composed"])
def test_two_groups_of_three_on_the_other_transform_plans(name, opt):
    p = PARAMS[name]
    from oracle.cno import COEFF_MODULUS_128
    q = p["q"] or COEFF_MODULUS_128[p["n"]]
    o, g = pair(p["n"], p["t"], q, **opt)
    try:
        run(o, g, [0, 3, 6], np.array([0, 1, 2, 2, 0, 0], dtype=np.uint32), 3, 0xD1B0, ci=0, pi=1, oi=0)
    finally:
        g.close()


def test_ring_without_the_kernel_composes_the_existing_calls():
    o, g = pair(512, T, ntt_primes(36, 512, 2))
    try:
        run(o, g, [0, 1, 4], np.array([1, 0, 1, 1], dtype=np.uint32), 2, 0xD1C0)
    finally:
        g.close()


def test_level_context():
    o, g = pair(1024, T, TINY_Q)
    try:
        from oracle.cno import Oracle
        lv, lo = g.level(2), Oracle(1024, T, q=TINY_Q[:2], dbc=60, gdbc=60)
        run(lo, lv, [0, 2, 5], np.array([0, 1, 1, 2, 0], dtype=np.uint32), 3, 0xD1D0)
    finally:
        g.close()


def test_recorded_graph_keeps_its_index_lists():
    """the host lists are captured by value (like those of cn_add_many): the caller's arrays are overwritten before the replay"""
    o, g = pair(1024, T, TINY_Q)
    try:
        rng = np.random.default_rng(5)
        grp_off, idx = np.array([0, 2, 5], dtype=np.uint32), np.array([0, 1, 1, 2, 0], dtype=np.uint32)
        cts, pts = inputs(o, 3, 0xD1E0), plaintexts(o, rng, 5)
        exp = expected(o, cts, pts, [0, 2, 5], [0, 1, 1, 2, 0])
        hc, hp, ho = g.ct_alloc(3), g.pt_alloc(5), g.ct_alloc(2)
        g.ct_upload(hc, 0, cts)
        g.pt_upload(hp, 0, pts)
        g.mul_plain_sum(hc, 0, hp, 0, grp_off, idx, ho, 0)                 # once outside: the scratch arena has its size
        g.graph_begin()
        g.mul_plain_sum(hc, 0, hp, 0, grp_off, idx, ho, 0)
        graph = g.graph_end()
        grp_off[:] = 0
        idx[:] = 2
        g.ct_upload(ho, 0, inputs(o, 2, 9))
        g.graph_launch(graph)
        assert np.array_equal(g.ct_download(ho, 0, 2), exp)
        g.free(graph)
    finally:
        g.close()


def test_refusals_write_nothing():
    from cryptonets_amd._native import CnError
    o, g = pair(1024, T, TINY_Q)
    try:
        rng = np.random.default_rng(6)
        cts, pts = inputs(o, 4, 0xD1F0), plaintexts(o, rng, 4)
        hc, hp, ho = g.ct_alloc(4), g.pt_alloc(5), g.ct_alloc(2)
        g.ct_upload(hc, 0, cts)
        g.pt_upload(hp, 0, np.concatenate([pts, np.zeros((1, o.n), dtype=np.uint64)]))
        g.ct_upload(ho, 0, cts[:2])

        def refused(code, *a):
            with pytest.raises(CnError) as ex:
                g.mul_plain_sum(*a)
            assert ex.value.code == code, ex.value

        refused(CN_ERR_ARG, hc, 0, hp, 0, [0, 2, 2, 3], [0, 1, 2], ho, 0)          # an empty group (and more groups than outputs)
        refused(CN_ERR_ARG, hc, 0, hp, 0, [0, 2, 2], [0, 1], ho, 0)                # an empty group
        refused(CN_ERR_ARG, hc, 0, hp, 0, [0, 2], [0, 4], ho, 0)                   # ciphertext index past the handle
        refused(CN_ERR_ARG, hc, 2, hp, 0, [0, 2], [0, 2], ho, 0)                   # ... past it through the offset
        refused(CN_ERR_ARG, hc, 0, hp, 3, [0, 3], [0, 1, 2], ho, 0)                # plaintext range past the handle
        refused(CN_ERR_ARG, hc, 0, hp, 0, [0, 1, 2, 3], [0, 1, 2], ho, 0)          # more groups than outputs
        refused(CN_ERR_ARG, hc, 0, hp, 0, [0, 2, 4], [0, 3, 2, 3], hc, 1)          # out[1 .. 2] overlaps ciphertext 2 of the same handle
        refused(CN_ERR_ZERO, hc, 0, hp, 3, [0, 2], [0, 1], ho, 0)                  # plaintext 4 is zero
        assert np.array_equal(g.ct_download(ho, 0, 2), cts[:2]) and np.array_equal(g.ct_download(hc, 0, 4), cts)
        g.mul_plain_sum(hc, 0, hp, 0, [0, 2, 4], [2, 3, 2, 3], hc, 0)               # the same handle, outputs beside the operands: allowed
        assert np.array_equal(g.ct_download(hc, 0, 2), expected(o, cts, pts, [0, 2, 4], [2, 3, 2, 3]))
    finally:
        g.close()
