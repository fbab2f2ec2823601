"""NTT-form plaintext arrays (cn_ptn_alloc, cn_pt_transform, cn_ptn_upload / cn_ptn_download) and the three products that take them - cn_mul_plain,
cn_rowdot_batch, cn_mul_plain_sum - word for word against the CPU oracle and against the same calls on the coefficient form.

Modular arithmetic is exact and every output is canonical, so a product with Evaluator.TransformToNtt(plain) must write the words of the product with `plain`.
Shapes: those of tests/test_gpu_mul_plain_sum.py (its moduli per arithmetic policy, its inputs, every handle at an offset, sentinels beside the outputs), plus one
group of 3 x interval + 1 terms of chosen NTT words on 49/49/47-bit moduli: the lazy FP64 accumulators of k_mul_ptn_sum recentre every `interval` terms
(cn_ptn_sum_interval, cn_policy.h; tests/test_ptn_accumulate_bound.py checks the interval itself).
"""
import numpy as np
import pytest

from conftest import PARAMS, get_gpu, get_oracle
from test_gpu_mul_plain_sum import CN_ERR_ARG, CN_ERR_ZERO, Q_POLICY, T, expected, main_lists, pair, plaintexts
from test_gpu_wide_moduli import TINY_Q, ntt_primes
from test_square_gemm import inputs

pytestmark = pytest.mark.gpu


def lift(o, j, m):
    """the fast plain lift into q_j: coefficients at or above (t + 1) / 2 stand for negative values"""
    m = np.asarray(m, dtype=np.uint64)
    return np.where(m >= np.uint64((o.t + 1) // 2), m + np.uint64(o.q[j] - o.t), m)


def ntt_form(o, pts):
    """[count][k][N]: limb j of plaintext p = NTT_j(lift_j(m_p)) by the oracle's transform"""
    return np.stack([np.stack([o.ntt_fwd(j, lift(o, j, p)) for j in range(o.k)]) for p in pts])


def with_zero(o, rng, count):
    """plaintexts() (t - 1, t / 2, t / 2 + 1 in the first, one non-zero coefficient in the second) and an all-zero plaintext behind them"""
    return np.concatenate([plaintexts(o, rng, count), np.zeros((1, o.n), dtype=np.uint64)])


def transformed(g, pts, pi=1, oi=2):
    """upload at an offset, transform at another: (coefficient handle, NTT handle, first NTT index)"""
    hp, hn = g.pt_alloc(pi + len(pts)), g.ptn_alloc(oi + len(pts) + 1)
    g.pt_upload(hp, pi, pts)
    g.pt_transform(hp, pi, len(pts), hn, oi)
    return hp, hn


# ---- the transform -----------------------------------------------------------------------------------------------------------------------------------------
def check_transform(o, g, count, seed):
    rng = np.random.default_rng(seed)
    pts = with_zero(o, rng, count)
    sentinel = rng.integers(0, min(o.q), size=(len(pts) + 3, o.k, o.n), dtype=np.uint64)
    hp, hn = g.pt_alloc(1 + len(pts)), g.ptn_alloc(len(pts) + 3)
    try:
        g.ptn_upload(hn, 0, sentinel)
        g.pt_upload(hp, 1, pts)
        before = g.stats()["ntt_forward_limbs"]
        g.pt_transform(hp, 1, len(pts), hn, 2)
        assert g.stats()["ntt_forward_limbs"] - before == len(pts) * o.k
        got = g.ptn_download(hn, 0, len(pts) + 3)
        assert np.array_equal(got[2:2 + len(pts)], ntt_form(o, pts))
        assert np.array_equal(got[:2], sentinel[:2]) and np.array_equal(got[-1], sentinel[-1])
        # the zero flag travelled with the all-zero plaintext: a product refuses it
        from cryptonets_amd._native import CnError
        hc = g.ct_alloc(1)
        g.ct_upload(hc, 0, inputs(o, 1, seed))
        with pytest.raises(CnError) as ex:
            g.mul_plain(hc, 0, hn, 2 + len(pts) - 1, hc, 0)
        assert ex.value.code == CN_ERR_ZERO
        g.free(hc)
    finally:
        g.free(hp)
        g.free(hn)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("policy", ["u64", "f64", "f64l"])
def test_transform_words_under_each_policy(policy, k):
    o, g = pair(1024, T, Q_POLICY[policy][:k])
    try:
        check_transform(o, g, 4, 0xA100 + k)
    finally:
        g.close()


def test_transform_words_integer_policy_by_option():
    o, g = pair(1024, T, TINY_Q, f64=0)
    try:
        check_transform(o, g, 4, 0xA110)
    finally:
        g.close()


def other_ring(name, **opt):
    from oracle.cno import COEFF_MODULUS_128
    if name == "n512":
        return pair(512, T, ntt_primes(36, 512, 2), **opt)
    p = PARAMS[name]
    return pair(p["n"], p["t"], p["q"] or COEFF_MODULUS_128[p["n"]], **opt)


@pytest.mark.parametrize("name", ["c3", "c5", "n512"])
def test_transform_words_on_the_other_rings(name):
    o, g = other_ring(name)
    try:
        check_transform(o, g, 1, 0xA120)
    finally:
        g.close()


# ---- cn_mul_plain_sum ---------------------------------------------------------------------------------------------------------------------------------------
def run_sum(o, g, grp_off, ct_idx, ncts, seed, ci=1, pi=2, oi=1, kernel=True):
    """the call of test_gpu_mul_plain_sum.run on the NTT-form handle: the oracle's words, the words of the coefficient-form call, the counters"""
    rng = np.random.default_rng(seed)
    G, E = len(grp_off) - 1, grp_off[-1]
    cts, pts = inputs(o, ncts, seed), plaintexts(o, rng, E)
    sentinel = inputs(o, G + 2, seed + 1)
    hc, ho, ho2 = g.ct_alloc(ci + ncts), g.ct_alloc(oi + G + 1), g.ct_alloc(G)
    hp, hn = transformed(g, pts, pi, pi + 1)
    try:
        g.ct_upload(hc, ci, cts)
        g.ct_upload(ho, 0, sentinel[:oi + G + 1])
        s0, l0 = g.stats(), g.get_option("ptn_sum")
        g.mul_plain_sum(hc, ci, hn, pi + 1, grp_off, ct_idx, ho, oi)
        s1, l1 = g.stats(), g.get_option("ptn_sum")
        got = g.ct_download(ho, 0, oi + G + 1)
        exp = expected(o, cts, pts, grp_off, ct_idx)
        assert np.array_equal(got[oi:oi + G], exp)
        assert np.array_equal(got[:oi], sentinel[:oi]) and np.array_equal(got[oi + G:], sentinel[oi + G:oi + G + 1])
        assert np.array_equal(g.ct_download(hc, ci, ncts), cts)
        g.mul_plain_sum(hc, ci, hp, pi, grp_off, ct_idx, ho2, 0)
        assert np.array_equal(g.ct_download(ho2, 0, G), got[oi:oi + G])
        assert s1["PlainMultiplication"] - s0["PlainMultiplication"] == E and s1["AddMany"] - s0["AddMany"] == G
        assert s1["AddManyItemCount"] - s0["AddManyItemCount"] == E
        if kernel:
            D = len(set(int(i) for i in ct_idx))
            assert s1["ntt_forward_limbs"] - s0["ntt_forward_limbs"] == D * 2 * o.k
            assert l1 == l0 + 1
        else:
            assert l1 == l0
            assert s1["ntt_forward_limbs"] - s0["ntt_forward_limbs"] == E * 2 * o.k      # composed: the ciphertext of every term, no plaintext
    finally:
        for h in (hc, ho, ho2, hp, hn):
            g.free(h)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("policy", ["u64", "f64", "f64l"])
def test_sum_words_under_each_policy(policy, k):
    o, g = pair(1024, T, Q_POLICY[policy][:k])
    try:
        grp_off, idx = main_lists(7 + k)
        run_sum(o, g, grp_off, idx, 6, 0xA200 + k)
    finally:
        g.close()


@pytest.mark.parametrize("name,opt,kernel", [("c3", {}, True), ("c5", {}, True), ("c5", {"f64": 0}, False), ("n512", {}, False)],
                         ids=["n8192", "n16384", "n16384-integer-composed", "n512-composed"])
def test_sum_two_groups_of_three_on_the_other_rings(name, opt, kernel):
    o, g = other_ring(name, **opt)
    try:
        run_sum(o, g, [0, 3, 6], np.array([0, 1, 2, 2, 0, 0], dtype=np.uint32), 3, 0xA210, ci=0, pi=1, oi=0, kernel=kernel)
    finally:
        g.close()


@pytest.mark.parametrize("policy", ["u64", "f64"])
def test_sum_words_in_the_other_workgroup_order(policy):
    """"ptn_order" = 1: limb = workgroup index mod k"""
    o, g = pair(1024, T, Q_POLICY[policy], ptn_order=1)
    try:
        assert g.get_option("ptn_order") == 1
        grp_off, idx = main_lists(4)
        run_sum(o, g, grp_off, idx, 6, 0xA230)
    finally:
        g.close()


def test_sum_composed_under_mp_fused_0():
    o, g = pair(1024, T, TINY_Q, mp_fused=0)
    try:
        run_sum(o, g, [0, 1, 4], np.array([1, 0, 1, 1], dtype=np.uint32), 2, 0xA220, kernel=False)
    finally:
        g.close()


def test_sum_of_chosen_words_across_three_recentrings():
    """One group of 3 x interval + 1 terms on 49/49/47-bit moduli.  The NTT words are uploaded, each drawn from {0, 1, (q - 1) / 2, (q + 1) / 2, q - 1}; the
    ciphertexts include the constant polynomial q - 1, whose NTT words are all q - 1.  Expected: INTT(sum NTT(ct) . w mod q) with the oracle's transforms and
    Python integers."""
    q = Q_POLICY["f64"]
    o, g = pair(1024, T, q)
    try:
        interval = g.get_option("ptn_sum_interval")
        # recomputed from the derivation: |term| <= q/2 + 3 q^2 / 2^53 (rounded up), interval = the largest count with count x bound < 2^52
        qmax = max(q)
        bound = qmax // 2 + 1 + -((-3 * qmax * qmax) >> 53)
        assert interval == (2 ** 52 - 1) // bound and 2 <= interval < 64
        E = 3 * interval + 1
        rng = np.random.default_rng(0xA300)
        cts = inputs(o, 3, 0xA301)
        const = np.zeros((2, o.k, o.n), dtype=np.uint64)
        for j in range(o.k):
            const[:, j, 0] = q[j] - 1                                # the constant polynomial q_j - 1 in both components
        cts[0] = const.reshape(-1)
        idx = (np.arange(E) % 3).astype(np.uint32)
        idx[:interval + 2] = 0                                       # more than a whole interval against the constant ciphertext ...
        words = np.empty((E, o.k, o.n), dtype=np.uint64)
        for j in range(o.k):
            choice = np.array([0, 1, (q[j] - 1) // 2, (q[j] + 1) // 2, q[j] - 1], dtype=np.uint64)
            words[:, j, :] = choice[rng.integers(0, 5, size=(E, o.n))]
        # ... of the word (q - 1) / 2 everywhere: every term is -(q - 1) / 2 mod q, the residue of largest magnitude, and the terms of a position share their sign
        words[:interval + 2] = np.array([(qq - 1) // 2 for qq in q], dtype=np.uint64)[None, :, None]
        ctn = np.stack([np.stack([np.stack([o.ntt_fwd(j, c.reshape(2, o.k, o.n)[p, j]) for j in range(o.k)]) for p in range(2)]) for c in cts])
        assert all(np.all(ctn[0, :, j] == q[j] - 1) for j in range(o.k))
        exp = np.empty((2, o.k, o.n), dtype=np.uint64)
        for p in range(2):
            for j in range(o.k):
                acc = np.zeros(o.n, dtype=object)
                for e in range(E):
                    acc += ctn[idx[e], p, j].astype(object) * words[e, j].astype(object)
                exp[p, j] = o.ntt_inv(j, np.array([int(a) % q[j] for a in acc], dtype=np.uint64))
        hc, hn, ho = g.ct_alloc(3), g.ptn_alloc(E), g.ct_alloc(1)
        g.ct_upload(hc, 0, cts)
        g.ptn_upload(hn, 0, words)
        assert np.array_equal(g.ptn_download(hn, 0, E), words)
        g.mul_plain_sum(hc, 0, hn, 0, [0, E], idx, ho, 0)
        assert np.array_equal(g.ct_download(ho, 0, 1)[0], exp.reshape(-1))
    finally:
        g.close()


# ---- cn_mul_plain -------------------------------------------------------------------------------------------------------------------------------------------
def oracle_products(o, cts, pts, stride):
    return np.stack([o.multiply_plain(c, pts[i * stride]) for i, c in enumerate(cts)])


@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("count,stride", [(1, 1), (3, 1), (3, 0)])
def test_mul_plain_words(count, stride, size):
    o, g = pair(1024, T, TINY_Q)
    try:
        rng = np.random.default_rng(0xA400 + count + size)
        pts = plaintexts(o, rng, 3)
        cts = inputs(o, count + 2, 0xA401) if size == 2 else np.stack([np.concatenate([c, c[o.k * o.n:]]) for c in inputs(o, count + 2, 0xA402)])
        hp, hn = transformed(g, pts)
        ha, ho = g.ct_alloc(count + 2, size), g.ct_alloc(count + 2, size)
        g.ct_upload(ha, 0, cts)
        g.ct_upload(ho, 0, cts[::-1].copy())
        exp = oracle_products(o, cts[1:1 + count], pts, stride)
        s0 = g.stats()
        g.mul_plain(ha, 1, hn, 2, ho, 1, count, pt_stride=stride)                  # disjoint
        s1 = g.stats()
        got = g.ct_download(ho, 0, count + 2, size)
        assert np.array_equal(got[1:1 + count], exp)
        assert np.array_equal(got[0], cts[-1]) and np.array_equal(got[-1], cts[0])  # the neighbours keep their words
        assert s1["kernel_launches"] - s0["kernel_launches"] == 1                  # k_mul_plain_fused alone
        assert s1["ntt_forward_limbs"] - s0["ntt_forward_limbs"] == count * size * o.k and s1["PlainMultiplication"] - s0["PlainMultiplication"] == count
        g.mul_plain(ha, 1, hn, 2, ha, 1, count, pt_stride=stride)                  # in place
        assert np.array_equal(g.ct_download(ha, 1, count, size), exp)
    finally:
        g.close()


def test_mul_plain_on_a_ring_without_the_register_radix_kernels():
    o, g = other_ring("n512")
    try:
        rng = np.random.default_rng(0xA410)
        pts, cts = plaintexts(o, rng, 3), inputs(o, 3, 0xA411)
        hp, hn = transformed(g, pts)
        ha, ho = g.ct_alloc(3), g.ct_alloc(3)
        g.ct_upload(ha, 0, cts)
        s0 = g.stats()
        g.mul_plain(ha, 0, hn, 2, ho, 0, 3)
        assert g.stats()["ntt_forward_limbs"] - s0["ntt_forward_limbs"] == 3 * 2 * o.k        # the ciphertexts alone
        assert np.array_equal(g.ct_download(ho, 0, 3), oracle_products(o, cts, pts, 1))
        g.mul_plain(ha, 0, hn, 3, ho, 0, 3, pt_stride=0)
        assert np.array_equal(g.ct_download(ho, 0, 3), oracle_products(o, cts, pts[1:], 0))
    finally:
        g.close()


def test_mul_plain_is_not_queued_under_defer():
    """"defer" = 1 with an addition queued ahead on the same array: the queue is flushed, the product runs at once - the words of the immediate sequence"""
    o, g = pair(1024, T, TINY_Q)
    try:
        rng = np.random.default_rng(0xA420)
        pts, cts = plaintexts(o, rng, 2), inputs(o, 2, 0xA421)
        hp, hn = transformed(g, pts)
        ha, hb, ho = g.ct_alloc(1), g.ct_alloc(1), g.ct_alloc(1)
        g.ct_upload(ha, 0, cts[:1])
        g.ct_upload(hb, 0, cts[1:])
        g.set_option("defer", 1)
        g.add(ha, 0, hb, 0, ha, 0)
        g.mul_plain(ha, 0, hn, 2, ho, 0)
        assert g.get_option("pending_calls") == 0
        g.set_option("defer", 0)
        assert np.array_equal(g.ct_download(ho, 0, 1)[0], o.multiply_plain(o.add(cts[0], cts[1]), pts[0]))
    finally:
        g.close()


# ---- cn_rowdot_batch ----------------------------------------------------------------------------------------------------------------------------------------
def check_rowdot(name, rows, length, seed):
    o, g = get_oracle(name), get_gpu(name)
    rng = np.random.default_rng(seed)
    pts = plaintexts(o, rng, rows)
    v = o.encrypt(o.encode(rng.integers(0, 8, size=o.n, dtype=np.uint64)))
    hp, hn = transformed(g, pts)
    hv, ho, ho2 = g.ct_alloc(1), g.ct_alloc(rows + 2), g.ct_alloc(rows)
    try:
        g.ct_upload(hv, 0, v[None, :])
        sentinel = np.stack([v, v])
        g.ct_upload(ho, 0, sentinel[:1])
        g.ct_upload(ho, rows + 1, sentinel[1:])
        s0, l0 = g.stats(), g.get_option("ptn_bcast")
        g.rowdot_batch(hv, 0, hn, 2, rows, length, ho, 1)
        s1, l1 = g.stats(), g.get_option("ptn_bcast")
        g.rowdot_batch(hv, 0, hp, 1, rows, length, ho2, 0)
        got = g.ct_download(ho, 0, rows + 2)
        assert np.array_equal(got[1:1 + rows], g.ct_download(ho2, 0, rows))
        assert np.array_equal(got[0], v) and np.array_equal(got[-1], v)
        s2 = g.stats()
        assert l1 == l0 + 1
        # the coefficient-form call transforms every row in both products' blocks on top of what this one ran
        assert (s2["ntt_forward_limbs"] - s1["ntt_forward_limbs"]) - (s1["ntt_forward_limbs"] - s0["ntt_forward_limbs"]) >= rows * 2 * o.k
        return got[1:1 + rows], o, pts, v
    finally:
        for h in (hp, hn, hv, ho, ho2):
            g.free(h)


@pytest.mark.parametrize("length", [0, 8])
def test_rowdot_batch_words(length):
    got, o, pts, v = check_rowdot("tiny", 5, length, 0xA500 + length)
    # and the first row against the oracle's own sequence: MultiplyPlain, then the rotate-and-add chain of SumAllSlots
    acc = o.multiply_plain(v, pts[0])
    ln = length or o.n
    if ln >= o.n // 2:
        acc = o.add(acc, o.rotate_columns(acc))
        ln = o.n // 2
    s = 1
    while s < ln:
        acc = o.add(acc, o.rotate_rows(acc, -s))
        s *= 2
    assert np.array_equal(got[0], acc)


def test_rowdot_batch_hands_the_permuted_c1_to_the_chain_at_16384():
    check_rowdot("c5", 4, 8, 0xA510)


# ---- level context, recorded graph, refusals ---------------------------------------------------------------------------------------------------------------
def test_level_context_makes_its_own_array():
    o, g = pair(1024, T, TINY_Q)
    try:
        from cryptonets_amd._native import CnError
        from oracle.cno import Oracle
        lv, lo = g.level(2), Oracle(1024, T, q=TINY_Q[:2], dbc=60, gdbc=60)
        rng = np.random.default_rng(0xA600)
        pts = plaintexts(o, rng, 5)
        filler = [g.ct_alloc(1) for _ in range(3)]                                 # the parent's table is ahead of the level's: its handles name nothing there
        hp, hn = transformed(g, pts)
        lp, ln = transformed(lv, pts)
        assert np.array_equal(lv.ptn_download(ln, 2, 5), ntt_form(lo, pts))
        assert np.array_equal(lv.ptn_download(ln, 2, 5), g.ptn_download(hn, 2, 5)[:, :2])         # the first `limbs` limbs, recomputed
        cts = inputs(lo, 3, 0xA601)
        hc, ho = lv.ct_alloc(3), lv.ct_alloc(2)
        lv.ct_upload(hc, 0, cts)
        with pytest.raises(CnError) as ex:                                         # a parent's handle in its level context
            lv.mul_plain_sum(hc, 0, hn, 2, [0, 2, 5], [0, 1, 1, 2, 0], ho, 0)
        assert ex.value.code == CN_ERR_ARG
        lv.mul_plain_sum(hc, 0, ln, 2, [0, 2, 5], [0, 1, 1, 2, 0], ho, 0)
        assert np.array_equal(lv.ct_download(ho, 0, 2), expected(lo, cts, pts, [0, 2, 5], [0, 1, 1, 2, 0]))
        assert filler
    finally:
        g.close()


def test_recorded_graph_keeps_its_index_lists():
    o, g = pair(1024, T, TINY_Q)
    try:
        rng = np.random.default_rng(0xA700)
        grp_off, idx = np.array([0, 2, 5], dtype=np.uint32), np.array([0, 1, 1, 2, 0], dtype=np.uint32)
        cts, pts = inputs(o, 3, 0xA701), plaintexts(o, rng, 5)
        exp = expected(o, cts, pts, [0, 2, 5], [0, 1, 1, 2, 0])
        hc, ho = g.ct_alloc(3), g.ct_alloc(2)
        hp, hn = transformed(g, pts)
        g.ct_upload(hc, 0, cts)
        g.mul_plain_sum(hc, 0, hn, 2, grp_off, idx, ho, 0)                 # once outside: the scratch arena has its size
        g.ptn_upload(hn, 2, np.ones((5, o.k, o.n), dtype=np.uint64))       # the recording transforms again
        g.graph_begin()
        g.pt_transform(hp, 1, 5, hn, 2)
        g.mul_plain_sum(hc, 0, hn, 2, grp_off, idx, ho, 0)
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
        live = g.live_handles()
        rng = np.random.default_rng(0xA800)
        cts, pts = inputs(o, 2, 0xA801), with_zero(o, rng, 3)
        hp, hn = transformed(g, pts)                                       # plaintexts 2 .. 5 of hn; 5 is zero
        hc, hq, ho = g.ct_alloc(2), g.pt_alloc(2), g.ct_alloc(1)
        g.ct_upload(hc, 0, cts)
        g.ct_upload(ho, 0, cts[1:])
        g.pt_upload(hq, 0, pts[:2])
        words = g.ptn_download(hn, 2, 4)

        def refused(code, fn, *a, **kw):
            with pytest.raises(CnError) as ex:
                fn(*a, **kw)
            assert ex.value.code == code, ex.value

        refused(CN_ERR_ARG, g.add_plain, hc, 0, hn, 2, hc, 0)
        g.keygen(5, galois=False)                                          # (cn_encrypt asks for the public key first)
        g.encrypt(hq, 0, hc, 1)
        g.ct_upload(hc, 0, cts)
        refused(CN_ERR_ARG, g.encrypt, hn, 2, hc, 0)
        refused(CN_ERR_ARG, g.decode_batch, hn, 2, 1)
        refused(CN_ERR_ARG, g.pt_download, hn, 2, 1)
        refused(CN_ERR_ARG, g.ptn_download, hp, 1, 1)
        refused(CN_ERR_ARG, g.pt_transform, hp, 1, 5, hn, 2)               # past the source
        refused(CN_ERR_ARG, g.pt_transform, hp, 1, 4, hn, 4)               # past the destination
        refused(CN_ERR_ARG, g.pt_transform, hn, 2, 1, hn, 2)               # the source is not a coefficient-form array
        refused(CN_ERR_ZERO, g.mul_plain, hc, 0, hn, 5, hc, 0)
        refused(CN_ERR_ZERO, g.mul_plain_sum, hc, 0, hn, 4, [0, 2], [0, 1], ho, 0)
        bad = words.copy()
        bad[1, 1, 7] = o.q[1]
        refused(CN_ERR_ARG, g.ptn_upload, hn, 2, bad)
        assert np.array_equal(g.ptn_download(hn, 2, 4), words) and np.array_equal(g.ct_download(hc, 0, 2), cts) and np.array_equal(g.ct_download(ho, 0, 1), cts[1:])
        assert np.array_equal(g.pt_download(hp, 1, 4), pts)
        g.ptn_upload(hn, 5, words[:1])                                     # the flag follows the words: plaintext 5 is no longer zero
        g.mul_plain(hc, 0, hn, 5, hc, 1)
        assert np.array_equal(g.ct_download(hc, 1, 1)[0], o.multiply_plain(cts[0], pts[0]))
        for h in (hp, hn, hc, hq, ho):
            g.free(h)
        assert g.live_handles() == live
    finally:
        g.close()
