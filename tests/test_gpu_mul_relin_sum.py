"""cn_mul_relin_sum - out[i] = sum_k Relinearize(Multiply(a_k[i], b_k[i])) in one call - against the CPU oracle and the library's literal sequence.

The call must write the words of K cn_mul_relin calls into a temporary followed by cn_add_many per output (tests/test_square_gemm_identity.py with unit
weights: why ONE key switch per output, fed with the per-product digits summed, gives them).  Every case is compared word for word with the oracle's
mul_relin_batch per term + add over the terms and with the library's own mul_relin x K + add_many; "mul_sum_fused" reads back which form ran.

Shapes: the smallest register-radix ring ("tiny": N = 1024, three limbs, dbc 10) with the term counts at which k_product_sum takes another path - K = 1 (no
kernel), the smallest fused K, 5 (one set of four terms and a tail of one), 9 (a pair of sets and a tail; b advancing with the output) - and the CryptoNets ring
("c3": N = 8192, five limbs of five digits) with K = 3 and 8.
"""
import os

import numpy as np
import pytest

from conftest import PARAMS
from test_square_gemm import COUNTERS, fresh_context, inputs

pytestmark = pytest.mark.gpu


def min_k(g):
    return max(2, g.get_option("mul_sum_min_k"))


def operands(o, K, count, b_stride, seed):
    """(A, B): K arrays of `count` ciphertexts, K arrays of count (b_stride 1) or 1 (b_stride 0) ciphertexts; edge residues in the first ciphertexts of either side"""
    cb = count if b_stride else 1
    A = inputs(o, K * count, seed).reshape(K, count, -1)
    B = inputs(o, K * cb, seed + 1000).reshape(K, cb, -1)
    return A, B


def expected(o, A, B, b_stride):
    """the oracle: Multiply + Relinearize per term, then add over the terms"""
    K, count = A.shape[0], A.shape[1]
    rows_a = np.stack([A[k, i] for i in range(count) for k in range(K)])
    rows_b = np.stack([B[k, i * b_stride] for i in range(count) for k in range(K)])
    P = o.mul_relin_batch(rows_a, rows_b).reshape(count, K, -1)
    out = []
    for i in range(count):
        acc = P[i, 0]
        for k in range(1, K):
            acc = o.add(acc, P[i, k])
        out.append(acc)
    return np.stack(out)


def upload(g, X):
    h = g.ct_alloc(len(X))
    g.ct_upload(h, 0, X)
    return h


def literal(g, ha, ia, hb, ib, b_stride, count):
    """the library's own literal sequence: mul_relin per term into a temporary, add_many per output"""
    K = len(ha)
    tmp, out = g.ct_alloc(K * count), g.ct_alloc(count)
    for k in range(K):
        g.mul_relin(ha[k], ia[k], hb[k], ib[k], tmp, k * count, count, a_stride=1, b_stride=b_stride)
    for i in range(count):
        g.add_many(tmp, [k * count + i for k in range(K)], out, i)
    w = g.ct_download(out, 0, count)
    g.free(tmp)
    g.free(out)
    return w


def run(g, o, K, count, b_stride, seed, fused):
    """one call on K separate handles per side; asserts the oracle's words, the literal sequence's words and the step of "mul_sum_fused" """
    A, B = operands(o, K, count, b_stride, seed)
    ha, hb = [upload(g, A[k]) for k in range(K)], [upload(g, B[k]) for k in range(K)]
    out = g.ct_alloc(count)
    before = g.get_option("mul_sum_fused")
    g.mul_relin_sum(ha, None, hb, None, b_stride, out, 0, count)
    step = g.get_option("mul_sum_fused") - before
    got = g.ct_download(out, 0, count)
    lit = literal(g, ha, [0] * K, hb, [0] * K, b_stride, count)
    exp = expected(o, A, B, b_stride)
    assert step == (1 if fused else 0), "mul_sum_fused moved by %d" % step
    assert np.array_equal(got, exp)
    assert np.array_equal(got, lit)
    for h in ha + hb + [out]:
        g.free(h)


@pytest.fixture(scope="module")
def tiny():
    o, g = fresh_context("tiny")
    yield o, g
    g.close()


@pytest.fixture(scope="module")
def c3():
    o, g = fresh_context("c3")
    yield o, g
    g.close()


# ------------------------------------------------------------------ 1. words
@pytest.mark.parametrize("K,count,b_stride", [(1, 1, 0), (2, 1, 0), (5, 3, 0), (9, 2, 1)])
def test_words_on_the_small_ring(tiny, K, count, b_stride):
    o, g = tiny
    if K == 2:
        K = min_k(g)                                                 # the smallest fused call
    run(g, o, K, count, b_stride, 0x900 + K, fused=K > 1)


@pytest.mark.parametrize("K,count", [(3, 2), (8, 1)])
def test_words_on_the_cryptonets_ring(c3, K, count):
    o, g = c3
    run(g, o, max(K, min_k(g)), count, 0, 0xC30 + K, fused=True)


# ------------------------------------------------------------------ 2. addressing
def test_operands_at_offsets_a_repeated_handle_and_outputs_inside_a_larger_handle(tiny):
    o, g = tiny
    K, count = max(3, min_k(g)), 2
    A, B = operands(o, K, count, 1, 0xADD)
    # a: term 0 and term 2 live in ONE handle at indices 1 and 4, term 1 (and any further) in its own at index 2; b: all terms in one handle at k * count + 3
    pad = inputs(o, 1, 5)[0]
    big = np.stack([pad, A[0, 0], A[0, 1], pad, A[2, 0], A[2, 1], pad])
    h02 = upload(g, big)
    ha, ia = [h02, None, h02], [1, 2, 4]
    own = []
    for k in range(K):
        if k in (0, 2):
            continue
        h = upload(g, np.stack([pad, pad, A[k, 0], A[k, 1]]))
        own.append(h)
        if k == 1:
            ha[1] = h
        else:
            ha.append(h)
            ia.append(2)
    hb_all = upload(g, np.concatenate([np.stack([pad] * 3), B.reshape(K * count, -1)]))
    hb, ib = [hb_all] * K, [3 + k * count for k in range(K)]
    sentinel = inputs(o, 6, 0x5E)
    out = upload(g, sentinel)
    before = g.get_option("mul_sum_fused")
    g.mul_relin_sum(ha, ia, hb, ib, 1, out, 3, count)
    assert g.get_option("mul_sum_fused") == before + 1
    got = g.ct_download(out, 0, 6)
    assert np.array_equal(got[3:5], expected(o, A, B, 1))
    assert np.array_equal(got[:3], sentinel[:3]) and np.array_equal(got[5:], sentinel[5:]), "ciphertexts beside the written range changed"
    assert np.array_equal(got[3:5], literal(g, ha, ia, hb, ib, 1, count))
    for h in [h02, hb_all, out] + own:
        g.free(h)


# ------------------------------------------------------------------ 3. the bound, at its edge
def test_the_digit_bound_at_its_edge():
    """dbc = 30 on tiny: the smallest modulus is 0xffffc4001, q / 2 = 34 359 615 488.  K = 31: 31 (2^30 - 1) = 33 285 996 513 < q / 2 - fused;
    K = 32: 32 (2^30 - 1) = 34 359 738 336 >= q / 2 - literal.  Both give the oracle's words."""
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    p = PARAMS["tiny"]
    assert min(p["q"]) == 0xffffc4001 and min(p["q"]) // 2 == 34359615488
    assert 31 * ((1 << 30) - 1) == 33285996513 < min(p["q"]) // 2 <= 32 * ((1 << 30) - 1) == 34359738336
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=30, gdbc=p["gdbc"])
    o.keygen(11, galois=False)
    g = Context(p["n"], p["t"], q=p["q"], dbc=30, gdbc=p["gdbc"], device=0)
    try:
        g.set_relin_key(o.relin_key())
        run(g, o, 31, 1, 0, 0xED6E, fused=True)
        run(g, o, 32, 1, 0, 0xED6F, fused=False)
    finally:
        g.close()


# ------------------------------------------------------------------ 4. ineligible contexts still agree
@pytest.mark.parametrize("why", ["ks_xi", "f64_off", "mul_sum_off"])
def test_ineligible_contexts_take_the_literal_sequence_and_still_agree(why):
    from cryptonets_amd._native import Context
    p = PARAMS["tiny"]
    if why == "f64_off":
        o, _g = fresh_context("tiny")
        _g.close()
        g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
        g.set_option("f64", 0)
        g.set_relin_key(o.relin_key())
    else:
        o, g = fresh_context("tiny", xi=why == "ks_xi")
    try:
        if why == "mul_sum_off":
            assert g.get_option("mul_sum") == 1
            g.set_option("mul_sum", 0)
            assert g.get_option("mul_sum") == 0
        run(g, o, 5, 2, 0, 0x1E1, fused=False)
        assert g.get_option("mul_sum_groups") == 0
    finally:
        g.close()


# ------------------------------------------------------------------ 5. counters
def test_counters_of_one_fused_call_are_those_of_the_literal_sequence(tiny):
    o, g = tiny
    K, count = 5, 2
    A, B = operands(o, K, count, 0, 0xC0)
    ha, hb = [upload(g, A[k]) for k in range(K)], [upload(g, B[k]) for k in range(K)]
    out = g.ct_alloc(count)
    g.stats(reset=True)
    before = g.get_option("mul_sum_fused")
    g.mul_relin_sum(ha, None, hb, None, 0, out, 0, count)
    one = g.stats(reset=True)
    assert g.get_option("mul_sum_fused") == before + 1
    literal(g, ha, [0] * K, hb, [0] * K, 0, count)
    lit = g.stats(reset=True)
    names = COUNTERS + ("AddMany", "AddManyItemCount")
    assert {c: one[c] for c in names} == {c: lit[c] for c in names}
    assert one["Multiplication"] == K * count and one["Relinarization"] == K * count and one["AddMany"] == count and one["AddManyItemCount"] == K * count
    for h in ha + hb + [out]:
        g.free(h)


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_output_alone(tiny):
    from cryptonets_amd._native import CnError, Context
    o, g = tiny
    K, count = 3, 2
    A, B = operands(o, K, count, 1, 0x4EF)
    ha, hb = [upload(g, A[k]) for k in range(K)], [upload(g, B[k]) for k in range(K)]
    sentinel = inputs(o, count, 0x5E1)
    out = upload(g, sentinel)
    h3 = g.ct_alloc(count, 3)
    z = [0] * K
    calls = {
        "K = 0": lambda c: c.mul_relin_sum([], None, [], None, 0, out, 0, count),
        "count = 0": lambda c: c.mul_relin_sum(ha, None, hb, None, 1, out, 0, 0),
        "b_stride = 2": lambda c: c.mul_relin_sum(ha, None, hb, None, 2, out, 0, 1),
        "a index": lambda c: c.mul_relin_sum(ha, [0, 1, 0], hb, None, 1, out, 0, count),
        "b index": lambda c: c.mul_relin_sum(ha, None, hb, [0, 0, 1], 1, out, 0, count),
        "b index, broadcast": lambda c: c.mul_relin_sum(ha, None, hb, [0, 0, 2], 0, out, 0, count),
        "output index": lambda c: c.mul_relin_sum(ha, None, hb, None, 1, out, 1, count),
        "out is operand a": lambda c: c.mul_relin_sum([ha[0], out, ha[2]], z, hb, None, 1, out, 0, count),
        "out is operand b": lambda c: c.mul_relin_sum(ha, None, [hb[0], hb[1], out], z, 1, out, 0, count),
        "operand of size 3": lambda c: c.mul_relin_sum([ha[0], h3, ha[2]], None, hb, None, 1, out, 0, count),
        "output of size 3": lambda c: c.mul_relin_sum(ha, None, hb, None, 1, h3, 0, count),
    }
    for what, call in calls.items():
        with pytest.raises(CnError) as e:
            call(g)
        assert e.value.code == -1, what                              # CN_ERR_ARG
        assert np.array_equal(g.ct_download(out, 0, count), sentinel), what
    # no relinearisation key
    p = PARAMS["tiny"]
    bare = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    try:
        xa, xb, xo = upload(bare, A[0]), upload(bare, B[0]), upload(bare, sentinel)
        with pytest.raises(CnError) as e:
            bare.mul_relin_sum([xa, xa], None, [xb, xb], None, 1, xo, 0, count)
        assert "relinearization keys not set" in str(e.value)
        assert np.array_equal(bare.ct_download(xo, 0, count), sentinel)
    finally:
        bare.close()
    # a one-limb context
    lv = g.level(1)
    one = inputs(type("Q", (), dict(q=o.q[:1], n=o.n, k=1))(), 3, 7)
    la, lo_ = upload(lv, one[:2]), upload(lv, one[2:])
    with pytest.raises(CnError) as e:
        lv.mul_relin_sum([la, la], [0, 1], [la, la], [1, 0], 0, lo_, 0, 1)
    assert e.value.code == -1 and "at least 2 coefficient moduli" in str(e.value)
    assert np.array_equal(lv.ct_download(lo_, 0, 1), one[2:])
    for h in ha + hb + [out, h3]:
        g.free(h)


# ------------------------------------------------------------------ 7. level context
def test_level_context_matches_the_prefix_oracle():
    from test_gpu_mod_switch import keyed, level_oracle
    o, g = keyed("c3", galois=False)
    try:
        lv = g.level(3)
        lo = level_oracle(o, "c3", 3, galois=False)
        run(lv, lo, max(3, min_k(lv)), 1, 0, 0x1E7, fused=True)
    finally:
        g.close()


# ------------------------------------------------------------------ 8. recorded
def test_recorded_call_replays_on_new_inputs(tiny):
    o, g = tiny
    K, count = 5, 2
    A, B = operands(o, K, count, 0, 0x6A1)
    ha, hb = [upload(g, A[k]) for k in range(K)], [upload(g, B[k]) for k in range(K)]
    out = g.ct_alloc(count)
    g.mul_relin_sum(ha, None, hb, None, 0, out, 0, count)            # once eagerly: the arenas have their sizes
    assert np.array_equal(g.ct_download(out, 0, count), expected(o, A, B, 0))
    before = g.get_option("mul_sum_fused")
    g.graph_begin()
    g.mul_relin_sum(ha, None, hb, None, 0, out, 0, count)
    graph = g.graph_end()
    assert g.get_option("mul_sum_fused") == before + 1
    A2, B2 = operands(o, K, count, 0, 0x6A2)
    for k in range(K):
        g.ct_upload(ha[k], 0, A2[k])
        g.ct_upload(hb[k], 0, B2[k])
    g.graph_launch(graph)
    assert np.array_equal(g.ct_download(out, 0, count), expected(o, A2, B2, 0))
    g.free(graph)
    for h in ha + hb + [out]:
        g.free(h)


# ------------------------------------------------------------------ 9. behind queued calls
@pytest.mark.parametrize("defer", [1, 2])
def test_the_call_sees_the_result_of_a_queued_add(defer):
    o, g = fresh_context("tiny")
    try:
        K, count = 3, 1
        A, B = operands(o, K, count, 0, 0xDEF + defer)
        x, y = inputs(o, 2, 0xD0)
        A[1, 0] = o.add(x, y)                                        # term 1 of a is produced by a queued cn_add
        ha, hb = [upload(g, A[k]) for k in range(K)], [upload(g, B[k]) for k in range(K)]
        hx, hy = upload(g, x[None, :]), upload(g, y[None, :])
        g.ct_upload(ha[1], 0, inputs(o, 1, 0xD1))                    # (something else until the add has run)
        out = g.ct_alloc(count)
        g.set_option("defer", defer)
        before = g.get_option("mul_sum_fused")
        g.add(hx, 0, hy, 0, ha[1], 0, 1)
        g.mul_relin_sum(ha, None, hb, None, 0, out, 0, count)
        assert g.get_option("pending_calls") == 0, "the call runs at once"
        got = g.ct_download(out, 0, count)
        g.set_option("defer", 0)
        assert g.get_option("mul_sum_fused") == before + 1
        assert np.array_equal(got, expected(o, A, B, 0))
    finally:
        g.close()


# ------------------------------------------------------------------ 10. groups
# (kernel_launches, Multiplication, Relinarization, mul_sum_groups) of the call below on the commit before cn_mul_plan.h (profiles/mul_plan_refactor.md): the groups
# and the chunks of products inside a group are mul_batch's, a count that moves is a boundary that moved
GROUPED_LITERALS = (252, 54, 54, 3)


def test_outputs_run_in_groups_when_the_scratch_limit_is_small():
    """K = 9, count = 6 on tiny: the products of one output are 9 * 3 * 3 * 1024 * 8 = 663 552 bytes, its digit sums 12 * 1024 * 8 = 98 304; a limit of 0.00224 GiB
    (2.4 MB) holds two or three outputs beside the scratch of one multiply (0.4-0.5 MB), so the six outputs take at least two groups"""
    from cryptonets_amd._native import Context
    p = PARAMS["tiny"]
    o, _g = fresh_context("tiny")
    _g.close()
    old = os.environ.get("CN_SCRATCH_GB")
    os.environ["CN_SCRATCH_GB"] = "0.00224"
    try:
        g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    finally:
        if old is None:
            del os.environ["CN_SCRATCH_GB"]
        else:
            os.environ["CN_SCRATCH_GB"] = old
    try:
        g.set_relin_key(o.relin_key())
        K, count = 9, 6
        A, B = operands(o, K, count, 0, 0x620)
        ha, hb = [upload(g, A[k]) for k in range(K)], [upload(g, B[k]) for k in range(K)]
        out = g.ct_alloc(count)
        before, s0 = g.get_option("mul_sum_fused"), g.stats()
        g.mul_relin_sum(ha, None, hb, None, 0, out, 0, count)
        groups, s1 = g.get_option("mul_sum_groups"), g.stats()
        moved = tuple(s1[c] - s0[c] for c in ("kernel_launches", "Multiplication", "Relinarization")) + (groups,)
        print("mul_sum_groups", groups, "moved", moved)
        assert g.get_option("mul_sum_fused") == before + 1
        assert groups >= 2
        assert moved == GROUPED_LITERALS
        assert np.array_equal(g.ct_download(out, 0, count), expected(o, A, B, 0))
    finally:
        g.close()


# ------------------------------------------------------------------ 11. wrapper
def test_wrapper_runs_both_encrypted_products_through_the_call():
    """hewrapper on the device at N = 1024 (tiny's moduli, one plaintext prime): DenseMatrixBySparseVectorMultiply with K = 4 encrypted columns of two blocks
    x an encrypted sparse vector, and DotProduct of two encrypted two-block vectors, decrypted to the integer results"""
    from cryptonets_amd.hewrapper import EMatrixFormat, EncryptedSealBfvFactory, EVectorFormat
    from oracle_backend import OracleHarness

    class TinyHarness(OracleHarness):
        def default_coeff_modulus(self, n):
            assert n == 1024
            return list(PARAMS["tiny"]["q"])

    h = TinyHarness("gpu")
    f = EncryptedSealBfvFactory([PARAMS["tiny"]["t"]], 1024, 10, 20, -1, client_factory=h.client_factory, context_factory=h, galois=True)
    env = f.AllocateComputationEnv()
    ctxs = [e.ctx for e in env.Environments]
    assert all(hasattr(c, "mul_relin_sum") for c in ctxs)
    rng = np.random.default_rng(0x11)
    dim, K = 1500, 4                                                 # two blocks of 1024 slots
    M = rng.integers(-3, 4, size=(dim, K)).astype(float)
    v = rng.integers(-3, 4, size=K).astype(float)
    mat = f.GetEncryptedMatrix(M, EMatrixFormat.ColumnMajor, 1.0)
    sparse = f.GetEncryptedVector(v, EVectorFormat.sparse, 1.0)
    before = [c.get_option("mul_sum_fused") for c in ctxs]
    got = mat.Mul(sparse, env).Decrypt(env)
    assert np.array_equal(np.asarray(got, dtype=float), M @ v)
    mid = [c.get_option("mul_sum_fused") for c in ctxs]
    assert all(b == a + 1 for a, b in zip(before, mid))
    assert all(c.get_option("mul_sum_groups") == 1 for c in ctxs)
    x, y = rng.integers(-1, 2, size=dim).astype(float), rng.integers(-1, 2, size=dim).astype(float)
    ex, ey = f.GetEncryptedVector(x, EVectorFormat.dense, 1.0), f.GetEncryptedVector(y, EVectorFormat.dense, 1.0)
    assert ex.DotProduct(ey, env).Decrypt(env)[0] == float(x @ y)
    after = [c.get_option("mul_sum_fused") for c in ctxs]
    assert all(b == a + 1 for a, b in zip(mid, after))
    for c in ctxs:
        c.close()
