"""The chunking of the BEHZ multiply family (mul_batch, csrc/cn_mul_plan.h) on the device: every site that cuts a batch of products into chunks by the scratch limit,
under a limit derived here so that 7 ciphertexts run as chunks of 3, 3 and 1 - more than one full chunk and a ragged last one.

Sets: "tiny" (N = 1024, k = 3, FP64 policies) and the N = 1024 integer-policy set of tests/size_policy_sets.py (60-, 60- and 50-bit limbs).  Every case makes its own
context with CN_SCRATCH_GB set while the context is created (the limit is read once, there).  The limit is 3.5 x the bytes a site counts per ciphertext:
    one product chain    al(((2 or 4) (k + kb) N + 3 (k + kb) N) 8) + 1024          (squaring: 2 - one operand extended; general product: 4)
    cn_multiply          that
    cn_mul_relin         + al(3 k N 8)                                              (the size-3 product)
    queued cn_mul_relin  + al(3 k N 8) + 3 x 8 + 64                                 (and three table entries)
    parked squarings     + 8 + 64
    cn_square_gemm       the same per product, beside al(7 x 3 k N 8) + al(O rl_tot N 4 or 8) + 8192 for all products and the digit sums
so a chunk is floor(3.5) = 3 ciphertexts.  Parked products may take a quarter of the limit at the most (DeferSwitches::park_max), and a product is 3 k N 8 bytes
where its chain counts 5 (k + kb) N 8, more than three times as many: whatever parks fits one chunk.  That case therefore parks 3 squarings, the most this limit
takes, and consumes them in a scalar product.  cn_mul_relin_sum in groups is test_outputs_run_in_groups_when_the_scratch_limit_is_small (tests/test_gpu_mul_relin_sum.py).

Every result is compared word for word with the oracle.  LITERALS: (kernel_launches, Multiplication, Relinarization, square_gemm_fused, mul_sum_groups) of every case,
measured on the commit BEFORE cn_mul_plan.h with this same file (profiles/mul_plan_refactor.md): a count that moves is a chunk boundary or a kernel form that moved.
"""
import os

import numpy as np
import pytest

from conftest import PARAMS, get_oracle
from size_policy_sets import SETS as SIZE_POLICY_SETS
from test_deferred import _fresh
from test_deferred_square_gemm import _dense, _squares, _upload_each, _weights
from test_square_gemm import expected as square_gemm_expected, inputs, res, small_weights

pytestmark = pytest.mark.gpu

SETS = {"tiny": PARAMS["tiny"], "u64": SIZE_POLICY_SETS["sp-u64-n1024"]}
COUNT = 7
LITERALS = {
    ("tiny", "multiply"): (27, 7, 0, 0, 0),                  # 3 chunks x (2 extensions, 4 transforms, 2 k_intt_tensor, floor)
    ("tiny", "mul_relin-square"): (16, 7, 7, 0, 0),          # 3 x (extension, 2 fused squarings, floor) + key switches of 1, 1 and 2 launches: the scratch limit is
    ("tiny", "mul_relin-general"): (31, 7, 7, 0, 0),         # also the key-switch arena's (KsSwitches::arena_max), three ciphertexts' 12 digit partials pass it
    ("tiny", "queued"): (16, 7, 7, 0, 0),
    ("tiny", "parked"): (8, 3, 3, 0, 0),
    ("tiny", "square_gemm"): (16, 7, 7, 1, 0),               # 3 x 4 + GEMM, digit GEMM, a two-launch key switch of the two outputs
    ("u64", "multiply"): (27, 7, 0, 0, 0),
    ("u64", "mul_relin-square"): (24, 7, 7, 0, 0),           # 3 x (extension, 2 transforms, 2 k_intt_tensor, floor) + 3 two-launch key switches
    ("u64", "mul_relin-general"): (33, 7, 7, 0, 0),
    ("u64", "queued"): (24, 7, 7, 0, 0),
    ("u64", "parked"): (18, 3, 3, 0, 0),
    ("u64", "square_gemm"): (17, 7, 7, 0, 0),                # the two steps: cn_mul_relin under the same limit (two chunks), the GEMM
}


def al(b):
    return (b + 255) & ~255


def chain_bytes(k, kb, n, square):
    return al(((2 if square else 4) * (k + kb) * n + 3 * (k + kb) * n) * 8) + 1024


@pytest.fixture(scope="module", params=sorted(SETS))
def keyed(request):
    """(set name, oracle with a relinearisation key, 7 + 7 operand ciphertexts with edge residues, the oracle's products and relinearised products): computed once"""
    name = request.param
    if name == "tiny":
        o = get_oracle("tiny", galois=False)
    else:
        from oracle.cno import Oracle
        p = SETS[name]
        o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
        o.keygen(29, galois=False)
    A, B = inputs(o, COUNT, 0x7A), inputs(o, COUNT, 0x7B)[::-1].copy()
    return name, o, A, B, o.mul_relin_batch(A, A), o.mul_relin_batch(A, B)


def limited(name, o, site_bytes, fixed=0):
    """a context of the set whose scratch limit is fixed + 3.5 x site_bytes(k, kb, N)"""
    from cryptonets_amd._native import Context
    p = SETS[name]
    probe = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    kb = probe.get_option("aux_primes")
    probe.close()
    k, n = len(p["q"]), p["n"]
    per = site_bytes(k, kb, n)
    smax = (fixed(k, n) if fixed else 0) + 3 * per + per // 2
    old = os.environ.get("CN_SCRATCH_GB")
    os.environ["CN_SCRATCH_GB"] = repr(smax / 2.0 ** 30)              # (a power of two: the library's product gives smax back exactly)
    try:
        g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    finally:
        if old is None:
            del os.environ["CN_SCRATCH_GB"]
        else:
            os.environ["CN_SCRATCH_GB"] = old
    g.set_relin_key(o.relin_key())
    return g


def upload(g, X):
    h = g.ct_alloc(len(X))
    g.ct_upload(h, 0, X)
    return h


class Counted:
    """the five figures a block moved"""

    def __init__(self, g):
        self.g = g

    def __enter__(self):
        self.g.sync()
        self.s0, self.f0 = self.g.stats(), self.g.get_option("square_gemm_fused")
        return self

    def __exit__(self, *exc):
        s1 = self.g.stats()
        self.got = tuple(s1[c] - self.s0[c] for c in ("kernel_launches", "Multiplication", "Relinarization")) + \
            (self.g.get_option("square_gemm_fused") - self.f0, self.g.get_option("mul_sum_groups"))


def settle(name, case, c):
    print("LITERAL", (name, case), c.got)
    assert LITERALS[(name, case)] == c.got


def test_multiply_of_two_operands(keyed):
    name, o, A, B, _, _ = keyed
    g = limited(name, o, lambda k, kb, n: chain_bytes(k, kb, n, False))
    try:
        ha, hb, out3 = upload(g, A), upload(g, B), g.ct_alloc(COUNT, 3)
        with Counted(g) as c:
            g.multiply(ha, 0, hb, 0, out3, 0, COUNT)
        assert np.array_equal(g.ct_download(out3, 0, COUNT, size=3), np.stack([o.multiply(a, b) for a, b in zip(A, B)]))
        settle(name, "multiply", c)
    finally:
        g.close()


@pytest.mark.parametrize("square", [True, False], ids=["square", "general"])
def test_mul_relin(keyed, square):
    name, o, A, B, AA, AB = keyed
    g = limited(name, o, lambda k, kb, n: chain_bytes(k, kb, n, square) + al(3 * k * n * 8))
    try:
        ha, hb, out = upload(g, A), upload(g, B), g.ct_alloc(COUNT)
        with Counted(g) as c:
            g.mul_relin(ha, 0, ha if square else hb, 0, out, 0, COUNT)
        assert np.array_equal(g.ct_download(out, 0, COUNT), AA if square else AB)
        settle(name, "mul_relin-" + ("square" if square else "general"), c)
    finally:
        g.close()


def test_queued_squarings_flushed(keyed):
    """"defer" 1: seven cn_mul_relin(h, h) calls on ciphertexts of their own are queued and run as one group at the download (flush_mulrelin_group)"""
    name, o, A, _, AA, _ = keyed
    g = limited(name, o, lambda k, kb, n: chain_bytes(k, kb, n, True) + al(3 * k * n * 8) + 3 * 8 + 64)
    try:
        hs = _upload_each(g, A)
        outs = [g.ct_alloc(1) for _ in hs]
        with Counted(g) as c:
            g.set_option("defer", 1)
            for h, r in zip(hs, outs):
                g.mul_relin(h, 0, h, 0, r, 0)
            assert g.get_option("pending_calls") == COUNT
            first = g.ct_download(outs[0], 0, 1)[0]
            assert g.get_option("pending_calls") == 0
            g.set_option("defer", 0)
        got = np.stack([first] + [g.ct_download(r, 0, 1)[0] for r in outs[1:]])
        assert np.array_equal(got, AA)
        settle(name, "queued", c)
    finally:
        g.close()


def test_parked_squarings_consumed_by_a_scalar_product(keyed):
    """"defer" 1 and "defer_square_gemm" 1: three squarings behind 61 independent additions, then a dense layer of two outputs whose first scalar product reaches the
    layer boundary (64 calls queued): the flush parks the squarings where the context takes the fused form (park_squarings; the integer-policy set relinearises them
    at once), the download runs the dense layer"""
    name, o, _, _, _, _ = keyed
    g = limited(name, o, lambda k, kb, n: chain_bytes(k, kb, n, True) + 8 + 64)
    try:
        cts = _fresh(o, np.random.default_rng(0x9A), 3)
        bias = np.stack([o.encode(np.full(o.n, b, dtype=np.uint64)) for b in (5, 12000)])
        W = _weights(np.random.default_rng(0x9B), 2, 3, o.t)
        idx = np.tile(np.append(np.arange(3, dtype=np.int32), -1), (2, 1)).astype(np.int32)
        exp = o.add_plain_batch(o.scalar_gemm(o.mul_relin_batch(cts, cts), W, idx=idx), bias)
        hs = _upload_each(g, cts)
        ph = g.pt_alloc(2)
        g.pt_upload(ph, 0, bias)
        parked = []
        with Counted(g) as c:
            g.set_option("defer_square_gemm", 1)
            g.set_option("defer", 1)
            rs, tmp = _squares(g, hs, fill=61)
            outs = _dense(g, rs + [0], W, ph, np.arange(2), after_first=lambda: parked.append(g.get_option("defer_pending_products")))
            for r in rs:
                g.free(r)
            got = np.stack([g.ct_download(h, 0, 1)[0] for h in outs])
            g.set_option("defer", 0)
        print("PARKED", name, parked)
        assert parked == [3 if name == "tiny" else 0]               # square_gemm_ctx_ok: FP64 policies only
        assert np.array_equal(got, exp)
        settle(name, "parked", c)
    finally:
        g.close()


def test_square_gemm_with_its_product_loop_chunked(keyed):
    """7 inputs -> 2 outputs: all products and the digit sums lie beside the scratch of a chunk of three product chains"""
    name, o, A, _, _, _ = keyed
    p = SETS[name]
    tot = sum((m.bit_length() + p["dbc"] - 1) // p["dbc"] for m in p["q"])
    O = 2
    g = limited(name, o, lambda k, kb, n: chain_bytes(k, kb, n, True),
                fixed=lambda k, n: al(COUNT * 3 * k * n * 8) + al(O * tot * n * 4) + 8192)      # (int32 digit sums; doubles are 0.34 of a chain more: still 3)
    try:
        t = p["t"]
        W = res(small_weights(np.random.default_rng(0x5C), O, COUNT, t, 1000), t)
        h, out = upload(g, A), g.ct_alloc(O)
        plan = g.gemm_plan(W)
        with Counted(g) as c:
            g.square_gemm(plan, h, 0, out, 0)
        assert np.array_equal(g.ct_download(out, 0, O), square_gemm_expected(o, A, W))
        assert c.got[3] == (1 if name == "tiny" else 0)             # the fused form needs the FP64 policies
        settle(name, "square_gemm", c)
    finally:
        g.close()
