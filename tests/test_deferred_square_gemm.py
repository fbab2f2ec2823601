"""Deferred squarings that feed the next dense layer (`cn_set_option("defer_square_gemm", 1)`, csrc/cn_defer.hip).

The reference's SquareActivation + PoolLayer issue one `cn_mul_relin(a, a)` per column and one `cn_scalar_dot` + `cn_add_plain` + `cn_free` per output.
A layer-boundary flush of the deferred queue runs only the Multiply half of the squarings it launches ("parks" them); the next flush runs the scalar
products that read them in cn_square_gemm's second half - one key switch per dense OUTPUT - or relinearises every product into its own array first.
Every comparison here is exact equality of u64 ciphertext words: with the immediate calls (`defer` = 0), with the batched entry points and with the oracle.

How the boundary is reached.  The queue flushes at a layer boundary when a heavy call (scalar product, multiplication) arrives whose operand is the queued
result of another heavy call (heavy depth 2), and only if at least DEFER_FLUSH_MIN = 64 calls are queued.  The toy layers are smaller, so independent queued
additions (`_fill`: not heavy, each into an array of its own) make up the number: in front of squarings of uploaded ciphertexts (heavy depth 1: they never trigger a
flush themselves) so that the dense layer's first scalar product (depth 2) finds 64 calls queued.  `defer_pending_products` is asserted right behind the call that
is meant to trigger the boundary.
"""
import os
import sys

import numpy as np
import pytest

from conftest import PARAMS, get_gpu, get_oracle
from test_deferred import _fresh, _small_network
from test_square_gemm import fresh_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

def res(w, t):
    return np.mod(np.asarray(w, dtype=np.int64), t).astype(np.uint64)


def _upload_each(g, cts):
    hs = []
    for c in cts:
        h = g.ct_alloc(1)
        g.ct_upload(h, 0, c[None, :])
        hs.append(h)
    return hs


_OWN = {}


def _defer(g, mode):
    """cn_set_option("defer", mode); the tests switch "defer_square_gemm" on themselves while they queue and put the context's own value back behind them"""
    if mode:
        _OWN.setdefault(id(g), g.get_option("defer_square_gemm"))
        g.set_option("defer_square_gemm", 1)
    g.set_option("defer", mode)
    if not mode and id(g) in _OWN:
        g.set_option("defer_square_gemm", _OWN.pop(id(g)))


def _fill(g, a, b, count):
    """`count` independent queued additions (each into an array of its own): they only make up the number of queued calls a boundary flush asks for"""
    tmp = [g.ct_alloc(1) for _ in range(count)]
    for h in tmp:
        g.add(a, 0, b, 0, h, 0)
    return tmp


def _squares(g, hs, fill=30):
    """SquareActivation: one Multiply + Relinearize per column, behind `fill` independent additions.  Returns (r_k handles, the additions' outputs)"""
    tmp = _fill(g, hs[0], hs[1], fill)
    rs = []
    for h in hs:
        r = g.ct_alloc(1)
        g.mul_relin(h, 0, h, 0, r, 0)
        rs.append(r)
    return rs, tmp


def _dense(g, rs, W, ph, bias_idx, after_first=None):
    """PoolLayer on separate handles: conv = Mul(column list); res = conv.Add(bias); conv.Dispose().  W [O, len(rs)]; handle 0 in rs = padded tap"""
    outs = []
    for o in range(W.shape[0]):
        conv, r = g.ct_alloc(1), g.ct_alloc(1)
        g.scalar_dot(rs, [0] * len(rs), W[o], conv, 0)
        if o == 0 and after_first:
            after_first()
        g.add_plain(conv, 0, ph, int(bias_idx[o]), r, 0)
        g.free(conv)
        outs.append(r)
    return outs


def _weights(rng, O, K, t):
    """signed weights in +-30, one exact zero; the last column belongs to the padded tap"""
    W = rng.integers(-30, 31, size=(O, K + 1))
    W[W == 0] = 7
    W[1, 2] = 0
    return res(W, t)


def _layer(g, cts, W, bias, defer, expect_parked=True, variant=None, check=None, switch=1):
    """40 x cn_mul_relin(h, h -> r_k); O x (cn_scalar_dot over every r_k and one padded tap -> tmp, cn_add_plain(tmp, bias) -> out_o, cn_free(tmp)); free every r_k;
    download.  Returns (words [O], fused groups counted, Relinarization counted).  variant / check: the ways out of the fused form (test 3)"""
    K, O = len(cts), W.shape[0]
    hs = _upload_each(g, cts)
    ph = g.pt_alloc(len(bias))
    g.pt_upload(ph, 0, bias)
    g.sync()
    g.stats(reset=True)
    fused0 = g.get_option("defer_square_gemm_fused")
    default = g.get_option("defer_square_gemm")         # (the tests set the switch themselves and put the context's own value back)
    g.set_option("defer_square_gemm", switch)
    g.set_option("defer", defer)
    extra = {}
    try:
        rs, tmp = _squares(g, hs)                        # 30 + 40 calls queued, none of heavy depth 2
        assert g.get_option("defer_pending_products") == 0

        def parked():
            if defer:
                assert g.get_option("defer_pending_products") == (K if expect_parked else 0)
            if variant == "download_one":                 # (c) a demand flush with products pending
                extra["r5"] = g.ct_download(rs[5], 0, 1)[0]
                assert g.get_option("defer_pending_products") == 0
            if variant == "stats":                        # (j) cn_stats_get between the layers
                st = g.stats()
                assert st["Multiplication"] == K and st["Relinarization"] == K
                assert g.get_option("pending_calls") == 0 and g.get_option("defer_pending_products") == 0

        terms = rs + ([hs[0]] if variant == "foreign_term" else [0])
        outs = _dense(g, terms, W, ph, np.arange(O) % len(bias), after_first=parked)
        if variant == "extra_reader":                     # (b) a queued addition reads r_3 as well
            extra["sum"] = g.ct_alloc(1)
            g.add(rs[3], 0, rs[4], 0, extra["sum"], 0)
        if variant == "overwrite":                        # (d) a queued call writes r_7 behind its readers; r_7 is released like the others, so that at the
            g.add(hs[0], 0, hs[1], 0, rs[7], 0)           # deciding flush (a), (b) and (c) hold and (d) alone fails
        keep = rs[2] if variant == "keep_one" else None   # (a) one r_k is still the caller's at the download
        for r in rs:
            if r != keep:
                g.free(r)
        got = np.stack([g.ct_download(h, 0, 1)[0] for h in outs])
        assert g.get_option("defer_pending_products") == 0 and g.get_option("pending_calls") == 0
        if keep:
            extra["kept"] = g.ct_download(keep, 0, 1)[0]
            g.free(keep)
        if "sum" in extra:
            h = extra["sum"]
            extra["sum"] = g.ct_download(h, 0, 1)[0]
            g.free(h)
        relin = g.stats()["Relinarization"]
    finally:
        g.set_option("defer", 0)
        g.set_option("defer_square_gemm", default)
    for h in hs + outs + tmp + [ph]:
        g.free(h)
    if check:
        check(extra)
    return got, g.get_option("defer_square_gemm_fused") - fused0, relin


@pytest.fixture(scope="module")
def tiny40():
    """40 fresh ciphertexts of the `tiny` ring, two bias plaintexts, the oracle's squarings: computed once, shared, never written"""
    o = get_oracle("tiny", galois=False)
    rng = np.random.default_rng(20251018)
    cts = _fresh(o, rng, 40)
    bias = np.stack([o.encode(np.full(o.n, b, dtype=np.uint64)) for b in (5, 12000)])
    return o, cts, bias, o.mul_relin_batch(cts, cts)


# ---------------------------------------------------------------- 1. the fused form gives the oracle's words
@pytest.mark.parametrize("O", [4, 16])
def test_fused_form_gives_the_oracle_words(O, tiny40):
    """O = 4: the FP64 digit GEMM; O = 16: the matrix-core form (the shape ("tiny", 40, 16) of tests/test_square_gemm.py)"""
    o, cts, bias, sq = tiny40
    g = get_gpu("tiny", galois=False)
    W = _weights(np.random.default_rng(100 + O), O, 40, o.t)
    idx = np.tile(np.append(np.arange(40, dtype=np.int32), -1), (O, 1)).astype(np.int32)
    exp = o.add_plain_batch(o.scalar_gemm(sq, W, idx=idx), bias[np.arange(O) % 2])
    live0 = g.live_handles()
    now, fused, relin = _layer(g, cts, W, bias, 0)
    assert fused == 0 and relin == 40
    assert np.array_equal(now, exp)
    for defer in (1, 2):
        mfma0 = g.get_option("digit_gemm_mfma")
        got, fused, relin = _layer(g, cts, W, bias, defer)
        assert fused == 1, "defer=%d" % defer
        assert relin == 40
        assert (g.get_option("digit_gemm_mfma") - mfma0) == (1 if O == 16 else 0)
        assert np.array_equal(got, now), "defer=%d" % defer
        assert np.array_equal(got, exp), "defer=%d" % defer
        assert g.get_option("defer_pending_products") == 0
        g.sync()
        assert g.live_handles() == live0


# ---------------------------------------------------------------- 2. the literal replay
@pytest.mark.parametrize("threads", [1, 6])
def test_literal_replay_fuses_the_dense_layer(threads, rng):
    """tools/replay_reference_calls.cpp on _small_network(12) with the dense layer widened to 16 outputs.  The network queues 30 calls for the convolution and 15
    squarings (heavy depth 2 each): 19 independent additions queued in front of it bring the queue to 49 calls at the first squaring and 63 at the last (below 64: no
    flush inside the squaring layer) and to 64 at the dense layer's first scalar product - the boundary flush that parks all 15 squarings."""
    import replay_reference_calls as rp
    o, g = get_oracle("tiny", galois=False), get_gpu("tiny", galois=False)
    n_in = 12
    cts = _fresh(o, rng, n_in)
    layers = _small_network(n_in, rng, o.t)
    O0 = layers[0]["idx"].shape[0]
    layers[1] = dict(idx=np.tile(np.arange(O0, dtype=np.int32), (16, 1)), W=res(rng.integers(-30, 31, size=(16, O0)), o.t),
                     bias_idx=np.arange(16, dtype=np.int32) % 2, square=False)
    bias = np.stack([o.encode(np.full(o.n, b, dtype=np.uint64)) for b in (3, 11)])
    ph = g.pt_alloc(2)
    g.pt_upload(ph, 0, bias)
    hin = g.ct_alloc(n_in)
    g.ct_upload(hin, 0, cts)
    h1, h2, h3 = g.ct_alloc(O0), g.ct_alloc(O0), g.ct_alloc(16)
    g.scalar_gemm(hin, layers[0]["W"], h1, 0, idx=layers[0]["idx"], bias_pt=ph, bias_idx=layers[0]["bias_idx"])
    g.mul_relin(h1, 0, h1, 0, h2, 0, O0)
    g.scalar_gemm(h2, layers[1]["W"], h3, 0, idx=layers[1]["idx"], bias_pt=ph, bias_idx=layers[1]["bias_idx"])
    ref = g.ct_download(h3, 0, 16)
    lin = o.add_plain_batch(o.scalar_gemm(cts, layers[0]["W"], idx=layers[0]["idx"]), bias[layers[0]["bias_idx"]])
    sq = o.mul_relin_batch(lin, lin)
    assert np.array_equal(ref, o.add_plain_batch(o.scalar_gemm(sq, layers[1]["W"], idx=layers[1]["idx"]), bias[layers[1]["bias_idx"]]))
    ins = rp.split_columns(g, hin, n_in)[None, :]
    net = rp.Replay([g], [dict(idx=L["idx"], W=[L["W"]], bias_pt=[ph], bias_idx=L["bias_idx"], square=L["square"]) for L in layers])
    for defer in (2, 1, 0):
        fused0 = g.get_option("defer_square_gemm_fused")
        _defer(g, defer)
        try:
            tmp = _fill(g, int(ins[0][0]), int(ins[0][1]), 19)
            out = net.run(ins, threads)
            got = np.stack([g.ct_download(int(h), 0, 1)[0] for h in out[0]])
        finally:
            _defer(g, 0)
        for h in list(out[0]) + tmp:
            g.free(int(h))
        assert np.array_equal(got, ref), "defer=%d" % defer
        assert g.get_option("defer_square_gemm_fused") - fused0 == (1 if defer else 0), "defer=%d" % defer
    for h in list(ins[0]) + [hin, h1, h2, h3, ph]:
        g.free(int(h))


# ---------------------------------------------------------------- 3. every way out of the fused form keeps the words and leaves the counter alone
@pytest.mark.parametrize("variant", ["keep_one", "extra_reader", "download_one", "overwrite", "foreign_term", "stats", "option_off"])
def test_ways_out_keep_the_words(variant, tiny40):
    """(a) one r_k not released before the download, (b) one r_k also read by a queued cn_add, (c) one r_k downloaded while the products are pending, (d) one r_k
    overwritten by a queued call, (e) a scalar product with a term that is not a pending array, (h) defer_square_gemm = 0, (j) cn_stats_get between the layers"""
    o, cts, bias, sq = tiny40
    g = get_gpu("tiny", galois=False)
    O = 4
    W = _weights(np.random.default_rng(7), O, 40, o.t)
    if variant == "foreign_term":
        src = np.concatenate([sq, cts[:1]])
        exp = o.add_plain_batch(o.scalar_gemm(src, W), bias[np.arange(O) % 2])
    else:
        exp = o.add_plain_batch(o.scalar_gemm(sq, W[:, :40]), bias[np.arange(O) % 2])

    def check(extra):
        if variant == "keep_one":
            assert np.array_equal(extra["kept"], sq[2])
        if variant == "extra_reader":
            assert np.array_equal(extra["sum"], o.add(sq[3], sq[4]))
        if variant == "download_one":
            assert np.array_equal(extra["r5"], sq[5])

    live0 = g.live_handles()
    off = variant == "option_off"
    for defer in (1, 2):
        got, fused, relin = _layer(g, cts, W, bias, defer, expect_parked=not off, variant=variant, check=check, switch=0 if off else 1)
        assert fused == 0, "defer=%d" % defer
        assert relin == 40
        assert np.array_equal(got, exp), "defer=%d" % defer
        g.sync()
        assert g.live_handles() == live0


def _uniform(q, n, count, seed):
    from bench import uniform_ct_words
    return uniform_ct_words(np.random.default_rng(seed), q, n, count)


def test_weights_outside_the_digit_bound_take_the_separate_steps():
    """(f) a weight of 2^20 (not small) and a row sum beyond the q_j / 2 bound.  `tiny`'s plain modulus 12289 holds no such weight: the ring of `tiny` with the
    plain modulus 7 * 2^20 + 1.  The bound there is sum |w| <= (min q_j - 1) / 2 / (2^10 - 1) = 33 587 111: forty weights of 2^20 - 1 (small) sum to 41 943 000."""
    from cryptonets_amd._native import Context
    p = PARAMS["tiny"]
    t = 7 * (1 << 20) + 1
    g = Context(p["n"], t, q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    try:
        g.keygen(5, galois=False)
        cts = _uniform(p["q"], p["n"], 40, 3)
        bias = np.zeros((1, p["n"]), dtype=np.uint64)
        bias[0, 0] = 9
        Wa = np.full((2, 41), 3, dtype=np.int64)
        Wa[0, 5] = 1 << 20                                # not a small weight
        Wb = np.full((2, 41), (1 << 20) - 1, dtype=np.int64)
        Wb[1, ::2] *= -1
        Wc = np.full((2, 41), (1 << 19) - 1, dtype=np.int64)      # within the bound: the same context does fuse
        for W, want in ((Wa, 0), (Wb, 0), (Wc, 1)):
            now, fused, _ = _layer(g, cts, res(W, t), bias, 0)
            assert fused == 0
            got, fused, relin = _layer(g, cts, res(W, t), bias, 1)
            assert fused == want and relin == 40
            assert np.array_equal(got, now)
    finally:
        g.close()


def test_xi_decomposition_takes_the_separate_steps(tiny40):
    """(g) ks_xi = 1 with the matching key: ineligible exactly as in cn_square_gemm - nothing is parked"""
    _, cts, bias, _ = tiny40
    o, g = fresh_context("tiny", xi=True)
    try:
        W = _weights(np.random.default_rng(8), 4, 40, o.t)
        idx = np.tile(np.append(np.arange(40, dtype=np.int32), -1), (4, 1)).astype(np.int32)
        sq = o.mul_relin_batch(cts, cts)
        exp = o.add_plain_batch(o.scalar_gemm(sq, W, idx=idx), bias[np.arange(4) % 2])
        got, fused, relin = _layer(g, cts, W, bias, 1, expect_parked=False)
        assert fused == 0 and relin == 40
        assert np.array_equal(got, exp)
    finally:
        g.close()


def test_released_products_without_a_reader_give_their_slots_back(tiny40):
    """(i) every r_k released with no reader at all; then new arrays (recycled ones among them) run the same layer: no stale entry.  The boundary behind the
    squarings is a scalar product that reads the queued scalar product x_0 = 1 * c_0 (heavy depth 2) and no r_k."""
    o, cts, bias, sq = tiny40
    g = get_gpu("tiny", galois=False)
    live0 = g.live_handles()
    fused0 = g.get_option("defer_square_gemm_fused")
    hs = _upload_each(g, cts)
    g.sync()
    g.stats(reset=True)
    _defer(g, 1)
    try:
        x0 = g.ct_alloc(1)
        g.scalar_dot([hs[0]], [0], [1], x0, 0)                             # heavy depth 1
        rs, tmp = _squares(g, hs)
        y = g.ct_alloc(1)
        g.scalar_dot([x0], [0], [2], y, 0)                                 # 71 calls queued, heavy depth 2: the boundary
        assert g.get_option("defer_pending_products") == 40
        for h in [x0] + rs:
            g.free(h)
        z = g.ct_alloc(1)
        g.ct_upload(z, 0, cts[3][None, :])                                 # an upload is a demand flush: nothing reads the products, all are released
        assert g.get_option("defer_pending_products") == 0
        z2 = g.ct_alloc(1)
        g.mul_relin(z, 0, z, 0, z2, 0)
        assert np.array_equal(g.ct_download(z2, 0, 1)[0], sq[3])
        assert np.array_equal(g.ct_download(y, 0, 1)[0], o.scalar_gemm(cts[:1], res([[2]], o.t))[0])
        st = g.stats()
        assert st["Relinarization"] == 41 and st["Multiplication"] == 41   # counted as for the literal calls
        for h in [y, z, z2] + tmp:
            g.free(h)
    finally:
        _defer(g, 0)
    for h in hs:
        g.free(h)
    assert g.get_option("defer_square_gemm_fused") == fused0
    # the released arrays are back in the pool: the next layer gets them again
    W = _weights(np.random.default_rng(9), 4, 40, o.t)
    idx = np.tile(np.append(np.arange(40, dtype=np.int32), -1), (4, 1)).astype(np.int32)
    got, fused, relin = _layer(g, cts, W, bias, 1)
    assert fused == 1 and relin == 40
    assert np.array_equal(got, o.add_plain_batch(o.scalar_gemm(sq, W, idx=idx), bias[np.arange(4) % 2]))
    g.sync()
    assert g.live_handles() == live0


def test_outputs_inside_a_released_handle_are_not_parked(tiny40):
    """squarings written into the elements of ONE handle of 40 ciphertexts that the caller releases before the boundary: the released buffer is one entry of the
    queue's release list, every element lies inside it - nothing is parked (a parked product would be relinearised into an array that went back to the pool at the end
    of that flush).  The same handle alive: parked, and its elements hold the oracle's words after the download."""
    o, cts, bias, sq = tiny40
    g = get_gpu("tiny", galois=False)
    live0 = g.live_handles()
    hs = _upload_each(g, cts)
    g.sync()
    g.stats(reset=True)
    for release in (True, False):
        _defer(g, 1)
        try:
            x0 = g.ct_alloc(1)
            g.scalar_dot([hs[0]], [0], [1], x0, 0)                         # heavy depth 1
            tmp = _fill(g, hs[0], hs[1], 30)
            many = g.ct_alloc(40)
            for k, h in enumerate(hs):
                g.mul_relin(h, 0, h, 0, many, k)
            if release:
                g.free(many)
            y = g.ct_alloc(1)
            g.scalar_dot([x0], [0], [2], y, 0)                             # 71 calls queued, heavy depth 2: the boundary
            assert g.get_option("defer_pending_products") == (0 if release else 40)
            if not release:
                assert np.array_equal(g.ct_download(many, 0, 40), sq)      # a demand flush: every product relinearised into its element
                assert g.get_option("defer_pending_products") == 0
                g.free(many)
            assert np.array_equal(g.ct_download(y, 0, 1)[0], o.scalar_gemm(cts[:1], res([[2]], o.t))[0])
            for h in [x0, y] + tmp:
                g.free(h)
        finally:
            _defer(g, 0)
    assert g.stats()["Relinarization"] == 80
    for h in hs:
        g.free(h)
    g.sync()
    assert g.live_handles() == live0


def test_destroy_with_products_pending(tiny40):
    """(k) cn_ctx_destroy with products pending, released arrays parked behind them: no crash, nothing left behind"""
    from cryptonets_amd._native import Context
    o, cts, bias, sq = tiny40
    p = PARAMS["tiny"]
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    g.set_relin_key(o.relin_key())
    hs = _upload_each(g, cts)
    ph = g.pt_alloc(2)
    g.pt_upload(ph, 0, bias)
    _defer(g, 1)
    rs, _ = _squares(g, hs)
    W = _weights(np.random.default_rng(10), 4, 40, o.t)
    _dense(g, rs + [0], W, ph, np.arange(4) % 2)
    assert g.get_option("defer_pending_products") == 40
    for r in rs[:20]:
        g.free(r)
    g.close()


# ---------------------------------------------------------------- 4. two layers in a row
def test_two_layers_in_a_row_both_fuse(tiny40):
    """squarings -> dense (16 outputs) -> squarings -> dense (2 outputs): the CryptoNets tail at toy size.  The first dense layer queues 32 calls and the second
    squaring layer 16: independent additions make up the 64 a boundary flush asks for, in front of the second squaring layer (its first multiplication has heavy
    depth 2 and flushes the first dense layer; the fifteen behind it read flushed values, depth 1) and in front of the second dense layer."""
    o, cts, bias, sq = tiny40
    g = get_gpu("tiny", galois=False)
    rng = np.random.default_rng(44)
    W1 = _weights(rng, 16, 40, o.t)
    W2 = res(rng.integers(-30, 31, size=(2, 16)), o.t)
    idx1 = np.tile(np.append(np.arange(40, dtype=np.int32), -1), (16, 1)).astype(np.int32)
    l1 = o.add_plain_batch(o.scalar_gemm(sq, W1, idx=idx1), bias[np.arange(16) % 2])
    sq2 = o.mul_relin_batch(l1, l1)
    exp = o.add_plain_batch(o.scalar_gemm(sq2, W2), bias[np.arange(2) % 2])
    live0 = g.live_handles()
    hs = _upload_each(g, cts)
    ph = g.pt_alloc(2)
    g.pt_upload(ph, 0, bias)
    for defer in (1, 2):
        fused0 = g.get_option("defer_square_gemm_fused")
        _defer(g, defer)
        try:
            rs, tmp = _squares(g, hs)
            o1 = _dense(g, rs + [0], W1, ph, np.arange(16) % 2, after_first=lambda: g.get_option("defer_pending_products") == 40 or pytest.fail("not parked"))
            for r in rs:
                g.free(r)
            tmp += _fill(g, hs[0], hs[1], 40)                               # 32 + 40 calls queued: the first squaring of the next layer is a boundary
            rs2 = []
            for h in o1:
                r = g.ct_alloc(1)
                g.mul_relin(h, 0, h, 0, r, 0)
                rs2.append(r)
            assert g.get_option("defer_square_gemm_fused") - fused0 == 1     # the first pair ran at that boundary
            for h in o1:
                g.free(h)
            tmp += _fill(g, hs[0], hs[1], 50)                               # 16 + 50
            o2 = _dense(g, rs2, W2, ph, np.arange(2) % 2, after_first=lambda: g.get_option("defer_pending_products") == 16 or pytest.fail("not parked"))
            for r in rs2:
                g.free(r)
            got = np.stack([g.ct_download(h, 0, 1)[0] for h in o2])
            assert g.get_option("defer_pending_products") == 0
        finally:
            _defer(g, 0)
        for h in o2 + tmp:
            g.free(h)
        assert g.get_option("defer_square_gemm_fused") - fused0 == 2, "defer=%d" % defer
        assert np.array_equal(got, exp), "defer=%d" % defer
    for h in hs + [ph]:
        g.free(h)
    g.sync()
    assert g.live_handles() == live0


# ---------------------------------------------------------------- 5. one check at C3 size
def test_c3_shape_equals_the_immediate_calls():
    """parameter set c3 (N = 8192, the CryptoNets moduli), 8 squarings -> 40 outputs (the shape ("c3", 8, 40) of tests/test_square_gemm.py: the fused key-switch
    kernel with its output table).  56 independent additions in front of the 8 squarings make up the boundary's 64."""
    p = PARAMS["c3"]
    g = get_gpu("c3", galois=False)
    o = get_oracle("c3", galois=False)
    cts = _uniform(o.q, o.n, 8, 0xC3)
    rng = np.random.default_rng(0xC38)
    W = rng.integers(-((1 << 20) - 1), 1 << 20, size=(40, 9))
    W[W == 0] = 1
    W[3, 1] = 0
    W = res(W, p["t"])
    bias = np.stack([o.encode(np.full(o.n, b, dtype=np.uint64)) for b in (5, p["t"] - 2)])

    def run(defer):
        hs = _upload_each(g, cts)
        ph = g.pt_alloc(2)
        g.pt_upload(ph, 0, bias)
        fused0 = g.get_option("defer_square_gemm_fused")
        _defer(g, defer)
        try:
            rs, tmp = _squares(g, hs, fill=56)                              # 56 + 8 calls queued
            outs = _dense(g, rs + [0], W, ph, np.arange(40) % 2, after_first=(lambda: g.get_option("defer_pending_products") == 8 or pytest.fail("not parked")) if defer else None)
            for r in rs:
                g.free(r)
            got = np.stack([g.ct_download(h, 0, 1)[0] for h in outs])
        finally:
            _defer(g, 0)
        for h in hs + outs + tmp + [ph]:
            g.free(h)
        return got, g.get_option("defer_square_gemm_fused") - fused0

    live0 = g.live_handles()
    now, fused = run(0)
    assert fused == 0
    got, fused = run(1)
    assert fused == 1
    assert np.array_equal(got, now)
    g.sync()
    assert g.live_handles() == live0
