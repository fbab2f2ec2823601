"""GPU: modulus switching (cn_mod_switch, cn_ctx_create_level) - word-exact against the model of tests/modswitch_model.py, the keys of a level
context against the host slice of its parent's, the evaluator on a level context against an oracle over q[:l] with the sliced keys, the ordering
of a switch between two contexts' streams, the argument errors, and the one-limb refusals."""
import numpy as np
import pytest

from conftest import PARAMS, get_oracle
from modswitch_model import digits, slice_key, slice_poly, switch_residues

pytestmark = pytest.mark.gpu


def qs(name):
    p = PARAMS[name]
    if p["q"] is not None:
        return list(p["q"])
    from oracle.cno import COEFF_MODULUS_128
    return list(COEFF_MODULUS_128[p["n"]])


def ctx(name, **opt):
    from cryptonets_amd._native import Context
    p = PARAMS[name]
    g = Context(p["n"], p["t"], q=qs(name), dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    for k, v in opt.items():
        g.set_option(k, v)
    return g


def rand_cts(rng, q, n, count, size):
    return np.stack([np.concatenate([rng.integers(0, m, size=n, dtype=np.uint64) for _ in range(size) for m in q]) for _ in range(count)])


def edge_cts(q, n, size):
    """coefficients 0, q_j - 1 and around q_last / 2 in every limb"""
    ql = q[-1]
    vals = [0, 1, ql // 2 - 1, ql // 2, ql // 2 + 1, ql - 1]
    row = np.concatenate([np.array([(vals[i % len(vals)] if j == len(q) - 1 else (m - 1 if i % 3 == 0 else i % m)) for i in range(n)], dtype=np.uint64)
                          for _ in range(size) for j, m in enumerate(q)])
    return row[None, :]


# ------------------------------------------------------------------ the kernel, word for word
@pytest.mark.parametrize("name", ["tiny", "c2", "c3", "c4", "c5", "n16k7"])
def test_mod_switch_words_every_level(name):
    g = ctx(name)
    q, n = g.q, g.n
    rng = np.random.default_rng(7)
    for size in (2, 3):
        src = np.concatenate([edge_cts(q, n, size), rand_cts(rng, q, n, 7, size)])
        h = g.ct_alloc(len(src) + 1, size)
        g.ct_upload(h, 1, src)
        for limbs in range(g.k - 1, 0, -1):
            lv = g.level(limbs)
            out = lv.ct_alloc(len(src) + 2, size)
            g.mod_switch(h, 1, 1, lv, out, 0)                           # count 1
            g.mod_switch(h, 2, 7, lv, out, 2)                           # count 7, non-zero ii / oi
            got = lv.ct_download(out, 0, 9, size)
            exp = switch_residues(src, q, n, limbs).reshape(len(src), -1)
            assert np.array_equal(got[0], exp[0]), (size, limbs)
            assert np.array_equal(got[2:9], exp[1:8]), (size, limbs)
            lv.free(out)
        g.free(h)


def test_mod_switch_words_845_and_chained_levels():
    g = ctx("c3")
    q, n = g.q, g.n
    rng = np.random.default_rng(8)
    src = rand_cts(rng, q, n, 845, 2)
    h = g.ct_alloc(845, 2)
    g.ct_upload(h, 0, src)
    l4 = g.level(4)
    o4 = l4.ct_alloc(845, 2)
    g.mod_switch(h, 0, 845, l4, o4, 0)
    assert np.array_equal(l4.ct_download(o4, 0, 845), switch_residues(src, q, n, 4).reshape(845, -1))
    # k -> l directly == k -> l + 1 -> l through a chained child
    l2 = g.level(2)
    l43 = l4.level(3)
    l432 = l43.level(2)
    assert l432.parent is l43 and l43.parent is l4 and l4.parent is g and l432.limbs == 2
    d = l2.ct_alloc(845, 2)
    g.mod_switch(h, 0, 845, l2, d, 0)
    o3 = l43.ct_alloc(845, 2)
    l4.mod_switch(o4, 0, 845, l43, o3, 0)
    c2 = l432.ct_alloc(845, 2)
    l43.mod_switch(o3, 0, 845, l432, c2, 0)
    assert np.array_equal(l2.ct_download(d, 0, 845), l432.ct_download(c2, 0, 845))
    # a direct switch into a chained level of another branch (same prefix) is accepted too
    e = l432.ct_alloc(2, 2)
    g.mod_switch(h, 0, 2, l432, e, 0)
    assert np.array_equal(l432.ct_download(e, 0, 2), l2.ct_download(d, 0, 2))


# ------------------------------------------------------------------ keys of a level context
def keyed(name, f64=True, ks_xi=False, galois=True, seed=11):
    from oracle.cno import Oracle
    p = PARAMS[name]
    if ks_xi:
        o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], ks_xi=True)
        o.keygen(seed, galois=galois)
    else:
        o = get_oracle(name, galois=galois, seed=seed)
    g = ctx(name, f64=int(f64), ks_xi=int(ks_xi))
    g.set_relin_key(o.relin_key())
    if galois:
        for i, e in enumerate(o.galois_elts()):
            g.set_galois_key(e, o.galois_key(i))
    g.set_public_key(o.public_key())
    g.set_secret_key(o.secret_key())
    return o, g


def level_oracle(o, name, limbs, galois=True):
    from oracle.cno import Oracle
    p = PARAMS[name]
    lo = Oracle(p["n"], p["t"], q=o.q[:limbs], dbc=p["dbc"], gdbc=p["gdbc"])
    lo.import_keys(slice_poly(o.secret_key(), o.k, o.n, limbs, 1), slice_poly(o.public_key(), o.k, o.n, limbs, 2))
    lo.import_relin_key(slice_key(o.relin_key(), o.k, o.n, digits(o.q, p["dbc"]), limbs))
    if galois:
        for i, e in enumerate(o.galois_elts()):
            lo.import_galois_key(e, slice_key(o.galois_key(i), o.k, o.n, digits(o.q, p["gdbc"]), limbs))
    return lo


@pytest.mark.parametrize("name,limbs", [("c3", 3), ("c3", 2), ("tiny", 1)])
def test_level_keys_are_the_slice_of_the_parents(name, limbs):
    o, g = keyed(name)
    lv = g.level(limbs)
    k, n = g.k, g.n
    p = PARAMS[name]
    assert np.array_equal(lv.get_key(0), slice_key(g.get_key(0), k, n, digits(g.q, p["dbc"]), limbs))
    for e in o.galois_elts()[:3]:
        assert np.array_equal(lv.get_key(1, e), slice_key(g.get_key(1, e), k, n, digits(g.q, p["gdbc"]), limbs))
    assert np.array_equal(lv.get_key(2), slice_poly(g.get_key(2), k, n, limbs, 2))
    assert np.array_equal(lv.get_key(3), slice_poly(g.get_key(3), k, n, limbs, 1))
    assert lv.get_option("f64") == g.get_option("f64") and lv.get_option("ks_xi") == g.get_option("ks_xi")


def test_level_context_refuses_key_generation_and_uploads():
    from cryptonets_amd._native import CnError
    o, g = keyed("tiny", galois=False)
    lv = g.level(2)
    for call in (lambda: lv.keygen(1), lambda: lv.set_relin_key(lv.get_key(0)), lambda: lv.set_public_key(lv.get_key(2)),
                 lambda: lv.set_secret_key(lv.get_key(3)), lambda: lv.load_key(0, lv.get_key(0)), lambda: lv.set_option("ks_xi", 1),
                 lambda: lv.set_galois_key(3, np.zeros(lv.key_words(True), dtype=np.uint64))):
        with pytest.raises(CnError) as e:
            call()
        assert e.value.code == -1


# ------------------------------------------------------------------ the evaluator on a level context
def up(g, cts, size=2):
    h = g.ct_alloc(len(cts), size)
    g.ct_upload(h, 0, cts)
    return h


@pytest.mark.parametrize("name,limbs,f64", [("c3", 3, True), ("c3", 3, False), ("c3", 2, True), ("c4", 2, True), ("c4", 2, False)])
def test_evaluator_on_a_level_context_matches_the_prefix_oracle(name, limbs, f64):
    o, g = keyed(name, f64=f64)
    lv = g.level(limbs)
    lo = level_oracle(o, name, limbs)
    rng = np.random.default_rng(limbs)
    t, n = o.t, o.n
    vals = rng.integers(0, 8, size=(4, n), dtype=np.uint64)
    cts = np.stack([lo.encrypt(lo.encode(v)) for v in vals])
    h = up(lv, cts)
    out = lv.ct_alloc(4, 2)
    lv.add(h, 0, h, 1, out, 0)
    lv.sub(h, 2, h, 3, out, 1)
    lv.negate(h, 1, out, 2)
    pt = lv.pt_alloc(1)
    plain = lo.encode(rng.integers(1, 8, size=n, dtype=np.uint64))
    lv.pt_upload(pt, 0, plain[None, :])
    lv.add_plain(h, 0, pt, 0, out, 3)
    got = lv.ct_download(out, 0, 4)
    assert np.array_equal(got[0], lo.add(cts[0], cts[1]))
    assert np.array_equal(got[1], lo.sub(cts[2], cts[3]))
    assert np.array_equal(got[2], lo.negate(cts[1]))
    assert np.array_equal(got[3], lo.add_plain(cts[0], plain))
    lv.mul_plain(h, 0, pt, 0, out, 0, 1, pt_stride=0)
    assert np.array_equal(lv.ct_download(out, 0, 1)[0], lo.multiply_plain(cts[0], plain))
    # multiply / relinearize / mul_relin
    m3 = lv.ct_alloc(1, 3)
    lv.multiply(h, 0, h, 1, m3, 0)
    e3 = lo.multiply(cts[0], cts[1])
    assert np.array_equal(lv.ct_download(m3, 0, 1, 3)[0], e3)
    lv.relinearize(m3, 0, out, 0)
    assert np.array_equal(lv.ct_download(out, 0, 1)[0], lo.relinearize(e3))
    lv.mul_relin(h, 0, h, 1, out, 1, 3)
    assert np.array_equal(lv.ct_download(out, 1, 3), lo.mul_relin_batch(cts[0:3], cts[1:4]))
    # rotations
    lv.rotate_rows(h, 0, 1, out, 0)
    lv.rotate_rows(h, 1, -3, out, 1)
    lv.rotate_columns(h, 2, out, 2)
    got = lv.ct_download(out, 0, 3)
    assert np.array_equal(got[0], lo.rotate_rows(cts[0], 1))
    assert np.array_equal(got[1], lo.rotate_rows(cts[1], -3))
    assert np.array_equal(got[2], lo.rotate_columns(cts[2]))
    # decryption on the device with the sliced secret key
    dp = lv.pt_alloc(4)
    lv.decrypt(h, 0, 4, dp, 0)
    assert np.array_equal(lv.pt_download(dp, 0, 4), np.stack([lo.decrypt(c) for c in cts]))


def test_mul_relin_pipelined_batch_on_a_level_context():
    o, g = keyed("c3", galois=False)
    lv = g.level(3)
    lo = level_oracle(o, "c3", 3, galois=False)
    rng = np.random.default_rng(5)
    base = np.stack([lo.encrypt(lo.encode(rng.integers(0, 8, size=o.n, dtype=np.uint64))) for _ in range(8)])
    cts = base[np.arange(520) % 8]
    h = up(lv, cts)
    out = lv.ct_alloc(520, 2)
    lv.mul_relin(h, 0, h, 0, out, 0, 520)
    got = lv.ct_download(out, 0, 520)
    exp = lo.mul_relin_batch(base, base)
    assert np.array_equal(got, exp[np.arange(520) % 8])


def test_ks_xi_level_context_decrypts_to_the_oracles_slots():
    """ks_xi = 1: the sliced keys carry [Q/q_l]_{q_l} of the TOP modulus; the level's digits use it (DevConsts::ks_inv_qhat_q)"""
    o, g = keyed("c3", ks_xi=True, seed=21)
    for limbs in (4, 3, 2):
        lv = g.level(limbs)
        lo = level_oracle(o, "c3", limbs)
        rng = np.random.default_rng(limbs)
        a = rng.integers(0, 16, size=o.n, dtype=np.uint64)
        ct = lo.encrypt(lo.encode(a))
        h = up(lv, ct[None, :])
        out = lv.ct_alloc(2, 2)
        lv.rotate_rows(h, 0, 1, out, 0)
        lv.rotate_columns(h, 0, out, 1)
        got = lv.ct_download(out, 0, 2)
        o0 = get_oracle("c3", galois=True)                                              # slots of the rotation (any keyed first-level oracle)
        exp_rot = o0.decode(o0.decrypt(o0.rotate_rows(o0.encrypt(o0.encode(a)), 1)))
        exp_col = o0.decode(o0.decrypt(o0.rotate_columns(o0.encrypt(o0.encode(a)))))
        assert np.array_equal(lo.decode(lo.decrypt(got[0])), exp_rot)
        assert np.array_equal(lo.decode(lo.decrypt(got[1])), exp_col)
        assert min(lv.invariant_noise_budget(out, 0, 2, exact_bits=True)) >= 1
        if limbs == 4:                  # (a fresh encryption at 3 limbs of c3 has too little budget for a product with t = 2^39)
            lv.mul_relin(h, 0, h, 0, out, 0, 1)
            dec = lo.decode(lo.decrypt(lv.ct_download(out, 0, 1)[0]))
            assert [int(x) for x in dec] == [int(x) * int(x) % o.t for x in a]
        # a switch from the ks_xi first level into the level decrypts unchanged
        top = up(g, o.encrypt(o.encode(a))[None, :])
        sw = lv.ct_alloc(1, 2)
        g.mod_switch(top, 0, 1, lv, sw, 0)
        assert np.array_equal(lo.decode(lo.decrypt(lv.ct_download(sw, 0, 1)[0])), a)


def test_one_limb_context_runs_the_linear_ops_and_refuses_the_rest():
    from cryptonets_amd._native import CnError
    o, g = keyed("tiny")
    lv = g.level(1)
    lo = level_oracle(o, "tiny", 1)
    rng = np.random.default_rng(4)
    a = rng.integers(0, o.t, size=o.n, dtype=np.uint64)
    cts = np.stack([lo.encrypt(lo.encode(a)), lo.encrypt(lo.encode(a))])
    h = up(lv, cts)
    out = lv.ct_alloc(2, 2)
    lv.add(h, 0, h, 1, out, 0)
    assert np.array_equal(lv.ct_download(out, 0, 1)[0], lo.add(cts[0], cts[1]))
    dp = lv.pt_alloc(1)
    lv.decrypt(h, 0, 1, dp, 0)
    assert np.array_equal(lv.pt_download(dp, 0, 1)[0], lo.decrypt(cts[0]))
    before = lv.ct_download(out, 0, 2)
    m3 = lv.ct_alloc(1, 3)
    for call in (lambda: lv.multiply(h, 0, h, 1, m3, 0), lambda: lv.relinearize(m3, 0, out, 0), lambda: lv.mul_relin(h, 0, h, 1, out, 0),
                 lambda: lv.rotate_rows(h, 0, 1, out, 0), lambda: lv.rotate_columns(h, 0, out, 0), lambda: lv.sum_slots(out, 0, 1),
                 lambda: lv.apply_galois(h, 0, 3, out, 0)):
        with pytest.raises(CnError) as e:
            call()
        assert e.value.code == -1
    assert np.array_equal(lv.ct_download(out, 0, 2), before)


# ------------------------------------------------------------------ ordering between the two contexts' streams
@pytest.mark.parametrize("defer", [0, 1, 2])
def test_mod_switch_ordering_without_host_waits(defer):
    g = ctx("c3")
    lv = g.level(2)
    g.set_option("defer", defer)
    lv.set_option("defer", defer)
    q, n = g.q, g.n
    rng = np.random.default_rng(defer)
    x, y = (rand_cts(rng, q, n, 1, 2) for _ in range(2))
    hx, hy, hin = up(g, x), up(g, y), g.ct_alloc(1, 2)
    z2 = rand_cts(rng, q[:2], n, 1, 2)
    hz, hout, hres = up(lv, z2), lv.ct_alloc(1, 2), lv.ct_alloc(1, 2)
    old = rand_cts(rng, q[:2], n, 1, 2)
    lv.ct_upload(hout, 0, old)
    g.sync(); lv.sync()
    # in written on src just before the switch; out read on dst just before it; in overwritten on src right after it
    g.add(hx, 0, hy, 0, hin, 0)
    lv.add(hout, 0, hz, 0, hres, 0)
    g.mod_switch(hin, 0, 1, lv, hout, 0)
    g.add(hx, 0, hx, 0, hin, 0)
    xy = ((x.reshape(2, 5, n).astype(object) + y.reshape(2, 5, n).astype(object)) % np.array(q, dtype=object)[None, :, None]).astype(np.uint64)
    got_out = lv.ct_download(hout, 0, 1)[0]
    got_res = lv.ct_download(hres, 0, 1)[0]
    assert np.array_equal(got_out, switch_residues(xy.reshape(-1), q, n, 2))
    oz = ((old.reshape(2, 2, n).astype(object) + z2.reshape(2, 2, n).astype(object)) % np.array(q[:2], dtype=object)[None, :, None]).astype(np.uint64)
    assert np.array_equal(got_res, oz.reshape(-1))
    xx = ((2 * x.reshape(2, 5, n).astype(object)) % np.array(q, dtype=object)[None, :, None]).astype(np.uint64)
    assert np.array_equal(g.ct_download(hin, 0, 1)[0], xx.reshape(-1))


@pytest.mark.parametrize("defer", [0, 2])
def test_mod_switch_ordering_behind_and_before_long_batches(defer):
    """the same three hazards around 845-ciphertext batches: the writer of `in` (cn_mul_relin, milliseconds) is still running on src's stream
    when the switch is submitted, the reader of `out` (cn_mul_relin on the level) still running on dst's, and the overwrite of `in` is queued on
    src's stream right behind the switch - only the events order them"""
    o, g = keyed("c3", galois=False)
    lv = g.level(2)
    g.set_option("defer", defer)
    lv.set_option("defer", defer)
    rng = np.random.default_rng(11)
    cnt = 845
    x = up(g, rand_cts(rng, g.q, g.n, 8, 2)[np.arange(cnt) % 8])
    old = up(lv, rand_cts(rng, lv.q, lv.n, 8, 2)[np.arange(cnt) % 8])
    hin, hout, hres = g.ct_alloc(cnt, 2), lv.ct_alloc(cnt, 2), lv.ct_alloc(cnt, 2)
    lv.copy(old, 0, hout, 0, cnt)
    g.sync(); lv.sync()
    g.mul_relin(x, 0, x, 0, hin, 0, cnt)                     # writes in
    lv.mul_relin(hout, 0, hout, 0, hres, 0, cnt)             # reads out
    g.mod_switch(hin, 0, cnt, lv, hout, 0)
    g.add(x, 0, x, 0, hin, 0, cnt)                           # overwrites in
    got_out, got_res, got_in = lv.ct_download(hout, 0, cnt), lv.ct_download(hres, 0, cnt), g.ct_download(hin, 0, cnt)
    # references, each step after a host wait
    g.set_option("defer", 0); lv.set_option("defer", 0)
    r_in, r_out, r_res, r_add = g.ct_alloc(cnt, 2), lv.ct_alloc(cnt, 2), lv.ct_alloc(cnt, 2), g.ct_alloc(cnt, 2)
    g.mul_relin(x, 0, x, 0, r_in, 0, cnt); g.sync()
    g.mod_switch(r_in, 0, cnt, lv, r_out, 0); lv.sync()
    lv.mul_relin(old, 0, old, 0, r_res, 0, cnt); lv.sync()
    g.add(x, 0, x, 0, r_add, 0, cnt); g.sync()
    assert np.array_equal(got_out, lv.ct_download(r_out, 0, cnt))
    assert np.array_equal(got_res, lv.ct_download(r_res, 0, cnt))
    assert np.array_equal(got_in, g.ct_download(r_add, 0, cnt))


# ------------------------------------------------------------------ argument errors leave `out` untouched
def test_mod_switch_argument_errors():
    from cryptonets_amd._native import CnError, Context
    g = ctx("c3")
    lv = g.level(2)
    rng = np.random.default_rng(1)
    h = up(g, rand_cts(rng, g.q, g.n, 2, 2))
    h3 = g.ct_alloc(2, 3)
    out = lv.ct_alloc(2, 2)
    keep = rand_cts(rng, g.q[:2], g.n, 2, 2)
    lv.ct_upload(out, 0, keep)
    p = PARAMS["c3"]
    foreign = Context(p["n"], p["t"], q=[g.q[1], g.q[0]], dbc=10, gdbc=20, device=0)
    fo = foreign.ct_alloc(2, 2)
    with pytest.raises(CnError):
        g.level(0)
    with pytest.raises(CnError):
        g.level(5)
    with pytest.raises(CnError):
        lv.level(2)
    calls = [lambda: g.mod_switch(h, 0, 1, foreign, fo, 0),                   # not on the chain
             lambda: lv.mod_switch(out, 0, 1, g, h, 0),                        # upwards
             lambda: g.mod_switch(h3, 0, 1, lv, out, 0),                       # size mismatch
             lambda: g.mod_switch(h, 1, 2, lv, out, 0),                        # source range
             lambda: g.mod_switch(h, 0, 2, lv, out, 1),                        # target range
             lambda: g.mod_switch(h, 0, 1, g, h, 1)]                           # same context
    for call in calls:
        with pytest.raises(CnError) as e:
            call()
        assert e.value.code == -1
    assert np.array_equal(lv.ct_download(out, 0, 2), keep)                     # the refused calls wrote nothing
    g.mod_switch(h, 0, 1, lv, out, 0)                                          # recorded once, so a capture can begin
    lv.sync()
    lv.ct_upload(out, 0, keep)
    g.add(h, 0, h, 1, h, 1)                                                    # the sequence that is recorded, run once first
    g.sync()
    g.graph_begin()
    try:
        g.add(h, 0, h, 1, h, 1)
        with pytest.raises(CnError) as e:
            g.mod_switch(h, 0, 1, lv, out, 0)
        assert e.value.code == -1
    finally:
        graph = g.graph_end()
        g.free(graph)
    assert np.array_equal(lv.ct_download(out, 0, 2), keep)


# ------------------------------------------------------------------ end to end: a squared layer switched to its lowest level
def test_square_then_switch_to_the_lowest_level_with_budget():
    """CryptoNets' output shape: fresh encryptions -> scalar product -> square -> switched down; the slots survive at the lowest level with
    a positive noise budget (c3: two of five primes)"""
    o, g = keyed("c3", galois=False)
    rng = np.random.default_rng(12)
    n, t = o.n, o.t
    vals = rng.integers(0, 64, size=(3, n), dtype=np.uint64)
    h = up(g, np.stack([o.encrypt(o.encode(v)) for v in vals]))
    W = np.array([[3, 1, 2]], dtype=np.uint64)
    lin = g.ct_alloc(1, 2)
    g.scalar_gemm(h, W, lin, 0)
    sq = g.ct_alloc(1, 2)
    g.mul_relin(lin, 0, lin, 0, sq, 0)
    exp = ((W.astype(object) @ vals.astype(object)) ** 2 % t)[0]
    for limbs in (4, 3, 2):
        lv = g.level(limbs)
        out = lv.ct_alloc(1, 2)
        g.mod_switch(sq, 0, 1, lv, out, 0)
        dp = lv.pt_alloc(1)
        lv.decrypt(out, 0, 1, dp, 0)
        assert [int(x) for x in lv.decode(dp, 0)] == [int(x) for x in exp], limbs
        assert lv.invariant_noise_budget(out)[0] > 0


# ------------------------------------------------------------------ more of the evaluator on level contexts
def rowdot_reference(lo, ct, pts, length):
    """the per-row MultiplyPlain, RotateColumns + Add, RotateRows(-2^s) + Add sequence of the reference (AtomicSealBfvVector.cs:888-935)"""
    n, half, res = lo.n, lo.n // 2, []
    for p in pts:
        c = lo.multiply_plain(ct, p)
        ln = length if length else n
        if ln >= half:
            c = lo.add(c, lo.rotate_columns(c))
            ln = half
        s = 1
        while s < ln:
            c = lo.add(c, lo.rotate_rows(c, -s))
            s *= 2
        res.append(c)
    return np.stack(res)


@pytest.mark.parametrize("name,limbs", [("c3", 2), ("c4", 2), ("c5", 4), ("tiny", 1)])
def test_gemm_scalar_slots_rowdot_noise_on_a_level_context(name, limbs):
    from cryptonets_amd._native import CnError
    o, g = keyed(name)
    lv = g.level(limbs)
    lo = level_oracle(o, name, limbs)
    rng = np.random.default_rng(30 + limbs)
    n = o.n
    vals = rng.integers(0, 8, size=(3, n), dtype=np.uint64)
    cts = np.stack([lo.encrypt(lo.encode(v)) for v in vals])
    h = up(lv, cts)
    out = lv.ct_alloc(4, 2)
    W = np.array([[3, 0, o.t - 2], [1, 5, 7]], dtype=np.uint64)
    lv.scalar_gemm(h, W, out, 0)
    assert np.array_equal(lv.ct_download(out, 0, 2), lo.scalar_gemm(cts, W))
    sc = np.array([3, o.t - 7, o.t - 1], dtype=np.uint64)
    lv.mul_scalar(h, 0, sc, out, 0, 3)
    got = lv.ct_download(out, 0, 3)
    for i in range(3):
        assert np.array_equal(got[i], lo.multiply_plain(cts[i], sc[i:i + 1]))
    # cn_noise_poly: t (c0 + c1 s) mod q_j with the level's slice of the secret key
    x = lo.dot_with_secret(cts[0]).reshape(limbs, n)
    exp = np.stack([np.array([(int(v) * o.t) % int(lo.q[j]) for v in x[j]], dtype=np.uint64) for j in range(limbs)])
    assert np.array_equal(lv.noise_poly(h, 0, 1)[0], exp)
    if limbs == 1:
        with pytest.raises(CnError) as e:
            lv.sum_slots(out, 0, 1)
        assert e.value.code == -1
        return
    # sum_slots / rowdot_batch: the reference's sequence word for word, and the slot sums
    R = 2
    w = rng.integers(1, 20, size=(R, n), dtype=np.uint64)
    pts = np.stack([lo.encode(r) for r in w])
    ph = lv.pt_alloc(R)
    lv.pt_upload(ph, 0, pts)
    for length in (0, 8):
        lv.rowdot_batch(h, 0, ph, 0, R, length, out, 1)
        assert np.array_equal(lv.ct_download(out, 1, R), rowdot_reference(lo, cts[0], pts, length)), length
    lv.rowdot_batch(h, 0, ph, 0, R, 0, out, 1)                   # every slot: sum(v * w_r) mod t
    if name != "c3":                                             # (c3 at 2 limbs, t = 2^39: a fresh encryption times an encoded plaintext has no budget left)
        assert lv.invariant_noise_budget(out, 1, 1, exact_bits=True)[0] >= 1
        dec = lo.decode(lo.decrypt(lv.ct_download(out, 1, 1)[0]))
        assert int(dec[0]) == int(np.sum(vals[0].astype(object) * w[0].astype(object)) % o.t) and len(set(int(v) for v in dec)) == 1
    lv.ct_upload(out, 0, np.stack([cts[1], cts[2]]))
    lv.sum_slots(out, 0, 2, 4)
    exp = []
    for c in (cts[1], cts[2]):
        for s in (1, 2):
            c = lo.add(c, lo.rotate_rows(c, -s))
        exp.append(c)
    assert np.array_equal(lv.ct_download(out, 0, 2), np.stack(exp))


@pytest.mark.parametrize("ks_xi", [False, True])
def test_n16384_key_switch_on_a_level_context(ks_xi):
    """c5 at 4 limbs: the one-launch N = 16384 key switch (k_keyswitch_pair14) on a level context; word for word against the prefix oracle
    under ks_xi = 0, slots under ks_xi = 1 (the digits then use the chain's top modulus)"""
    o, g = keyed("c5", ks_xi=ks_xi, seed=23)
    lv = g.level(4)
    lo = level_oracle(o, "c5", 4)
    rng = np.random.default_rng(9)
    vals = rng.integers(0, 16, size=(8, o.n), dtype=np.uint64)
    cts = np.stack([lo.encrypt(lo.encode(v)) for v in vals])
    h = up(lv, cts)
    out = lv.ct_alloc(8, 2)
    lv.mul_relin(h, 0, h, 0, out, 0, 8)
    sq = lv.ct_download(out, 0, 8)
    lv.rotate_rows(h, 0, 1, out, 0, 8)
    rot = lv.ct_download(out, 0, 8)
    if not ks_xi:
        assert np.array_equal(sq, lo.mul_relin_batch(cts, cts))
        assert np.array_equal(rot, np.stack([lo.rotate_rows(c, 1) for c in cts]))
    o0 = get_oracle("c5", galois=True)
    for i in (0, 7):
        assert [int(x) for x in lo.decode(lo.decrypt(sq[i]))] == [int(v) * int(v) % o.t for v in vals[i]]
        assert np.array_equal(lo.decode(lo.decrypt(rot[i])), o0.decode(o0.decrypt(o0.rotate_rows(o0.encrypt(o0.encode(vals[i])), 1))))


# a ring whose last prime is above 2^49: the first level keeps its keys as u64 words (integer key switch), its 2-limb level on the FP64 path
WIDE = dict(n=1024, t=12289, q=[0xffffee001, 0xffffc4001, 0x7ffffffff5001], dbc=10, gdbc=20)


def test_level_converts_its_keys_when_the_dropped_prime_decides_the_arithmetic():
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    p = WIDE
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    o.keygen(5, galois=True)
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    g.set_relin_key(o.relin_key())
    for i, e in enumerate(o.galois_elts()):
        g.set_galois_key(e, o.galois_key(i))
    lv = g.level(2)
    assert np.array_equal(lv.get_key(0), slice_key(o.relin_key(), 3, p["n"], digits(p["q"], p["dbc"]), 2))
    from oracle.cno import Oracle as O2
    lo = O2(p["n"], p["t"], q=p["q"][:2], dbc=p["dbc"], gdbc=p["gdbc"])
    lo.import_keys(slice_poly(o.secret_key(), 3, p["n"], 2, 1), slice_poly(o.public_key(), 3, p["n"], 2, 2))
    lo.import_relin_key(slice_key(o.relin_key(), 3, p["n"], digits(p["q"], p["dbc"]), 2))
    for i, e in enumerate(o.galois_elts()):
        lo.import_galois_key(e, slice_key(o.galois_key(i), 3, p["n"], digits(p["q"], p["gdbc"]), 2))
    rng = np.random.default_rng(2)
    cts = np.stack([lo.encrypt(lo.encode(rng.integers(0, 8, size=p["n"], dtype=np.uint64))) for _ in range(2)])
    h = up(lv, cts)
    out = lv.ct_alloc(2, 2)
    lv.mul_relin(h, 0, h, 1, out, 0)
    lv.rotate_rows(h, 0, 3, out, 1)
    got = lv.ct_download(out, 0, 2)
    assert np.array_equal(got[0], lo.mul_relin_batch(cts[:1], cts[1:])[0])
    assert np.array_equal(got[1], lo.rotate_rows(cts[0], 3))
