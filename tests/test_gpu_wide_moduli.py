"""GPU: the integer path at 50-60-bit moduli and the ring sizes the rest of the suite does not run (N = 256, 512, 2048), word for word against
the CPU oracle.

The kernels choose their arithmetic by modulus width and ring size: FP64 transforms and GEMMs up to 49 bits (two 22-bit limbs up to 44, the int8
matrix cores up to 46), integer transforms, key switch and SEAL's 61-bit auxiliary base as soon as one modulus has 50 bits or more, the u64 GEMM with
one reduction per lazy = 2^(127 - 2 bits) terms (128 at 60 bits); the legacy radix-2 kernels below N = 1024 and the L = 11 register-radix kernels at
N = 2048.  The sets below sit on either side of each of those lines; the operands at the edges of the residue range (0, q - 1, +-q/2) and the GEMMs at
their exactness limits (every input word q_j - 1, every weight t - 1 or +-(2^20 - 1), term counts around each window).

The primes are found at import by a deterministic search - the largest primes below 2^b that are 1 mod 2N - and checked for primality and width.
Moduli of 2^60 and more are refused (SEAL 3.2 takes at most 60 bits; the 61-bit primes are its m_sk, gamma and auxiliary base)."""
import numpy as np
import pytest

from modswitch_model import digits, slice_key, slice_poly, switch_residues
from noise_norm_model import centred, prod
from oracle_backend import OracleClient
from test_gpu_noise_norm import edge_values, planted
from test_oracle_math import is_prime

pytestmark = pytest.mark.gpu


def ntt_primes(bits, n, count, avoid=()):
    """the `count` largest primes below 2^bits that are 1 mod 2n and not in `avoid`, decreasing"""
    out, x = [], ((1 << bits) - 1) // (2 * n) * (2 * n) + 1
    while len(out) < count:
        if x not in avoid and is_prime(x):
            out.append(x)
        x -= 2 * n
    for p in out:
        assert is_prime(p) and p.bit_length() == bits and p % (2 * n) == 1, hex(p)
    return out


TINY_Q = [0xffffee001, 0xffffc4001, 0x1ffffe0001]          # CoeffModulus128(4096): 36, 36, 37 bits, 1 mod 8192
SEAL2048 = 0x3fffffff000001                                # CoeffModulus128(2048): one 54-bit prime
M_SK, GAMMA, B_0 = 0x1fffffffffe00001, 0x1fffffffffc80001, 0x1fffffffffb40001    # SEAL's largest 61-bit primes == 1 mod 2^18
T_WIDE_W = 2101249                                         # the smallest prime above 2^21 that is 1 mod 2048: weights +-(2^20 - 1) are residues of it
assert is_prime(T_WIDE_W) and T_WIDE_W > 2 * (2 ** 20 - 1) and T_WIDE_W % 2048 == 1

P60_4096 = ntt_primes(60, 4096, 3)
P60_1024 = ntt_primes(60, 1024, 2)
WIDTHS = (44, 45, 46, 47, 49, 50, 60)
P_WIDTH = {b: ntt_primes(b, 1024, 1, avoid=TINY_Q)[0] for b in WIDTHS}

SETS = {
    "W60": dict(n=4096, t=40961, q=P60_4096, dbc=60, gdbc=60),
    "W60d": dict(n=1024, t=12289, q=P60_1024 + [TINY_Q[0]], dbc=10, gdbc=20),          # digit-heavy: six 10-bit relin digits per wide limb
    "W60d59": dict(n=1024, t=12289, q=P60_1024 + [TINY_Q[0]], dbc=59, gdbc=59),        # the top digit of a 60-bit limb is 1 bit wide
    "S2048": dict(n=2048, t=12289, q=[SEAL2048], dbc=60, gdbc=60),                     # SEAL 3.2's default at N = 2048 (k = 1)
    "MIX2048": dict(n=2048, t=12289, q=TINY_Q[:2] + [SEAL2048], dbc=60, gdbc=60),      # FP64-capable limbs, integer key switch and BEHZ
    "F2048": dict(n=2048, t=12289, q=TINY_Q, dbc=60, gdbc=60),                         # L = 11 kernels on both policies
    "R256": dict(n=256, t=12289, q=ntt_primes(36, 256, 2), dbc=60, gdbc=60),           # legacy radix-2 kernels, group-major GEMM order
    "R512": dict(n=512, t=12289, q=ntt_primes(36, 512, 2), dbc=60, gdbc=60),
    "WIDE": dict(n=1024, t=12289, q=[0xffffee001, 0xffffc4001, 0x7ffffffff5001], dbc=10, gdbc=20),   # test_gpu_mod_switch's ring, top level
}
for _b in WIDTHS:
    SETS["B%d" % _b] = dict(n=1024, t=12289, q=[TINY_Q[0], P_WIDTH[_b]], dbc=60, gdbc=60)

# (set, f64 option): every set on its default policy, F2048 on the integer one as well
ALL = [(s, 1) for s in SETS] + [("F2048", 0)]
MULTI = [c for c in ALL if len(SETS[c[0]]["q"]) > 1]          # one-limb contexts refuse multiply and the key switches (cnhip.h)
IDS = lambda c: "%s-f64_%d" % c

_oracles, _gpus = {}, {}


def oracle(name):
    from oracle.cno import Oracle
    if name not in _oracles:
        p = SETS[name]
        o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
        o.keygen(23, galois=len(p["q"]) > 1)
        _oracles[name] = o
    return _oracles[name]


def gpu(name, f64=1):
    """a context with the oracle's keys (relinearisation, Galois, public, secret), cached per (set, f64)"""
    from cryptonets_amd._native import Context
    if (name, f64) not in _gpus:
        p, o = SETS[name], oracle(name)
        g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
        if not f64:
            g.set_option("f64", 0)
        if o.k > 1:
            g.set_relin_key(o.relin_key())
            for i, e in enumerate(o.galois_elts()):
                g.set_galois_key(e, o.galois_key(i))
        g.set_public_key(o.public_key())
        g.set_secret_key(o.secret_key())
        _gpus[(name, f64)] = g
    return _gpus[(name, f64)]


def up(g, cts, size=2):
    h = g.ct_alloc(len(cts), size)
    g.ct_upload(h, 0, cts)
    return h


def fresh(o, rng, count):
    return np.stack([o.encrypt(o.encode(rng.integers(0, o.t, size=o.n, dtype=np.uint64))) for _ in range(count)])


def edges(o):
    """ciphertext words (not encryptions: the evaluator is a function of words) at the edges of the residue range: every coefficient 0, q - 1,
    floor(q/2) and ceil(q/2) (the largest centred magnitudes), alternating +-q/2, and one limb at q_j - 1 beside zeros"""
    Q, n = prod(o.q), o.n
    pats = [[0] * n, [Q - 1] * n, [Q // 2] * n, [Q // 2 + 1] * n, [(Q // 2) if i % 2 else (Q - Q // 2) for i in range(n)]]
    cts = []
    for pa in pats:
        for pb in (pats[2], pa):
            cts.append(np.concatenate([np.array([x % qj for x in poly], dtype=np.uint64) for poly in (pa, pb) for qj in o.q]))
    lone = np.zeros((2, o.k, n), dtype=np.uint64)
    lone[:, 0, :] = o.q[0] - 1
    cts.append(lone.reshape(-1))
    return np.stack(cts)


def operands(o, rng, count=3):
    return np.concatenate([fresh(o, rng, count), edges(o)])


# ------------------------------------------------------------------ transforms, linear operations, plaintext products
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_ntt_forward_and_inverse(case, rng):
    name, f64 = case
    o, g = oracle(name), gpu(name, f64)
    cts = np.stack([np.concatenate([rng.integers(0, q, size=o.n, dtype=np.uint64) for _ in range(2) for q in o.q]) for _ in range(2)])
    cts = np.concatenate([cts, edges(o)[[1, 2, 4]]])
    h = up(g, cts)
    g.ct_ntt(h, 0, len(cts))
    exp = np.stack([np.concatenate([o.ntt_fwd(j % o.k, c.reshape(2 * o.k, o.n)[j]) for j in range(2 * o.k)]) for c in cts])
    assert np.array_equal(g.ct_download(h, 0, len(cts)), exp)
    g.ct_ntt(h, 0, len(cts), inverse=True)
    assert np.array_equal(g.ct_download(h, 0, len(cts)), cts)
    g.free(h)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_linear_ops_and_plaintext_products(case, rng):
    from cryptonets_amd._native import CnError
    name, f64 = case
    o, g = oracle(name), gpu(name, f64)
    cts = operands(o, rng)
    m = len(cts)
    h, out = up(g, cts), g.ct_alloc(m)
    g.add(h, 0, h, 1, out, 0, m - 1)
    assert np.array_equal(g.ct_download(out, 0, m - 1), np.stack([o.add(cts[i], cts[i + 1]) for i in range(m - 1)]))
    g.sub(h, 1, h, 0, out, 0, m - 1)
    assert np.array_equal(g.ct_download(out, 0, m - 1), np.stack([o.sub(cts[i + 1], cts[i]) for i in range(m - 1)]))
    g.negate(h, 0, out, 0, m)
    assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.negate(c) for c in cts]))
    plains = rng.integers(0, o.t, size=(m, o.n), dtype=np.uint64)
    plains[0, :6] = [0, 1, o.t // 2, (o.t + 1) // 2, o.t - 1, o.t - 2]               # both sides of the upper-half threshold
    plains[1] = o.t - 1
    ph = g.pt_alloc(m)
    g.pt_upload(ph, 0, plains)
    for sub in (False, True):
        g.add_plain(h, 0, ph, 0, out, 0, m, subtract=sub)
        assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.add_plain(cts[i], plains[i], sub) for i in range(m)])), sub
    g.mul_plain(h, 0, ph, 0, out, 0, m)
    assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.multiply_plain(cts[i], plains[i]) for i in range(m)]))
    g.mul_plain(h, 0, ph, 1, out, 0, m, pt_stride=0)                                  # the all-(t - 1) plaintext against every operand
    assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.multiply_plain(c, plains[1]) for c in cts]))
    sc = np.array([[1, 2, o.t - 1, (o.t + 1) // 2, o.t // 2, 3][i % 6] for i in range(m)], dtype=np.uint64)
    g.mul_scalar(h, 0, sc, out, 0, m)
    assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.multiply_plain(cts[i], sc[i:i + 1]) for i in range(m)]))
    with pytest.raises(CnError):
        g.mul_scalar(h, 0, np.zeros(1, dtype=np.uint64), out, 0, 1)
    for x in (h, out, ph):
        g.free(x)


# ------------------------------------------------------------------ multiplication, relinearisation, key switches
@pytest.mark.parametrize("case", MULTI, ids=IDS)
def test_multiply_and_relinearize_on_edge_operands(case, rng):
    name, f64 = case
    o, g = oracle(name), gpu(name, f64)
    cts = operands(o, rng, 2)
    m = len(cts)
    pairs = [(i, (i + 3) % m) for i in range(m)]
    h, out3, out2 = up(g, cts), g.ct_alloc(m, 3), g.ct_alloc(m)
    for i, (a, b) in enumerate(pairs):
        g.multiply(h, a, h, b, out3, i, 1)
    exp3 = np.stack([o.multiply(cts[a], cts[b]) for a, b in pairs])
    assert np.array_equal(g.ct_download(out3, 0, m, size=3), exp3)
    g.relinearize(out3, 0, out2, 0, m)
    assert np.array_equal(g.ct_download(out2, 0, m), np.stack([o.relinearize(c) for c in exp3]))
    g.mul_relin(h, 0, h, 0, out2, 0, m)                                              # squarings, as a batch
    assert np.array_equal(g.ct_download(out2, 0, m), o.mul_relin_batch(cts, cts))
    g.mul_relin(h, 0, h, 1, out2, 0, m - 1, b_stride=0)                              # one operand broadcast
    assert np.array_equal(g.ct_download(out2, 0, m - 1), o.mul_relin_batch(cts[:m - 1], np.repeat(cts[1:2], m - 1, axis=0)))
    vals = o.decode(o.decrypt(cts[0]))
    got = o.decode(o.decrypt(g.ct_download(out2, 0, 1)[0]))                          # the compared words are a valid product
    assert np.array_equal(got, np.array([int(a) * int(b) % o.t for a, b in zip(vals, o.decode(o.decrypt(cts[1])))], dtype=np.uint64))
    for x in (h, out3, out2):
        g.free(x)


@pytest.mark.parametrize("case", MULTI, ids=IDS)
def test_key_switch_forms(case, rng):
    """"ks_wide" -1 (automatic), 0 (fused), 1 and 2 (two launches): Multiply + Relinearize and a rotation give the oracle's words in every form"""
    name, f64 = case
    o, g = oracle(name), gpu(name, f64)
    cts = operands(o, rng, 2)[:6]
    m = len(cts)
    exp = o.mul_relin_batch(cts, cts[::-1].copy())
    rot = np.stack([o.rotate_rows(c, 1) for c in cts])
    h, out = up(g, cts), g.ct_alloc(m)
    try:
        for wide in (-1, 0, 1, 2):
            g.set_option("ks_wide", wide)
            for i in range(m):
                g.mul_relin(h, i, h, m - 1 - i, out, i, 1)
            assert np.array_equal(g.ct_download(out, 0, m), exp), wide
            g.mul_relin(h, 0, h, 0, out, 0, m)
            assert np.array_equal(g.ct_download(out, 0, m), o.mul_relin_batch(cts, cts)), wide
            g.rotate_rows(h, 0, 1, out, 0, m)
            assert np.array_equal(g.ct_download(out, 0, m), rot), wide
    finally:
        g.set_option("ks_wide", -1)
    for x in (h, out):
        g.free(x)


def test_pipelined_batch_at_60_bits(rng):
    """>= 512 squarings run in parts over two streams ("sq_halves"): on three 60-bit primes the batch gives the one-stream words everywhere and the
    oracle's words on a sample of indices around the part boundaries"""
    o, g = oracle("W60"), gpu("W60")
    cnt = 520
    cts = np.stack([np.concatenate([rng.integers(0, q, size=o.n, dtype=np.uint64) for _ in range(2) for q in o.q]) for _ in range(cnt)])
    e = edges(o)
    cts[[0, 1, 2, 260, 519]] = e[[1, 2, 4, 3, 10]]
    cts[3] = fresh(o, rng, 1)[0]
    h, out = up(g, cts), g.ct_alloc(cnt)
    words = {}
    try:
        for halves in (1, 0):
            g.set_option("sq_halves", halves)
            g.mul_relin(h, 0, h, 0, out, 0, cnt)
            words[halves] = g.ct_download(out, 0, cnt)
    finally:
        g.set_option("sq_halves", 1)
    assert np.array_equal(words[1], words[0])
    sample = [0, 1, 2, 3, 155, 156, 157, 259, 260, 363, 364, 518, 519]
    assert np.array_equal(words[1][sample], o.mul_relin_batch(cts[sample], cts[sample]))
    for x in (h, out):
        g.free(x)


@pytest.mark.parametrize("case", MULTI, ids=IDS)
def test_rotations_galois_and_slot_sums(case, rng):
    name, f64 = case
    o, g = oracle(name), gpu(name, f64)
    cts = operands(o, rng, 2)[:5]
    m = len(cts)
    h, out = up(g, cts), g.ct_alloc(m)
    for steps in (1, -1):
        g.rotate_rows(h, 0, steps, out, 0, m)
        assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.rotate_rows(c, steps) for c in cts])), steps
    g.rotate_columns(h, 0, out, 0, m)
    assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.rotate_columns(c) for c in cts]))
    elt = o.galois_elts()[-1]
    g.apply_galois(h, 0, elt, out, 0, m)
    assert np.array_equal(g.ct_download(out, 0, m), np.stack([o.apply_galois(c, elt) for c in cts])), elt
    g.copy(h, 0, out, 0, 2)
    g.sum_slots(out, 0, 2)                                                            # every slot: the sum of all slots
    exp = []
    for c in cts[:2]:
        c = o.add(c, o.rotate_columns(c))
        s = 1
        while s < o.n // 2:
            c = o.add(c, o.rotate_rows(c, -s))
            s *= 2
        exp.append(c)
    got = g.ct_download(out, 0, 2)
    assert np.array_equal(got, np.stack(exp))
    vals = o.decode(o.decrypt(cts[0]))
    assert set(int(x) for x in o.decode(o.decrypt(got[0]))) == {int(np.sum(vals.astype(object)) % o.t)}
    for x in (h, out):
        g.free(x)


def test_one_limb_context_refuses_multiply_and_rotations(rng):
    from cryptonets_amd._native import CnError
    o, g = oracle("S2048"), gpu("S2048")
    cts = fresh(o, rng, 2)
    h, out, m3 = up(g, cts), g.ct_alloc(2), g.ct_alloc(1, 3)
    before = g.ct_download(out, 0, 2)
    for call in (lambda: g.multiply(h, 0, h, 1, m3, 0), lambda: g.mul_relin(h, 0, h, 1, out, 0), lambda: g.rotate_rows(h, 0, 1, out, 0),
                 lambda: g.rotate_rows(h, 0, -1, out, 0), lambda: g.rotate_columns(h, 0, out, 0), lambda: g.apply_galois(h, 0, 3, out, 0),
                 lambda: g.sum_slots(out, 0, 1)):
        with pytest.raises(CnError) as e:
            call()
        assert e.value.code == -1
    assert np.array_equal(g.ct_download(out, 0, 2), before)
    for x in (h, out, m3):
        g.free(x)


def test_multiply_refused_at_ten_limbs():
    from cryptonets_amd._native import CnError, Context
    q = ntt_primes(40, 1024, 10)
    g = Context(1024, 12289, q=q, dbc=60, gdbc=60, device=0)
    h, m3 = g.ct_alloc(2), g.ct_alloc(1, 3)
    with pytest.raises(CnError) as e:
        g.multiply(h, 0, h, 1, m3, 0)
    assert e.value.code == -1
    g.close()


# ------------------------------------------------------------------ encryption and decryption across implementations, noise
@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_encrypt_and_decrypt_across_implementations(case, rng):
    """the device encrypts and the oracle decrypts, under every "enc_fused" form; the oracle encrypts and the device decrypts.  Device encryption
    needs 1024 <= N (the samplers run on the register-radix transforms): below, CN_ERR_ARG and nothing written"""
    from cryptonets_amd._native import CnError
    name, f64 = case
    o, g = oracle(name), gpu(name, f64)
    vals = rng.integers(0, o.t, size=(3, o.n), dtype=np.uint64)
    vals[0, :4] = [0, 1, o.t - 1, (o.t + 1) // 2]
    plains = np.stack([o.encode(v) for v in vals])
    ph, ch, dp = g.pt_alloc(3), g.ct_alloc(3), g.pt_alloc(3)
    g.pt_upload(ph, 0, plains)
    try:
        for fused in (0, 1, 2):
            g.set_option("enc_fused", fused)
            if o.n < 1024:
                before = g.ct_download(ch, 0, 3)
                with pytest.raises(CnError) as e:
                    g.encrypt(ph, 0, ch, 0, 3, seed=11 + fused)
                assert e.value.code == -1 and np.array_equal(g.ct_download(ch, 0, 3), before)
                continue
            g.encrypt(ph, 0, ch, 0, 3, seed=11 + fused)
            for i, c in enumerate(g.ct_download(ch, 0, 3)):
                assert np.array_equal(o.decode(o.decrypt(c)), vals[i]), (fused, i)
    finally:
        g.set_option("enc_fused", 2)
    cts = fresh(o, rng, 3)
    g.ct_upload(ch, 0, cts)
    g.decrypt(ch, 0, 3, dp, 0)
    assert np.array_equal(g.pt_download(dp, 0, 3), np.stack([o.decrypt(c) for c in cts]))
    for x in (ph, ch, dp):
        g.free(x)


def host_norm(o, ct):
    """|| t (c0 + c1 s) mod q ||_inf, centred, composed with Python integers from the oracle's residues"""
    w = OracleClient(o.t, o.n, o.q, o.dbc, o.gdbc, oracle=o).noise_poly(ct)
    Q = prod(o.q)
    coef = [(Q // m) * pow((Q // m) % m, -1, m) for m in o.q]
    x = sum(w[j].astype(object) * coef[j] for j in range(o.k)) % Q
    return max(centred(int(v), Q) for v in x)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_noise_norm_of_real_ciphertexts(case, rng):
    name, f64 = case
    o, g = oracle(name), gpu(name, f64)
    cts = fresh(o, rng, 2)
    if o.k > 1:
        cts = np.concatenate([cts, o.mul_relin_batch(cts[:1], cts[1:]), o.rotate_rows(cts[0], 1)[None, :]])
    h = up(g, cts)
    exp = [host_norm(o, c) for c in cts]
    assert g.noise_norm(h, 0, len(cts)) == exp
    Q = prod(o.q)
    budgets = [OracleClient(o.t, o.n, o.q, o.dbc, o.gdbc, oracle=o).noise_budget_words(c) for c in cts]
    assert g.invariant_noise_budget(h, 0, len(cts), exact_bits=True) == budgets == [max(0, Q.bit_length() - e.bit_length() - 1) for e in exp]
    g.free(h)


@pytest.mark.parametrize("name", ["W60", "W60d"])
def test_noise_norm_of_planted_polynomials_at_60_bits(name, rng):
    """noise polynomials of known exact norm (c1 = 0, c0 = [X t^-1]_q): every edge value of Q (products of 60-bit primes) beside a smaller decoy"""
    g = gpu(name)
    Q, n = prod(g.q), g.n
    cts = []
    for i, X in enumerate(edge_values(Q)):
        pos = [0, n - 1, int(rng.integers(1, n - 1))][i % 3]
        m = centred(X, Q) // 3
        cts.append({pos: X, (pos + 1 + int(rng.integers(0, n - 2))) % n: m if i % 2 else (Q - m) % Q})
    for i in range(6):
        X = int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % Q
        cts.append({int(rng.integers(0, n)): X, int(rng.integers(0, n)): (Q - X // 2) % Q})
    for size in (2, 3):
        h, exp = planted(g, cts, size)
        assert g.noise_norm(h, 0, len(cts)) == exp, size
        g.free(h)


# ------------------------------------------------------------------ modulus switching off 60-bit primes
def level_oracle(o, name, limbs):
    from oracle.cno import Oracle
    p = SETS[name]
    lo = Oracle(p["n"], p["t"], q=o.q[:limbs], dbc=p["dbc"], gdbc=p["gdbc"])
    lo.import_keys(slice_poly(o.secret_key(), o.k, o.n, limbs, 1), slice_poly(o.public_key(), o.k, o.n, limbs, 2))
    lo.import_relin_key(slice_key(o.relin_key(), o.k, o.n, digits(o.q, p["dbc"]), limbs))
    for i, e in enumerate(o.galois_elts()):
        lo.import_galois_key(e, slice_key(o.galois_key(i), o.k, o.n, digits(o.q, p["gdbc"]), limbs))
    return lo


def test_mod_switch_from_three_60_bit_primes(rng):
    o, g = oracle("W60"), gpu("W60")
    q, n = g.q, g.n
    vals = rng.integers(0, 16, size=(2, n), dtype=np.uint64)
    real = np.stack([o.encrypt(o.encode(v)) for v in vals])
    src = np.concatenate([real, edges(o)[[1, 2, 3, 4, 10]], np.stack([np.concatenate([rng.integers(0, m, size=n, dtype=np.uint64) for _ in range(2)
                                                                                      for m in q]) for _ in range(3)])])
    h = up(g, src)
    for limbs in (2, 1):
        lv = g.level(limbs)
        out = lv.ct_alloc(len(src))
        g.mod_switch(h, 0, len(src), lv, out, 0)
        got = lv.ct_download(out, 0, len(src))
        assert np.array_equal(got, switch_residues(src, q, n, limbs).reshape(len(src), -1)), limbs
        lo = level_oracle(o, "W60", limbs)
        for i in range(2):
            assert np.array_equal(lo.decode(lo.decrypt(got[i])), vals[i]), limbs
        if limbs == 2:                                  # the evaluator on the level: 120-bit q, still the integer path
            m = len(src)
            res = lv.ct_alloc(m)
            lv.mul_relin(out, 0, out, 0, res, 0, m)
            assert np.array_equal(lv.ct_download(res, 0, m), lo.mul_relin_batch(got, got))
            lv.rotate_rows(out, 0, -1, res, 0, m)
            assert np.array_equal(lv.ct_download(res, 0, m), np.stack([lo.rotate_rows(c, -1) for c in got]))
            lv.free(res)
        lv.free(out)
    # chained: the level-2 words switched again give the direct switch to one limb
    l2, l1 = g.level(2), g.level(1)
    a, b = l2.ct_alloc(len(src)), l1.ct_alloc(len(src))
    g.mod_switch(h, 0, len(src), l2, a, 0)
    l2.mod_switch(a, 0, len(src), l1, b, 0)
    assert np.array_equal(l1.ct_download(b, 0, len(src)), switch_residues(src, q, n, 1).reshape(len(src), -1))
    l2.free(a)
    l1.free(b)
    g.free(h)


# ------------------------------------------------------------------ scalar GEMMs at their exactness limits
def gemm_oracle(bits):
    """N = 1024, a 36-bit prime and one of exactly `bits` bits, t a prime above 2^21 (weights +-(2^20 - 1) are centred residues); no keys"""
    from oracle.cno import Oracle
    return Oracle(1024, T_WIDE_W, q=[TINY_Q[0], P_WIDTH[bits]], dbc=60, gdbc=60)


def gemm_context(bits, **opt):
    """the oracle of gemm_oracle(bits) and a device context over the same parameters with the given options"""
    from cryptonets_amd._native import Context
    o = gemm_oracle(bits)
    g = Context(1024, T_WIDE_W, q=list(o.q), dbc=60, gdbc=60, device=0)
    for k, v in opt.items():
        g.set_option(k, v)
    return o, g


def all_max(o):
    return np.concatenate([np.full(o.n, qj - 1, dtype=np.uint64) for _ in range(2) for qj in o.q])


def random_words(o, rng, count):
    return np.stack([np.concatenate([rng.integers(0, m, size=o.n, dtype=np.uint64) for _ in range(2) for m in o.q]) for _ in range(count)])


def limit_weights(t, rows, K, rng):
    """weights at the magnitude limits of the small-weight kernels: t - 1 (= -1), 2^20 - 1, -(2^20 - 1), every term of a row the same sign - each
    partial sum over all-(q_j - 1) inputs as large as it gets - and one row of random signs"""
    w = 2 ** 20 - 1
    Ws = np.empty((rows, K), dtype=np.int64)
    for r in range(rows):
        Ws[r] = [-1, w, -w, w - r, -(w - r)][r % 5] if r < rows - 1 else rng.choice([w, -w], size=K)
    return np.where(Ws < 0, t + Ws, Ws).astype(np.uint64)


def run_gemm(g, h, W, idx):
    out = g.ct_alloc(W.shape[0])
    g.scalar_gemm(h, W, out, 0, idx=idx)
    got = g.ct_download(out, 0, W.shape[0])
    g.free(out)
    return got


@pytest.mark.parametrize("bits,windows", [(60, (128,)), (44, (1024,)), (49, (32768,))], ids=["u64-60", "f64-two-limb-44", "f64-three-limb-49"])
def test_scalar_gemm_term_counts_at_the_exactness_windows(bits, windows, rng):
    """K = lazy, lazy + 1 and 2 lazy + 1 terms over inputs whose words are all q_j - 1: the u64 kernel (one Barrett reduction per 128 terms at 60
    bits - the intermediate reduction runs), the two-limb (1024 terms) and three-limb (32768 terms) FP64 kernels (gemm_mfma 0: one list of 6 rows)"""
    o, g = gemm_context(bits, gemm_mfma=0)
    cts = np.stack([all_max(o), random_words(o, rng, 1)[0]])
    h = up(g, cts)
    for lazy in windows:
        for K in (lazy, lazy + 1, 2 * lazy + 1):
            W = limit_weights(o.t, 6, K, rng)
            idx = np.zeros((6, K), dtype=np.int32)
            idx[-1, ::7] = 1                                                            # the random-sign row also reads random words
            assert np.array_equal(run_gemm(g, h, W, idx), o.scalar_gemm(cts, W, idx)), (bits, K)
    g.free(h)
    g.close()


@pytest.mark.parametrize("bits,option", [(46, "gemm_mfma"), (47, "gemm_mfma"), (49, "f64"), (50, "f64")])
def test_scalar_gemm_on_both_sides_of_a_width_threshold(bits, option, rng):
    """the int8 matrix-core GEMM is allowed up to 46 bits, the FP64 small-weight kernels up to 49: at 46 / 47 bits M >= 16 outputs per list with
    "gemm_mfma" 1 and 0, at 49 / 50 bits with "f64" 1 and 0 - the oracle's words every time, over edge and random words, limit and random weights"""
    words = {}
    o = gemm_oracle(bits)
    cts = np.concatenate([edges(o)[[0, 1, 2, 3, 4]], all_max(o)[None, :], random_words(o, rng, 2)])
    O, K = 20, 40
    idx = np.tile(rng.integers(0, len(cts), size=K, dtype=np.int32), (O, 1))
    idx[:, 1] = -1                                                                      # a padded tap
    W = limit_weights(o.t, O, K, rng)
    W[O // 2:] = (rng.integers(-(2 ** 20 - 1), 2 ** 20, size=(O - O // 2, K)) % o.t).astype(np.uint64)
    exp = o.scalar_gemm(cts, W, idx)
    for on in (1, 0):
        o, g = gemm_context(bits, **{option: on})
        h = up(g, cts)
        got = run_gemm(g, h, W, idx)
        assert np.array_equal(got, exp), (bits, option, on)
        words[on] = got
        g.free(h)
        g.close()
    assert np.array_equal(words[1], words[0])


# ------------------------------------------------------------------ refusals
def test_moduli_of_61_bits_are_refused_without_a_leak():
    """SEAL 3.2's own 61-bit primes (m_sk, gamma, the first auxiliary prime) and a 61-bit NTT prime of no special form, as a data modulus beside a
    valid 60-bit prime: CN_ERR_ARG, no context, and no handle of a live context disturbed"""
    from cryptonets_amd._native import CnError, Context
    g = gpu("B60")
    base = g.live_handles()
    h = g.ct_alloc(1)
    other = next(x for x in range((1 << 61) - 2047, 1 << 60, -2048) if is_prime(x) and x % (1 << 18) != 1)
    for wide in (M_SK, GAMMA, B_0, other):
        assert is_prime(wide) and wide.bit_length() == 61 and wide % 2048 == 1
        for q in ([P60_1024[0], wide], [wide, P60_1024[0]], [wide]):
            with pytest.raises(CnError) as e:
                Context(1024, 12289, q=q, dbc=60, gdbc=60, device=0)
            assert e.value.code == -1 and "60" in str(e.value), hex(wide)
    assert g.live_handles() == base + 1
    g.free(h)
    assert g.live_handles() == base
    top = Context(1024, 12289, q=[ntt_primes(60, 1024, 1)[0]], dbc=60, gdbc=60, device=0)      # the largest NTT prime below 2^60 is accepted
    top.close()


@pytest.mark.parametrize("name,f64,legacy", [("R256", 1, 0), ("R512", 1, 0), ("F2048", 0, 1)])
def test_rotate_and_add_in_place_on_the_radix_2_key_switch(name, f64, legacy, rng):
    """below N = 1024 (and under "legacy_ntt", with integer keys) the key switch has no fused accumulator: a rotate-and-add whose accumulator is
    its own result (cn_sum_slots works in place) must add the rotation to the accumulator as it was, not to the rotation just written over it"""
    o, g = oracle(name), gpu(name, f64)
    cts = fresh(o, rng, 2)
    h = up(g, cts)
    try:
        g.set_option("legacy_ntt", legacy)
        g.rotate_rows_add(h, 0, -1, h, 0, h, 0, 2)
        exp = np.stack([o.add(c, o.rotate_rows(c, -1)) for c in cts])
        assert np.array_equal(g.ct_download(h, 0, 2), exp)
        g.rotate_columns_add(h, 0, h, 0, h, 0, 2)
        exp = np.stack([o.add(c, o.rotate_columns(c)) for c in exp])
        assert np.array_equal(g.ct_download(h, 0, 2), exp)
        g.ct_upload(h, 0, cts)
        g.sum_slots(h, 0, 2, 8)
        exp = []
        for c in cts:
            for s in (1, 2, 4):
                c = o.add(c, o.rotate_rows(c, -s))
            exp.append(c)
        assert np.array_equal(g.ct_download(h, 0, 2), np.stack(exp))
    finally:
        g.set_option("legacy_ntt", 0)
    g.free(h)
