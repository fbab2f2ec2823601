"""GPU: seeded symmetric ciphertexts (include/cnhip.h: cn_encrypt_symmetric, cn_ct_expand, cn_ct_upload_compact, cn_ct_download_compact), word for
word against the model of the draw (tests/seeded_model.py) and the CPU oracle's transforms - no tolerances.  Every parameter set of the suite that
device encryption supports (1024 <= N <= 16384), the 50-60-bit modulus sets included.

Choice tested here (include/cnhip.h): a level context expands (limbs are independent: its c1 is the first limbs of its parent's) AND encrypts, as it does
with cn_encrypt - its slice of the secret key, its own Delta."""
import io
import math

import numpy as np
import pytest

import seeded_model as sm
from conftest import PARAMS
from test_gpu_wide_moduli import SETS as WIDE_SETS
from test_oracle_math import is_prime

pytestmark = pytest.mark.gpu

NOISE_CLIP = 19          # thresholds of cn_noise_table(): |e| <= 19 (sigma 3.2 clipped at 6 sigma = 19.2, rounded towards zero)
SEED_A = bytes((7 * i + 3) & 0xff for i in range(32))

ALL_SETS = dict(PARAMS)
for _n in ("W60", "W60d", "S2048", "MIX2048", "F2048", "WIDE", "B49", "B50", "B60"):          # 1024 <= N: the legacy rings R256 / R512 cannot encrypt on the device
    ALL_SETS[_n] = WIDE_SETS[_n]
CASES = [(s, 1) for s in ALL_SETS] + [("F2048", 0), ("c3", 0), ("c5", 0), ("default4096", 0), ("tiny", 0)]          # f64 = 0: the integer policy at every transform size
IDS = lambda c: "%s-f64_%d" % c

_made = {}


def resolved_q(p):
    from cryptonets_amd._native import default_coeff_modulus
    return list(p["q"]) if p["q"] is not None else default_coeff_modulus(p["n"])


def make(name, f64=1):
    """a client context with device-made keys and an oracle that holds the same secret and public key; cached"""
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    if (name, f64) not in _made:
        p = ALL_SETS[name]
        q = resolved_q(p)
        g = Context(p["n"], p["t"], q=q, dbc=p["dbc"], gdbc=p["gdbc"], device=0)
        if not f64:
            g.set_option("f64", 0)
        g.keygen(77, galois=False)
        o = Oracle(p["n"], p["t"], q=q, dbc=p["dbc"], gdbc=p["gdbc"])
        o.import_keys(g.get_key(3), g.get_key(2))
        _made[(name, f64)] = (g, o)
    return _made[(name, f64)]


def expected_c1(o, a_seed, a_nonce, item, limbs=None):
    a = sm.seeded_a(a_seed, a_nonce, item, o.n, o.q[:limbs or o.k])
    return np.concatenate([o.ntt_inv(j, a[j]) for j in range(a.shape[0])])


def centred(x, q):
    x = x.astype(object)
    return np.where(x > q // 2, x - q, x)


def plaintexts(o, rng):
    """dense, constant, zero"""
    return np.stack([o.encode(rng.integers(0, o.t, size=o.n, dtype=np.uint64)), o.encode(np.full(o.n, o.t - 3, dtype=np.uint64)), np.zeros(o.n, dtype=np.uint64)])


# ---------------------------------------------------------------- 1. expansion
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_expansion_is_the_inverse_transform_of_the_model_draw(case):
    g, o = make(*case)
    kn = o.k * o.n
    h = g.ct_alloc(3)
    g.ct_upload(h, 0, np.zeros((3, 2 * kn), dtype=np.uint64))
    g.ct_expand(h, 0, 3, SEED_A, a_nonce=9, a_item0=5)
    got = g.ct_download(h, 0, 3)
    for i in range(3):
        assert not got[i, :kn].any()                                           # poly 0 is left alone
        assert np.array_equal(got[i, kn:], expected_c1(o, SEED_A, 9, 5 + i)), (case, i)
    # a does not depend on the context's sampler key or salt
    g.set_rng_key(bytes(range(100, 132)))
    g.set_rng_salt(0x1234567890abcdef)
    g.ct_expand(h, 1, 1, SEED_A, a_nonce=9, a_item0=6)
    assert np.array_equal(g.ct_download(h, 1, 1)[0], got[1])
    g.set_rng_key(bytes(32))
    # another nonce, item or seed gives other words; a range in the middle of the array touches nothing else
    g.ct_expand(h, 1, 1, SEED_A, a_nonce=10, a_item0=6)
    other = g.ct_download(h, 0, 3)
    assert np.array_equal(other[0], got[0]) and np.array_equal(other[2], got[2]) and not np.array_equal(other[1], got[1])
    assert np.array_equal(other[1, kn:], expected_c1(o, SEED_A, 10, 6))
    g.ct_expand(h, 1, 1, bytes(32), a_nonce=9, a_item0=6)
    assert not np.array_equal(g.ct_download(h, 1, 1)[0], got[1])
    g.free(h)


def test_expansion_redraws_rejected_words():
    """a 60-bit modulus near 2^64 / 16.5 rejects about 3 % of the generator's words: the redraw path of the kernel, against the model"""
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    n = 1024
    x = ((1 << 64) * 2 // 33) // (2 * n) * (2 * n) + 1
    while not is_prime(x):
        x -= 2 * n
    assert x < 1 << 60 and ((1 << 64) - 1) % x > x // 4
    for f64 in (1, 0):
        g = Context(n, 12289, q=[x], dbc=60, gdbc=60, device=0)
        g.set_option("f64", f64)
        o = Oracle(n, 12289, q=[x], dbc=60, gdbc=60)
        _, rejected = sm.sample_uniform8(SEED_A, 1, sm.STREAM_A, 0, np.arange(n // 8), x)
        assert rejected > 0
        h = g.ct_alloc(2)
        g.ct_expand(h, 0, 2, SEED_A, a_nonce=1, a_item0=0)
        got = g.ct_download(h, 0, 2)
        for i in range(2):
            assert np.array_equal(got[i, n:], expected_c1(o, SEED_A, 1, i))
        g.close()


# ---------------------------------------------------------------- 2. symmetric encryption
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_symmetric_encryption(case, rng):
    g, o = make(*case)
    kn = o.k * o.n
    plains = plaintexts(o, rng)
    ph, ch, dh = g.pt_alloc(3), g.ct_alloc(4), g.pt_alloc(4)
    g.pt_upload(ph, 0, plains)
    g.encrypt_symmetric(ph, 0, ch, 0, 3, seed=21, a_seed=SEED_A, a_nonce=2, a_item0=40)
    g.encrypt_symmetric(0, 0, ch, 3, 1, seed=22, a_seed=SEED_A, a_nonce=2, a_item0=43)          # pt = 0 encrypts zero
    cts = g.ct_download(ch, 0, 4)
    msgs = list(plains) + [np.zeros(o.n, dtype=np.uint64)]
    noises = []
    for i in range(4):
        assert np.array_equal(cts[i, kn:], expected_c1(o, SEED_A, 2, 40 + i)), "c1 is not the expansion"
        x = o.dot_with_secret(cts[i]).reshape(o.k, o.n)
        ref = o.add_plain(np.zeros(2 * kn, dtype=np.uint64), msgs[i])[:kn].reshape(o.k, o.n) if msgs[i].any() else np.zeros((o.k, o.n), dtype=np.uint64)
        e = [centred((x[j].astype(object) - ref[j].astype(object)) % o.q[j], o.q[j]) for j in range(o.k)]
        for j in range(1, o.k):
            assert np.array_equal(e[j], e[0]), "the noise differs between limbs"
        assert e[0].any(), "no noise at all"
        assert max(abs(int(v)) for v in e[0]) <= NOISE_CLIP
        noises.append(e[0])
        assert np.array_equal(o.decrypt(cts[i]), msgs[i])
    assert not np.array_equal(noises[0], noises[1])                            # every ciphertext draws its own noise
    g.decrypt(ch, 0, 4, dh, 0)
    assert np.array_equal(g.pt_download(dh, 0, 4), np.stack(msgs))
    # the noise comes from the context's sampler key, never from the public seed: another key, other c0 words under the same a
    g.set_rng_key(bytes(range(32)))
    g.encrypt_symmetric(ph, 0, ch, 0, 1, seed=21, a_seed=SEED_A, a_nonce=2, a_item0=40)
    g.set_rng_key(bytes(32))
    again = g.ct_download(ch, 0, 1)[0]
    assert np.array_equal(again[kn:], cts[0, kn:]) and not np.array_equal(again[:kn], cts[0, :kn])
    # the same plaintext for every ciphertext (pt_stride 0)
    g.encrypt_symmetric(ph, 1, ch, 0, 2, seed=23, a_seed=SEED_A, a_nonce=3, a_item0=0, pt_stride=0)
    both = g.ct_download(ch, 0, 2)
    assert np.array_equal(o.decrypt(both[0]), plains[1]) and np.array_equal(o.decrypt(both[1]), plains[1])
    for h in (ph, ch, dh):
        g.free(h)


# ---------------------------------------------------------------- 3. compact route
def server_for(g, o, case):
    """a second context that holds evaluation keys only (the client's relinearisation key and one Galois key)"""
    from cryptonets_amd._native import Context
    p = ALL_SETS[case[0]]
    s = Context(p["n"], p["t"], q=resolved_q(p), dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    if not case[1]:
        s.set_option("f64", 0)
    elt = 0
    if o.k > 1:
        s.set_relin_key(g.get_key(0))
        elt = g.galois_elt_from_step(1)
        s.set_galois_key(elt, g.get_key(1, elt))
    return s, elt


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_compact_route_reproduces_the_ciphertexts_on_an_evaluation_only_context(case, rng):
    from cryptonets_amd import serialization as ser
    from cryptonets_amd._native import CnError
    from cryptonets_amd.client import DeviceClient
    name, f64 = case
    g, o = make(name, f64)
    if o.k > 1 and not g.has_galois_key(g.galois_elt_from_step(1)):
        g.keygen(77, galois=True)                                              # same seed: the same secret key, now with Galois keys
        o.import_keys(g.get_key(3), g.get_key(2))
    s, elt = server_for(g, o, case)
    plains = plaintexts(o, rng)
    ph, ch = g.pt_alloc(3), g.ct_alloc(3)
    g.pt_upload(ph, 0, plains)
    g.encrypt_symmetric(ph, 0, ch, 0, 3, seed=31, a_seed=SEED_A, a_nonce=4, a_item0=100)
    full = g.ct_download(ch, 0, 3)
    c0 = g.ct_download_compact(ch, 0, 3)
    assert np.array_equal(c0, full[:, :o.k * o.n])
    sh = s.ct_alloc(4)
    s.ct_upload_compact(sh, 1, c0, SEED_A, a_nonce=4, a_item0=100)
    assert np.array_equal(s.ct_download(sh, 1, 3), full)
    with pytest.raises(CnError) as err:                                        # the server holds no secret key
        s.encrypt_symmetric(0, 0, sh, 0, 1, seed=1, a_seed=SEED_A)
    assert err.value.code == -3
    if o.k > 1:                                                                # evaluation on both copies: identical words
        g2, s2 = g.ct_alloc(3), s.ct_alloc(3)
        g.mul_relin(ch, 0, ch, 0, g2, 0, 3)
        s.mul_relin(sh, 1, sh, 1, s2, 0, 3)
        assert np.array_equal(g.ct_download(g2, 0, 3), s.ct_download(s2, 0, 3))
        g.rotate_rows(ch, 0, 1, g2, 0, 3)
        s.rotate_rows(sh, 1, 1, s2, 0, 3)
        rot = s.ct_download(s2, 0, 3)
        assert np.array_equal(g.ct_download(g2, 0, 3), rot)
        assert np.array_equal(o.decode(o.decrypt(rot[0])), o.decode(o.decrypt(o.rotate_rows(full[0], 1)))) if elt in o.galois_elts() else True
    # the device client and the framing: encrypt_compact -> bytes -> load -> upload_compact == the client's own ciphertexts
    client = DeviceClient(g, seed=5)
    c0b, desc = client.encrypt_compact(ph, 0, 3, a_item0=7)
    assert len(desc.a_seed) == 32 and desc.a_seed != bytes(32) and desc.count == 3 and desc.a_item0 == 7
    c0c, desc2 = client.encrypt_compact(ph, 0, 3)
    assert desc2.a_seed != desc.a_seed                                         # OS entropy per call
    f = io.BytesIO()
    ser.save_compact_batch(f, c0b, desc)
    parms = ser.Parameters(o.n, o.q, o.t)
    words, d, limbs = ser.load_compact_batch(io.BytesIO(f.getvalue()), parms)
    assert d == desc and limbs == o.k and d.parms_id == parms.parms_id()
    s.ct_upload_compact(sh, 0, words, d.a_seed, d.a_nonce, d.a_item0)
    back = s.ct_download(sh, 0, 3)
    for i in range(3):
        assert np.array_equal(back[i, :o.k * o.n], c0b[i]) and np.array_equal(o.decrypt(back[i]), plains[i])
    for h in (ph, ch):
        g.free(h)
    s.close()


# ---------------------------------------------------------------- 4. budget
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fresh_symmetric_noise_is_not_larger_than_public_key_noise(case, rng):
    """cn_noise_norm is || t e_fresh - (q mod t) m~ + rounding ||_inf with m~ the centred plaintext: the second term does not depend on how the ciphertext was
    encrypted and reaches t^2 / 2 for a dense plaintext - above t || e_fresh || of either route as soon as t exceeds a few hundred, and then the comparison is
    decided by the signs at one coefficient, not by the fresh noise (c2, dense: 38221365860357514529374 for cn_encrypt against 38221365950518851799810, both
    (q mod t) m~ to 9 digits).  So the assertion runs on the plaintexts whose message term stays below the fresh noise - zero and a constant (one coefficient,
    |m~| = 3: at most 3 t + t against the 19 t of e) - where the symmetric norm is at most 23 t and cn_encrypt's u e_pk + e1 + e2 s is the maximum of N sums of 2 N
    products; the dense plaintext is measured and printed with them."""
    g, o = make(*case)
    plains = plaintexts(o, rng)
    ph, ca, cb = g.pt_alloc(3), g.ct_alloc(3), g.ct_alloc(3)
    g.pt_upload(ph, 0, plains)
    g.encrypt(ph, 0, ca, 0, 3, seed=41)
    g.encrypt_symmetric(ph, 0, cb, 0, 3, seed=41, a_seed=SEED_A, a_nonce=5, a_item0=0)
    pk, sym = g.noise_norm(ca, 0, 3), g.noise_norm(cb, 0, 3)
    gain = [math.log2(a) - math.log2(b) for a, b in zip(pk, sym)]
    print("seeded budget gain %s-f64_%d (dense, constant, zero): %s bits" % (case[0], case[1], ", ".join("%.2f" % x for x in gain)))
    for a, b in list(zip(pk, sym))[1:]:
        assert 0 < b <= a and b <= 23 * o.t, (a, b)
    # the dense plaintext: the two norms are norms of vectors that differ by t (e_pk - e_sym) alone (message and rounding terms are the same words), so they agree
    # to within t times the bounds of the two fresh noises: |u e_pk + e1 + e2 s| <= 19 N + 19 + 19 N (u, s ternary, |e| <= 19) and |e_sym| <= 19
    assert abs(pk[0] - sym[0]) <= o.t * (NOISE_CLIP * (2 * o.n + 1) + NOISE_CLIP), (pk[0], sym[0])
    for h in (ph, ca, cb):
        g.free(h)


# ---------------------------------------------------------------- 5. refusals and levels
def test_refusals(rng):
    from cryptonets_amd._native import CnError, Context
    g, o = make("tiny")
    h, ph = g.ct_alloc(2), g.pt_alloc(1)
    h3 = g.ct_alloc(1, 3)
    g.pt_upload(ph, 0, plaintexts(o, rng)[:1])

    def refused(code, fn, *a, **kw):
        with pytest.raises(CnError) as err:
            fn(*a, **kw)
        assert err.value.code == code, err.value

    before = g.ct_download(h, 0, 2)
    refused(-1, g.encrypt_symmetric, ph, 0, h, 1, 2, a_seed=SEED_A)                       # range
    refused(-1, g.encrypt_symmetric, ph, 1, h, 0, 1, a_seed=SEED_A)                       # plaintext range
    refused(-1, g.encrypt_symmetric, ph, 0, h3, 0, 1, a_seed=SEED_A)                      # size-3 ciphertexts
    refused(-1, g.ct_expand, h, 2, 1, SEED_A)
    refused(-1, g.ct_expand, h3, 0, 1, SEED_A)
    refused(-1, g.ct_expand, h, 0, 1, SEED_A, a_item0=1 << 40)                            # 40 item bits
    refused(-1, g._chk, g.L.cn_ct_expand(g._h, h, 0, 1, None, 0, 0))                      # null seed
    refused(-1, g._chk, g.L.cn_ct_upload_compact(g._h, h, 0, 1, None, SEED_A, 0, 0))      # null c0 words
    refused(-1, g._chk, g.L.cn_ct_download_compact(g._h, h, 0, 1, None))
    refused(-1, g.ct_download_compact, h, 1, 2)
    with pytest.raises(ValueError):                                                       # wrong row width: full ciphertext rows where c0 rows belong
        g.ct_upload_compact(h, 0, before, SEED_A)
    with pytest.raises(ValueError):
        g.ct_upload_compact(h, 1, before[:, :o.k * o.n], SEED_A)                          # two rows from index 1 of a two-ciphertext array
    with pytest.raises(ValueError):
        g.ct_upload_compact(h3, 0, before[:1, :o.k * o.n], SEED_A)
    with pytest.raises(ValueError):
        g.ct_expand(h, 0, 1, b"short")
    spare = g.ct_alloc(1)
    g.graph_begin()                                                                       # while a graph is recorded
    try:
        refused(-1, g.encrypt_symmetric, ph, 0, h, 0, 1, a_seed=SEED_A)
        refused(-1, g.ct_expand, h, 0, 1, SEED_A)
        refused(-1, g.ct_upload_compact, h, 0, before[:, :o.k * o.n], SEED_A)
        refused(-1, g.ct_download_compact, h, 0, 1)
        g.add(spare, 0, spare, 0, spare, 0)                                               # (the recording can still be closed)
    finally:
        g.free(g.graph_end())
    g.free(spare)
    assert np.array_equal(g.ct_download(h, 0, 2), before)                                 # nothing was written
    # no secret key
    p = ALL_SETS["tiny"]
    s = Context(p["n"], p["t"], q=p["q"], device=0)
    sh = s.ct_alloc(1)
    refused(-3, s.encrypt_symmetric, 0, 0, sh, 0, 1, a_seed=SEED_A)
    s.ct_expand(sh, 0, 1, SEED_A)                                                         # ... but it expands
    s.close()
    # a ring outside the range of device encryption
    r = WIDE_SETS["R512"]
    small = Context(r["n"], r["t"], q=r["q"], dbc=r["dbc"], gdbc=r["gdbc"], device=0)
    small.set_secret_key(np.ones(len(r["q"]) * r["n"], dtype=np.uint64))
    hh = small.ct_alloc(1)
    refused(-1, small.encrypt_symmetric, 0, 0, hh, 0, 1, a_seed=SEED_A)
    refused(-1, small.ct_expand, hh, 0, 1, SEED_A)
    refused(-1, small.ct_upload_compact, hh, 0, np.zeros((1, len(r["q"]) * r["n"]), dtype=np.uint64), SEED_A)
    small.close()
    for x in (h, h3, ph):
        g.free(x)


def test_level_contexts_expand_and_encrypt(rng):
    """a level's c1 is the first limbs of its parent's expansion; a level encrypts with its slice of the secret key, as cn_encrypt does there"""
    from oracle.cno import Oracle
    g, o = make("tiny")
    lv = g.level(2)
    ol = Oracle(o.n, o.t, q=o.q[:2], dbc=o.dbc, gdbc=o.gdbc)
    ol.import_keys(np.ascontiguousarray(o.secret_key().reshape(o.k, o.n)[:2]).reshape(-1), np.ascontiguousarray(o.public_key().reshape(2, o.k, o.n)[:, :2]).reshape(-1))
    kn = 2 * o.n
    h, hp = lv.ct_alloc(2), g.ct_alloc(2)
    lv.ct_expand(h, 0, 2, SEED_A, a_nonce=6, a_item0=1)
    g.ct_expand(hp, 0, 2, SEED_A, a_nonce=6, a_item0=1)
    low, top = lv.ct_download(h, 0, 2), g.ct_download(hp, 0, 2)
    for i in range(2):
        assert np.array_equal(low[i, kn:], top[i, o.k * o.n:o.k * o.n + kn])
        assert np.array_equal(low[i, kn:], expected_c1(ol, SEED_A, 6, 1 + i))
    plains = plaintexts(o, rng)
    ph, dh = lv.pt_alloc(3), lv.pt_alloc(2)
    lv.pt_upload(ph, 0, plains)
    lv.encrypt_symmetric(ph, 0, h, 0, 2, seed=51, a_seed=SEED_A, a_nonce=6, a_item0=1)
    cts = lv.ct_download(h, 0, 2)
    for i in range(2):
        assert np.array_equal(cts[i, kn:], low[i, kn:]) and np.array_equal(ol.decrypt(cts[i]), plains[i])
    lv.decrypt(h, 0, 2, dh, 0)
    assert np.array_equal(lv.pt_download(dh, 0, 2), plains[:2])
    for x in (h, ph, dh):
        lv.free(x)
    g.free(hp)


# ---------------------------------------------------------------- 6. end to end
def test_cryptonets_mnist_batch_through_the_compact_route():
    """the data owner encrypts the 784 input ciphertexts symmetrically and sends c0 words + a descriptor; a server that holds the relinearisation key only
    ingests them, evaluates CryptoNets-MNIST, and the owner decrypts the integer model's logits - both plaintext primes"""
    from cryptonets_amd import cryptonets_mnist as cm
    from cryptonets_amd import serialization as ser
    from cryptonets_amd._native import Context
    from cryptonets_amd.client import DeviceClient
    from test_cryptonets_mnist import weights
    layers = cm.layer_tables(*weights())
    x_int = np.rint(cm.synthetic_images(cm.N, seed=9) * cm.NORMALIZATION * cm.INPUT_SCALE).astype(np.int64)
    for p in cm.PLAIN_PRIMES:
        owner = Context(cm.N, p, dbc=10, gdbc=20, device=0)
        owner.keygen(0x51CE ^ p, galois=False)
        ph = owner.pt_alloc(784)
        owner.encode_batch(np.mod(x_int.T, p).astype(np.uint64), ph, 0)
        c0, desc = DeviceClient(owner, seed=123).encrypt_compact(ph, 0, 784)
        owner.free(ph)
        f = io.BytesIO()
        ser.save_compact_batch(f, c0, desc)
        assert f.tell() < 0.51 * 784 * owner.ctw * 8                           # half the bytes of the full ciphertexts
        server = Context(cm.N, p, dbc=10, gdbc=20, device=0)
        server.set_relin_key(owner.get_key(0))
        words, d, limbs = ser.load_compact_batch(io.BytesIO(f.getvalue()), ser.Parameters(cm.N, owner.q, p))
        ch = cm.CryptoNetsChannel(server, layers, cm.constant_plaintext(cm.N))
        server.ct_upload_compact(ch.h_in, 0, words, d.a_seed, d.a_nonce, d.a_item0)
        ch.forward()
        out = server.ct_download(ch.h5, 0, 10)
        server.close()
        oh, dh = owner.ct_alloc(10), owner.pt_alloc(10)
        owner.ct_upload(oh, 0, out)
        owner.decrypt(oh, 0, 10, dh, 0)
        got = owner.decode_batch(dh, 0, 10).T
        assert np.array_equal(got, cm.model_mod_p_dense(x_int, layers, p))
        owner.close()
