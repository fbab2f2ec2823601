"""GPU: known answers for the data owner's side - cn_keygen, cn_keygen_galois, cn_encrypt, cn_encrypt_zero_new, cn_encrypt_symmetric - word for word against
the model of the draws (tests/sampler_model.py), no tolerances.  The device's randomness is a function of (sampler key, nonce, item, stream, trial, block), so
EVERY word of a generated key and of a fresh ciphertext is predicted: the secret key, both halves of the public key, every entry of the relinearisation and
Galois keys, c0 and c1 of every ciphertext, with the item counter followed across the calls.  What tests/test_sampler_model.py shows about the model's
distribution (chi-square against the exact probabilities, rejected near misses, independent streams) therefore holds for the device's draws.

Parameter sets: tests/sampler_cases.py.  Which assertion catches which slip of the device code:
  * the highest instead of the lowest non-3 pair in sample_ternary16, a shifted threshold index, a sign from another bit: get_key(3) / get_key(2) in `keys`
    (the secret key and the public noise are the first draws), and every ciphertext after them;
  * e1 and e2 from one stream, or swapped: c1 of the first ciphertext of `public-key encryption` (c0 as well when swapped);
  * a block reused between ciphertexts or key entries (item / blk / stream packing): the second ciphertext, the second key entry;
  * a nonce cut to 32 bits on its way through the binding: every comparison (all seeds here are above 2^32 and differ only in their high words from one
    another in places), first get_key(3)."""
import numpy as np
import pytest

import sampler_model as M
from sampler_cases import CASES, make_oracle

pytestmark = pytest.mark.gpu

KEY = bytes((37 * i + 11) & 0xff for i in range(32))
SEED_A = bytes((7 * i + 3) & 0xff for i in range(32))
SALT = 0xfeedc0de12345678
HI = 0x5ca1ab1e << 32                     # every nonce of the test is at or above 2^32
RUNS = [("A", 1, 0), ("B", 1, SALT), ("C", 1, 0), ("C", 0, 0), ("D", 1, 0), ("E", 1, 0)]          # (case, "f64" option, salt set after the key)


class Owner:
    """a device context with the fixed sampler key, its oracle (transforms, Delta, decryption) and the model's view of the item counter"""

    def __init__(self, name, f64, salt):
        from cryptonets_amd._native import Context
        c = CASES[name]
        self.case, self.o = c, make_oracle(c)
        self.g = g = Context(c["n"], c["t"], q=c["q"], dbc=c["dbc"], gdbc=c["gdbc"], device=0)
        if not f64:
            g.set_option("f64", 0)
        if c["ks_xi"]:
            g.set_option("ks_xi", 1)
        g.set_rng_key(KEY)
        self.key = KEY
        if salt:
            g.set_rng_salt(salt)
            self.key = M.with_salt(KEY, salt)
        self.item = None
        self.made = []                    # (ciphertext words, message polynomial) of every ciphertext checked: decrypted at the end

    def keygen(self, seed):
        g, o, c = self.g, self.o, self.case
        g.keygen(seed, galois=c["galois"])
        K = self.K = M.keygen_model(o, self.key, seed, c["galois"], ks_xi=bool(c["ks_xi"]))
        assert np.array_equal(g.get_key(3), K["sk"]), "secret key"
        pk = g.get_key(2)
        assert np.array_equal(pk[o.k * o.n:], K["pk"][o.k * o.n:]), "public key: a"
        assert np.array_equal(pk, K["pk"]), "public key: b"
        rl = g.get_key(0).reshape(-1, 2, o.k * o.n)
        want = K["rlk"].reshape(-1, 2, o.k * o.n)
        assert rl.shape == want.shape
        for e in range(rl.shape[0]):
            assert np.array_equal(rl[e, 1], want[e, 1]), "relinearisation key entry %d: a" % e
            assert np.array_equal(rl[e, 0], want[e, 0]), "relinearisation key entry %d: b" % e
        assert sorted(g.galois_elts()) == sorted(K["gk"])
        for elt, words in K["gk"].items():
            assert np.array_equal(g.get_key(1, elt), words), "Galois key of element %d" % elt
        self.item = K["items"]
        o.import_keys(K["sk"], K["pk"])

    def keygen_galois(self, seed, elts):
        self.g.keygen_galois(seed, elts)
        gk, self.item = M.keygen_galois_model(self.o, self.key, seed, self.item, self.K["s"], elts, ks_xi=bool(self.case["ks_xi"]))
        for elt in elts:
            assert np.array_equal(self.g.get_key(1, elt), gk[elt]), "cn_keygen_galois: element %d" % elt

    def expect(self, seed, plains):
        """the model's ciphertexts of one call (or of one deferred per-ciphertext call); the item counter moves on"""
        want = M.encrypt_model(self.o, self.key, seed, self.item, self.K["pk"], plains)
        self.item += len(plains)
        return want

    def check(self, got, want, plains, what):
        kn = self.o.k * self.o.n
        for i in range(len(plains)):
            assert np.array_equal(got[i, kn:], want[i, kn:]), "%s: c1 of ciphertext %d" % (what, i)
            assert np.array_equal(got[i, :kn], want[i, :kn]), "%s: c0 of ciphertext %d" % (what, i)
            self.made.append((got[i], np.zeros(self.o.n, dtype=np.uint64) if plains[i] is None else plains[i]))

    def decrypt_all(self, g=None, o=None):
        g, o = g or self.g, o or self.o
        cts = np.stack([c for c, _ in self.made])
        msgs = np.stack([m for _, m in self.made])
        h, dh = g.ct_alloc(len(cts)), g.pt_alloc(len(cts))
        g.ct_upload(h, 0, cts)
        g.decrypt(h, 0, len(cts), dh, 0)
        assert np.array_equal(g.pt_download(dh, 0, len(cts)), msgs), "device decryption"
        for c, m in self.made:
            assert np.array_equal(o.decrypt(c), m), "oracle decryption"
        g.free(h)
        g.free(dh)
        self.made = []


def plaintexts(o):
    """dense, constant (upper half of the plain range: the rounding correction of Delta m), dense"""
    r = np.random.default_rng(20261019)
    return np.stack([o.encode(r.integers(0, o.t, size=o.n, dtype=np.uint64)), o.encode(np.full(o.n, o.t - 3, dtype=np.uint64)),
                     o.encode(r.integers(0, o.t, size=o.n, dtype=np.uint64))])


def public_key_encryptions(w, ph, plains, base):
    """3 plaintexts, one plaintext twice (pt_stride 0), pt = 0, cn_encrypt_zero_new: the items run on across the calls"""
    g = w.g
    ch = g.ct_alloc(6)
    g.encrypt(ph, 0, ch, 0, 3, seed=base + 1)
    g.encrypt(ph, 1, ch, 3, 2, seed=base + 2, pt_stride=0)
    g.encrypt(0, 0, ch, 5, 1, seed=base + (1 << 40))
    z = g.encrypt_zero_new(seed=base + 4)
    got = np.concatenate([g.ct_download(ch, 0, 6), g.ct_download(z, 0, 1)])
    sets = [(base + 1, list(plains)), (base + 2, [plains[1], plains[1]]), (base + (1 << 40), [None]), (base + 4, [None])]
    want = np.concatenate([w.expect(seed, pl) for seed, pl in sets])
    w.check(got, want, [p for _, pl in sets for p in pl], "public-key encryption")
    g.free(ch)
    g.free(z)


def per_ciphertext_calls(w, ph, plains, base, defer):
    """deferred per-ciphertext calls, each with its own nonce, merged into one launch chain at the flush: the items follow call order"""
    g = w.g
    ch = g.ct_alloc(3)
    g.set_option("defer", defer)
    try:
        g.encrypt(ph, 0, ch, 0, 1, seed=base + 10)
        z = g.encrypt_zero_new(seed=base + 11)
        g.encrypt(ph, 1, ch, 1, 2, seed=base + 12)
        g.sync()
    finally:
        g.set_option("defer", 0)
    got = np.concatenate([g.ct_download(ch, 0, 1), g.ct_download(z, 0, 1), g.ct_download(ch, 1, 2)])
    sets = [(base + 10, [plains[0]]), (base + 11, [None]), (base + 12, [plains[1], plains[2]])]
    want = np.concatenate([w.expect(seed, pl) for seed, pl in sets])
    w.check(got, want, [p for _, pl in sets for p in pl], "defer = %d" % defer)
    g.free(ch)
    g.free(z)


def symmetric_encryptions(w, ph, plains, base):
    g, o = w.g, w.o
    sh = g.ct_alloc(2)
    g.encrypt_symmetric(ph, 1, sh, 0, 2, seed=base + 20, a_seed=SEED_A, a_nonce=HI + 9, a_item0=5)
    want = M.encrypt_symmetric_model(o, w.key, base + 20, w.item, w.K["sk"], SEED_A, HI + 9, 5, [plains[1], plains[2]])
    w.item += 2
    w.check(g.ct_download(sh, 0, 2), want, [plains[1], plains[2]], "symmetric encryption")
    g.free(sh)


def level_encryption(w, plains, base):
    """the level context over the first two of case A's three moduli: the parent's sampler key and public key (sliced), its own Delta, its OWN item counter
    (a new context: it starts at 0)"""
    g, o, c = w.g, w.o, w.case
    lv = g.level(2)
    ol = make_oracle(c, limbs=2)
    kn = o.k * o.n
    sk2 = np.ascontiguousarray(w.K["sk"].reshape(o.k, o.n)[:2]).reshape(-1)
    pk2 = np.ascontiguousarray(w.K["pk"].reshape(2, o.k, o.n)[:, :2]).reshape(-1)
    assert np.array_equal(lv.get_key(3), sk2) and np.array_equal(lv.get_key(2), pk2) and len(w.K["pk"]) == 2 * kn
    ol.import_keys(sk2, pk2)
    ph, ch = lv.pt_alloc(3), lv.ct_alloc(3)
    lv.pt_upload(ph, 0, plains)
    lv.encrypt(ph, 0, ch, 0, 2, seed=base + 30)
    lv.encrypt(0, 0, ch, 2, 1, seed=base + 31)
    got = lv.ct_download(ch, 0, 3)
    want = np.concatenate([M.encrypt_model(ol, w.key, base + 30, 0, pk2, [plains[0], plains[1]]), M.encrypt_model(ol, w.key, base + 31, 2, pk2, [None])])
    assert got.shape == (3, 2 * 2 * o.n)
    sub = Owner.__new__(Owner)                                       # (check / decrypt_all over the level's oracle and context)
    sub.o, sub.made = ol, []
    sub.check(got, want, [plains[0], plains[1], None], "level context")
    sub.decrypt_all(g=lv, o=ol)
    lv.free(ph)
    lv.free(ch)
    lv.close()


@pytest.mark.parametrize("name,f64,salt", RUNS, ids=["%s-f64_%d%s" % (n, f, "-salt" if s else "") for n, f, s in RUNS])
def test_keys_and_ciphertexts_are_the_models(name, f64, salt):
    w = Owner(name, f64, salt)
    g, o, c = w.g, w.o, w.case
    base = HI + (ord(name) << 8)
    try:
        w.keygen(base)
        plains = plaintexts(o)
        ph = g.pt_alloc(3)
        g.pt_upload(ph, 0, plains)
        if c["galois"]:                                              # two elements outside the default set; the item counter goes on from items + 2 entries
            extra = [e for e in range(5, 2 * o.n, 2) if e not in w.K["gk"]][:2]
            w.keygen_galois(base + (7 << 36), extra)
        public_key_encryptions(w, ph, plains, base + (1 << 44))
        symmetric_encryptions(w, ph, plains, base + (2 << 44))
        if name == "A":
            default = g.get_option("enc_fused")
            for fused in (0, 1):                                     # the three-launch chain, the per-ciphertext fused kernel
                g.set_option("enc_fused", fused)
                public_key_encryptions(w, ph, plains, base + ((3 + fused) << 44))
            g.set_option("enc_fused", default)
            for defer in (1, 2):
                per_ciphertext_calls(w, ph, plains, base + ((5 + defer) << 44), defer)
            level_encryption(w, plains, base + (8 << 44))
        w.decrypt_all()
        g.free(ph)
    finally:
        g.close()
