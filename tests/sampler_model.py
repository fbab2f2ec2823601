"""Restatement of the data owner's side of the library - the device samplers (cn_dev_common.hip.h: sample_ternary16, sample_noise8; the thresholds of
cn_noise_table.h), cn_keygen, cn_keygen_galois, cn_encrypt / cn_encrypt_zero_new and cn_encrypt_symmetric (cn_client.hip, cn_k_keygen.hip.h, cn_k_seeded.hip.h) -
from their documented behaviour, with numpy and Python integers on the CPU.  Every draw is a function of (256-bit key, 64-bit nonce, item, stream, trial, block),
so the model predicts EVERY word of a generated key and of a fresh ciphertext.  Nothing of the library is imported; the generator, the counter layout and the
uniform draw come from tests/seeded_model.py, the transforms and the Delta term from the CPU oracle handed in as `o`.

Draws (block counter = item (40 bits) | stream (4) | trial (4) | block (16), nonce = the `seed` argument of the call):
  stream 0  ternary: the secret key (item 0 of cn_keygen), u of an encryption        16 coefficients per block, coefficient c from word c
  stream 1  noise:   key noise, e1 of an encryption, e of a symmetric encryption      8 coefficients per block, coefficient c from the word (w[2c] << 32) | w[2c+1]
  stream 2  noise:   e2 of an encryption
  stream 3  uniform: the `a` of keys, limb j at blocks j N/8 + b                      seeded_model.sample_uniform8
  stream 4  uniform: the public `a` of seeded ciphertexts (under the PUBLIC seed)     seeded_model.seeded_a

The distribution functions take the parameters of the documented distribution as arguments (sigma, clip, rounding, threshold shift, sign probability, P(0) of
the ternary draw) so that tests/test_sampler_model.py can build the near misses its statistic has to reject; the defaults are the library's."""
import numpy as np

import seeded_model as sm

SIGMA, CLIP, NTHR = 3.2, 19.2, 19
ST_TERNARY, ST_E1, ST_E2, ST_KEY_A = 0, 1, 2, 3
TWO63 = 1 << 63


# ---------------------------------------------------------------- thresholds and exact probabilities
def _mp():
    try:
        import mpmath
    except ImportError:                                       # (mpmath comes with sympy; a test without it skips)
        import pytest
        pytest.skip("mpmath is not installed: no exact thresholds")
    return mpmath


def noise_thresholds(sigma=SIGMA, clip=CLIP, nearest=False, prec=256):
    """thr[i] = floor(2^63 P(|x| < i + 1 | |x| <= clip)), x ~ N(0, sigma^2), i = 0 .. 18, as Python integers (mpmath at `prec` bits).
    nearest: the thresholds of a draw that rounds to nearest instead of towards zero (|value| = k from k - 1/2 on)"""
    mp = _mp()
    with mp.workprec(prec):
        s = mp.mpf(repr(sigma)) * mp.sqrt(2)
        norm = mp.erf(mp.mpf(repr(clip)) / s)
        out = []
        for i in range(NTHR):
            edge = mp.mpf(i + 1) - (mp.mpf(1) / 2 if nearest else 0)
            c = mp.erf(edge / s) / norm
            out.append(TWO63 - 1 if c >= 1 else int(mp.floor(c * TWO63)))
    return out


def shifted(thr):
    """the table read one index too far: magnitude k where the documented draw gives k + 1"""
    return list(thr[1:]) + [TWO63 - 1]


def noise_probabilities(thr, sign_p=None):
    """exact probabilities of the values -19 .. 19 (index v + 19) of a draw with the thresholds `thr`, as floats: |v| = k has (thr[k] - thr[k-1]) / 2^63,
    halved between the signs for k > 0 (sign_p: the probability of the negative sign, 1/2 in the library)"""
    edges = [0] + [int(x) for x in thr] + [TWO63]
    mag = [(edges[k + 1] - edges[k]) / TWO63 for k in range(NTHR + 1)]
    neg = 0.5 if sign_p is None else sign_p
    p = np.zeros(2 * NTHR + 1)
    p[NTHR] = mag[0]
    for k in range(1, NTHR + 1):
        p[NTHR - k], p[NTHR + k] = mag[k] * neg, mag[k] * (1 - neg)
    return p


# ---------------------------------------------------------------- generator blocks over a grid
def blocks(key, nonce, stream, items, blks, trial=0):
    """the generator's blocks of (item, blk) for every item of `items` and every block index of `blks`: uint32 [len(items) * len(blks), 16], items major.
    Every block of the model, the uniform draw's included, comes out of seeded_model.chacha20_block (the collision test records its arguments there)"""
    items = np.atleast_1d(np.asarray(items, dtype=np.uint64))
    blks = np.atleast_1d(np.asarray(blks, dtype=np.uint64))
    assert int(items.max()) < 1 << 40 and int(blks.max()) < 1 << 16 and 0 <= stream < 16 and 0 <= trial < 16
    ctr = ((items[:, None] << np.uint64(24)) | np.uint64((stream << 20) | (trial << 16)) | blks[None, :]).reshape(-1)
    assert int(ctr[0]) == sm.rng_counter(int(items[0]), stream, trial, int(blks[0])) and int(ctr[-1]) == sm.rng_counter(int(items[-1]), stream, trial, int(blks[-1]))
    step = 1 << 14                                           # pieces that stay in the cache: the same blocks, several times faster on large grids
    return np.concatenate([sm.chacha20_block(key, ctr[i:i + step], nonce) for i in range(0, len(ctr), step)])


# ---------------------------------------------------------------- ternary
def ternary_from_words(w, p0=None):
    """value of every 32-bit word: (the LOWEST two-bit pair that is not 3) - 1, or 2 when every pair is 3 (the caller redraws).
    p0: a near miss that is not the library's draw - 0 with probability p0, else +-1 by the lowest bit"""
    w = np.asarray(w, dtype=np.uint32)
    if p0 is not None:
        zero = w < np.uint32(int(p0 * (1 << 32)))
        return np.where(zero, 0, np.where(w & np.uint32(1), 1, -1)).astype(np.int8)
    v = np.full(w.shape, 2, dtype=np.int8)
    for b in range(30, -2, -2):                              # from the top pair down: the last assignment, the lowest pair, stands
        t = ((w >> np.uint32(b)) & np.uint32(3)).astype(np.int8)
        v = np.where(t != 3, t - 1, v).astype(np.int8)
    return v


def sample_ternary_items(key, nonce, stream, items, n, block_fn=blocks):
    """ternary polynomials of `items`: (int8 [len(items), n], number of redrawn coefficients).  Coefficient c of block blk takes word c of that block; a word
    whose sixteen pairs are all 3 (probability 4^-16) takes word c of the block of trial 1, 2, ... instead"""
    items = np.atleast_1d(np.asarray(items, dtype=np.uint64))
    assert n % 16 == 0
    bpp = n // 16
    v = ternary_from_words(block_fn(key, nonce, stream, items, np.arange(bpp), 0)).reshape(len(items), bpp, 16)
    redrawn, trial = 0, 0
    while (v == 2).any():
        trial += 1
        assert trial < 16, "more redraws than the counter has trial bits"
        for it, blk in sorted(set(zip(*np.nonzero(v == 2)[:2]))):
            again = ternary_from_words(block_fn(key, nonce, stream, [items[it]], [blk], trial))[0]
            pend = v[it, blk] == 2
            redrawn += int((pend & (again != 2)).sum())
            v[it, blk] = np.where(pend, again, v[it, blk])
    return v.reshape(len(items), n), redrawn


def sample_ternary(key, nonce, stream, item, n, **kw):
    return sample_ternary_items(key, nonce, stream, [item], n, **kw)[0][0]


# ---------------------------------------------------------------- clipped normal
def noise_from_blocks(w, thr, sign_p=None):
    """8 values per block: word c = (w[2c] << 32) | w[2c+1]; the top bit is the sign, |value| = the number of thresholds at or below the low 63 bits.
    sign_p: a near miss - negative with probability sign_p, decided by the low 32 bits, instead of the top bit"""
    w = np.asarray(w, dtype=np.uint32).astype(np.uint64)
    v = (w[:, 0::2] << np.uint64(32)) | w[:, 1::2]
    mag = v & np.uint64(TWO63 - 1)
    k = np.searchsorted(np.asarray(thr, dtype=np.uint64), mag, side="right").astype(np.int8)      # thresholds <= mag
    neg = (v >> np.uint64(63)).astype(bool) if sign_p is None else (v & np.uint64(0xffffffff)) < np.uint64(int(sign_p * (1 << 32)))
    return np.where(neg, -k, k).astype(np.int8)


def sample_noise_items(key, nonce, stream, items, n, thr=None, sign_p=None):
    """noise polynomials of `items`: int8 [len(items), n] (no redraws: the inversion of the cumulative distribution has no rejection)"""
    assert n % 8 == 0
    thr = noise_thresholds() if thr is None else thr
    items = np.atleast_1d(np.asarray(items, dtype=np.uint64))
    return noise_from_blocks(blocks(key, nonce, stream, items, np.arange(n // 8), 0), thr, sign_p).reshape(len(items), n)


def sample_noise(key, nonce, stream, item, n, **kw):
    return sample_noise_items(key, nonce, stream, [item], n, **kw)[0]


# ---------------------------------------------------------------- arithmetic on residues (exact: Python integers)
def mulmod(a, b, q):
    return ((np.asarray(a).astype(object) * np.asarray(b).astype(object)) % q).astype(np.uint64)


def addmod(a, b, q):
    return ((np.asarray(a).astype(object) + np.asarray(b).astype(object)) % q).astype(np.uint64)


def negmod(a, q):
    return ((-np.asarray(a).astype(object)) % q).astype(np.uint64)


def residues(small, qs):
    """a polynomial of small signed integers as residues: uint64 [k, n] (k_expand_small)"""
    s = np.asarray(small).astype(np.int64)
    return np.stack([np.where(s >= 0, s, s + q).astype(np.uint64) for q in qs])


def ntt(o, x):
    return np.stack([o.ntt_fwd(j, x[j]) for j in range(x.shape[0])])


def intt(o, x):
    return np.stack([o.ntt_inv(j, x[j]) for j in range(x.shape[0])])


def uniform_poly(key, nonce, stream, item, n, qs):
    """uniform residues [k, n]: limb j from blocks j N/8 .. (j + 1) N/8 - 1 (k_sample_uniform; the layout of seeded_model.seeded_a)"""
    bpl = n // 8
    assert len(qs) * bpl <= 1 << 16
    out = []
    for j, q in enumerate(qs):
        out.append(sm.sample_uniform8(key, nonce, stream, item, j * bpl + np.arange(bpl), q)[0].reshape(n))
    return np.stack(out)


def automorphism(s, elt):
    """x -> x^elt on a polynomial of small integers mod x^n + 1"""
    n = len(s)
    idx = (np.arange(n, dtype=np.int64) * elt) % (2 * n)
    out = np.zeros(n, dtype=np.int64)
    out[idx % n] = np.where(idx >= n, -s.astype(np.int64), s.astype(np.int64))
    return out


def with_salt(key, salt):
    """cn_set_rng_salt after cn_set_rng_key: key words 0 and 1 are the low and the high half of the salt"""
    return int(salt & 0xffffffffffffffff).to_bytes(8, "little") + bytes(key)[8:]


# ---------------------------------------------------------------- keys
def digit_counts(qs, dbc):
    return [-(-q.bit_length() // dbc) for q in qs]


def default_galois_elts(n):
    """cn_keygen's order: 2N - 1, then 3^(2^i), 3^-(2^i) for i = 0 .. log2(N) - 2"""
    m = 2 * n
    p3, ip3, out = 3, pow(3, -1, m), [m - 1]
    for _ in range(n.bit_length() - 2):
        out += [p3, ip3]
        p3, ip3 = p3 * p3 % m, ip3 * ip3 % m
    return out


def ksk_model(o, key, seed, item0, s_hat, snew_hat, dbc, ks_xi, thr):
    """one key-switch key [(l, d)][2][k][N] for the NTT-form target snew: entry e = (l, d) in order takes item0 + 2 e (a, stream 3) and item0 + 2 e + 1
    (noise, stream 1); b = -(a s + NTT(e)) + f snew with f = 2^(dbc d) in limb l only - under ks_xi (q / q_l mod q_j) 2^(dbc d), again zero unless j = l"""
    n, qs = o.n, o.q
    entries = [(l, d) for l in range(len(qs)) for d in range(digit_counts(qs, dbc)[l])]
    Q = 1
    for q in qs:
        Q *= q
    noise = sample_noise_items(key, seed, ST_E1, [item0 + 2 * e + 1 for e in range(len(entries))], n, thr=thr)
    out = np.zeros((len(entries), 2, len(qs), n), dtype=np.uint64)
    for e, (l, d) in enumerate(entries):
        a = uniform_poly(key, seed, ST_KEY_A, item0 + 2 * e, n, qs)
        eh = ntt(o, residues(noise[e], qs))
        for j, q in enumerate(qs):
            b = negmod(addmod(mulmod(a[j], s_hat[j], q), eh[j], q), q)
            f = (pow(2, dbc * d, q) * ((Q // qs[l]) % q if ks_xi else 1)) % q if (j == l or ks_xi) else 0
            if f:
                b = addmod(b, mulmod(snew_hat[j], f, q), q)
            out[e, 0, j], out[e, 1, j] = b, a[j]
    return out.reshape(-1), item0 + 2 * len(entries)


def keygen_model(o, key, seed, galois, ks_xi=False):
    """cn_keygen(seed, galois): {"s": the ternary secret, "sk", "pk", "rlk": words as cn_get_key(3 / 2 / 0) exports them, "gk": {element: words of cn_get_key(1,
    element)}, "items": the item counter after the call}.  Items: 0 the secret (stream 0), 1 the public a (stream 3), 2 the public noise (stream 1), then two per
    relinearisation entry, then two per entry of every default Galois element in the order of default_galois_elts"""
    n, qs = o.n, o.q
    thr = noise_thresholds()
    s, _ = sample_ternary_items(key, seed, ST_TERNARY, [0], n)
    s = s[0]
    s_hat = ntt(o, residues(s, qs))
    a = uniform_poly(key, seed, ST_KEY_A, 1, n, qs)
    eh = ntt(o, residues(sample_noise(key, seed, ST_E1, 2, n, thr=thr), qs))
    b = np.stack([negmod(addmod(mulmod(a[j], s_hat[j], q), eh[j], q), q) for j, q in enumerate(qs)])
    s2 = np.stack([mulmod(s_hat[j], s_hat[j], q) for j, q in enumerate(qs)])
    rlk, item = ksk_model(o, key, seed, 3, s_hat, s2, o.dbc, ks_xi, thr)
    gk = {}
    if galois:
        for elt in default_galois_elts(n):
            gk[elt], item = ksk_model(o, key, seed, item, s_hat, ntt(o, residues(automorphism(s, elt), qs)), o.gdbc, ks_xi, thr)
    return {"s": s, "sk": s_hat.reshape(-1), "pk": np.concatenate([b.reshape(-1), a.reshape(-1)]), "rlk": rlk, "gk": gk, "items": item}


def keygen_galois_model(o, key, seed, item0, s, elts, ks_xi=False):
    """cn_keygen_galois(seed, elts) from the item counter item0 on: ({element: words}, the item counter after the call).  Entry i of the call (elements in the
    order listed, their (l, d) entries in order) takes item0 + 2 i for a and item0 + 2 i + 1 for the noise: what cn_keygen's loop gives these elements"""
    s_hat = ntt(o, residues(s, o.q))
    thr = noise_thresholds()
    gk, item = {}, item0
    for elt in elts:
        gk[elt], item = ksk_model(o, key, seed, item, s_hat, ntt(o, residues(automorphism(s, elt), o.q)), o.gdbc, ks_xi, thr)
    return gk, item


# ---------------------------------------------------------------- encryption
def _delta_m(o, plain):
    """Delta m (+ the rounding correction of the upper half) as residues [k, n]: the oracle's add_plain on a zero ciphertext"""
    kn = o.k * o.n
    if plain is None or not np.asarray(plain).any():
        return np.zeros((o.k, o.n), dtype=np.uint64)
    return o.add_plain(np.zeros(2 * kn, dtype=np.uint64), np.ascontiguousarray(plain, dtype=np.uint64))[:kn].reshape(o.k, o.n)


def encrypt_model(o, key, seed, item0, pk, plains):
    """cn_encrypt / cn_encrypt_zero_new: ciphertext i draws u (stream 0), e1 (stream 1), e2 (stream 2) at item item0 + i under the nonce `seed`;
    (c0, c1) = (INTT(pk0 NTT(u)) + e1 + Delta m, INTT(pk1 NTT(u)) + e2).  plains: one coefficient-form plaintext (or None = zero) per ciphertext -> uint64 [count, 2 k n]"""
    n, qs, k = o.n, o.q, o.k
    pk = np.asarray(pk, dtype=np.uint64).reshape(2, k, n)
    thr = noise_thresholds()
    items = [item0 + i for i in range(len(plains))]
    u, _ = sample_ternary_items(key, seed, ST_TERNARY, items, n)
    e1 = sample_noise_items(key, seed, ST_E1, items, n, thr=thr)
    e2 = sample_noise_items(key, seed, ST_E2, items, n, thr=thr)
    out = np.zeros((len(plains), 2, k, n), dtype=np.uint64)
    for i, plain in enumerate(plains):
        uh = ntt(o, residues(u[i], qs))
        for p, e in ((0, e1[i]), (1, e2[i])):
            c = intt(o, np.stack([mulmod(pk[p, j], uh[j], q) for j, q in enumerate(qs)]))
            er = residues(e, qs)
            c = np.stack([addmod(c[j], er[j], q) for j, q in enumerate(qs)])
            if p == 0:
                dm = _delta_m(o, plain)
                c = np.stack([addmod(c[j], dm[j], q) for j, q in enumerate(qs)])
            out[i, p] = c
    return out.reshape(len(plains), -1)


def encrypt_symmetric_model(o, key, seed, item0, sk, a_seed, a_nonce, a_item0, plains):
    """cn_encrypt_symmetric: ciphertext i has a = seeded_a(a_seed, a_nonce, a_item0 + i) (NTT form) and e from stream 1 at item item0 + i under the context's
    key and the nonce `seed`; (c0, c1) = (INTT(-a s) + e + Delta m, INTT(a))"""
    n, qs, k = o.n, o.q, o.k
    sk = np.asarray(sk, dtype=np.uint64).reshape(k, n)
    e = sample_noise_items(key, seed, ST_E1, [item0 + i for i in range(len(plains))], n)
    out = np.zeros((len(plains), 2, k, n), dtype=np.uint64)
    for i, plain in enumerate(plains):
        a = sm.seeded_a(a_seed, a_nonce, a_item0 + i, n, qs)
        c0 = intt(o, np.stack([negmod(mulmod(a[j], sk[j], q), q) for j, q in enumerate(qs)]))
        er, dm = residues(e[i], qs), _delta_m(o, plain)
        out[i, 0] = np.stack([addmod(addmod(c0[j], er[j], q), dm[j], q) for j, q in enumerate(qs)])
        out[i, 1] = intt(o, a)
    return out.reshape(len(plains), -1)
