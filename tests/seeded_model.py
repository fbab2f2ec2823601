"""Restatement of the device sampler's uniform draw (cn_dev_common.hip.h: chacha20_block, rng_counter, sample_uniform8) for the seeded symmetric
ciphertexts of include/cnhip.h: the public polynomial `a` of item i, limb j is sample_uniform8(a_seed, a_nonce, STREAM_A, a_item0 + i, j (N/8) + b, q_j)
for b = 0 .. N/8 - 1.  Vectorised over blocks with numpy (uint32 lanes), nothing else: no library code is imported."""
import numpy as np

STREAM_A = 4
M32 = np.uint32(0xffffffff)


def _rotl(x, r):
    return ((x << np.uint32(r)) | (x >> np.uint32(32 - r))).astype(np.uint32)


def _qr(w, a, b, c, d):
    w[a] = w[a] + w[b]; w[d] = _rotl(w[d] ^ w[a], 16)
    w[c] = w[c] + w[d]; w[b] = _rotl(w[b] ^ w[c], 12)
    w[a] = w[a] + w[b]; w[d] = _rotl(w[d] ^ w[a], 8)
    w[c] = w[c] + w[d]; w[b] = _rotl(w[b] ^ w[c], 7)


def key_words(key32):
    key32 = bytes(key32)
    assert len(key32) == 32
    return [int.from_bytes(key32[4 * i:4 * i + 4], "little") for i in range(8)]


def chacha20_block(key32, counter, nonce):
    """RFC 7539 block function; state words 12-13 = the 64-bit counter(s), 14-15 = the 64-bit nonce.  counter: int or array of ints -> uint32 [B, 16]"""
    counter = np.atleast_1d(np.asarray(counter, dtype=np.uint64))
    B = counter.shape[0]
    const = [0x61707865, 0x3320646e, 0x79622d32, 0x6b206574]
    x = [np.full(B, v, dtype=np.uint32) for v in const + key_words(key32)]
    x.append((counter & np.uint64(0xffffffff)).astype(np.uint32))
    x.append((counter >> np.uint64(32)).astype(np.uint32))
    x.append(np.full(B, nonce & 0xffffffff, dtype=np.uint32))
    x.append(np.full(B, (nonce >> 32) & 0xffffffff, dtype=np.uint32))
    w = [v.copy() for v in x]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(w, 0, 4, 8, 12); _qr(w, 1, 5, 9, 13); _qr(w, 2, 6, 10, 14); _qr(w, 3, 7, 11, 15)
            _qr(w, 0, 5, 10, 15); _qr(w, 1, 6, 11, 12); _qr(w, 2, 7, 8, 13); _qr(w, 3, 4, 9, 14)
        return np.stack([a + b for a, b in zip(w, x)], axis=1)


def rng_counter(item, stream, trial, blk):
    """item (40 bits) | stream (4) | trial (4) | block index inside the polynomial (16)"""
    return (int(item) << 24) | ((stream & 15) << 20) | ((trial & 15) << 16) | (blk & 0xffff)


def sample_uniform8(key32, nonce, stream, item, blks, q):
    """8 residues mod q per block index in `blks` -> (uint64 [B, 8], number of rejected words)"""
    blks = np.atleast_1d(np.asarray(blks, dtype=np.int64))
    lim = (1 << 64) - 1 - ((1 << 64) - 1) % q - 1
    out = np.zeros((blks.shape[0], 8), dtype=np.uint64)
    pending = np.ones((blks.shape[0], 8), dtype=bool)
    rejected, trial = 0, 0
    while pending.any():
        rows = np.nonzero(pending.any(axis=1))[0]
        ctr = np.array([rng_counter(item, stream, trial, int(b)) for b in blks[rows]], dtype=np.uint64)
        w = chacha20_block(key32, ctr, nonce).astype(np.uint64)
        v = (w[:, 0::2] << np.uint64(32)) | w[:, 1::2]
        ok = pending[rows] & (v <= np.uint64(lim))
        rejected += int((pending[rows] & ~ok).sum())
        sub = out[rows]
        sub[ok] = v[ok] % np.uint64(q)
        out[rows] = sub
        pending[rows] &= ~ok
        trial += 1
        assert trial < 16, "more redraws than the counter has trial bits"
    return out, rejected


def seeded_a(a_seed, a_nonce, item, n, qs):
    """the NTT-form `a` of one item: uint64 [k, n]"""
    bpl = n // 8
    return np.stack([sample_uniform8(a_seed, a_nonce, STREAM_A, item, j * bpl + np.arange(bpl), q)[0].reshape(n) for j, q in enumerate(qs)])
