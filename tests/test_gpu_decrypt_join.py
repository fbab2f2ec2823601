"""cn_decrypt_join: Decrypt + BatchEncoder.Decode + JoinSplitNumbers (EncryptedSealBfvVector.cs:381-411) of the reply ciphertexts of all plaintext-prime
contexts in one call.  Every comparison is exact: the words equal Python's integers, the doubles equal float(x) / scale as bit patterns, the arg max equals
the model on the exact integers (lowest index on ties)."""
import ctypes as C

import numpy as np
import pytest

from conftest import PARAMS

pytestmark = pytest.mark.gpu

TINY_PRIMES = (12289, 18433, 40961, 65537)                    # all == 1 (mod 2048)
CN_PRIMES = (549764251649, 549764284417)                       # the CryptoNets plaintext primes (40 bits, == 1 mod 16384)
SCALES = (1.0, float(32 * 32 * 16), 3.0)
TIES = (2 ** 53 + 1, 2 ** 53 + 3, 2 ** 60 + 2 ** 7, 2 ** 200 + 2 ** 147)


def is_prime(n):
    if n < 2 or n % 2 == 0:
        return n == 2
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if a % n == 0:
            continue
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def product(ts):
    M = 1
    for t in ts:
        M *= t
    return M


def model(ints, M, signed, scale):
    """(joined integers [count][nslots], values as bit patterns, arg max per slot) of the unsigned representatives `ints`"""
    xs = [[(x - M) if (signed and 2 * x > M) else x for x in row] for row in ints]
    vals = np.array([[float(x) / scale for x in row] for row in xs], dtype=np.float64).view(np.uint64)
    arg = [max(range(len(xs)), key=lambda c: (xs[c][s], -c)) for s in range(len(xs[0]))]
    return xs, vals, np.array(arg, dtype=np.int32)


_contexts = {}


def contexts(ring, primes):
    """one keyed context per plaintext prime on the ring (cached for the module): keys from the device client"""
    from cryptonets_amd._native import Context
    from cryptonets_amd.client import DeviceClient
    key = (ring, tuple(primes))
    if key not in _contexts:
        p = PARAMS[ring]
        out = []
        for t in primes:
            assert is_prime(t) and t % (2 * p["n"]) == 1
            g = Context(p["n"], t, q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
            DeviceClient(g, seed=0x5EED ^ t).generate_keys(with_galois=False)
            out.append(g)
        _contexts[key] = out
    return _contexts[key]


def encrypt_ints(ctxs, ints, seed=77):
    """ints [count][nvalues] (unsigned representatives) -> one handle of `count` ciphertexts per context: split mod t_i, cn_encode_batch, cn_encrypt"""
    handles = []
    for g in ctxs:
        res = np.array([[x % g.t for x in row] for row in ints], dtype=np.uint64)
        pt, ct = g.pt_alloc(len(ints)), g.ct_alloc(len(ints))
        g.encode_batch(res, pt, 0)
        g.encrypt(pt, 0, ct, 0, len(ints), seed=seed)
        g.free(pt)
        handles.append(ct)
    return handles


def edge_values(M):
    e = [0, 1, M - 1, (M - 1) // 2, (M + 1) // 2]
    for tie in TIES:
        for x in (tie - 1, tie, tie + 1):
            if x < M:
                e.append(x)
            if 2 * x <= M:
                e.append(M - x)                          # -x under the signed flag
    return e


def case1_ints(M, n, rng):
    """3 ciphertexts: edge values in the first slots (forwards in ciphertext 0, backwards in 1), random elsewhere; slot 3: ciphertexts 0 and 1 share the largest
    signed value; slot 30: ciphertexts 1 and 2 tie below (signed) / beside (unsigned) ciphertext 0"""
    ints = [[int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % M for _ in range(n)] for _ in range(3)]
    e = edge_values(M)
    ints[0][:len(e)] = e
    ints[1][:len(e)] = e[::-1]
    ints[0][3] = ints[1][3] = (M - 1) // 2
    ints[2][3] = 1
    ints[0][30], ints[1][30], ints[2][30] = M - 2, 5, 5
    return ints


_case1 = {}


def case1(P):
    if P not in _case1:
        ctxs = contexts("tiny", TINY_PRIMES[:P])
        M = product(TINY_PRIMES[:P])
        ints = case1_ints(M, PARAMS["tiny"]["n"], np.random.default_rng(100 + P))
        _case1[P] = (ctxs, M, ints, encrypt_ints(ctxs, ints))
    return _case1[P]


def check(ctxs, handles, firsts, ints, M, nslots, signed, coeff0=False, scales=SCALES):
    from cryptonets_amd import _native
    count = len(ints)
    cut = [row[:nslots] for row in ints]
    for scale in scales:
        r = _native.decrypt_join(ctxs, handles, firsts, count, nslots, signed=signed, scale=scale, coeff0=coeff0, words=True, argmax=True)
        xs, vals, arg = model(cut, M, signed, scale)
        assert r.words.shape == (count, nslots, (M.bit_length() + 1 + 63) // 64) == (count, nslots, _native.join_words(ctxs))
        assert r.ints() == xs
        assert np.array_equal(r.values.view(np.uint64), vals)
        assert np.array_equal(r.argmax, arg)


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("nslots", [1024, 5])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_dense_join_equals_python_integers(P, nslots, signed):
    ctxs, M, ints, handles = case1(P)
    check(ctxs, handles, None, ints, M, nslots, signed)
    # only one of the three outputs, and a first index: ciphertexts 1 and 2
    from cryptonets_amd import _native
    r = _native.decrypt_join(ctxs, handles, [1] * P, 2, nslots, signed=signed, scale=3.0)
    assert r.words is None and r.argmax is None
    assert np.array_equal(r.values.view(np.uint64), model([row[:nslots] for row in ints[1:]], M, signed, 3.0)[1])


def test_coeff0_join_of_constant_plaintexts():
    """the wrapper's sparse format: coefficient 0 of each of 7 plaintexts, no transform (the other coefficients are not read)"""
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    M, n = product(TINY_PRIMES[:2]), 1024
    rng = np.random.default_rng(5)
    ints = [[x] for x in [0, 1, M - 1, (M - 1) // 2, (M + 1) // 2, int(rng.integers(0, M)), int(rng.integers(0, M))]]
    handles = []
    for g in ctxs:
        polys = rng.integers(0, g.t, size=(7, n), dtype=np.uint64)
        polys[:, 0] = [row[0] % g.t for row in ints]
        pt, ct = g.pt_alloc(7), g.ct_alloc(9)
        g.pt_upload(pt, 0, polys)
        g.encrypt(pt, 0, ct, 2, 7, seed=9)
        g.free(pt)
        handles.append(ct)
    for signed in (True, False):
        check(ctxs, handles, [2, 2], ints, M, 1, signed, coeff0=True)
    for g, h in zip(ctxs, handles):
        g.free(h)


def test_rounding_ties_at_the_cryptonets_primes():
    """ring c3 (N = 8192), the two 40-bit plaintext primes: |x| reaches 2^79, ties of the 53-bit mantissa and both neighbours in slots 0-7"""
    ctxs = contexts("c3", CN_PRIMES)
    M, n = product(CN_PRIMES), 8192
    rng = np.random.default_rng(8)
    ints = [[int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) % M for _ in range(n)] for _ in range(2)]
    t0, t1, t2 = TIES[:3]
    ints[0][:8] = [t0, t0 - 1, t0 + 1, t1, t2, t2 - 1, t2 + 1, M - t2]
    ints[1][:8] = [M - t0, M - t0 + 1, M - t0 - 1, M - t1, (M - 1) // 2, (M + 1) // 2, M - t2 - 1, M - t2 + 1]
    handles = encrypt_ints(ctxs, ints)
    for signed in (True, False):
        check(ctxs, handles, None, ints, M, n, signed, scales=(float(32 * 32 * 16), 3.0))
    for g, h in zip(ctxs, handles):
        g.free(h)


def test_size3_operands():
    """cn_multiply leaves size-3 ciphertexts: their join is the product of the integers mod M"""
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    M, n = product(TINY_PRIMES[:2]), 1024
    rng = np.random.default_rng(4)
    a = [[int(x) for x in rng.integers(0, M, size=n)]]
    b = [[int(x) for x in rng.integers(0, M, size=n)]]
    ha, hb = encrypt_ints(ctxs, a, seed=1), encrypt_ints(ctxs, b, seed=2)
    prods = []
    for g, x, y in zip(ctxs, ha, hb):
        h3 = g.ct_alloc(1, 3)
        g.multiply(x, 0, y, 0, h3, 0, 1)
        prods.append(h3)
    check(ctxs, prods, None, [[x * y % M for x, y in zip(a[0], b[0])]], M, n, True, scales=(3.0,))
    for g, hs in zip(ctxs, zip(ha, hb, prods)):
        for h in hs:
            g.free(h)


def test_level_contexts_join_the_same_words():
    """the case-1 ciphertexts switched down to two limbs (cn_mod_switch): the level contexts hold a slice of the secret key, the words are those of the top level"""
    from cryptonets_amd import _native
    ctxs, M, ints, handles = case1(2)
    top = _native.decrypt_join(ctxs, handles, None, 3, 1024, signed=True, words=True, values=False)
    levels, low = [g.level(2) for g in ctxs], []
    for g, l, h in zip(ctxs, levels, handles):
        out = l.ct_alloc(3)
        g.mod_switch(h, 0, 3, l, out, 0)
        low.append(out)
    r = _native.decrypt_join(levels, low, None, 3, 1024, signed=True, words=True, values=False)
    assert np.array_equal(r.words, top.words)
    check(levels, low, None, ints, M, 1024, True, scales=(1.0,))
    for l, h in zip(levels, low):
        l.free(h)


def test_deferred_work_is_submitted_first():
    """"defer" = 1 with a queued cn_add in front: the join sees the sum"""
    ctxs, M, ints, handles = case1(2)
    outs = []
    for g, h in zip(ctxs, handles):
        out = g.ct_alloc(1)
        g.set_option("defer", 1)
        g.add(h, 0, h, 2, out, 0, 1)
        outs.append(out)
    try:
        check(ctxs, outs, None, [[(x + y) % M for x, y in zip(ints[0], ints[2])]], M, 1024, True, scales=(1.0,))
    finally:
        for g, h in zip(ctxs, outs):
            g.set_option("defer", 0)
            g.free(h)


def raw_call(ctxs, handles, firsts, count, nslots, flags, outs=(True, True, True), W=1, P=None):
    """cn_decrypt_join on pre-filled output arrays: (return code, are all of them untouched)"""
    from cryptonets_amd import _native
    L = _native.lib()
    P = len(ctxs) if P is None else P
    arr = (C.c_void_p * max(1, len(ctxs)))(*[g._h for g in ctxs])
    hs = (C.c_uint64 * max(1, len(handles)))(*handles)
    fs = None if firsts is None else (C.c_uint32 * len(firsts))(*firsts)
    room = max(1, count) * max(1, min(nslots, 1 << 14))
    v = np.full(room, -7.25, dtype=np.float64)
    w = np.full(room * 4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    a = np.full(max(1, min(nslots, 1 << 14)), -99, dtype=np.int32)
    rc = L.cn_decrypt_join(arr, P, hs, fs, count, nslots, flags, 1.0,
                           v.ctypes.data_as(C.POINTER(C.c_double)) if outs[0] else None, w.ctypes.data_as(C.POINTER(C.c_uint64)) if outs[1] else None,
                           a.ctypes.data_as(C.POINTER(C.c_int32)) if outs[2] else None)
    untouched = bool(np.all(v == -7.25) and np.all(w == 0xA5A5A5A5A5A5A5A5) and np.all(a == -99))
    return rc, untouched


def test_refusals_write_nothing():
    from cryptonets_amd._native import Context
    ctxs, M, ints, handles = case1(2)
    g0, g1 = ctxs
    h0, h1 = handles
    ARG, NOKEY = -1, -3
    assert raw_call(ctxs, handles, None, 3, 5, 1) == (0, False)                                 # the call itself is fine
    assert raw_call([], [], None, 3, 5, 1, P=0) == (ARG, True)                                  # P = 0
    assert raw_call([g0, g1] * 5, [h0, h1] * 5, None, 3, 5, 1, P=9) == (ARG, True)              # P > 8
    assert raw_call([g0, g0], [h0, h0], None, 3, 5, 1) == (ARG, True)                           # equal moduli (the same context twice)
    q = PARAMS["tiny"]["q"]
    twin = Context(1024, 12289, q=q)
    twin.keygen(3, galois=False)
    ht = twin.ct_alloc(3)
    assert raw_call([g0, twin], [h0, ht], None, 3, 5, 1) == (ARG, True)                         # equal moduli (two contexts)
    wide = Context(2048, 12289, q=q)                                                            # another N (q_j, t == 1 mod 4096 as well)
    wide.keygen(3, galois=False)
    hw = wide.ct_alloc(3)
    assert raw_call([g1, wide], [h1, hw], None, 3, 5, 1) == (ARG, True)
    assert raw_call(ctxs, handles, None, 3, 0, 1) == (ARG, True)                                # nslots = 0
    assert raw_call(ctxs, handles, None, 3, 1025, 1) == (ARG, True)                             # nslots > N
    assert raw_call(ctxs, handles, None, 3, 2, 1 | 2) == (ARG, True)                            # CN_JOIN_COEFF0 with nslots != 1
    t_plain = next(t for t in range(12291, 20000, 2) if is_prime(t) and t % 2048 != 1)
    flat = Context(1024, t_plain, q=q)                                                          # a prime plain modulus without batching
    flat.keygen(3, galois=False)
    hf = flat.ct_alloc(3)
    assert raw_call([g0, flat], [h0, hf], None, 3, 5, 1) == (ARG, True)                         # the dense form without batching
    assert raw_call(ctxs, handles, None, 3, 5, 1, outs=(False, False, False)) == (ARG, True)    # no output
    assert raw_call(ctxs, handles, [0, 1], 3, 5, 1) == (ARG, True)                              # range outside its handle
    assert raw_call(ctxs, [h0, 0xDEAD], None, 3, 5, 1) == (ARG, True)                           # not a handle
    bare = Context(1024, 40961, q=q)                                                            # no secret key
    hb = bare.ct_alloc(3)
    assert raw_call([g0, bare], [h0, hb], None, 3, 5, 1) == (NOKEY, True)
    g1.graph_begin()                                                                            # a recording in progress on one of the contexts
    try:
        assert raw_call(ctxs, handles, None, 3, 5, 1) == (ARG, True)
        g1.add(h1, 0, h1, 0, h1, 0)
    finally:
        graph = g1.graph_end()
    g1.free(graph)
    assert raw_call(ctxs, handles, None, 0, 5, 1) == (0, True)                                  # count = 0
    for g in (twin, wide, flat, bare):
        g.close()
    _case1.pop(2)                                                                               # (ciphertext 0 of prime 1 was doubled while recording)
    for g, h in zip(ctxs, handles):
        g.free(h)


class Calls:
    """counts the per-prime steps of the present path on a set of contexts: a thin wrapper around the context methods"""
    NAMES = ("decrypt", "pt_download", "pt_upload", "decode_batch", "ct_download")

    def __init__(self, ctxs):
        self.ctxs, self.n = ctxs, dict.fromkeys(self.NAMES, 0)
        for g in ctxs:
            for name in self.NAMES:
                setattr(g, name, self._wrap(name, getattr(g, name)))

    def _wrap(self, name, fn):
        def call(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return call

    def reset(self):
        launches = sum(g.stats()["kernel_launches"] for g in self.ctxs)
        self.n = dict.fromkeys(self.NAMES, 0)
        return launches

    def undo(self):
        for g in self.ctxs:
            for name in self.NAMES:
                delattr(g, name)


def test_wrapper_takes_the_device_path_and_agrees_with_the_present_one(monkeypatch):
    from cryptonets_amd import hewrapper as hw
    from cryptonets_amd._native import Context
    from cryptonets_amd.client import DeviceClient
    p = PARAMS["tiny"]

    def context_factory(n, t, q, dbc, gdbc):
        return Context(n, t, q=q, dbc=dbc, gdbc=gdbc, device=0)
    context_factory.default_coeff_modulus = lambda n: p["q"]
    F = hw.EncryptedSealBfvFactory(primes=list(TINY_PRIMES[:2]), n=1024, context_factory=context_factory, galois=False,
                                   device_client_factory=lambda ctx, t: DeviceClient(ctx, seed=0xC0FFEE ^ t))
    env = F.AllocateComputationEnv()
    M = env.bigFactor
    rng = np.random.default_rng(12)
    dense = F.GetEncryptedVector([int(x) for x in rng.integers(-(M // 2), M // 2, size=1500)], hw.EVectorFormat.dense)       # two blocks
    dense.Scale = 48.0
    sparse = F.GetEncryptedVector([int(x) for x in rng.integers(-(M // 2), M // 2, size=6)] + [(M - 1) // 2], hw.EVectorFormat.sparse)
    sparse.Scale = 3.0
    # a 3-column matrix whose columns lie in one range of one array per prime (the batched layers' form), and one of separate vectors
    cols = [F.GetEncryptedVector([int(x) for x in rng.integers(-(M // 2), M // 2, size=700)], hw.EVectorFormat.dense) for _ in range(3)]
    for c in cols:
        c.Scale = 16.0
    loose = F.GetMatrix(cols, hw.EMatrixFormat.ColumnMajor, CopyVectors=False)
    packed_cols = []
    bufs = []
    for i, e in enumerate(env.Environments):
        b = hw._Buf(e.ctx, "ct", 3)
        e.ctx.copy_many([c.eVectors[i].encData.h for c in cols], [c.eVectors[i].encData.first for c in cols], b.h, 0)
        bufs.append(b)
    for j, c in enumerate(cols):
        atoms = [hw.AtomicSealBfvEncryptedVector._new(Scale=a.Scale, Dim=a.Dim, Format=a.Format, IsSigned=a.IsSigned, encData=bufs[i].view(j, 1)) for i, a in enumerate(c.eVectors)]
        packed_cols.append(hw.EncryptedSealBfvVector._of(atoms, c.Scale))
    packed = F.GetMatrix(packed_cols, hw.EMatrixFormat.ColumnMajor, CopyVectors=False)

    calls = Calls([e.ctx for e in env.Environments])
    results = {}
    for on in (True, False):
        monkeypatch.setattr(hw, "DEVICE_JOIN", on)
        before = calls.reset()
        results[on] = [dense.Decrypt(env), dense.DecryptFullPrecision(env), sparse.Decrypt(env), sparse.DecryptFullPrecision(env), packed.Decrypt(env), loose.Decrypt(env)]
        launches = sum(g.stats()["kernel_launches"] for g in calls.ctxs) - before
        if on:                                                     # no cn_decrypt into a plaintext handle, no per-prime download, upload or cn_decode_batch
            assert calls.n == dict.fromkeys(Calls.NAMES, 0), calls.n
            device_launches = launches
        else:
            assert calls.n["decode_batch"] > 0 and calls.n["pt_download"] > 0 and launches > device_launches
    calls.undo()
    a, b = results[True], results[False]
    for x, y in ((a[0], b[0]), (a[2], b[2]), (a[4], b[4]), (a[5], b[5])):
        assert x.dtype == y.dtype == np.float64 and x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert a[1] == b[1] and a[3] == b[3] and all(type(v) is int for v in a[1] + a[3])
    assert a[0].shape == (1500,) and len(a[1]) == 1500 and a[2].shape == (7,) and a[4].shape == (700, 3)
    assert np.array_equal(a[4], a[5])


def test_predict_equals_the_integer_model():
    """cryptonets_mnist.predict on a 1024-point ring (the coefficient modulus of the 8192-point configuration, so that the two squarings have their noise room; the
    two CryptoNets plaintext primes): the arg max per image equals the arg max of the exact integer logits"""
    import os
    from cryptonets_amd import cryptonets_mnist as cm
    from cryptonets_amd._native import Context, default_coeff_modulus
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cryptonets_weights.npz"))
    layers = cm.layer_tables(w["Weights_0"], w["Weights_1"], w["Biases_2"], w["Weights_3"], w["Biases_3"])
    n = 1024
    images = cm.synthetic_images(n, seed=3)
    x_int = np.rint(images * cm.NORMALIZATION * cm.INPUT_SCALE).astype(np.int64)
    channels, per_prime = [], []
    for p in cm.PLAIN_PRIMES:
        g = Context(n, p, q=default_coeff_modulus(cm.N), dbc=10, gdbc=20, device=0)
        g.keygen(0x51CE ^ p, galois=False)
        ch = cm.CryptoNetsChannel(g, layers, cm.constant_plaintext(n))
        ph = g.pt_alloc(784)
        g.encode_batch(np.mod(x_int.T, p).astype(np.uint64), ph, 0)
        g.encrypt(ph, 0, ch.h_in, 0, 784, seed=123)
        g.free(ph)
        ch.forward()
        channels.append(ch)
        per_prime.append(cm.model_mod_p_dense(x_int, layers, p))
    got = cm.predict(channels)
    p0, p1 = cm.PLAIN_PRIMES
    M, inv = p0 * p1, pow(p0, -1, p1)
    want = []
    for s in range(n):
        logits = []
        for c in range(10):
            r0, r1 = int(per_prime[0][s][c]), int(per_prime[1][s][c])
            logits.append(r0 + p0 * ((r1 - r0) * inv % p1))
        logits = cm.centred(logits, M)
        if s % 341 == 0:
            assert logits == cm.int_logits(w, images[s])          # the joined residues are the exact integer logits
        want.append(max(range(10), key=lambda c: (logits[c], -c)))
    assert got.dtype == np.int32 and got.shape == (n,) and got.tolist() == want
    assert np.array_equal(cm.predict(channels, nslots=7), got[:7])
    for ch in channels:
        ch.g.close()
