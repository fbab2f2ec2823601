"""cn_split_encode / cn_split_encrypt: SplitBigNumbers + BatchEncoder.Encode [+ Encryptor.Encrypt] of the request of all plaintext-prime contexts in one call.
Every comparison is exact: the plaintext words equal cn_encode_batch of the residues Python's integers give, the ciphertext words equal cn_encode_batch +
cn_encrypt on a context in the same sampler state, the round trip through cn_decrypt_join returns the integers that went in."""
import ctypes as C

import numpy as np
import pytest

from conftest import PARAMS

pytestmark = pytest.mark.gpu

TINY_PRIMES = (12289, 18433, 40961, 65537)                    # all == 1 (mod 2048)
CN_PRIMES = (549764251649, 549764284417)                       # the CryptoNets plaintext primes (40 bits, == 1 mod 16384)
SCALE = 16.0
ARG, NOKEY, ZERO = -1, -3, -4
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

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
            assert t % (2 * p["n"]) == 1
            g = Context(p["n"], t, q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
            DeviceClient(g, seed=0x5EED ^ t).generate_keys(with_galois=False)
            out.append(g)
        _contexts[key] = out
    return _contexts[key]


def make_values(kind, count, nvalues, rng):
    """[count][nvalues]: doubles with quarters (ties after the scale 16 included) of either sign, or int64 over the whole range with the extremes in front"""
    if kind == "f64":
        v = rng.integers(-2 ** 24, 2 ** 24, size=(count, nvalues)).astype(np.float64) / 64.0
        v.flat[:3] = [0.5 / SCALE, -1.5 / SCALE, 2.5 / SCALE][:v.size]
        return v
    v = rng.integers(I64_MIN, I64_MAX, size=(count, nvalues), dtype=np.int64, endpoint=True)
    v.flat[:4] = [I64_MIN, I64_MAX, -1, 0][:v.size]
    return v


def integers_of(values, scale=SCALE):
    """the integers w the call must split, as Python ints [count][nvalues]"""
    if values.dtype == np.int64:
        return [[int(x) for x in row] for row in values]
    return [[int(round(float(x) * scale)) for x in row] for row in values]         # round(): nearest, ties to even; x * scale: one double multiply


def laid_out(values, layout):
    """the same [count][nvalues] elements behind other strides: "slot" = stride_slot 1 (rows 3 elements longer than nvalues), "ct" = stride_ct 1 (the image-major
    request: rows of count + 3 elements, no multiple of the kernel's tile)"""
    count, nvalues = values.shape
    if layout == "slot":
        base = np.full((count, nvalues + 3), 7, dtype=values.dtype)
        base[:, :nvalues] = values
        v = base[:, :nvalues]
        assert v.strides == (8 * (nvalues + 3), 8)
    else:
        base = np.full((nvalues, count + 3), 7, dtype=values.dtype)
        base[:, :count] = values.T
        v = base[:, :count].T
        assert v.strides == (8, 8 * (count + 3))
    assert np.array_equal(v, values)
    return v


def expected_plaintexts(ctxs, ints):
    """per context: the words of cn_encode_batch of the residues Python's integers give"""
    out = []
    for g in ctxs:
        res = np.array([[w % g.t for w in row] for row in ints], dtype=np.uint64)
        pt = g.pt_alloc(len(ints))
        g.encode_batch(res, pt, 0)
        out.append(g.pt_download(pt, 0, len(ints)))
        g.free(pt)
    return out


def check_encode(ctxs, values, layout, coeff0=False, first=1):
    from cryptonets_amd import _native
    count = values.shape[0]
    ints = integers_of(values)
    pts = [g.pt_alloc(count + 2) for g in ctxs]
    try:
        zero = _native.split_encode(ctxs, laid_out(values, layout), pts, [first] * len(ctxs), scale=SCALE, coeff0=coeff0)
        if coeff0:
            want = []
            for g in ctxs:
                w = np.zeros((count, g.n), dtype=np.uint64)
                w[:, 0] = [row[0] % g.t for row in ints]
                want.append(w)
        else:
            want = expected_plaintexts(ctxs, ints)
        for i, g in enumerate(ctxs):
            assert np.array_equal(g.pt_download(pts[i], first, count), want[i]), (i, layout)
            assert zero[i].tolist() == [all(w % g.t == 0 for w in row) for row in ints]
    finally:
        for g, h in zip(ctxs, pts):
            g.free(h)


@pytest.mark.parametrize("kind", ["f64", "i64"])
@pytest.mark.parametrize("layout", ["slot", "ct"])
@pytest.mark.parametrize("nvalues", [1, 5, 1023, 1024])
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("P", [1, 2, 4])
def test_plaintext_words_equal_encode_batch(P, count, nvalues, layout, kind):
    ctxs = contexts("tiny", TINY_PRIMES[:P])
    rng = np.random.default_rng(1000 * P + 100 * count + nvalues)
    check_encode(ctxs, make_values(kind, count, nvalues, rng), layout)


@pytest.mark.parametrize("layout", ["slot", "ct"])
def test_more_than_one_tile_of_plaintexts(layout):
    """35 plaintexts: three tiles of 16 along the plaintexts, the last one partial, 100 slots: two tiles of 64 along the slots"""
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    check_encode(ctxs, make_values("f64", 35, 100, np.random.default_rng(35)), layout)


@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_coeff0_writes_constant_plaintexts(kind):
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    v = make_values(kind, 7, 1, np.random.default_rng(7))
    for layout in ("slot", "ct"):
        check_encode(ctxs, v, layout, coeff0=True)


def test_zero_flags_are_exact_and_mul_plain_refuses_by_them():
    """row 0: all zero; row 1: multiples of t_0 alone (zero under prime 0 only); row 2: anything"""
    from cryptonets_amd import _native
    from cryptonets_amd._native import CnError
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    g0, g1 = ctxs
    rng = np.random.default_rng(3)
    v = rng.integers(-1000, 1000, size=(3, 40)).astype(np.int64)
    v[0] = 0
    v[1] = g0.t * rng.integers(1, 5, size=40)                    # (below t_1: not a multiple of it)
    pts = [g.pt_alloc(3) for g in ctxs]
    zero = _native.split_encode(ctxs, v, pts, None)
    assert zero.tolist() == [[True, True, False], [True, False, False]]
    for i, g in enumerate(ctxs):
        assert np.array_equal(g.pt_download(pts[i], 0, 3).any(axis=1), ~zero[i])
        ct, out = g.ct_alloc(1), g.ct_alloc(1)
        g.encrypt(0, 0, ct, 0, 1, seed=5)
        for row in range(3):
            if zero[i][row]:
                with pytest.raises(CnError) as e:
                    g.mul_plain(ct, 0, pts[i], row, out, 0)
                assert e.value.code == ZERO
            else:
                g.mul_plain(ct, 0, pts[i], row, out, 0)
        for h in (ct, out, pts[i]):
            g.free(h)
    # the f64 kind: -0.0 and values that round to zero are zero
    pts = [g.pt_alloc(1) for g in ctxs]
    assert _native.split_encode(ctxs, np.array([[-0.0, 0.01, -0.03]]), pts, None, scale=SCALE).tolist() == [[True], [True]]
    for g, h in zip(ctxs, pts):
        g.free(h)


def test_cryptonets_primes_on_ring_c3():
    ctxs = contexts("c3", CN_PRIMES)
    rng = np.random.default_rng(83)
    for kind in ("f64", "i64"):
        for layout in ("slot", "ct"):
            check_encode(ctxs, make_values(kind, 2, 8192 if layout == "slot" else 777, rng), layout)
    check_encode(ctxs, make_values("i64", 2, 1, rng), "slot", coeff0=True)


def test_ring_n16k7():
    ctxs = contexts("n16k7", (PARAMS["n16k7"]["t"],))
    rng = np.random.default_rng(16)
    check_encode(ctxs, make_values("f64", 1, 16384, rng), "slot", first=0)
    check_encode(ctxs, make_values("i64", 2, 1, rng), "slot", coeff0=True)


def test_ciphertext_words_equal_encode_batch_and_encrypt():
    """two fresh contexts with identical parameters and keys (the item counters must agree): cn_split_encrypt on one, cn_encode_batch + cn_encrypt on the other"""
    from cryptonets_amd import _native
    from cryptonets_amd._native import Context
    from cryptonets_amd.client import DeviceClient
    p = PARAMS["tiny"]
    pair = []
    for _ in range(2):
        g = Context(p["n"], 18433, q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
        DeviceClient(g, seed=0xABCD).generate_keys(with_galois=False)
        pair.append(g)
    a, b = pair
    rng = np.random.default_rng(21)
    for call, (count, nvalues, nonce) in enumerate([(3, 700, 11), (2, 1024, 12)]):
        v = make_values("f64", count, nvalues, rng)
        ha, hb, pt = a.ct_alloc(count + 1), b.ct_alloc(count + 1), b.pt_alloc(count)
        _native.split_encrypt([a], laid_out(v, "ct"), [ha], [1], [nonce], scale=SCALE)
        b.encode_batch(np.array([[w % b.t for w in row] for row in integers_of(v)], dtype=np.uint64), pt, 0)
        b.encrypt(pt, 0, hb, 1, count, seed=nonce)
        assert np.array_equal(a.ct_download(ha, 1, count), b.ct_download(hb, 1, count)), call          # the second call: the counters advanced equally
        a.free(ha), b.free(hb), b.free(pt)
    for g in pair:
        g.close()


@pytest.mark.parametrize("ring,primes", [("tiny", TINY_PRIMES[:2]), ("tiny", TINY_PRIMES), ("c3", CN_PRIMES)])
def test_round_trip_through_decrypt_join(ring, primes):
    from cryptonets_amd import _native
    ctxs = contexts(ring, primes)
    n, P = PARAMS[ring]["n"], len(primes)
    M = 1
    for t in primes:
        M *= t
    half = min((M - 1) // 2, 2 ** 62 - 1)
    rng = np.random.default_rng(P)
    v = rng.integers(-half, half, size=(2, n), dtype=np.int64, endpoint=True)
    v[0, :4] = [-half, half, -1, 0]
    cts = [g.ct_alloc(2) for g in ctxs]
    _native.split_encrypt(ctxs, v, cts, None, [31 + i for i in range(P)])
    r = _native.decrypt_join(ctxs, cts, None, 2, n, signed=True, words=True, values=False)
    assert r.ints() == [[int(x) for x in row] for row in v]
    # the f64 kind, image-major
    f = rng.integers(-2 ** 20, 2 ** 20, size=(2, 50)).astype(np.float64) / 32.0
    _native.split_encrypt(ctxs, laid_out(f, "ct"), cts, None, [41 + i for i in range(P)], scale=SCALE)
    r = _native.decrypt_join(ctxs, cts, None, 2, 50, signed=True, words=True, values=False)
    assert r.ints() == integers_of(f)
    for g, h in zip(ctxs, cts):
        g.free(h)


def raw(fn, ctxs, handles, count, nvalues, flags=0, firsts=None, values=True, seeds=True, P=None, strides=None):
    """the C entry point itself: its return code"""
    from cryptonets_amd import _native
    L = _native.lib()
    P = len(ctxs) if P is None else P
    arr = (C.c_void_p * max(1, len(ctxs)))(*[g._h for g in ctxs])
    hs = (C.c_uint64 * max(1, len(handles)))(*handles) if handles is not None else None
    fs = None if firsts is None else (C.c_uint32 * len(firsts))(*firsts)
    v = np.ones((max(1, count), max(1, min(nvalues, 1 << 14))), dtype=np.float64)
    sc, ss = strides or (v.shape[1], 1)
    vp = C.c_void_p(v.ctypes.data) if values else None
    if fn == "encode":
        return L.cn_split_encode(arr, P, vp, sc, ss, count, nvalues, flags, 1.0, hs, fs, None)
    sd = (C.c_uint64 * 8)(*range(1, 9)) if seeds else None
    return L.cn_split_encrypt(arr, P, vp, sc, ss, count, nvalues, flags, 1.0, hs, fs, sd)


def test_refusals_leave_the_handles_alone():
    from cryptonets_amd import _native
    from cryptonets_amd._native import Context
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    g0, g1 = ctxs
    q = PARAMS["tiny"]["q"]
    wide = Context(2048, 12289, q=q)                                                            # another N
    wide.keygen(3, galois=False)
    t_plain = next(t for t in range(12291, 20000, 2) if all(t % d for d in range(3, 142, 2)) and t % 2048 != 1)
    flat = Context(1024, t_plain, q=q)                                                          # a plain modulus without batching
    flat.keygen(3, galois=False)
    bare = Context(1024, 40961, q=q)                                                            # no public key
    small = Context(512, 12289, q=q)                                                            # below cn_encrypt's limit
    everyone = [g0, g1, wide, flat, bare, small]
    pts = {g: g.pt_alloc(3) for g in everyone}
    cts = {g: g.ct_alloc(3) for g in everyone}
    c3 = g1.ct_alloc(3, 3)
    live = [g.live_handles() for g in everyone]
    for fn, hs in (("encode", pts), ("encrypt", cts)):
        ok = [hs[g0], hs[g1]]
        assert raw(fn, ctxs, ok, 3, 5) == 0                                                     # the call itself is fine
        assert raw(fn, [], [], 3, 5, P=0) == ARG                                                # P = 0
        assert raw(fn, [g0, g1] * 5, ok * 5, 3, 5, P=9) == ARG                                  # P > 8
        assert raw(fn, [g0, wide], [hs[g0], hs[wide]], 3, 5) == ARG                             # another N
        assert raw(fn, ctxs, ok, 3, 1025) == ARG                                                # nvalues > N
        assert raw(fn, ctxs, ok, 3, 0) == ARG                                                   # nvalues = 0 in the dense form
        assert raw(fn, ctxs, ok, 3, 2, flags=2) == ARG                                          # CN_SPLIT_COEFF0 with nvalues != 1
        assert raw(fn, [g0, flat], [hs[g0], hs[flat]], 3, 5) == ARG                             # the dense form without batching
        assert raw(fn, [g0, flat], [hs[g0], hs[flat]], 3, 1, flags=2) == 0                      # ... but the constant form is fine there
        assert raw(fn, ctxs, ok, 3, 5, values=False) == ARG                                     # null values
        assert raw(fn, ctxs, None, 3, 5) == ARG                                                 # null handles
        assert raw(fn, ctxs, ok, 3, 5, firsts=[0, 1]) == ARG                                    # range outside its handle
        assert raw(fn, ctxs, [hs[g0], 0xDEAD], 3, 5) == ARG                                     # not a handle
        assert raw(fn, ctxs, [hs[g0], pts[g1] if fn == "encrypt" else cts[g1]], 3, 5) == ARG    # a handle of the other kind
        assert raw(fn, ctxs, ok, 3, 5, flags=4) == ARG                                          # unknown flag
        g1.graph_begin()                                                                        # a recording in progress on one of the contexts
        try:
            assert raw(fn, ctxs, ok, 3, 5) == ARG
            g1.add(cts[g1], 0, cts[g1], 0, cts[g1], 0)
        finally:
            graph = g1.graph_end()
        g1.free(graph)
        assert raw(fn, ctxs, ok, 0, 5) == 0                                                     # count = 0
    assert raw("encrypt", ctxs, [cts[g0], cts[g1]], 3, 5, seeds=False) == ARG                   # null seeds
    assert raw("encrypt", ctxs, [cts[g0], c3], 3, 5) == ARG                                     # a ciphertext array of size 3
    assert raw("encrypt", [small], [cts[small]], 3, 5) == ARG                                   # N < 1024
    assert raw("encode", [small], [pts[small]], 3, 5) == 0                                      # (the encoding alone runs there)
    assert raw("encrypt", [g0, bare], [cts[g0], cts[bare]], 3, 5) == NOKEY
    assert [g.live_handles() for g in everyone] == live
    # a value out of range is found on the device; the next valid call on the same contexts is correct
    for bad in (2.0 ** 62, float("nan"), float("-inf")):
        v = np.ones((3, 5))
        v[2, 4] = bad
        with pytest.raises(_native.CnError) as e:
            _native.split_encode(ctxs, v, [pts[g0], pts[g1]], None)
        assert e.value.code == ARG and "does not fit" in str(e.value)
        with pytest.raises(_native.CnError) as e:
            _native.split_encrypt(ctxs, v, [cts[g0], cts[g1]], None, [1, 2])
        assert e.value.code == ARG
    assert [g.live_handles() for g in everyone] == live
    check_encode(ctxs, make_values("f64", 3, 5, np.random.default_rng(0)), "ct")
    g1.free(c3)
    for g in everyone:
        g.free(pts[g]), g.free(cts[g])
    for g in (wide, flat, bare, small):
        g.close()


def test_more_than_one_pass():
    """16384 + 5 plaintexts on the 1024-point ring: a second pass of 5 (2^24 / N plaintexts per pass) - rows, flags and staged values continue where the first ended"""
    from cryptonets_amd import _native
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    count = 16384 + 5
    rows = [0, 1, 16383, 16384, 16385, count - 1]
    c = np.arange(count, dtype=np.int64)
    pts = [g.pt_alloc(count) for g in ctxs]
    # the constant form: every third value zero, the others -c
    v = np.where(c % 3 == 0, 0, -c).reshape(count, 1)
    zero = _native.split_encode(ctxs, v, pts, None, coeff0=True)
    for i, g in enumerate(ctxs):
        assert zero[i].tolist() == [int(x) % g.t == 0 for x in v[:, 0]]
        for r in rows:
            got = g.pt_download(pts[i], r, 1)[0]
            assert got[0] == int(v[r, 0]) % g.t and not got[1:].any()
    # the dense form, image-major, two slots
    f = np.stack([c * 0.25, -c * 0.5], axis=1)
    zero = _native.split_encode(ctxs, laid_out(f, "ct"), pts, None, scale=SCALE)
    want = expected_plaintexts(ctxs, integers_of(f[rows]))
    for i, g in enumerate(ctxs):
        assert zero[i].tolist() == [(4 * r) % g.t == 0 and (8 * r) % g.t == 0 for r in range(count)]        # (row 0, and row 12289 under that prime)
        for k, r in enumerate(rows):
            assert np.array_equal(g.pt_download(pts[i], r, 1)[0], want[i][k]), r
    for g, h in zip(ctxs, pts):
        g.free(h)


def test_level_contexts_encrypt_at_their_level():
    """cn_split_encrypt on the two-limb level contexts: cn_decrypt_join there (their slice of the secret key) returns the integers that went in"""
    from cryptonets_amd import _native
    ctxs = contexts("tiny", TINY_PRIMES[:2])
    levels = [g.level(2) for g in ctxs]
    v = np.random.default_rng(2).integers(-10 ** 8, 10 ** 8, size=(2, 1024), dtype=np.int64)
    cts = [l.ct_alloc(2) for l in levels]
    _native.split_encrypt(levels, v, cts, None, [3, 4])
    r = _native.decrypt_join(levels, cts, None, 2, 1024, signed=True, words=True, values=False)
    assert r.ints() == [[int(x) for x in row] for row in v]
    for l, h in zip(levels, cts):
        l.free(h)
