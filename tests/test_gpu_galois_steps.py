"""Galois keys for a caller's own rotation steps (include/cnhip.h: cn_keygen_galois, cn_galois_elts, cn_rotation_steps) on the MI355X.

Shapes: C2 (N = 8192, two 43-bit limbs), C4 (N = 8192, CoeffModulus128, gdbc as the reference), a two-limb set of 60-bit primes (the integer policy) and
N = 16384 with 8 limbs (dbc 60/60).  Where keys are generated the tests run under both key-switch conventions ("ks_xi" 0 and 1)."""
import io

import numpy as np
import pytest

from conftest import PARAMS

pytestmark = pytest.mark.gpu

SEED = 77


def _is_prime(p):
    if p < 2:
        return False
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if p % a == 0:
            return p == a
    d, s = p - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, p)
        if x in (1, p - 1):
            continue
        for _ in range(s - 1):
            x = x * x % p
            if x == p - 1:
                break
        else:
            return False
    return True


def _primes_below(bits, n, count):
    out, p = [], (1 << bits) - (1 << bits) % (2 * n) + 1
    while len(out) < count:
        p -= 2 * n
        if _is_prime(p):
            out.append(p)
    return out


SETS = dict(PARAMS)
SETS["w60"] = dict(n=4096, t=40961, q=_primes_below(60, 4096, 2), dbc=60, gdbc=60)       # 50-60-bit two-limb set: the integer (Shoup) policy
SHAPES = ["c2", "c4", "w60", "c5"]
CASES = [(s, xi) for s in SHAPES for xi in (0, 1)]
IDS = lambda c: "%s-xi%d" % c if isinstance(c, tuple) else str(c)


def _ctx(name, xi=0):
    from cryptonets_amd._native import Context
    p = SETS[name]
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    if xi:
        g.set_option("ks_xi", 1)
    return g


def _oracle(g, xi=0):
    """the CPU oracle with the device's keys (secret, public, relinearisation, every Galois key the context holds)"""
    from oracle.cno import Oracle
    o = Oracle(g.n, g.t, q=g.q, dbc=g.dbc, gdbc=g.gdbc, ks_xi=bool(xi))
    o.import_keys(g.get_key(3), g.get_key(2))
    o.import_relin_key(g.get_key(0))
    for e in g.galois_elts():
        o.import_galois_key(e, g.get_key(1, e))
    return o


def keygen_order(n):
    """the elements cn_keygen(with_galois) generates, in its order: 2N - 1, then 3^(2^i), 3^-(2^i) for i = 0 .. log2(N) - 2.  The last two coincide
    (3^(N/4) has order 2 modulo 2N): cn_keygen generates that element twice and keeps the second key."""
    m = 2 * n
    out, p3, ip3 = [m - 1], 3, pow(3, -1, m)
    for _ in range(n.bit_length() - 2):
        out += [p3, ip3]
        p3, ip3 = p3 * p3 % m, ip3 * ip3 % m
    assert out[-1] == out[-2] and len(set(out)) == len(out) - 1
    return out


def default_enumeration(g):
    """the element enumeration of the serializer before cn_galois_elts existed: the default set, asked for element by element"""
    m, n = 2 * g.n, g.n
    cand, e = {m - 1}, 3
    for _ in range(max(1, n.bit_length() - 2)):
        cand.add(e)
        cand.add(pow(e, -1, m))
        e = e * e % m
    return sorted(x for x in cand if g.has_galois_key(x))


def _steps_for(n):
    return [169, -5] + ([3 * 1024] if n >= 8192 else [])


# ---------------------------------------------------------------- 1. word identity with cn_keygen
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_keygen_galois_reproduces_cn_keygens_words(case):
    """cn_keygen(seed, 1) against cn_keygen(seed, 0) + cn_keygen_galois(seed, cn_keygen's element order): every Galois key word, the other keys and the
    sampler's item counter (a following encryption with the same nonce) are equal.  cn_keygen generates the last element of its list twice and keeps the
    second key; a list with a repeated element is refused, so the second generation is a second call - the same sampler items."""
    name, xi = case
    a, b = _ctx(name, xi), _ctx(name, xi)
    try:
        a.keygen(SEED, galois=True)
        b.keygen(SEED, galois=False)
        assert b.galois_elts() == []
        order = keygen_order(a.n)
        b.keygen_galois(SEED, order[:-1])
        b.keygen_galois(SEED, order[-1:])
        assert a.galois_elts() == b.galois_elts() == sorted(set(order))
        for which in (0, 2, 3):
            assert np.array_equal(a.get_key(which), b.get_key(which)), "key kind %d differs" % which
        for e in sorted(set(order)):
            assert np.array_equal(a.get_key(1, e), b.get_key(1, e)), "Galois key of element %d differs" % e
        pa, pb, ca, cb = a.pt_alloc(1), b.pt_alloc(1), a.ct_alloc(1), b.ct_alloc(1)
        v = (np.arange(a.n, dtype=np.uint64) * np.uint64(31)) % np.uint64(a.t)
        a.encode(v, pa, 0), b.encode(v, pb, 0)
        a.encrypt(pa, 0, ca, 0, 1, seed=5), b.encrypt(pb, 0, cb, 0, 1, seed=5)
        assert np.array_equal(a.ct_download(ca, 0, 1), b.ct_download(cb, 0, 1)), "the item counters differ after key generation"
    finally:
        a.close(), b.close()


# ---------------------------------------------------------------- 2. key validity for non-default elements
def _sigma_coeff(p, g, q):
    """x -> x^g on a coefficient-form polynomial mod q"""
    n = p.size
    i = np.arange(n, dtype=np.int64)
    raw = i * int(g)
    out = np.zeros(n, dtype=object)
    neg = ((raw // n) & 1).astype(bool)
    vals = p.astype(object)
    out[raw % n] = np.where(neg, (q - vals) % q, vals)
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_generated_keys_are_valid_key_switch_keys(case):
    """b + a s - f sigma_g(s) of every entry and limb is, in the coefficient domain, ONE small polynomial: centred coefficients within the clipped
    normal's bound 19 (6 sigma of 3.2, cn_noise_table), the same in every limb of the entry"""
    from oracle.cno import Oracle
    name, xi = case
    g = _ctx(name, xi)
    try:
        n, k, q = g.n, g.k, g.q
        g.keygen(SEED, galois=False)
        steps = _steps_for(n)
        elts = [g.galois_elt_from_step(s) for s in steps] + [2 * n - 1]
        g.keygen_galois(SEED + 1, elts)
        assert g.galois_elts() == sorted(elts)
        o = Oracle(n, g.t, q=q, dbc=g.dbc, gdbc=g.gdbc)
        s_ntt = g.get_key(3).reshape(k, n)
        s_coef = o.ntt_inv_batch(s_ntt).reshape(k, n)
        digits = [-(-qj.bit_length() // g.gdbc) for qj in q]
        Q = 1
        for qj in q:
            Q *= qj
        for elt in elts:
            key = g.get_key(1, elt).reshape(sum(digits), 2, k, n)
            e_idx = 0
            for l in range(k):
                for d in range(digits[l]):
                    b, a = key[e_idx, 0], key[e_idx, 1]
                    ref = None
                    for j in range(k):
                        qj = q[j]
                        r = (b[j].astype(object) + a[j].astype(object) * s_ntt[j].astype(object)) % qj
                        rc = o.ntt_inv(j, np.array(r, dtype=np.uint64)).astype(object)
                        if j == l:
                            f = pow(2, g.gdbc * d, qj) * ((Q // q[l]) % qj if xi else 1) % qj
                            rc = (rc - f * _sigma_coeff(s_coef[j], elt, qj)) % qj
                        cen = np.where(rc > qj // 2, rc - qj, rc)
                        assert max(abs(int(x)) for x in (cen.max(), cen.min())) <= 19, "element %d entry (%d, %d) limb %d is not a key-switch key" % (elt, l, d, j)
                        if ref is None:
                            ref = cen
                        assert np.array_equal(ref, cen), "element %d entry (%d, %d): limb %d carries another noise polynomial" % (elt, l, d, j)
                    e_idx += 1
    finally:
        g.close()


# ---------------------------------------------------------------- 3. rotation parity with the oracle under direct keys
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rotations_with_direct_keys_equal_the_oracle(case, rng):
    name, xi = case
    g = _ctx(name, xi)
    try:
        n = g.n
        g.keygen(SEED, galois=False)
        steps = _steps_for(n)
        # direct keys for the steps, and the +-2^i keys the NAF rotation by 7 (= 8 - 1) needs: a mixed cn_rotate_rows_many
        elts = [g.galois_elt_from_step(s) for s in steps + [8, -1]] + [2 * n - 1]
        g.keygen_galois(SEED + 2, elts)
        o = _oracle(g, xi)
        vals = rng.integers(0, g.t, size=(4, n), dtype=np.uint64)
        cts = np.stack([o.encrypt(o.encode(v)) for v in vals])
        h, out = g.ct_alloc(4), g.ct_alloc(4)
        g.ct_upload(h, 0, cts)
        half = n // 2

        def rot(v, s):
            return np.concatenate([np.roll(v[:half], -s), np.roll(v[half:], -s)])
        for s in steps:
            g.rotate_rows(h, 0, s, out, 0, 1)
            got = g.ct_download(out, 0, 1)[0]
            assert np.array_equal(got, o.rotate_rows(cts[0], s)), "rotate_rows(%d)" % s
            assert np.array_equal(o.decode(o.decrypt(got)), rot(vals[0], s))
        many = [steps[0], 7, steps[1], 8]
        g.rotate_rows_many(h, np.arange(4, dtype=np.uint32), np.array(many, dtype=np.int32), out, np.arange(4, dtype=np.uint32))
        got = g.ct_download(out, 0, 4)
        for i, s in enumerate(many):
            assert np.array_equal(got[i], o.rotate_rows(cts[i], s)), "rotate_rows_many step %d" % s
            assert np.array_equal(o.decode(o.decrypt(got[i])), rot(vals[i], s))
        g.rotate_rows_add(h, 0, steps[0], h, 1, out, 0, 1)
        assert np.array_equal(g.ct_download(out, 0, 1)[0], o.add(o.rotate_rows(cts[0], steps[0]), cts[1]))
        for e in (elts[0], 2 * n - 1):
            g.apply_galois(h, 2, e, out, 1, 1)
            assert np.array_equal(g.ct_download(out, 1, 1)[0], o.apply_galois(cts[2], e)), "apply_galois(%d)" % e
    finally:
        g.close()


# ---------------------------------------------------------------- 5. record_steps (entry points; the networks' lists: test_lola_under_direct_keys)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_record_steps_notes_what_was_asked_for(case, rng):
    from cryptonets_amd._native import CnError
    name, xi = case
    g = _ctx(name, xi)
    try:
        g.keygen(SEED, galois=True)
        h, out = g.ct_alloc(4), g.ct_alloc(4)
        pt = g.pt_alloc(1)
        g.encode(rng.integers(0, g.t, size=g.n, dtype=np.uint64), pt, 0)
        g.encrypt(pt, 0, h, 0, 4, seed=3, pt_stride=0)
        assert g.get_option("record_steps") == 0
        g.rotate_rows(h, 0, 5, out, 0, 1)
        assert g.rotation_steps() == ([], False)                       # off by default
        g.set_option("record_steps", 1)
        g.rotate_rows(h, 0, 169, out, 0, 1)
        g.rotate_rows(h, 0, 0, out, 0, 1)
        g.rotate_rows_many(h, np.arange(2, dtype=np.uint32), np.array([-12, 169], dtype=np.int32), out, np.arange(2, dtype=np.uint32))
        g.rotate_rows_add(h, 0, 7, h, 1, out, 0, 1)
        assert g.rotation_steps() == ([-12, 7, 169], False)
        for bad in (lambda: g.rotate_rows(h, 0, g.n // 2, out, 0, 1), lambda: g.rotate_rows(h, 9, 3, out, 0, 1),
                    lambda: g.rotate_rows_add(h, 0, g.n, h, 1, out, 0, 1), lambda: g.apply_galois(h, 0, g.galois_elt_from_step(-3), out, 0, 1)):
            with pytest.raises(CnError):                               # step too large, index out of range, no key for the element (cn_apply_galois takes no detour)
                bad()
        assert g.rotation_steps() == ([-12, 7, 169], False)            # a refused call leaves nothing behind
        g.sum_slots(out, 0, 1, 8)
        assert g.rotation_steps() == ([-12, -4, -2, -1, 7, 169], False)
        g.apply_galois(h, 0, g.galois_elt_from_step(-16), out, 0, 1)
        g.apply_galois(h, 0, 2 * g.n - 1, out, 0, 1)
        assert g.rotation_steps() == ([-16, -12, -4, -2, -1, 7, 169], True)
        lv = g.level(g.k - 1)
        assert lv.get_option("record_steps") == 1 and lv.rotation_steps() == ([], False)      # created while its parent records: it records too, into its own list
        lv.set_option("record_steps", 0)
        g.set_option("record_steps", 0)
        assert g.rotation_steps() == ([], False)                       # cleared
        g.set_option("defer", 1)
        g.set_option("record_steps", 1)
        g.rotate_rows(h, 0, -9, out, 0, 1)                             # queued: noted when it is asked for
        assert g.rotation_steps() == ([-9], False)
        g.set_option("defer", 0)
    finally:
        g.close()


# ---------------------------------------------------------------- 6. cn_galois_elts
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_galois_elts_lists_the_keys_held(case, rng):
    import ctypes as C
    from cryptonets_amd import _native
    name, xi = case
    g = _ctx(name, xi)
    try:
        n = g.n
        assert g.galois_elts() == []
        g.keygen(SEED, galois=True)
        assert g.galois_elts() == sorted(set(keygen_order(n)))
        g.close()
        g = _ctx(name, xi)
        g.keygen(SEED, galois=False)
        steps = _steps_for(n)
        elts = [g.galois_elt_from_step(s) for s in steps] + [2 * n - 1]
        g.keygen_galois(SEED, elts)
        assert g.galois_elts() == sorted(elts)
        # cap and null handling
        cnt = C.c_uint32(99)
        assert g.L.cn_galois_elts(g._h, None, 0, C.byref(cnt)) == 0 and cnt.value == len(elts)
        buf = np.zeros(len(elts), dtype=np.uint64)
        cnt = C.c_uint32(0)
        assert g.L.cn_galois_elts(g._h, buf.ctypes.data_as(_native.U64P), len(elts) - 1, C.byref(cnt)) == -1 and cnt.value == len(elts)
        assert not buf.any()
        assert g.L.cn_galois_elts(g._h, buf.ctypes.data_as(_native.U64P), len(elts), None) == -1
        # a level context reports its parent's list and rotates by a chosen step to the same plaintext (under ks_xi = 1 with the chain's top modulus)
        lv = g.level(g.k - 1)
        assert lv.galois_elts() == sorted(elts)
        if lv.k >= 2:                                                  # (the two-limb sets: their only level has one limb, which runs no key switch)
            v = rng.integers(0, g.t, size=n, dtype=np.uint64)
            pt, h, hl, po = g.pt_alloc(1), g.ct_alloc(1), lv.ct_alloc(2), lv.pt_alloc(1)
            g.encode(v, pt, 0)
            g.encrypt(pt, 0, h, 0, 1, seed=9)
            g.mod_switch(h, 0, 1, lv, hl, 0)
            lv.rotate_rows(hl, 0, steps[0], hl, 1, 1)
            lv.decrypt(hl, 1, 1, po, 0)
            half = n // 2
            assert np.array_equal(lv.decode(po, 0), np.concatenate([np.roll(v[:half], -steps[0]), np.roll(v[half:], -steps[0])]))
    finally:
        g.close()


# ---------------------------------------------------------------- 7. persistence and replication
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_save_and_load_carry_every_key_the_context_holds(case):
    from cryptonets_amd import serialization as ser
    from cryptonets_amd._native import Context
    from cryptonets_amd.client import DeviceClient
    from cryptonets_amd.hewrapper import AtomicSealBfvEncryptedEnvironment
    name, xi = case
    g = _ctx(name, xi)
    g.keygen(SEED, galois=False)
    elts = [g.galois_elt_from_step(s) for s in (169, -5)] + [2 * g.n - 1]
    g.keygen_galois(SEED, elts)
    env = AtomicSealBfvEncryptedEnvironment(g, DeviceClient(g, seed=1))
    f = io.BytesIO()
    ser.save_environment(f, env, withPrivateKeys=True)
    env2 = ser.load_environment(io.BytesIO(f.getvalue()), lambda n, t, q, dbc, gdbc: Context(n, t, q=q, dbc=dbc, gdbc=gdbc, device=0))
    g2 = env2.ctx
    try:
        assert g2.galois_elts() == sorted(elts)
        for e in elts:
            assert np.array_equal(g2.get_key(1, e), g.get_key(1, e))
        assert np.array_equal(g2.get_key(0), g.get_key(0)) and np.array_equal(g2.get_key(3), g.get_key(3))
    finally:
        g.close(), g2.close()


# N = 16384 with 8 limbs stays out of this one test: its default set is 26 keys of 16.8 MB - a 436 MB stream that would be written twice and compared in host
# memory.  The framing code is the same at every shape; the chosen-step round trip above runs there.
@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "c5"], ids=IDS)
def test_default_only_stream_bytes_are_unchanged(case, monkeypatch):
    """a context that holds only default-set keys is written byte for byte as with the earlier element enumeration (restated: default_enumeration)"""
    from cryptonets_amd import serialization as ser
    from cryptonets_amd.client import DeviceClient
    from cryptonets_amd.hewrapper import AtomicSealBfvEncryptedEnvironment
    name, xi = case
    g = _ctx(name, xi)
    try:
        g.keygen(SEED, galois=True)
        env = AtomicSealBfvEncryptedEnvironment(g, DeviceClient(g, seed=1))
        new = io.BytesIO()
        ser.save_environment(new, env, withPrivateKeys=True)
        assert g.galois_elts() == default_enumeration(g)
        monkeypatch.setattr(ser, "_galois_elements", default_enumeration)
        old = io.BytesIO()
        ser.save_environment(old, env, withPrivateKeys=True)
        assert new.getvalue() == old.getvalue()
    finally:
        g.close()


_BCAST_SCRIPT = r"""
import os, sys, tempfile
import numpy as np
import torch
import torch.distributed as dist
torch.cuda.set_device(0)
torch.zeros(1, device="cuda")
sys.path.insert(0, %r)
from cryptonets_amd._native import Context
from cryptonets_amd.distributed import BroadcastKeys
p, xi = %r, %r
g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
if xi:
    g.set_option("ks_xi", 1)
g.keygen(77, galois=False)
e169 = g.galois_elt_from_step(169)
g.keygen_galois(77, [e169, 3])
want = {e: g.get_key(1, e) for e in (e169, 3)}
dist.init_process_group("nccl", init_method="file://" + os.path.join(tempfile.mkdtemp(), "store"), rank=0, world_size=1)
bk = BroadcastKeys(g, 0, torch.device("cuda", 0), dist, with_galois=True)
assert g.galois_elts() == sorted([3, e169]), g.galois_elts()
for e, w in want.items():
    assert np.array_equal(g.get_key(1, e), w), e
assert g.get_option("ks_xi") == xi
assert bk.bytes == (g.key_words(False) + 2 * g.key_words(True)) * 8 and len(bk.tensors) == 3, (bk.bytes, len(bk.tensors))
dist.destroy_process_group()
g.close()
print("BCAST_OK")
"""


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_broadcast_keys_carries_a_non_default_key(case):
    """BroadcastKeys at world 1 with the process group forced (the adoption path runs; a process of its own, the framework initialises the device first):
    the element list travels ahead of the keys and a key for a non-default element arrives"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _BCAST_SCRIPT % (root, SETS[case[0]], case[1])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BCAST_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_refusals_leave_the_key_set_unchanged(case):
    from cryptonets_amd._native import CnError
    name, xi = case
    g = _ctx(name, xi)
    bare = _ctx(name, xi)
    try:
        n = g.n
        g.keygen(SEED, galois=False)
        g.keygen_galois(SEED, [3])
        before = g.get_key(1, 3)
        for bad in ([4], [5, 2 * n + 1], [5, 7, 5], [2 * n]):
            with pytest.raises(CnError) as ei:
                g.keygen_galois(SEED, bad)
            assert ei.value.code == -1, bad                            # CN_ERR_ARG
            assert g.galois_elts() == [3]
        with pytest.raises(CnError) as ei:
            bare.keygen_galois(SEED, [3])
        assert ei.value.code == -3 and bare.galois_elts() == []       # CN_ERR_NOKEY
        lv = g.level(g.k - 1)
        with pytest.raises(CnError) as ei:
            lv.keygen_galois(SEED, [5])
        assert ei.value.code == -1 and lv.galois_elts() == [3]
        spare = g.ct_alloc(1)
        g.graph_begin()
        try:
            with pytest.raises(CnError) as ei:
                g.keygen_galois(SEED, [5])
            assert ei.value.code == -1
            g.add(spare, 0, spare, 0, spare, 0)                        # (the recording can still be closed)
        finally:
            g.free(g.graph_end())
        assert g.galois_elts() == [3] and np.array_equal(g.get_key(1, 3), before)
        g.keygen_galois(SEED, [])                                      # n = 0: nothing to do
        assert g.galois_elts() == [3]
    finally:
        g.close(), bare.close()


# ---------------------------------------------------------------- 4. + 5. one image: recorded steps, fewer key switches, same plaintext
# (the networks fix their own parameters - N = 8192, CoeffModulus128 with 5 / 4 limbs, their decomposition bit counts: not a matter of the four shapes above)
@pytest.mark.parametrize("name", ["LoLa", "LoLaSmall"])
def test_lola_under_direct_keys(name):
    """One image with the default key set and with keys for exactly the steps a recorded dry run reports (networks.rotation_steps): the recorded list is the
    step list of tests/test_galois_steps_model.py, the decrypted logits are equal (LoLa: the exact integer model's), the key switches executed per plaintext
    prime drop from that model's default count to its direct count - one per rotation - and the final noise budget is not lower."""
    import os
    from cryptonets_amd import cryptonets_mnist as cm
    from cryptonets_amd import networks
    from cryptonets_amd.cryptotracker import CryptoTracker
    from cryptonets_amd.hewrapper import EncryptedSealBfvFactory
    from test_galois_steps_model import lola_key_switches, lola_rotations, lola_step_families
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small_model_weights.npz" if name == "LoLaSmall" else "cryptonets_weights.npz"))
    parms = dict(networks.FACTORY_PARAMETERS[name])
    if "SmallModulusCount" in parms:
        parms["SmallModulusCount"] += 1                                # as examples/lola.py runs it (DESIGN, LoLa sections)
    primes = len(parms["primes"])
    r = np.random.default_rng(3)
    img = np.where(r.random(784) < 0.81, 0, r.integers(1, 256, size=784)).astype(float)

    def net_of(F):
        reader = networks.lola_reader(name, Factory=F)
        reader.Features = img / 256.0
        return networks.LOLA_NETWORKS[name](F, reader, gold)

    def run(F):
        env = F.AllocateComputationEnv()
        ctxs = [e.ctx for e in env.Environments]
        for c in ctxs:
            c.stats(reset=True)
        net = net_of(F)
        net.PrepareNetwork()
        out = net.GetNext()
        col = out.GetColumn(0)
        got = [int(x) for x in col.DecryptFullPrecision(env)]
        CryptoTracker.Reset()
        budget = CryptoTracker.TestVectorBudget(col, env)
        return got, [c.stats()["Rotation"] for c in ctxs], budget, env.bigFactor

    F0 = EncryptedSealBfvFactory(client_seed=5, **parms)
    for e in F0.AllocateComputationEnv().Environments:
        assert e.ctx.get_option("record_steps") == 0
    steps, columns = networks.rotation_steps(net_of(F0), F0, 1)
    for e in F0.AllocateComputationEnv().Environments:
        assert e.ctx.get_option("record_steps") == 0 and e.ctx.rotation_steps() == ([], False)
    print("recorded steps:", steps, "columns:", columns)
    assert steps == lola_step_families(name) and columns
    got0, rot0, bud0, M = run(F0)
    for e in F0.AllocateComputationEnv().Environments:                 # (as examples/lola.py --direct-keys: the default keys leave before the new ones arrive)
        e.ctx.close()
    F1 = EncryptedSealBfvFactory(client_seed=5, steps=steps, **parms)
    n = 8192
    for e in F1.AllocateComputationEnv().Environments:
        assert e.ctx.galois_elts() == sorted({e.ctx.galois_elt_from_step(s) for s in steps} | {2 * n - 1})
    got1, rot1, bud1, _ = run(F1)
    default, direct = lola_key_switches(name)
    print("%s key switches per image and prime: default set %s, direct keys %s; final budget %d -> %d bits" % (name, rot0, rot1, bud0, bud1))
    assert got0 == got1
    if name == "LoLa":
        assert got0 == [((v % M) - M) if (v % M) * 2 > M else (v % M) for v in cm.int_logits(gold, img)]
    assert rot0 == primes * [default] and rot1 == primes * [direct] and direct == len(lola_rotations(name)) < default
    assert bud1 >= bud0
