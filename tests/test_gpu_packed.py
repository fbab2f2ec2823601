"""GPU: packed rows (include/cnhip.h: cn_packed_words, cn_ct_download_packed, cn_ct_upload_packed) against the vectorised codecs of
cryptonets_amd.serialization, which tests/test_packed_model.py pins to the big-integer statement of the format.  Exact word equality everywhere."""
import numpy as np
import pytest

import packed_model as pm
from conftest import PARAMS
from cryptonets_amd import serialization as ser
from test_gpu_wide_moduli import SETS as WIDE_SETS

pytestmark = pytest.mark.gpu

CN_ERR_ARG = -1
SEED_A = bytes((5 * i + 1) & 0xff for i in range(32))
COUNT = 3
SETS = {"tiny": PARAMS["tiny"], "c3": PARAMS["c3"], "n16k7": PARAMS["n16k7"], "B60": WIDE_SETS["B60"], "B50": WIDE_SETS["B50"]}
NAMES = list(SETS)
_made = {}


def make(name):
    """a context without keys: packing, unpacking and the expansion from a public seed need none"""
    from cryptonets_amd._native import Context, default_coeff_modulus
    if name not in _made:
        p = SETS[name]
        q = list(p["q"]) if p["q"] is not None else default_coeff_modulus(p["n"])
        _made[name] = Context(p["n"], p["t"], q=q, dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    return _made[name]


@pytest.mark.parametrize("name", NAMES)
def test_packed_words_is_the_formula(name):
    g = make(name)
    for polys in (1, 2, 3):
        assert g.packed_words(polys) == pm.packed_words(g.n, g.q, polys)


@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_download_packed_equals_packed_download(name, size, rng):
    g = make(name)
    w = pm.random_words(rng, g.q, g.n, COUNT, size)
    h = g.ct_alloc(COUNT, size)
    g.ct_upload(h, 0, w)
    plain = g.ct_download(h, 0, COUNT, size)
    assert np.array_equal(plain, w)
    assert np.array_equal(g.ct_download_packed(h, 0, COUNT, polys=0), ser.pack_ciphertexts(plain, g.q, g.n))
    kn = g.k * g.n
    assert np.array_equal(g.ct_download_packed(h, 1, 2, polys=1), ser.pack_ciphertexts(plain[1:, :kn], g.q, g.n))      # c0 only, from the middle
    g.free(h)


@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("name", NAMES)
def test_upload_packed_restores_the_words(name, size, rng):
    """rows with 0 and q_j - 1 at their ends (packed_model.random_words)"""
    g = make(name)
    w = pm.random_words(rng, g.q, g.n, COUNT, size)
    h = g.ct_alloc(COUNT, size)
    g.ct_upload(h, 0, np.full_like(w, 1))
    g.ct_upload_packed(h, 0, ser.pack_ciphertexts(w, g.q, g.n), polys=0)
    assert np.array_equal(g.ct_download(h, 0, COUNT, size), w)
    g.free(h)


@pytest.mark.parametrize("f64", [1, 0])
@pytest.mark.parametrize("name", NAMES)
def test_upload_packed_c0_equals_upload_compact(name, f64, rng):
    g = make(name)
    g.set_option("f64", f64)
    try:
        c0 = pm.random_words(rng, g.q, g.n, COUNT, 1)
        a, b = g.ct_alloc(COUNT), g.ct_alloc(COUNT)
        g.ct_upload_compact(a, 0, c0, SEED_A, a_nonce=3, a_item0=11)
        g.ct_upload_packed(b, 0, ser.pack_ciphertexts(c0, g.q, g.n), polys=1, a_seed=SEED_A, a_nonce=3, a_item0=11)
        wa, wb = g.ct_download(a, 0, COUNT), g.ct_download(b, 0, COUNT)
        assert np.array_equal(wa[:, :g.k * g.n], c0) and wa[:, g.k * g.n:].any()
        assert np.array_equal(wa, wb)
        g.free(a), g.free(b)
    finally:
        g.set_option("f64", 1)


@pytest.mark.parametrize("polys", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_sub_range_leaves_its_neighbours_untouched(name, polys, rng):
    g = make(name)
    kn = g.k * g.n
    before = pm.random_words(rng, g.q, g.n, COUNT + 2, 2)
    w = pm.random_words(rng, g.q, g.n, COUNT, 2)
    h = g.ct_alloc(COUNT + 2)
    g.ct_upload(h, 0, before)
    if polys:
        g.ct_upload_packed(h, 1, ser.pack_ciphertexts(w[:, :kn], g.q, g.n), polys=1, a_seed=SEED_A, a_nonce=1, a_item0=0)
    else:
        g.ct_upload_packed(h, 1, ser.pack_ciphertexts(w, g.q, g.n), polys=0)
    got = g.ct_download(h, 0, COUNT + 2)
    assert np.array_equal(got[0], before[0]) and np.array_equal(got[-1], before[-1])
    assert np.array_equal(got[1:-1, :kn], w[:, :kn])
    assert polys or np.array_equal(got[1:-1], w)
    g.free(h)


@pytest.mark.parametrize("name,limbs", [("tiny", 2), ("tiny", 1), ("c3", 3)])
def test_level_context_packs_with_its_own_limbs(name, limbs, rng):
    top = make(name)
    g = top.level(limbs)
    assert g.packed_words(2) == pm.packed_words(g.n, g.q, 2) < top.packed_words(2)
    w = pm.random_words(rng, g.q, g.n, COUNT, 2)
    h = g.ct_alloc(COUNT)
    g.ct_upload_packed(h, 0, ser.pack_ciphertexts(w, g.q, g.n), polys=0)
    assert np.array_equal(g.ct_download(h, 0, COUNT), w)
    assert np.array_equal(g.ct_download_packed(h, 0, COUNT, polys=0), ser.pack_ciphertexts(w, g.q, g.n))
    c0 = w[:, :g.k * g.n]
    a = g.ct_alloc(COUNT)
    g.ct_upload_compact(a, 0, c0, SEED_A, a_nonce=2, a_item0=7)
    g.ct_upload_packed(h, 0, ser.pack_ciphertexts(c0, g.q, g.n), polys=1, a_seed=SEED_A, a_nonce=2, a_item0=7)
    assert np.array_equal(g.ct_download(h, 0, COUNT), g.ct_download(a, 0, COUNT))
    g.free(h), g.free(a)


@pytest.mark.parametrize("name", NAMES)
def test_residue_not_below_its_modulus_is_reduced_and_reported(name, rng):
    """one row holds q_j, another 2^b_j - 1: CN_ERR_ARG, the counter advances, the array holds canonical words; a valid upload afterwards is exact"""
    from cryptonets_amd._native import CnError
    g = make(name)
    n, k = g.n, g.k
    w = pm.random_words(rng, g.q, n, COUNT, 2)
    h = g.ct_alloc(COUNT)
    for where, value in (((0, 0, 0, n // 2), lambda j: g.q[j]), ((COUNT - 1, 1, k - 1, n - 1), lambda j: (1 << g.q[j].bit_length()) - 1)):
        bad = w.copy().reshape(COUNT, 2, k, n)
        bad[where] = value(where[2])
        before = g.get_option("packed_bad_residues")
        with pytest.raises(CnError) as e:
            g.ct_upload_packed(h, 0, ser.pack_ciphertexts(bad.reshape(COUNT, -1), g.q, n), polys=0)
        assert e.value.code == CN_ERR_ARG and "residue not below its modulus" in str(e.value)
        assert g.get_option("packed_bad_residues") == before + 1
        got = g.ct_download(h, 0, COUNT).reshape(COUNT, 2, k, n)
        want = bad.copy()
        want[where] = value(where[2]) - g.q[where[2]]
        assert np.array_equal(got, want)                                       # v - q_j: canonical
    before = g.get_option("packed_bad_residues")
    g.ct_upload_packed(h, 0, ser.pack_ciphertexts(w, g.q, n), polys=0)
    assert np.array_equal(g.ct_download(h, 0, COUNT), w) and g.get_option("packed_bad_residues") == before
    g.free(h)


def test_arguments_are_checked(rng):
    from cryptonets_amd._native import CnError, U64P
    g = make("tiny")
    h2, h3 = g.ct_alloc(COUNT), g.ct_alloc(COUNT, 3)
    row = np.zeros((1, g.packed_words(1)), dtype=np.uint64)
    ptr = row.ctypes.data_as(U64P)
    for call in (lambda: g._chk(g.L.cn_ct_upload_packed(g._h, h3, 0, 1, 1, ptr, SEED_A, 0, 0)),   # c0 + seed needs size 2
                 lambda: g._chk(g.L.cn_ct_upload_packed(g._h, h2, COUNT, 1, 1, ptr, SEED_A, 0, 0)),        # range
                 lambda: g._chk(g.L.cn_ct_upload_packed(g._h, h2, 0, 1, 2, ptr, SEED_A, 0, 0)),            # polys
                 lambda: g._chk(g.L.cn_ct_upload_packed(g._h, h2, 0, 1, 1, ptr, None, 0, 0))):               # null seed
        with pytest.raises(CnError) as e:
            call()
        assert e.value.code == CN_ERR_ARG
    with pytest.raises(ValueError):
        g.ct_upload_packed(h2, 0, np.zeros((1, 5), dtype=np.uint64), polys=1, a_seed=SEED_A)
    g.free(h2), g.free(h3)
