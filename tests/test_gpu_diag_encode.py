"""cn_diag_scan and cn_diag_encode on the device, word for word: the flags against the numpy model of the header's formula, the plaintexts against
encode_batch(diagonal.pre_rotated_rows(...)) - and against pt_transform of those for an NTT-form output - on the two plaintext primes of diag_helpers at N = 1024
(m = 512: 16 tiles of 32 slots per slot row, terms with J != 0 and with p + b wrapping at m inside a tile) and on the c5 ring (N = 16384, 8 moduli) with a 40 x 9000
matrix.  The term lists hold EVERY structural candidate, the all-zero ones included, in plan order (runs of 32) and shuffled (runs of 1)."""
import numpy as np
import pytest

from cryptonets_amd import diagonal
import diag_helpers as dh
from conftest import PARAMS
from test_diagonal_flags_plan import CASES, candidates, scan_model

pytestmark = pytest.mark.gpu
CN_ERR_ARG, CN_ERR_ZERO = -1, -4
N, M = dh.N, dh.N // 2


@pytest.fixture(scope="module")
def ctxs():
    from cryptonets_amd._native import Context
    gs = [Context(N, t, q=list(dh.TINY_Q), dbc=10, gdbc=20, device=0) for t in dh.PRIMES]
    yield gs
    for g in gs:
        g.close()


@pytest.fixture(scope="module")
def c5():
    from cryptonets_amd._native import Context
    p = PARAMS["c5"]
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    yield g
    g.close()


def matrices(t):
    """the shapes of tests/test_diagonal_flags_plan.py as residues mod t, and a 300 x 900 matrix of full-range residues with t - 1 and 1 among them"""
    out = {name: np.asarray(make()) % t for name, make in CASES.items()}
    W = np.random.default_rng(t).integers(0, t, size=(300, 900))
    W[0, :3] = (t - 1, 1, t // 2)
    out["fullrange300x900"] = W
    return out


def upload_rows(g, W, ri=1):
    """the row plaintexts as _row_plaintexts keeps them, at an offset: encode_batch of W (slots at dim and above zero)"""
    h = g.pt_alloc(ri + W.shape[0] + 1)
    g.encode_batch(np.zeros((ri + W.shape[0] + 1, 1), dtype=np.uint64), h, 0)
    g.encode_batch(np.ascontiguousarray(W, dtype=np.uint64), h, ri)
    return h


def reference(g, W, terms, chunk=256):
    """handle of encode_batch(pre_rotated_rows(W, n, terms))"""
    h = g.pt_alloc(len(terms))
    for k0 in range(0, len(terms), chunk):
        g.encode_batch(diagonal.pre_rotated_rows(W, g.n, terms[k0:k0 + chunk]).astype(np.uint64), h, k0)
    return h


@pytest.mark.parametrize("prime", [0, 1])
def test_scan_equals_the_numpy_flags(ctxs, prime):
    g = ctxs[prime]
    s0 = g.get_option("diag_scan")
    for name, W in matrices(g.t).items():
        R, dim = W.shape
        h = upload_rows(g, W)
        try:
            got = g.diag_scan(h, 1, R, dim)
        finally:
            g.free(h)
        assert got.shape == (2, M) and got.dtype == bool
        assert np.array_equal(got, scan_model(W, N)), name
    assert g.get_option("diag_scan") - s0 == len(matrices(g.t))


def check_encode(g, W, terms, oi=2):
    R, dim = W.shape
    rows, ref = upload_rows(g, W), reference(g, W, terms)
    out = g.pt_alloc(oi + len(terms) + 1)
    try:
        sentinel = np.full((1, g.n), 7, dtype=np.uint64)
        g.pt_upload(out, oi - 1, sentinel)
        g.pt_upload(out, oi + len(terms), sentinel)
        g.diag_encode(rows, 1, R, dim, terms, out, oi)
        got = g.pt_download(out, oi - 1, len(terms) + 2)
        assert np.array_equal(got[1:-1], g.pt_download(ref, 0, len(terms)))
        assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[-1], sentinel[0])
    finally:
        for h in (rows, ref, out):
            g.free(h)


@pytest.mark.parametrize("prime", [0, 1])
@pytest.mark.parametrize("name", ["37x700", "600x300", "512x512", "banded300x900", "600x1024", "1x1", "3x1000", "fullrange300x900"])
def test_encode_equals_encode_batch_of_the_pre_rotated_rows(ctxs, prime, name):
    g = ctxs[prime]
    W = matrices(g.t)[name]
    mask, B, cand = candidates(W.shape[0], W.shape[1], N)
    e0 = g.get_option("diag_encode")
    check_encode(g, W, cand)                                         # plan order: runs of up to 32 terms
    assert 0 < g.get_option("diag_encode") - e0 <= 1 + len(cand) // 8192
    shuffled = [cand[i] for i in np.random.default_rng(5).permutation(len(cand))]
    check_encode(g, W, shuffled)                                     # runs of length 1 (almost all)


def test_encode_with_explicit_giant_steps_and_short_runs(ctxs):
    """B = 8: runs of 8 terms, J = 8 j up to m - 8; and a hand-made list: a run that ends at b = m - 1, J = m - 1, repeated terms"""
    g = ctxs[0]
    W = matrices(g.t)["fullrange300x900"]
    mask = diagonal.structural_diagonals(300, 900, N)
    check_encode(g, W, [(c, j * 8, b) for j in range(M // 8) for c in (0, 1) for b in range(8) if mask[c, j * 8 + b]])
    check_encode(g, W, [(1, M - 1, b) for b in range(M - 40, M)] + [(0, 0, 0), (0, 0, 0), (0, 5, 2), (0, 5, 4), (1, 0, M - 1), (0, M - 32, 31)])


@pytest.mark.parametrize("level", [False, True])
def test_ntt_form_output_equals_pt_transform_across_staging_chunks(ctxs, level):
    g = ctxs[1].level(ctxs[1].k - 1) if level else ctxs[1]
    W = matrices(g.t)["banded300x900"]
    mask, B, cand = candidates(300, 900, N)
    assert len(cand) > 2 * 256                                       # three staging chunks and a partial one
    rows, ref = upload_rows(g, W), reference(g, W, cand)
    want, out = g.ptn_alloc(len(cand)), g.ptn_alloc(len(cand) + 2)
    try:
        g.pt_transform(ref, 0, len(cand), want, 0)
        sentinel = np.full((1, g.k, g.n), 3, dtype=np.uint64)
        g.ptn_upload(out, 0, sentinel)
        g.ptn_upload(out, len(cand) + 1, sentinel)
        g.diag_encode(rows, 1, 300, 900, cand, out, 1)
        got = g.ptn_download(out, 0, len(cand) + 2)
        assert np.array_equal(got[1:-1], g.ptn_download(want, 0, len(cand)))
        assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[-1], sentinel[0])
    finally:
        for h in (rows, ref, want, out):
            g.free(h)


def random_cts(g, count, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([np.stack([rng.integers(0, q, size=g.n, dtype=np.uint64) for q in g.q]) for _ in range(2)]) for _ in range(count)])


@pytest.mark.parametrize("kind", ["pt", "ptn"])
def test_an_all_zero_term_is_a_zero_plaintext_to_mul_plain(ctxs, kind):
    from cryptonets_amd._native import CnError
    g = ctxs[0]
    W = matrices(g.t)["banded300x900"]
    nz = scan_model(W, N)
    zero = next((c, 0, i) for c in (0, 1) for i in range(M) if not nz[c, i])
    live = next((c, 0, i) for c in (0, 1) for i in range(M) if nz[c, i])
    terms = [live, zero]
    rows, ref = upload_rows(g, W), reference(g, W, terms)
    out = (g.ptn_alloc if kind == "ptn" else g.pt_alloc)(2)
    ct, res = g.ct_alloc(1), g.ct_alloc(2)
    try:
        g.diag_encode(rows, 1, 300, 900, terms, out, 0)
        if kind == "ptn":
            ref, coeff = g.ptn_alloc(2), ref
            g.pt_transform(coeff, 0, 2, ref, 0)
            g.free(coeff)
        g.ct_upload(ct, 0, random_cts(g, 1, 1))
        keep = random_cts(g, 2, 2).reshape(2, -1)
        g.ct_upload(res, 0, keep)
        codes = []
        for i, h in enumerate((ref, out)):
            with pytest.raises(CnError) as ex:
                g.mul_plain(ct, 0, h, 1, res, i)
            codes.append(ex.value.code)
        assert codes == [CN_ERR_ZERO, CN_ERR_ZERO]
        assert np.array_equal(g.ct_download(res, 0, 2), keep)       # neither wrote anything
        g.mul_plain(ct, 0, ref, 0, res, 0)
        g.mul_plain(ct, 0, out, 0, res, 1)
        got = g.ct_download(res, 0, 2)
        assert np.array_equal(got[0], got[1]) and not np.array_equal(got[0], keep[0])
        g.diag_encode(rows, 1, 300, 900, [live], out, 1)             # the flag of a place that held a zero plaintext is cleared again
        g.mul_plain(ct, 0, out, 1, res, 1)
        assert np.array_equal(g.ct_download(res, 1, 1)[0], got[0])
    finally:
        for h in (rows, ref, out, ct, res):
            g.free(h)


def test_c5_ring_forty_rows(c5):
    """N = 16384, m = 8192, t of 40 bits: 256 tiles per slot row, rows and columns in both slot rows (9000 > m), terms around the wrap and at large J"""
    g = c5
    n, m = g.n, g.n // 2
    rng = np.random.default_rng(40)
    W = rng.integers(0, g.t, size=(40, 9000))
    W[:, 100:200] = 0
    rows = upload_rows(g, W)
    try:
        assert np.array_equal(g.diag_scan(rows, 1, 40, 9000), scan_model(W, n))
    finally:
        g.free(rows)
    terms = ([(0, 0, b) for b in range(70)] + [(1, 128 * 63, b) for b in range(128)] + [(0, m - 128, b) for b in range(96, 128)]
             + [(1, 0, b) for b in range(m - 33, m)] + [(0, 4096, 5), (1, 0, 807), (1, 0, 808), (0, 0, m - 1)])
    check_encode(g, W, terms)
    few = terms[60:76] + terms[-4:]
    rows, ref = upload_rows(g, W), reference(g, W, few)
    want, out = g.ptn_alloc(len(few)), g.ptn_alloc(len(few))
    try:
        g.pt_transform(ref, 0, len(few), want, 0)
        g.diag_encode(rows, 1, 40, 9000, few, out, 0)
        assert np.array_equal(g.ptn_download(out, 0, len(few)), g.ptn_download(want, 0, len(few)))
    finally:
        for h in (rows, ref, want, out):
            g.free(h)


def test_argument_errors_write_nothing(ctxs):
    from cryptonets_amd._native import CnError
    g = ctxs[0]
    W = matrices(g.t)["37x700"]
    rows = upload_rows(g, W)
    big = g.pt_alloc(N + 2)
    out, ptn, ct = g.pt_alloc(3), g.ptn_alloc(2), g.ct_alloc(2)
    keep = np.random.default_rng(1).integers(0, g.t, size=(3, N), dtype=np.uint64)
    g.pt_upload(out, 0, keep)
    g.ct_upload(ct, 0, random_cts(g, 2, 3))
    ok = [(0, 0, 1), (1, 0, 2)]

    def refused(*a, fn=g.diag_encode):
        with pytest.raises(CnError) as ex:
            fn(*a)
        assert ex.value.code == CN_ERR_ARG, ex.value
        return str(ex.value)
    try:
        assert "R" in refused(big, 0, N + 1, 700, ok, out, 0)
        assert "dim" in refused(rows, 1, 37, 0, ok, out, 0) and "dim" in refused(rows, 1, 37, N + 1, ok, out, 0)
        assert "c =" in refused(rows, 1, 37, 700, [(0, 0, 1), (2, 0, 0)], out, 0)
        assert "b =" in refused(rows, 1, 37, 700, [(0, 0, M)], out, 0)
        assert "J =" in refused(rows, 1, 37, 700, [(0, M, 0)], out, 0)
        assert "out" in refused(rows, 1, 37, 700, ok, out, 2)                     # out too short
        assert "rows" in refused(rows, 3, 37, 700, ok, out, 0)                    # the rows leave their handle
        assert "rows" in refused(ptn, 0, 2, 700, ok, out, 0)                      # rows of kind 4
        assert "rows" in refused(rows, 1, 37, 700, ok, rows, 0)                   # out is rows
        assert "out" in refused(rows, 1, 37, 700, ok, ct, 0)
        assert "R" in refused(big, 0, N + 1, 700, fn=g.diag_scan)
        assert "rows" in refused(ptn, 0, 2, 700, fn=g.diag_scan)
        g.graph_begin()
        try:
            g.add(ct, 0, ct, 1, ct, 1)
            assert "graph" in refused(rows, 1, 37, 700, ok, out, 0)
            assert "graph" in refused(rows, 1, 37, 700, fn=g.diag_scan)
        finally:
            graph = g.graph_end()
        g.free(graph)
        assert np.array_equal(g.pt_download(out, 0, 3), keep)
        assert np.array_equal(g.decode_batch(rows, 1, 37)[:, :700], W.astype(np.uint64))
        g.diag_encode(rows, 1, 37, 700, [], out, 0)                                # count = 0: nothing to do
        g.diag_encode(rows, 1, 37, 700, ok, out, 1)
        assert np.array_equal(g.pt_download(out, 0, 1), keep[:1])
    finally:
        for h in (rows, big, out, ptn, ct):
            g.free(h)
