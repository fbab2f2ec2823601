"""cn_mul_relin (hot loop B) on every code path it can take, against the CPU oracle word for word.

The library picks the path of a Multiply + Relinearize by the ciphertext count and the context's options: the key-switch variant
(cn_ks_plan, cn_ks_plan.h: fused kernel, two launches with a workgroup per digit, two launches with a workgroup per source limb; "ks_wide"
forces one), and for >= 512 ciphertexts at N <= 8192 the batch in parts over the context's two streams ("sq_halves", pipelined_halves).  The
counts below sit on both sides of every threshold; each is derived from the number of limbs k and the block limits, not written out.
Every result is compared with the oracle, never with another GPU setting.  "mul_relin_pipelined" reads back whether a call ran in parts:
a deterministic check of which path was taken, independent of whether a race between the two streams happens to fire in one run.

Each test makes and closes its own context: forced two-launch key switches of 845 ciphertexts at c3 grow the key-switch arena to
~14 GB, which must not outlive the test.
"""
import numpy as np
import pytest

from conftest import PARAMS, get_oracle

pytestmark = pytest.mark.gpu

KS_DIGIT_MAX_BLOCKS = 10      # (ciphertext, limb) blocks up to which the two-launch key switch has a workgroup per digit (cn_ks_plan.h: KsSwitches::digit_max_blocks)
KS_WIDE_MAX_BLOCKS = 160      # ... up to which a key switch runs as two launches at all (KsSwitches::wide_max_blocks)
SQ_HALVES_MIN = 512           # ciphertexts from which cn_mul_relin runs in parts over two streams (cn_mul_plan.h)
SETS = ("tiny", "c3")
LARGEST = {"tiny": 700, "c3": 845}             # c3: the squaring layer of CryptoNets
SETTINGS = [(wide, halves) for wide in (-1, 0, 1, 2) for halves in (0, 1)]


def ks_edges(k):
    """the last counts of the two-launch forms and the first counts after them: (mode 1 | mode 2) and (mode 2 | fused) in automatic mode"""
    m1, m2 = KS_DIGIT_MAX_BLOCKS // k, KS_WIDE_MAX_BLOCKS // k
    return (m1, m1 + 1, m2, m2 + 1)


def counts(name, k):
    extra = (1, SQ_HALVES_MIN + 1) if name == "tiny" else ()
    return sorted(set(ks_edges(k) + (SQ_HALVES_MIN - 1, SQ_HALVES_MIN, LARGEST[name]) + extra))


def fresh_context(name, galois=False):
    from cryptonets_amd._native import Context
    p, o = PARAMS[name], get_oracle(name, galois=galois)
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    g.set_relin_key(o.relin_key())
    if galois:
        for i, e in enumerate(o.galois_elts()):
            g.set_galois_key(e, o.galois_key(i))
    return o, g


def extreme(cts, o, first):
    """residues at the edges of the range in three ciphertexts from `first` on: q-1 everywhere, 0 everywhere, q/2 in c0"""
    w = cts[first:first + 3].reshape(3, 2, o.k, o.n)
    for j, qj in enumerate(o.q):
        w[0, :, j, :] = qj - 1
        w[1, :, j, :] = 0
        w[2, 0, j, :] = qj // 2


def up(g, cts):
    h = g.ct_alloc(len(cts))
    g.ct_upload(h, 0, cts)
    return h


@pytest.fixture(scope="module")
def cases():
    """operands and the oracle's results per parameter set, computed once for the largest count: the results for `n` ciphertexts are the
    first n rows (every operand form reads its ciphertexts from fixed first indices)"""
    cache = {}

    def get(name):
        if name not in cache:
            o = get_oracle(name, galois=False)
            from bench import uniform_ct_words
            rng = np.random.default_rng(0x5E1F + len(name))
            M = LARGEST[name]
            X, Y = uniform_ct_words(rng, o.q, o.n, M + 8), uniform_ct_words(rng, o.q, o.n, M + 8)
            extreme(X, o, 2)
            extreme(Y, o, 5)
            xb = np.repeat(X[1:2], M, axis=0)
            exp = {"square": o.mul_relin_batch(X[2:2 + M], X[2:2 + M]),        # X[2+i]^2
                   "ranges": o.mul_relin_batch(X[2:2 + M], X[7:7 + M]),        # X[2+i] X[7+i]: two overlapping ranges of one handle
                   "handles": o.mul_relin_batch(X[2:2 + M], Y[5:5 + M]),       # X[2+i] Y[5+i]
                   "a_bcast": o.mul_relin_batch(xb, Y[5:5 + M]),               # X[1] Y[5+i]
                   "b_bcast": o.mul_relin_batch(Y[5:5 + M], xb)}               # Y[5+i] X[1]
            cache[name] = (X, Y, exp)
        return cache[name]
    yield get
    cache.clear()


def download_into(g, h, first, buf):
    """ct_download into a buffer that is reused (hundreds of MiB per call at c3: no fresh allocation per comparison)"""
    from cryptonets_amd._native import _p64
    g._chk(g.L.cn_ct_download(g._h, h, first, buf.shape[0], _p64(buf)))
    return buf


@pytest.mark.parametrize("name", SETS)
def test_every_path_gives_the_oracle_words(name, cases):
    """five operand forms (squaring, two ranges of one handle, two handles, a broadcast first or second operand) and the exact in-place call
    (squaring and product) at every threshold count, under every key-switch variant with and without the two-stream parts"""
    o, g = fresh_context(name)
    X, Y, exp = cases(name)
    M, k = LARGEST[name], o.k
    assert (SQ_HALVES_MIN // 4) * k > KS_WIDE_MAX_BLOCKS        # every part of a pipelined batch is large enough for the fused key switch in automatic mode
    forms = (("square", (0, 2, 1, 0, 2, 1)), ("ranges", (0, 2, 1, 0, 7, 1)), ("handles", (0, 2, 1, 1, 5, 1)),
             ("a_bcast", (0, 1, 0, 1, 5, 1)), ("b_bcast", (1, 5, 1, 0, 1, 0)))
    buf = np.empty((M, 2 * k * o.n), dtype=np.uint64)
    edge = np.empty((1, 2 * k * o.n), dtype=np.uint64)
    fill = np.full((1, 2 * k * o.n), 7, dtype=np.uint64)
    wrong_path, wrong_words = [], []                    # every call is checked; the failures are reported together
    try:
        hx, hy = up(g, X), up(g, Y)
        ho, hz = g.ct_alloc(M + 8), g.ct_alloc(M + 4)
        hs = (hx, hy)

        def check(what, before, pipelined, got, want):
            if (g.get_option("mul_relin_pipelined") > before) != pipelined:
                wrong_path.append(what)
            if not np.array_equal(got, want):
                wrong_words.append(what)
        for wide, halves in SETTINGS:
            g.set_option("ks_wide", wide)
            g.set_option("sq_halves", halves)
            for n in counts(name, k):
                pipelined = halves == 1 and wide in (-1, 0) and n >= SQ_HALVES_MIN
                for form, (a, ai, ast, b, bi, bst) in forms:
                    g.ct_upload(ho, 4 + n, fill)                                   # a sentinel right behind the output range
                    before = g.get_option("mul_relin_pipelined")
                    g.mul_relin(hs[a], ai, hs[b], bi, ho, 4, n, a_stride=ast, b_stride=bst)
                    check((form, n, wide, halves), before, pipelined, download_into(g, ho, 4, buf[:n]), exp[form][:n])
                    if not np.array_equal(download_into(g, ho, 4 + n, edge), fill):
                        wrong_words.append((form, n, wide, halves, "written behind the range"))
                for form, b, bi in (("square", hz, 3), ("handles", hy, 5)):         # exactly in place: out == a, oi == ai
                    g.copy(hx, 2, hz, 3, n)
                    before = g.get_option("mul_relin_pipelined")
                    g.mul_relin(hz, 3, b, bi, hz, 3, n)
                    check(("in place " + form, n, wide, halves), before, pipelined, download_into(g, hz, 3, buf[:n]), exp[form][:n])
        assert not wrong_words, wrong_words
        assert not wrong_path, wrong_path
        assert np.array_equal(g.ct_download(hx, 0, M + 8), X)        # operands intact
        assert np.array_equal(g.ct_download(hy, 0, M + 8), Y)
    finally:
        g.close()


@pytest.mark.parametrize("name", SETS)
def test_defaults_pipeline_the_batch(name, cases):
    """with the default options a batch of >= 512 ciphertexts runs in parts over the two streams (the CryptoNets squaring layer at c3:
    845 ciphertexts) and a smaller one does not; the words are the oracle's"""
    o, g = fresh_context(name)
    X, Y, exp = cases(name)
    M = LARGEST[name]
    try:
        assert g.get_option("ks_wide") == -1 and g.get_option("sq_halves") == 1
        hx, ho = up(g, X), g.ct_alloc(M)
        for n in (SQ_HALVES_MIN - 1, M):
            before = g.get_option("mul_relin_pipelined")
            g.mul_relin(hx, 2, hx, 2, ho, 0, n)
            assert g.get_option("mul_relin_pipelined") == before + (n >= SQ_HALVES_MIN), n
            assert np.array_equal(g.ct_download(ho, 0, n), exp["square"][:n]), n
    finally:
        g.close()


@pytest.mark.parametrize("name", SETS)
def test_queued_calls_flushed_as_one_group(name, cases):
    """per-ciphertext calls queued by "defer" 1 and 2 and flushed as one group of >= 512 ("sq_halves" 2 pipelines such a group): with a forced
    two-launch key switch the group must not run in parts; in automatic mode it does.  Squarings and products of two handles."""
    o, g = fresh_context(name)
    X, Y, exp = cases(name)
    n = SQ_HALVES_MIN + 1
    try:
        hx, hy = up(g, X), up(g, Y)
        xs, ys = [g.ct_alloc(1) for _ in range(n)], [g.ct_alloc(1) for _ in range(n)]
        for i in range(n):
            g.copy(hx, 2 + i, xs[i], 0, 1)
            g.copy(hy, 5 + i, ys[i], 0, 1)
        g.set_option("sq_halves", 2)
        for wide, mode in ((1, 1), (1, 2), (-1, 1)):
            g.set_option("ks_wide", wide)
            for form in ("square", "handles"):
                before = g.get_option("mul_relin_pipelined")
                rs = [g.ct_alloc(1) for _ in range(n)]
                g.set_option("defer", mode)
                for i in range(n):
                    g.mul_relin(xs[i], 0, xs[i] if form == "square" else ys[i], 0, rs[i], 0, 1)
                g.set_option("defer", 0)                                # flushes the queue
                assert (g.get_option("mul_relin_pipelined") > before) == (wide == -1), (form, wide, mode)
                got = np.stack([g.ct_download(r, 0, 1)[0] for r in rs])
                assert np.array_equal(got, exp[form][:n]), (form, wide, mode)
                g.free_many(rs)
    finally:
        g.close()


@pytest.mark.parametrize("name", SETS)
def test_partial_overlaps_are_refused(name, cases):
    """an output range that overlaps an operand's range partially is refused (CN_ERR_ARG) by the immediate call and by both queued forms, and
    nothing is written: one operand shifted by +1 or -1 against the output, the second operand shifted, a broadcast operand inside the output"""
    from cryptonets_amd._native import CnError
    o, g = fresh_context(name)
    X, Y, _ = cases(name)
    M = LARGEST[name]
    small = ks_edges(o.k)[1]
    assert small >= 3                                   # the broadcast operand (index 4) lies inside [2, 2 + small)
    try:
        hx, hy = up(g, X), up(g, Y)
        for n in (small, SQ_HALVES_MIN):
            calls = (("oi = ai + 1", (hx, 2, 1, hy, 5, 1, hx, 3)),
                     ("oi + 1 = ai", (hx, 3, 1, hx, 3, 1, hx, 2)),
                     ("b shifted", (hy, 5, 1, hx, 1, 1, hx, 2)),
                     ("a broadcast inside", (hx, 4, 0, hy, 5, 1, hx, 2)),
                     ("b broadcast inside", (hy, 5, 1, hx, 4, 0, hx, 2)))
            for mode in (0, 1, 2) if n <= 4 else (0, 1):     # (defer 2 passes calls of up to 4 ciphertexts through the lock-free ring)
                for what, (a, ai, ast, b, bi, bst, out, oi) in calls:
                    before = g.get_option("mul_relin_pipelined")
                    g.set_option("defer", mode)
                    with pytest.raises(CnError):
                        g.mul_relin(a, ai, b, bi, out, oi, n, a_stride=ast, b_stride=bst)
                    assert g.get_option("pending_calls") == 0, (what, n, mode)
                    g.set_option("defer", 0)
                    assert g.get_option("mul_relin_pipelined") == before, (what, n, mode)
                    assert np.array_equal(g.ct_download(hx, 0, M + 8), X), (what, n, mode)
                    assert np.array_equal(g.ct_download(hy, 0, M + 8), Y), (what, n, mode)
    finally:
        g.set_option("defer", 0)
        g.close()


@pytest.mark.parametrize("name", SETS)
def test_rotations_at_the_key_switch_thresholds(name, rng):
    """cn_rotate_rows, cn_rotate_columns and cn_rotate_rows_add at the counts where the key-switch variant changes, under automatic and both forced
    two-launch variants: in place, disjoint ranges, and a range shifted by one (the rotations take the permutation pass; the _add form refuses
    it and writes nothing).  This is where ks_perm_fused and the shifted-overlap choice meet the variant switch."""
    from bench import uniform_ct_words
    from cryptonets_amd._native import CnError
    o, g = fresh_context(name, galois=True)
    ns = ks_edges(o.k)
    N = max(ns) + 2
    X, A = uniform_ct_words(rng, o.q, o.n, N), uniform_ct_words(rng, o.q, o.n, N)
    extreme(X, o, 0)
    ops = {"rows": (lambda c: o.rotate_rows(c, 1)), "cols": o.rotate_columns}
    exp = {op: np.stack([f(c) for c in X]) for op, f in ops.items()}
    add = lambda rot, acc: np.stack([o.add(acc[i], rot[i]) for i in range(len(rot))])     # noqa: E731
    try:
        hx, ha, h, ho = up(g, X), up(g, A), g.ct_alloc(N), g.ct_alloc(N)
        rot = {"rows": lambda s, si, d, di, n: g.rotate_rows(s, si, 1, d, di, n),
               "cols": lambda s, si, d, di, n: g.rotate_columns(s, si, d, di, n)}
        for wide in (-1, 1, 2):
            g.set_option("ks_wide", wide)
            for n in ns:
                where = (name, n, wide)
                for op, f in rot.items():
                    g.copy(hx, 0, h, 0, N)
                    f(h, 1, h, 1, n)                                               # in place
                    assert np.array_equal(g.ct_download(h, 1, n), exp[op][1:1 + n]), (op, "in place") + where
                    f(hx, 1, ho, 2, n)                                             # disjoint
                    assert np.array_equal(g.ct_download(ho, 2, n), exp[op][1:1 + n]), (op, "disjoint") + where
                    g.copy(hx, 0, h, 0, N)
                    f(h, 0, h, 1, n)                                               # shifted overlap: oi = ii + 1
                    assert np.array_equal(g.ct_download(h, 1, n), exp[op][:n]), (op, "shifted") + where
                g.rotate_rows_add(hx, 1, 1, ha, 0, ho, 2, n)                       # disjoint operand, accumulator and result
                assert np.array_equal(g.ct_download(ho, 2, n), add(exp["rows"][1:1 + n], A[:n])), ("rows_add", "disjoint") + where
                g.copy(hx, 0, h, 0, N)
                g.rotate_rows_add(h, 1, 1, h, 1, h, 1, n)                          # all three the same range
                assert np.array_equal(g.ct_download(h, 1, n), add(exp["rows"][1:1 + n], X[1:1 + n])), ("rows_add", "in place") + where
                g.copy(hx, 0, h, 0, N)
                for args in ((h, 0, 1, ha, 0, h, 1, n), (hx, 0, 1, h, 0, h, 1, n)):    # shifted operand / shifted accumulator
                    with pytest.raises(CnError):
                        g.rotate_rows_add(*args)
                    assert np.array_equal(g.ct_download(h, 0, N), X), ("rows_add", "shifted") + where
    finally:
        g.close()
