"""GPU: the summed rotations (cn_apply_galois_sum / cn_rotate_rows_sum: the term MAC of the two-launch key switch + k_ks_sum_terms) word for word against the
oracle alone - o.add over o.apply_galois / o.rotate_rows: the call writes the words of the literal sequence, with any key set.

Cells of tests/size_policy_sets.py: all five ring sizes x three policies at width 60, width 10 at (u64, 1024), (f64, 8192), (f64l, 16384) and (f64, 16384).
Inputs: edge_words (the residues 0, 1, (q - 1) / 2, (q + 1) / 2, q - 1 in every limb, and q - 1 everywhere) and uniform words.  G = 3 in every cell: a group of
four terms (step 1 of a, step -2 of b, element 1 of c, the column swap of a again), a group of one rotated term, a group of two element-1 terms; sentinels on both
sides of the outputs and the inputs keep their words.  Beside the cells: term counts on both sides of each threshold of the plan (per digit up to 10 (term, limb)
blocks, per source limb up to 160, per term above; N = 16384: per digit whatever the count) with the q - 1-everywhere ciphertext among 40 terms at 49 bits, the steps form
with non-adjacent-form hops and the closed forms of its counters, the other key-switch convention, a level context, integer keys on FP64-capable moduli, a
recorded call launched twice, the deferred queue flushed in front of the call, "legacy_ntt" composing the same words, and every refusal (error code, outputs and
`kernel_launches` unchanged)."""
import numpy as np
import pytest

from cryptonets_amd._native import CnError, Context
from oracle.cno import Oracle
from size_policy_sets import CELLS, Q, T, Cell, edge_words, uniform

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOKEY = -1, -3
WIDE = [(p, n, 60) for p, n in CELLS]
NARROW = [("u64", 1024, 10), ("f64", 8192, 10), ("f64l", 16384, 10), ("f64", 16384, 10)]


@pytest.fixture(scope="module", params=WIDE + NARROW, ids=lambda c: "%s-n%d-w%d" % c)
def cell(request):
    c = Cell(*request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """(f64, 1024, width 10): the cell of the tests that need one cell only"""
    c = Cell("f64", 1024, 10)
    yield c
    c.close()


def inputs(o, seed):
    """[edge residues cycling, q - 1 everywhere, uniform]"""
    rng = np.random.default_rng(seed)
    return np.concatenate([edge_words(o, rng, 2), uniform(o, rng, 1)])


def setup(g, cts, outputs):
    """the inputs at index 1 .. of their handle; `outputs` + 2 sentinel ciphertexts (first and last must keep their words)"""
    hin = g.ct_alloc(len(cts) + 1)
    g.ct_upload(hin, 1, cts)
    rng = np.random.default_rng(len(cts) * 1000 + outputs)
    sentinel = np.stack([rng.integers(0, 1 << 30, size=cts.shape[1], dtype=np.uint64) for _ in range(outputs + 2)])
    hout = g.ct_alloc(outputs + 2)
    g.ct_upload(hout, 0, sentinel)
    return hin, hout, sentinel


def moved(g, fn):
    s0, h0 = g.stats(), g.get_option("ks_summed")
    fn()
    s1 = g.stats()
    d = {k: s1[k] - s0[k] for k in s1}
    d["ks_summed"] = g.get_option("ks_summed") - h0
    return d


class Terms:
    """the oracle's rotated terms, each computed once: (input index, element) -> words"""

    def __init__(self, o, cts):
        self.o, self.cts, self.memo = o, cts, {}

    def term(self, i, e):
        if e == 1:
            return self.cts[i]
        if (i, e) not in self.memo:
            self.memo[(i, e)] = self.o.apply_galois(self.cts[i], e)
        return self.memo[(i, e)]

    def total(self, pairs):
        acc = self.term(*pairs[0])
        for p in pairs[1:]:
            acc = self.o.add(acc, self.term(*p))
        return acc


def check_three_groups(o, g, cts, tot, fused=True):
    """the G = 3 call of the module text on inputs a, b, c = cts[0..2]; the counters' closed forms; then the group of plain addends alone.  fused = False: the
    plan composes the literal sequence (the same words; 2 k inverse transforms per rotation, "ks_summed" unchanged)"""
    n, k = o.n, o.k
    e1, em2, cols = o.galois_elt_from_step(1), o.galois_elt_from_step(-2), 2 * n - 1
    groups = [[(0, e1), (1, em2), (2, 1), (0, cols)], [(2, em2)], [(1, 1), (2, 1)]]
    ii = [1 + i for grp in groups for i, _ in grp]
    elts = [e for grp in groups for _, e in grp]
    off = [0, 4, 5, 7]
    hin, hout, sentinel = setup(g, cts, 3)
    d = moved(g, lambda: g.apply_galois_sum(hin, ii, elts, off, hout, 1))
    got = g.ct_download(hout, 0, 5)
    assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[4], sentinel[4]), "a ciphertext beside the outputs changed"
    assert np.array_equal(g.ct_download(hin, 1, 3), cts), "an input changed"
    ref = Terms(o, cts)
    for r, grp in enumerate(groups):
        exp = ref.total(grp)
        assert np.array_equal(got[1 + r], exp), ("group %d" % r, int((got[1 + r] != exp).sum()))
    # four rotated terms in two outputs: tot k forward transforms each, 2 k inverse ones per OUTPUT; two launches + AddMany's kernel for the plain group
    if fused:
        assert (d["ntt_forward_limbs"], d["ntt_inverse_limbs"], d["kernel_launches"], d["Rotation"], d["ks_summed"]) == (4 * tot * k, 2 * 2 * k, 3, 4, 1), d
    else:
        assert (d["ntt_forward_limbs"], d["ntt_inverse_limbs"], d["Rotation"], d["ks_summed"]) == (4 * tot * k, 4 * 2 * k, 4, 0), d
    assert (d["AddMany"], d["AddManyItemCount"]) == (3, 7), d
    # a group made only of element-1 terms: cn_add_many's kernel and nothing else
    g.ct_upload(hout, 0, sentinel)
    d = moved(g, lambda: g.apply_galois_sum(hin, [2, 3], [1, 1], [0, 2], hout, 2))
    got = g.ct_download(hout, 0, 5)
    assert np.array_equal(got[2], o.add(cts[1], cts[2])) and np.array_equal(got[[0, 1, 3, 4]], sentinel[[0, 1, 3, 4]])
    assert (d["kernel_launches"], d["ks_summed"], d["ntt_forward_limbs"], d["ntt_inverse_limbs"], d["Rotation"], d["AddMany"], d["AddManyItemCount"]) == (1, 0, 0, 0, 0, 1, 2), d
    # a group of one rotated term is cn_apply_galois
    g.apply_galois_sum(hin, [1], [cols], [0, 1], hout, 3)
    assert np.array_equal(g.ct_download(hout, 3, 1)[0], ref.term(0, cols))
    g.free(hin)
    g.free(hout)


COMPOSED = ("u64", 16384)                                   # cn_ks_sum_built: no kernel under the integer policy at N = 16384 - the same words through the literal sequence


def test_words_equal_the_literal_sequence_in_every_cell(cell):
    check_three_groups(cell.o, cell.g, inputs(cell.o, 0x53 + cell.n + cell.width), cell.tot, fused=(cell.policy, cell.n) != COMPOSED)


@pytest.mark.parametrize("policy, n, counts", [("f64", 1024, (3, 4, 40, 53, 54)), ("f64", 16384, (3, 40, 54))],
                         ids=["f64-n1024-w10", "f64-n16384-w10"])
def test_every_granularity_of_the_plan(policy, n, counts, small):
    """term counts on both sides of each threshold (cn_ks_sum_plan; k = 3: 10 blocks = 3 terms per digit, 160 blocks = 53 terms per source limb - N = 16384: per
    digit, as are 54 -, 54 per term), all terms in ONE group with the q - 1-everywhere ciphertext among them: 49-bit moduli, 15 digits -
    lazy accumulators and the sum of the partials at their bound"""
    c = small if n == 1024 else Cell(policy, n, 10)
    try:
        o, g = c.o, c.g
        cts = inputs(o, 0x71 + n)
        ref = Terms(o, cts)
        hin, hout, sentinel = setup(g, cts, 1)
        for count in counts:
            pairs = [((e + 1) % 3, c.elts[e % 5]) for e in range(count)]          # every input under every key, the q - 1 ciphertext first
            g.ct_upload(hout, 0, sentinel)
            d = moved(g, lambda: g.apply_galois_sum(hin, [1 + i for i, _ in pairs], [e for _, e in pairs], [0, count], hout, 1))
            got = g.ct_download(hout, 0, 3)
            assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[2], sentinel[2])
            exp = ref.total(pairs)
            assert np.array_equal(got[1], exp), (count, int((got[1] != exp).sum()))
            assert (d["ks_summed"], d["Rotation"], d["ntt_forward_limbs"], d["ntt_inverse_limbs"], d["kernel_launches"]) == (1, count, count * c.tot * 3, 2 * 3, 2), (count, d)
        g.free(hin)
        g.free(hout)
    finally:
        if c is not small:
            c.close()


def test_steps_form_runs_its_hops_and_counts_them(small):
    """keys for steps 1, -1, -2, -4 (the cell's) and 2, -8: -3 = 1 - 4, -5 = -1 - 4 and -6 = 2 - 8 run two hops each, the first one as a rotation into a
    temporary (it pays its inverse transforms), the last one inside the sum (it does not)"""
    o, g = small.o, small.g
    have = o.galois_elts()
    for s in (2, -8):
        e = o.galois_elt_from_step(s)
        g.set_galois_key(e, o.galois_key(have.index(e)))
    cts = inputs(o, 21)
    steps = [-3, -5, -6, 0, 1]
    ii = [1, 2, 3, 2, 1]
    hin, hout, sentinel = setup(g, cts, 1)
    g.set_option("record_steps", 1)
    d = moved(g, lambda: g.rotate_rows_sum(hin, ii, steps, [0, 5], hout, 1))
    rec, columns = g.rotation_steps()
    g.set_option("record_steps", 0)
    exp = None
    for i, s in zip(ii, steps):
        term = o.rotate_rows(cts[i - 1], s) if s else cts[i - 1]
        exp = term if exp is None else o.add(exp, term)
    got = g.ct_download(hout, 0, 3)
    assert np.array_equal(got[1], exp), int((got[1] != exp).sum())
    assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[2], sentinel[2]) and np.array_equal(g.ct_download(hin, 1, 3), cts)
    k, tot = o.k, small.tot
    # 2 + 2 + 2 + 0 + 1 hops; three of them are not the last of their term; one output
    assert (d["Rotation"], d["ntt_forward_limbs"], d["ntt_inverse_limbs"], d["ks_summed"]) == (7, 7 * tot * k, 3 * 2 * k + 2 * k, 1), d
    assert (d["AddMany"], d["AddManyItemCount"]) == (1, 5), d
    assert (sorted(rec), bool(columns)) == ([-6, -5, -3, 1], False)
    g.free(hin)
    g.free(hout)


def test_the_other_key_switch_convention():
    n, q, w = 1024, list(Q["f64"]), 10
    o = Oracle(n, T, q=q, dbc=w, gdbc=w, ks_xi=True)
    o.keygen(29, galois=True)
    g = Context(n, T, q=q, dbc=w, gdbc=w, device=0)
    try:
        g.set_option("ks_xi", 1)
        have = o.galois_elts()
        for e in (o.galois_elt_from_step(1), o.galois_elt_from_step(-2), 2 * n - 1):
            g.set_galois_key(e, o.galois_key(have.index(e)))
        check_three_groups(o, g, inputs(o, 9), 15)
    finally:
        g.close()


def test_level_context_with_the_sliced_keys(small):
    lo, lv = small.level(2)
    check_three_groups(lo, lv, inputs(lo, 10), 10)          # 49 + 49 bits at width 10: 5 + 5 digits


def test_integer_keys_on_moduli_that_could_run_fp64():
    """ "f64" 0 at upload: the integer kernels on moduli below 2^49"""
    n, q, w = 1024, list(Q["f64l"]), 60
    o = Oracle(n, T, q=q, dbc=w, gdbc=w)
    o.keygen(31, galois=True)
    g = Context(n, T, q=q, dbc=w, gdbc=w, device=0)
    try:
        g.set_option("f64", 0)
        have = o.galois_elts()
        for e in (o.galois_elt_from_step(1), o.galois_elt_from_step(-2), 2 * n - 1):
            g.set_galois_key(e, o.galois_key(have.index(e)))
        check_three_groups(o, g, inputs(o, 11), 3)
        # ... and keys of both forms in one call are refused
        g.set_option("f64", 1)
        e4 = o.galois_elt_from_step(-4)
        g.set_galois_key(e4, o.galois_key(have.index(e4)))
        hin, hout, sentinel = setup(g, inputs(o, 12), 1)
        s0 = g.stats()
        with pytest.raises(CnError) as e:
            g.apply_galois_sum(hin, [1, 2], [o.galois_elt_from_step(1), e4], [0, 2], hout, 1)
        assert e.value.code == ERR_ARG and "different forms" in str(e.value)
        assert np.array_equal(g.ct_download(hout, 0, 3), sentinel) and g.stats()["kernel_launches"] == s0["kernel_launches"]
    finally:
        g.close()


@pytest.mark.parametrize("n, legacy", [(1024, 1), (512, 0)], ids=["legacy_ntt", "n512"])
def test_without_register_radix_kernels_the_call_composes_the_same_words(n, legacy):
    """ "legacy_ntt" (set before the keys are uploaded: they stay 64-bit words) and N < 1024: the literal sequence through a temporary, no error, "ks_summed"
    unchanged"""
    q, w = list(Q["f64"]), 10
    o = Oracle(n, T, q=q, dbc=w, gdbc=w)
    o.keygen(33, galois=True)
    g = Context(n, T, q=q, dbc=w, gdbc=w, device=0)
    try:
        if legacy:
            g.set_option("legacy_ntt", 1)
        e1, cols = o.galois_elt_from_step(1), 2 * n - 1
        have = o.galois_elts()
        for e in (e1, cols):
            g.set_galois_key(e, o.galois_key(have.index(e)))
        cts = inputs(o, 16)
        hin, hout, sentinel = setup(g, cts, 1)
        d = moved(g, lambda: g.apply_galois_sum(hin, [1, 2, 3], [e1, 1, cols], [0, 3], hout, 1))
        got = g.ct_download(hout, 0, 3)
        exp = o.add(o.add(o.apply_galois(cts[0], e1), cts[1]), o.apply_galois(cts[2], cols))
        assert np.array_equal(got[1], exp) and np.array_equal(got[0], sentinel[0]) and np.array_equal(got[2], sentinel[2])
        assert (d["ks_summed"], d["Rotation"], d["AddMany"], d["AddManyItemCount"]) == (0, 2, 1, 3), d
    finally:
        g.close()


def test_every_refusal_leaves_outputs_and_launches_untouched(small):
    o, g, n = small.o, small.g, small.n
    cts = inputs(o, 13)
    hin, hout, sentinel = setup(g, cts, 3)
    h3 = g.ct_alloc(4, 3)
    e1, em2 = o.galois_elt_from_step(1), o.galois_elt_from_step(-2)
    cases = [
        ("no group", ERR_ARG, lambda: g.apply_galois_sum(hin, [], [], [0], hout, 1)),
        ("grp_off does not start at 0", ERR_ARG, lambda: g.apply_galois_sum(hin, [1, 2], [e1, em2], [1, 2], hout, 1)),
        ("an empty group", ERR_ARG, lambda: g.apply_galois_sum(hin, [1, 2], [e1, em2], [0, 2, 2], hout, 1)),
        ("an empty group of steps", ERR_ARG, lambda: g.rotate_rows_sum(hin, [1, 2], [1, -2], [0, 0, 2], hout, 1)),
        ("an input index out of range", ERR_ARG, lambda: g.apply_galois_sum(hin, [1, 4], [e1, em2], [0, 2], hout, 1)),
        ("an output index out of range", ERR_ARG, lambda: g.apply_galois_sum(hin, [1, 2], [e1, em2], [0, 1, 2], hout, 4)),
        ("a size-3 input", ERR_ARG, lambda: g.apply_galois_sum(h3, [1], [e1], [0, 1], hout, 1)),
        ("a size-3 output", ERR_ARG, lambda: g.apply_galois_sum(hin, [1], [e1], [0, 1], h3, 1)),
        ("an output the call reads", ERR_ARG, lambda: g.apply_galois_sum(hout, [1, 3], [e1, 1], [0, 1, 2], hout, 2)),
        ("an output the call reads as a plain addend", ERR_ARG, lambda: g.rotate_rows_sum(hout, [0, 2], [1, 0], [0, 2], hout, 2)),
        ("an even element", ERR_ARG, lambda: g.apply_galois_sum(hin, [1, 2], [e1, 4], [0, 2], hout, 1)),
        ("an element of 2N", ERR_ARG, lambda: g.apply_galois_sum(hin, [1, 2], [e1, 2 * n + 1], [0, 2], hout, 1)),
        ("a step of N / 2", ERR_ARG, lambda: g.rotate_rows_sum(hin, [1, 2], [1, n // 2], [0, 2], hout, 1)),
        ("a step beyond -N / 2", ERR_ARG, lambda: g.rotate_rows_sum(hin, [1, 2], [1, -n], [0, 2], hout, 1)),
        ("an element without its own key", ERR_NOKEY, lambda: g.apply_galois_sum(hin, [1, 2], [e1, o.galois_elt_from_step(-3)], [0, 2], hout, 1)),
        ("a step without a chain", ERR_NOKEY, lambda: g.rotate_rows_sum(hin, [1, 2], [1, 16], [0, 2], hout, 1)),
    ]
    for what, code, call in cases:
        s0, h0 = g.stats(), g.get_option("ks_summed")
        with pytest.raises(CnError) as e:
            call()
        assert e.value.code == code, (what, str(e.value))
        assert g.stats()["kernel_launches"] == s0["kernel_launches"] and g.get_option("ks_summed") == h0, what
        assert np.array_equal(g.ct_download(hout, 0, 5), sentinel), what
    for h in (hin, hout, h3):
        g.free(h)


def test_a_context_with_one_coefficient_modulus_is_refused():
    g = Context(1024, T, q=[Q["f64"][0]], dbc=10, gdbc=10, device=0)
    try:
        hin, hout = g.ct_alloc(2), g.ct_alloc(2)
        s0 = g.stats()
        with pytest.raises(CnError) as e:
            g.rotate_rows_sum(hin, [0, 1], [1, 0], [0, 2], hout, 0)
        assert e.value.code == ERR_ARG and g.stats()["kernel_launches"] == s0["kernel_launches"]
    finally:
        g.close()


def test_recorded_call_launched_twice_gives_the_same_words(small):
    o, g = small.o, small.g
    a, b = inputs(o, 14), inputs(o, 15)
    em1, cols = o.galois_elt_from_step(-1), 2 * o.n - 1
    ii, elts, off = [1, 2, 3, 3], [em1, 1, cols, em1], [0, 3, 4]
    hin, hout, sentinel = setup(g, a, 2)
    g.apply_galois_sum(hin, ii, elts, off, hout, 1)          # once before recording: the arenas have their size
    g.graph_begin()
    g.apply_galois_sum(hin, np.array(ii, dtype=np.uint32), np.array(elts, dtype=np.uint64), np.array(off, dtype=np.uint32), hout, 1)
    graph = g.graph_end()
    for cts in (a, b):                                       # the second launch on other input words: the lists were captured by value, the operands are read anew
        g.ct_upload(hin, 1, cts)
        g.ct_upload(hout, 0, sentinel)
        g.graph_launch(graph)
        got = g.ct_download(hout, 0, 4)
        assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[3], sentinel[3])
        ref = Terms(o, cts)
        assert np.array_equal(got[1], ref.total([(0, em1), (1, 1), (2, cols)])) and np.array_equal(got[2], ref.term(2, em1))
    g.free(graph)
    g.free(hin)
    g.free(hout)


def test_queued_calls_are_submitted_first(small):
    """ "defer" 1: a queued cn_rotate_rows writes the ciphertext the call reads - the queue is flushed, the call runs at once"""
    o, g = small.o, small.g
    cts = inputs(o, 17)
    e = o.galois_elt_from_step(-4)
    hin, hout, _ = setup(g, cts, 1)
    hmid = g.ct_alloc(2)
    g.ct_upload(hmid, 1, cts[1:2])
    g.set_option("defer", 1)
    try:
        g.rotate_rows(hin, 3, 1, hmid, 0)
        assert g.get_option("pending_calls") == 1
        g.apply_galois_sum(hmid, [0, 1], [e, 1], [0, 2], hout, 1)
        assert g.get_option("pending_calls") == 0
    finally:
        g.set_option("defer", 0)
    assert np.array_equal(g.ct_download(hout, 1, 1)[0], o.add(o.apply_galois(o.rotate_rows(cts[2], 1), e), cts[1]))
    for h in (hin, hout, hmid):
        g.free(h)
