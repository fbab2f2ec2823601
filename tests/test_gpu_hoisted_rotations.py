"""GPU: the hoisted rotations (cn_rotate_rows_hoisted / cn_apply_galois_hoisted: k_ks_digit_ntt + k_ks_hoist_mac) word for word against the integer model of
tests/hoisted_model.py - NOT against the oracle's rotations, whose words differ (SEAL permutes c1 before it cuts digits); the plaintext is the same and is checked
on a fresh encryption against cn_rotate_rows.

Cells of tests/size_policy_sets.py: all five ring sizes x three policies at width 60 with n = 3 (a row step, a negative step, the column swap), width 10 at
(u64, 1024), (f64, 8192), (f64l, 16384) and (f64, 16384).  Inputs: edge_words (the residues 0, 1, (q - 1) / 2, (q + 1) / 2, q - 1 in every limb, and q - 1
everywhere) and uniform words - the contract holds for any words, so full-range digits and the reduction of digits 2^gdbc > q_j are exercised (width 60: a 60-bit
digit of limb 0 against the 36-bit modulus of f64l).  (u64, 16384) is refused by the planner's predicate (cn_ks_hoist_built): asserted as a refusal.
Beside the cells: the other key-switch convention ("ks_xi" 1), a level context with the sliced keys, twelve rotations at k = 3 (more than the 32 / k rounds of
cn_rotate_rows_many), keys kept as 64-bit words on moduli that could run FP64, every refusal (outputs and `kernel_launches` unchanged), the closed forms of the
counters, a recorded call launched twice, and the deferred queue flushed in front of the call."""
import numpy as np
import pytest

from cryptonets_amd._native import CnError, Context
from hoisted_model import hoisted
from oracle.cno import Oracle
from size_policy_sets import CELLS, Q, T, Cell, edge_words, uniform

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOKEY = -1, -3
WIDE = [(p, n, 60) for p, n in CELLS]
NARROW = [("u64", 1024, 10), ("f64", 8192, 10), ("f64l", 16384, 10), ("f64", 16384, 10)]
REFUSED = ("u64", 16384)                                    # cn_ks_hoist_built: no kernel under the integer policy at N = 16384


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


def key_of(o, e):
    return o.galois_key(o.galois_elts().index(e))


def inputs(o, seed):
    """[edge residues cycling, q - 1 everywhere, uniform]"""
    rng = np.random.default_rng(seed)
    return np.concatenate([edge_words(o, rng, 2), uniform(o, rng, 1)])


def setup(g, cts, outputs):
    """the inputs at index 1 .. of their handle; `outputs` + 2 sentinel ciphertexts (first and last must keep their words)"""
    o_words = cts.shape[1]
    hin = g.ct_alloc(len(cts) + 1)
    g.ct_upload(hin, 1, cts)
    rng = np.random.default_rng(len(cts) * 1000 + outputs)
    sentinel = np.stack([rng.integers(0, 1 << 30, size=o_words, dtype=np.uint64) for _ in range(outputs + 2)])
    hout = g.ct_alloc(outputs + 2)
    g.ct_upload(hout, 0, sentinel)
    return hin, hout, sentinel


def moved(g, fn):
    s0, h0 = g.stats(), g.get_option("ks_hoisted")
    fn()
    s1 = g.stats()
    d = {k: s1[k] - s0[k] for k in s1}
    d["ks_hoisted"] = g.get_option("ks_hoisted") - h0
    return d


def check_words(o, g, elts, cts, tot, xi=False):
    """every input rotated by every element of `elts`, in one call per input: the model's words, the sentinels untouched, the counters' closed forms"""
    n_rot = len(elts)
    hin, hout, sentinel = setup(g, cts, n_rot)
    order = list(range(n_rot, 0, -1))                       # outputs in descending order: oi is a list, not a range
    for i, ct in enumerate(cts):
        d = moved(g, lambda: g.apply_galois_hoisted(hin, 1 + i, elts, hout, order))
        got = g.ct_download(hout, 0, n_rot + 2)
        assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[-1], sentinel[-1]), "a ciphertext beside the outputs changed"
        for r, e in enumerate(elts):
            exp = hoisted(o, ct, e, key_of(o, e), ks_xi=xi)
            assert np.array_equal(got[order[r]], exp), ("input %d, element %d" % (i, e), int((got[order[r]] != exp).sum()))
        # tot k forward transforms ONCE, 2 k inverse ones per rotation, two launches: a loop of plain rotations runs n (tot k + 2 k) transforms
        assert (d["ntt_forward_limbs"], d["ntt_inverse_limbs"], d["kernel_launches"], d["Rotation"], d["ks_hoisted"]) == (tot * o.k, n_rot * 2 * o.k, 2, n_rot, 1), d
        assert np.array_equal(g.ct_download(hin, 1 + i, 1)[0], ct), "the input changed"
    g.free(hin)
    g.free(hout)


def test_words_equal_the_model_in_every_cell(cell):
    o, g = cell.o, cell.g
    elts = [o.galois_elt_from_step(1), o.galois_elt_from_step(-2), 2 * o.n - 1]
    cts = inputs(o, 0x51 + cell.n + cell.width)
    if (cell.policy, cell.n) == REFUSED:
        hin, hout, sentinel = setup(g, cts, 3)
        s0 = g.stats()
        with pytest.raises(CnError) as e:
            g.apply_galois_hoisted(hin, 1, elts, hout, [1, 2, 3])
        assert e.value.code == ERR_ARG and "integer policy at N = 16384" in str(e.value)
        assert np.array_equal(g.ct_download(hout, 0, 5), sentinel) and g.stats()["kernel_launches"] == s0["kernel_launches"]
        g.free(hin)
        g.free(hout)
        return
    check_words(o, g, elts, cts, cell.tot)


def test_steps_form_maps_through_the_element_and_step_zero_copies(small):
    o, g = small.o, small.g
    cts = inputs(o, 7)[2:]
    hin, hout, sentinel = setup(g, cts, 3)
    d = moved(g, lambda: g.rotate_rows_hoisted(hin, 1, [-4, 0, 1], hout, [1, 2, 3]))
    got = g.ct_download(hout, 0, 5)
    assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[4], sentinel[4])
    for r, s in ((1, -4), (3, 1)):
        e = o.galois_elt_from_step(s)
        assert np.array_equal(got[r], hoisted(o, cts[0], e, key_of(o, e)))
    assert np.array_equal(got[2], cts[0])                   # step 0: a copy, no rotation counted
    assert (d["ntt_forward_limbs"], d["ntt_inverse_limbs"], d["kernel_launches"], d["Rotation"], d["ks_hoisted"]) == (small.tot * 3, 2 * 2 * 3, 2, 2, 1)
    # element 1 alone: copies only, no kernel of the key switch
    d = moved(g, lambda: g.apply_galois_hoisted(hin, 1, [1], hout, [2]))
    assert np.array_equal(g.ct_download(hout, 2, 1)[0], cts[0]) and (d["kernel_launches"], d["ks_hoisted"], d["ntt_forward_limbs"]) == (0, 0, 0)
    g.free(hin)
    g.free(hout)


def test_recorded_steps(small):
    g = small.g
    cts = inputs(small.o, 8)[2:]
    hin, hout, _ = setup(g, cts, 3)
    g.set_option("record_steps", 1)
    g.rotate_rows_hoisted(hin, 1, [-4, 0, 1], hout, [1, 2, 3])
    g.apply_galois_hoisted(hin, 1, [small.o.galois_elt_from_step(-2), 2 * small.n - 1, 1], hout, [1, 2, 3])
    steps, columns = g.rotation_steps()
    g.set_option("record_steps", 0)
    assert (sorted(steps), bool(columns)) == ([-4, -2, 1], True)
    g.free(hin)
    g.free(hout)


def test_the_other_key_switch_convention():
    n, q, w = 1024, list(Q["f64"]), 10
    o = Oracle(n, T, q=q, dbc=w, gdbc=w, ks_xi=True)
    o.keygen(29, galois=True)
    g = Context(n, T, q=q, dbc=w, gdbc=w, device=0)
    try:
        g.set_option("ks_xi", 1)
        elts = [o.galois_elt_from_step(2), o.galois_elt_from_step(-1), 2 * n - 1]
        for e in elts:
            g.set_galois_key(e, key_of(o, e))
        check_words(o, g, elts, inputs(o, 9)[[0, 2]], 15, xi=True)
    finally:
        g.close()


def test_level_context_with_the_sliced_keys(small):
    lo, lv = small.level(2)
    elts = [lo.galois_elt_from_step(-1), 2 * small.n - 1, lo.galois_elt_from_step(-4)]
    check_words(lo, lv, elts, inputs(lo, 10)[[0, 2]], 10)    # 49 + 49 bits at width 10: 5 + 5 digits


def test_twelve_rotations_of_one_ciphertext_and_integer_keys():
    """n = 12 at k = 3 (more than the 32 / k rounds of cn_rotate_rows_many) with extra keys of the oracle's default set; the same with the keys kept as 64-bit
    words ("f64" 0 at upload: the integer kernels on moduli below 2^49)"""
    n, q, w = 1024, list(Q["f64l"]), 60
    o = Oracle(n, T, q=q, dbc=w, gdbc=w)
    o.keygen(31, galois=True)
    elts = [e for e in o.galois_elts() if e != 2 * n - 1][:11] + [2 * n - 1]
    assert len(set(elts)) == 12
    cts = inputs(o, 11)[[0, 2]]
    for f64 in (1, 0):
        g = Context(n, T, q=q, dbc=w, gdbc=w, device=0)
        try:
            g.set_option("f64", f64)
            for e in elts:
                g.set_galois_key(e, key_of(o, e))
            check_words(o, g, elts, cts, 3)
        finally:
            g.close()


def test_fresh_encryption_decrypts_to_the_slots_of_rotate_rows(small):
    o, g = small.o, small.g
    rng = np.random.default_rng(12)
    ct = o.encrypt(o.encode(rng.integers(0, T, size=o.n, dtype=np.uint64)))
    hin, hout, _ = setup(g, ct[None, :], 3)
    href = g.ct_alloc(3)
    steps = [1, -2, -4]
    g.rotate_rows_hoisted(hin, 1, steps, hout, [1, 2, 3])
    for r, s in enumerate(steps):
        g.rotate_rows(hin, 1, s, href, r)
    got, ref = g.ct_download(hout, 1, 3), g.ct_download(href, 0, 3)
    for r in range(3):
        assert not np.array_equal(got[r], ref[r])           # other words ...
        assert np.array_equal(o.decode(o.decrypt(got[r])), o.decode(o.decrypt(ref[r])))      # ... the same slots
    for h in (hin, hout, href):
        g.free(h)


def test_every_refusal_leaves_outputs_and_launches_untouched(small):
    o, g, n = small.o, small.g, small.n
    cts = inputs(o, 13)[2:]
    hin, hout, sentinel = setup(g, cts, 3)
    h3 = g.ct_alloc(2, 3)
    e1, em2 = o.galois_elt_from_step(1), o.galois_elt_from_step(-2)
    cases = [
        ("a step of N / 2", ERR_ARG, lambda: g.rotate_rows_hoisted(hin, 1, [1, n // 2], hout, [1, 2])),
        ("a step beyond -N / 2", ERR_ARG, lambda: g.rotate_rows_hoisted(hin, 1, [1, -n], hout, [1, 2])),
        ("an even element", ERR_ARG, lambda: g.apply_galois_hoisted(hin, 1, [e1, 4], hout, [1, 2])),
        ("an element of 2N", ERR_ARG, lambda: g.apply_galois_hoisted(hin, 1, [e1, 2 * n + 1], hout, [1, 2])),
        ("an empty list", ERR_ARG, lambda: g.apply_galois_hoisted(hin, 1, [], hout, [])),
        ("an empty list of steps", ERR_ARG, lambda: g.rotate_rows_hoisted(hin, 1, [], hout, [])),
        ("an output index listed twice", ERR_ARG, lambda: g.apply_galois_hoisted(hin, 1, [e1, em2], hout, [2, 2])),
        ("an output index out of range", ERR_ARG, lambda: g.apply_galois_hoisted(hin, 1, [e1, em2], hout, [1, 5])),
        ("an input index out of range", ERR_ARG, lambda: g.apply_galois_hoisted(hin, 2, [e1], hout, [1])),
        ("a size-3 input", ERR_ARG, lambda: g.apply_galois_hoisted(h3, 0, [e1], hout, [1])),
        ("a size-3 output", ERR_ARG, lambda: g.apply_galois_hoisted(hin, 1, [e1], h3, [1])),
        ("an output that is the input", ERR_ARG, lambda: g.apply_galois_hoisted(hout, 1, [e1, em2], hout, [2, 1])),
        ("a step without its own key", ERR_NOKEY, lambda: g.rotate_rows_hoisted(hin, 1, [1, 3], hout, [1, 2])),      # 3 = 4 - 1 in hops: refused, not split
        ("an element without a key", ERR_NOKEY, lambda: g.apply_galois_hoisted(hin, 1, [e1, o.galois_elt_from_step(8)], hout, [1, 2])),
    ]
    for what, code, call in cases:
        s0, h0 = g.stats(), g.get_option("ks_hoisted")
        with pytest.raises(CnError) as e:
            call()
        assert e.value.code == code, (what, str(e.value))
        assert g.stats()["kernel_launches"] == s0["kernel_launches"] and g.get_option("ks_hoisted") == h0, what
        assert np.array_equal(g.ct_download(hout, 0, 5), sentinel), what
    # "legacy_ntt": no register-radix kernels
    g.set_option("legacy_ntt", 1)
    try:
        with pytest.raises(CnError) as e:
            g.apply_galois_hoisted(hin, 1, [e1], hout, [1])
        assert e.value.code == ERR_ARG and np.array_equal(g.ct_download(hout, 0, 5), sentinel)
    finally:
        g.set_option("legacy_ntt", 0)
    for h in (hin, hout, h3):
        g.free(h)


def test_recorded_call_launched_twice_gives_the_same_words(small):
    o, g = small.o, small.g
    cts = inputs(o, 14)[[0, 2]]
    elts = [o.galois_elt_from_step(-1), 2 * o.n - 1, 1]
    hin, hout, sentinel = setup(g, cts[:1], 3)
    order = [3, 1, 2]
    g.apply_galois_hoisted(hin, 1, elts, hout, order)        # once before recording: the arenas have their size
    exp = [hoisted(o, c, e, None if e == 1 else key_of(o, e)) for c in cts for e in elts]
    g.graph_begin()
    g.apply_galois_hoisted(hin, 1, np.array(elts, dtype=np.uint64), hout, np.array(order, dtype=np.uint32))
    graph = g.graph_end()
    for lap, first in ((0, 0), (1, 3)):                     # the second launch on other input words: the lists were captured by value, the operands are read anew
        g.ct_upload(hin, 1, cts[lap:lap + 1])
        g.ct_upload(hout, 0, sentinel)
        g.graph_launch(graph)
        got = g.ct_download(hout, 0, 5)
        assert np.array_equal(got[0], sentinel[0]) and np.array_equal(got[4], sentinel[4])
        for r in range(3):
            assert np.array_equal(got[order[r]], exp[first + r]), (lap, r)
    g.free(graph)
    g.free(hin)
    g.free(hout)


def test_queued_calls_are_submitted_first(small):
    """ "defer" 1: a queued cn_rotate_rows writes the ciphertext the hoisted call reads - the queue is flushed, the call runs at once"""
    o, g = small.o, small.g
    ct = inputs(o, 15)[2]
    e = o.galois_elt_from_step(-4)
    hin, hout, sentinel = setup(g, ct[None, :], 1)
    hmid = g.ct_alloc(1)
    g.set_option("defer", 1)
    try:
        g.rotate_rows(hin, 1, 1, hmid, 0)
        assert g.get_option("pending_calls") == 1
        g.apply_galois_hoisted(hmid, 0, [e], hout, [1])
        assert g.get_option("pending_calls") == 0
    finally:
        g.set_option("defer", 0)
    assert np.array_equal(g.ct_download(hout, 1, 1)[0], hoisted(o, o.rotate_rows(ct, 1), e, key_of(o, e)))
    for h in (hin, hout, hmid):
        g.free(h)
