"""The forms of the plaintext family (cn_plain_plan.h) seen from the API: the words against the oracle and what every call moves of `kernel_launches`,
`ntt_forward_limbs`, `ntt_inverse_limbs`, `PlainMultiplication`, `ptn_bcast` and `ptn_sum`, at the two smallest cells of tests/size_policy_sets.py and the two
N = 16384 cells (digit width 60) - where the (integer policy, N = 16384) exception and the one-launch SumAllSlots chain live.  The forms give the same words, so
only the counters can tell a wrong pick: the literals of PARENT were recorded on the commit before the planner (profiles/plain_plan_refactor.md), with nothing but
the existing API, and hold unchanged behind it.  A figure is the tuple FIG of differences around the call."""
import numpy as np
import pytest

from cryptonets_amd import diagonal
from size_policy_sets import Cell, edge_words
from test_gpu_mul_plain_sum import expected as sum_expected, plaintexts
from test_gpu_ptn import ntt_form, transformed
from test_gpu_size_policy_matrix import Options, Out, up1

pytestmark = pytest.mark.gpu

FIG = ("kernel_launches", "ntt_forward_limbs", "ntt_inverse_limbs", "PlainMultiplication", "ptn_bcast", "ptn_sum")
CELLS = [("f64", 1024), ("u64", 1024), ("u64", 16384), ("f64", 16384)]
NAMES = ["sp-%s-n%d" % c for c in CELLS]
FORMS = ("coeff", "ntt")
GRP_OFF, IDX = [0, 3, 6], np.array([0, 1, 0, 2, 3, 1], dtype=np.uint32)      # two groups of three terms: repeats, and the sources 0, 1, 2, 3 are one run

# (case, plaintext form) -> FIG, per cell; recorded on the parent commit
PARENT = {
    "sp-f64-n1024": {
        ("diag_encode_3", "ntt"): (5, 14, 3, 0, 0, 0), ("mul_plain_3", "coeff"): (2, 27, 18, 3, 0, 0), ("mul_plain_3", "ntt"): (1, 18, 18, 3, 0, 0),
        ("mul_plain_4", "coeff"): (2, 36, 24, 4, 0, 0), ("mul_plain_4", "ntt"): (1, 24, 24, 4, 0, 0), ("mul_plain_sum", "coeff"): (2, 60, 12, 6, 0, 0),
        ("mul_plain_sum", "ntt"): (2, 24, 12, 6, 0, 1), ("mul_plain_sum_mp_fused_0", "coeff"): (32, 54, 36, 6, 0, 0),
        ("mul_plain_sum_mp_fused_0", "ntt"): (20, 36, 36, 6, 0, 0), ("pt_transform_3", "-"): (1, 9, 0, 0, 0, 0), ("rowdot_3_1", "coeff"): (2, 27, 18, 3, 0, 0),
        ("rowdot_3_1", "ntt"): (1, 18, 18, 3, 0, 0), ("rowdot_3_8", "coeff"): (8, 108, 72, 3, 0, 0), ("rowdot_3_8", "ntt"): (7, 99, 72, 3, 0, 0),
        ("rowdot_4_1", "coeff"): (2, 30, 24, 4, 0, 0), ("rowdot_4_1", "ntt"): (2, 6, 24, 4, 1, 0), ("rowdot_4_8", "coeff"): (8, 138, 96, 4, 0, 0),
        ("rowdot_4_8", "ntt"): (8, 114, 96, 4, 1, 0),
    },
    "sp-u64-n1024": {
        ("mul_plain_3", "coeff"): (2, 27, 18, 3, 0, 0), ("mul_plain_3", "ntt"): (1, 18, 18, 3, 0, 0), ("mul_plain_4", "coeff"): (2, 36, 24, 4, 0, 0),
        ("mul_plain_4", "ntt"): (1, 24, 24, 4, 0, 0), ("mul_plain_sum", "coeff"): (2, 60, 12, 6, 0, 0), ("mul_plain_sum", "ntt"): (2, 24, 12, 6, 0, 1),
        ("pt_transform_3", "-"): (1, 9, 0, 0, 0, 0), ("rowdot_3_1", "coeff"): (2, 27, 18, 3, 0, 0), ("rowdot_3_1", "ntt"): (1, 18, 18, 3, 0, 0),
        ("rowdot_3_8", "coeff"): (8, 108, 72, 3, 0, 0), ("rowdot_3_8", "ntt"): (7, 99, 72, 3, 0, 0), ("rowdot_4_1", "coeff"): (2, 30, 24, 4, 0, 0),
        ("rowdot_4_1", "ntt"): (2, 6, 24, 4, 1, 0), ("rowdot_4_8", "coeff"): (8, 138, 96, 4, 0, 0), ("rowdot_4_8", "ntt"): (8, 114, 96, 4, 1, 0),
    },
    "sp-u64-n16384": {
        ("mul_plain_3", "coeff"): (2, 27, 18, 3, 0, 0), ("mul_plain_3", "ntt"): (1, 18, 18, 3, 0, 0), ("mul_plain_4", "coeff"): (2, 36, 24, 4, 0, 0),
        ("mul_plain_4", "ntt"): (1, 24, 24, 4, 0, 0), ("mul_plain_sum", "coeff"): (14, 54, 36, 6, 0, 0), ("mul_plain_sum", "ntt"): (8, 36, 36, 6, 0, 0),
        ("pt_transform_3", "-"): (1, 9, 0, 0, 0, 0), ("rowdot_3_1", "coeff"): (2, 27, 18, 3, 0, 0), ("rowdot_3_1", "ntt"): (1, 18, 18, 3, 0, 0),
        ("rowdot_3_8", "coeff"): (8, 108, 72, 3, 0, 0), ("rowdot_3_8", "ntt"): (7, 99, 72, 3, 0, 0), ("rowdot_4_1", "coeff"): (2, 30, 24, 4, 0, 0),
        ("rowdot_4_1", "ntt"): (1, 24, 24, 4, 0, 0), ("rowdot_4_8", "coeff"): (8, 138, 96, 4, 0, 0), ("rowdot_4_8", "ntt"): (7, 132, 96, 4, 0, 0),
        ("sum_slots_4_0_wide-1", "-"): (28, 504, 336, 0, 0, 0), ("sum_slots_4_0_wide0", "-"): (28, 504, 336, 0, 0, 0),
        ("sum_slots_4_8_wide-1", "-"): (6, 108, 72, 0, 0, 0), ("sum_slots_4_8_wide0", "-"): (6, 108, 72, 0, 0, 0),
    },
    "sp-f64-n16384": {
        ("mul_plain_3", "coeff"): (2, 27, 18, 3, 0, 0), ("mul_plain_3", "ntt"): (1, 18, 18, 3, 0, 0), ("mul_plain_4", "coeff"): (2, 36, 24, 4, 0, 0),
        ("mul_plain_4", "ntt"): (1, 24, 24, 4, 0, 0), ("mul_plain_sum", "coeff"): (2, 60, 12, 6, 0, 0), ("mul_plain_sum", "ntt"): (2, 24, 12, 6, 0, 1),
        ("pt_transform_3", "-"): (1, 9, 0, 0, 0, 0), ("rowdot_3_1", "coeff"): (2, 27, 18, 3, 0, 0), ("rowdot_3_1", "ntt"): (1, 18, 18, 3, 0, 0),
        ("rowdot_3_8", "coeff"): (8, 108, 72, 3, 0, 0), ("rowdot_3_8", "ntt"): (7, 99, 72, 3, 0, 0), ("rowdot_3_8_ks_wide", "coeff"): (6, 108, 72, 3, 0, 0),
        ("rowdot_3_8_ks_wide", "ntt"): (5, 99, 72, 3, 0, 0), ("rowdot_3_8_ks_wide-ks_chain", "coeff"): (8, 108, 72, 3, 0, 0),
        ("rowdot_3_8_ks_wide-ks_chain", "ntt"): (7, 99, 72, 3, 0, 0), ("rowdot_3_8_ks_wide-mp_bcast", "coeff"): (6, 108, 72, 3, 0, 0),
        ("rowdot_3_8_ks_wide-mp_bcast", "ntt"): (5, 99, 72, 3, 0, 0), ("rowdot_4_1", "coeff"): (2, 30, 24, 4, 0, 0), ("rowdot_4_1", "ntt"): (2, 6, 24, 4, 1, 0),
        ("rowdot_4_8", "coeff"): (8, 138, 96, 4, 0, 0), ("rowdot_4_8", "ntt"): (8, 114, 96, 4, 1, 0), ("rowdot_4_8_ks_wide", "coeff"): (5, 138, 96, 4, 0, 0),
        ("rowdot_4_8_ks_wide", "ntt"): (5, 114, 96, 4, 1, 0), ("rowdot_4_8_ks_wide-ks_chain", "coeff"): (8, 138, 96, 4, 0, 0),
        ("rowdot_4_8_ks_wide-ks_chain", "ntt"): (8, 114, 96, 4, 1, 0), ("rowdot_4_8_ks_wide-mp_bcast", "coeff"): (6, 144, 96, 4, 0, 0),
        ("rowdot_4_8_ks_wide-mp_bcast", "ntt"): (5, 132, 96, 4, 0, 0), ("sum_slots_4_0_wide-1", "-"): (28, 504, 336, 0, 0, 0),
        ("sum_slots_4_0_wide0", "-"): (15, 504, 336, 0, 0, 0), ("sum_slots_4_8_wide-1", "-"): (6, 108, 72, 0, 0, 0),
        ("sum_slots_4_8_wide0", "-"): (4, 108, 72, 0, 0, 0),
    },
}


@pytest.fixture(scope="module")
def cells():
    out = {}
    for name, (policy, n) in zip(NAMES, CELLS):
        c = Cell(policy, n, 60)
        if n == 16384:                                              # SumAllSlots(0) walks every power of two below N / 2: all the oracle's keys
            have = c.o.galois_elts()
            for i, e in enumerate(have):
                if e not in c.elts:
                    c.g.set_galois_key(e, c.o.galois_key(i))
        out[name] = c
    yield out
    for c in out.values():
        c.close()


def figures(g, fn):
    s0, b0 = g.stats(), (g.get_option("ptn_bcast"), g.get_option("ptn_sum"))
    fn()
    s1, b1 = g.stats(), (g.get_option("ptn_bcast"), g.get_option("ptn_sum"))
    return tuple(int(s1[f] - s0[f]) for f in FIG[:4]) + (b1[0] - b0[0], b1[1] - b0[1])


def check(name, case, form, got):
    print("FIGURE %s %s %s %s" % (name, case, form, got))
    assert got == PARENT[name][(case, form)], (name, case, form, got)


def sum_slots_model(o, c, length):
    n = o.n
    ln = length if length else n
    if ln >= n // 2:
        c = o.add(c, o.rotate_columns(c))
        ln = n // 2
    s = 1
    while s < ln:
        c = o.add(c, o.rotate_rows(c, -s))
        s *= 2
    return c


@pytest.mark.parametrize("name", NAMES)
def test_mul_plain_of_3_and_4(cells, name):
    c = cells[name]
    o, g = c.o, c.g
    rng = np.random.default_rng(0x1F0 + c.n)
    pts, cts = plaintexts(o, rng, 4), edge_words(o, rng, 4)
    exp = np.stack([o.multiply_plain(x, p) for x, p in zip(cts, pts)])
    hp, hn = transformed(g, pts)
    ha = up1(g, cts)
    for count in (3, 4):
        for form, (h, first) in zip(FORMS, ((hp, 1), (hn, 2))):
            out = Out(g, o, count, 0x1F1)
            got = figures(g, lambda: g.mul_plain(ha, 1, h, first, out.h, 1, count, pt_stride=1))
            assert np.array_equal(out.words(), exp[:count]), (count, form)
            out.free()
            check(name, "mul_plain_%d" % count, form, got)
    for h in (hp, hn, ha):
        g.free(h)


def rowdot(c, name, case, rows, length, **opt):
    o, g = c.o, c.g
    rng = np.random.default_rng(0x2F0 + c.n + rows)
    pts = plaintexts(o, rng, rows)
    v = edge_words(o, rng, 3)[2]
    exp = np.stack([sum_slots_model(o, o.multiply_plain(v, p), length) for p in pts])
    hp, hn = transformed(g, pts)
    hv = up1(g, v[None, :])
    with Options(g, **opt):
        for form, (h, first) in zip(FORMS, ((hp, 1), (hn, 2))):
            out = Out(g, o, rows, 0x2F1)
            got = figures(g, lambda: g.rowdot_batch(hv, 1, h, first, rows, length, out.h, 1))
            assert np.array_equal(out.words(), exp), (case, form)
            out.free()
            check(name, case, form, got)
    assert np.array_equal(g.ct_download(hv, 1, 1)[0], v)
    for h in (hp, hn, hv):
        g.free(h)


@pytest.mark.parametrize("length", [1, 8])
@pytest.mark.parametrize("rows", [3, 4])
@pytest.mark.parametrize("name", NAMES)
def test_rowdot_batch_either_side_of_the_broadcast_threshold(cells, name, rows, length):
    """at sp-u64-n16384 the NTT-form rows of 4 take the product kernel alone (no wide kernel: `ptn_bcast` stays)"""
    rowdot(cells[name], name, "rowdot_%d_%d" % (rows, length), rows, length)


@pytest.mark.parametrize("opt", ["ks_wide", "ks_wide-ks_chain", "ks_wide-mp_bcast"])
@pytest.mark.parametrize("rows", [3, 4])
def test_rowdot_batch_hands_the_chain_its_first_link(cells, rows, opt):
    """sp-f64-n16384 under "ks_wide" 0: every link is k_keyswitch_pair14, so 4 rows run the chained form (the broadcast kernel leaves the first permuted c1: one
    launch fewer than product + chain); "ks_chain" 0 and "mp_bcast" 0 take it away in two different ways"""
    name = "sp-f64-n16384"
    rowdot(cells[name], name, "rowdot_%d_8_%s" % (rows, opt), rows, 8, **{o: 0 for o in opt.split("-")})


@pytest.mark.parametrize("ks_wide", [-1, 0])
@pytest.mark.parametrize("length", [8, 0])
@pytest.mark.parametrize("name", NAMES[2:])
def test_sum_slots_of_4(cells, name, length, ks_wide):
    """"ks_wide" -1: 4 ciphertexts of 3 limbs take the two-launch key switch, no chain; 0: the one-launch chain at sp-f64-n16384 (a permutation pass in front)"""
    c = cells[name]
    o, g = c.o, c.g
    X = edge_words(o, np.random.default_rng(0x3F0 + length), 4)
    exp = np.stack([sum_slots_model(o, x, length) for x in X])
    out = Out(g, o, 4, 0x3F1)
    g.ct_upload(out.h, 1, X)
    with Options(g, ks_wide=ks_wide):
        got = figures(g, lambda: g.sum_slots(out.h, 1, 4, length))
    assert np.array_equal(out.words(), exp)
    out.free()
    check(name, "sum_slots_4_%d_wide%d" % (length, ks_wide), "-", got)


def plain_sum(c, name, case, **opt):
    o, g = c.o, c.g
    rng = np.random.default_rng(0x4F0 + c.n)
    pts, cts = plaintexts(o, rng, 6), edge_words(o, rng, 4)
    exp = sum_expected(o, cts, pts, GRP_OFF, IDX)
    hp, hn = transformed(g, pts)
    ha = up1(g, cts)
    with Options(g, **opt):
        for form, (h, first) in zip(FORMS, ((hp, 1), (hn, 2))):
            out = Out(g, o, 2, 0x4F1)
            got = figures(g, lambda: g.mul_plain_sum(ha, 1, h, first, GRP_OFF, IDX, out.h, 1))
            assert np.array_equal(out.words(), exp), (case, form)
            out.free()
            check(name, case, form, got)
    assert np.array_equal(g.ct_download(ha, 1, 4), cts)
    for h in (hp, hn, ha):
        g.free(h)


@pytest.mark.parametrize("name", NAMES)
def test_mul_plain_sum_kernel_and_composed(cells, name):
    """the kernel at three cells, composed (cn_mul_plain per term + k_add_many) at sp-u64-n16384"""
    plain_sum(cells[name], name, "mul_plain_sum")


def test_mul_plain_sum_composed_under_mp_fused_0(cells):
    plain_sum(cells[NAMES[0]], NAMES[0], "mul_plain_sum_mp_fused_0", mp_fused=0)


@pytest.mark.parametrize("name", NAMES)
def test_pt_transform_of_3(cells, name):
    c = cells[name]
    o, g = c.o, c.g
    pts = plaintexts(o, np.random.default_rng(0x5F0 + c.n), 3)
    hp, hn = g.pt_alloc(4), g.ptn_alloc(6)
    g.pt_upload(hp, 1, pts)
    got = figures(g, lambda: g.pt_transform(hp, 1, 3, hn, 2))
    words = g.ptn_download(hn, 2, 3)
    exp = ntt_form(o, pts)
    assert np.array_equal(words, exp)
    for h in (hp, hn):
        g.free(h)
    check(name, "pt_transform_3", "-", got)


def test_diag_encode_into_ntt_form_is_encode_then_pt_transform(cells):
    name = NAMES[0]
    g = cells[name].g
    W = np.random.default_rng(0x6F0).integers(0, g.t, size=(5, 40))
    terms = [(0, 0, 0), (0, 0, 1), (1, 0, 3)]
    rows = g.pt_alloc(7)
    g.encode_batch(np.zeros((7, 1), dtype=np.uint64), rows, 0)
    g.encode_batch(np.ascontiguousarray(W, dtype=np.uint64), rows, 1)
    ref, want, out = g.pt_alloc(3), g.ptn_alloc(3), g.ptn_alloc(5)
    g.encode_batch(diagonal.pre_rotated_rows(W, g.n, terms).astype(np.uint64), ref, 0)
    g.pt_transform(ref, 0, 3, want, 0)
    got = figures(g, lambda: g.diag_encode(rows, 1, 5, 40, terms, out, 1))
    assert np.array_equal(g.ptn_download(out, 1, 3), g.ptn_download(want, 0, 3))
    for h in (rows, ref, want, out):
        g.free(h)
    check(name, "diag_encode_3", "ntt", got)
