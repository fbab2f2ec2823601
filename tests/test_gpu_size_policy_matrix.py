"""GPU: every size-templated kernel family at every ring size N = 1024 .. 16384 under every arithmetic policy (ArU64, ArF64, ArF64L; cn_policy.h) and at two
digit widths, word for word against the CPU oracle (oracle/cno.py).  The three policies write the same words: every comparison is np.array_equal.

A cell is (policy, N, width) of tests/size_policy_sets.py: 3 x 5 x 2 = 30 module-scoped fixtures (oracle, context, keys), each closed before the next opens.
Every family below runs in every cell with the smallest shapes that reach every branch; handles are used at non-zero offsets, outputs lie between sentinel
ciphertexts that must keep their words, and the operands carry the edge residues 0, 1, (q - 1) / 2, (q + 1) / 2 and q - 1 (edge_words; inputs() of
test_square_gemm inside the reused helpers).  The helpers of the other modules are reused where they take an (oracle, context) pair; check_rowdot of
test_gpu_ptn looks its context up by name in conftest.PARAMS, so the row-dot family restates it here on the cell's own context - and compares every row with
the oracle's chain, not only the first.

FORM - which form of a call must run in a cell - is written by hand below from cn_policy.h, cn_ks_plan.h (the key switch: ks_form), cn_mul_plan.h (the gates of family f) and the launchers and asserted through the library's counters, so a
silent fall-back cannot pass as coverage:
  kernel     the size-templated kernel (named in the rule)
  composed   other calls of the library do the work (named in the rule)
  literal    the literal two-step sequence inside the same call
No cell of this matrix is refused by the library: every call has some form at every (policy, N).

Coverage before this module, read from the tests, and what is new.  The sets the suite had, by ring and policy of their q range:
    1024   U64, F64, F64L   Q_POLICY of test_gpu_mul_plain_sum / test_gpu_ptn (no keys); B44 .. B60, W60d, WIDE of test_gpu_wide_moduli; "tiny" (F64L)
    2048   U64, F64L        S2048 (one limb), MIX2048, F2048 of test_gpu_wide_moduli
    4096   U64, F64L        W60 of test_gpu_wide_moduli; default4096 and the 37-bit sets of test_digit_sums_i32
    8192   F64L             c2, c3, c4
    16384  F64              c5, n16k7 (dbc 60: the WHOLE form of k_keyswitch_pair14 only)
and U64 by the option "f64" = 0 on FP64-capable moduli (test_gpu_evaluator: transforms, products, rotations on "tiny", c3, c4; the broadcast product on n16k7;
cn_mul_plain_sum composed on c5).  ArF64 (45 - 49 bits) therefore ran at N = 1024 and 16384 only, and nothing ran (16384, F64L).
  family: kernels (launcher)                                 ran before                                                      new cells
  a  k_ntt_rr (cn_l_rr.inc.h)                                 every set above (test_gpu_wide_moduli, test_gpu_evaluator)      F64 at 2048, 4096, 8192; U64 by moduli at 8192,
                                                                                                                              16384; F64L at 16384
  b  k_intt_tensor, k_square_fused, k_square_pipe             test_gpu_wide_moduli (MULTI sets, "ks_wide" 0 .. 2),            the same cells; "sq_lds" / "sq_pipe" forms off
     (cn_l_rr.inc.h); k_keyswitch_rr, k_ks_digit_mac,         test_gpu_mul_relin_paths ("tiny", c3), test_gpu_evaluator       F64L; the LDS-twiddle key switch on F64 and at
     k_ks_limb_mac, k_ks_sum_intt, k_keyswitch_pair14                                                                         2048, 4096; pair14 multi-digit and on F64L
     (cn_l_ks.inc.h)
  c  rotations through the same key switch                    test_gpu_wide_moduli (rows, columns, sum_slots; MULTI sets),    as b; cn_rotate_rows_many / cn_rotate_rows_add on
                                                              test_gpu_evaluator ("tiny", c4, c5: rows_many, rows_add)        every cell but (1024, F64L), (8192, F64L), (16384, F64)
  d  k_lift_ntt, k_mul_plain_fused, k_mul_plain_bcast<.., ptn> test_gpu_ptn (transform: 1024 x 3, c3, c5; products on NTT     NTT-form products and rows on every cell but
     (cn_l_rr.inc.h)                                          form: "tiny"; rowdot on NTT rows: "tiny", c5)                   (1024, F64L); rowdot on NTT rows but those two
  e  k_mul_plain_sum (cn_l_diag.hip), k_mul_ptn_sum           test_gpu_mul_plain_sum, test_gpu_ptn: 1024 x 3, c3, c5,         2048 and 4096 x 3; 8192 x {U64, F64}; 16384 x F64L;
     (cn_l_ptn.hip)                                           (16384, U64 by option) composed; a recentring at 1024           a recentring inside the kernel at every F64 size
  f  cn_square_gemm, cn_mul_relin_sum: k_digit_gemm(_mfma),   test_square_gemm, test_gpu_mul_relin_sum ("tiny", c3),          2048; ArF64 at every size (digit GEMM off the
     k_product_sum, the KsDigits key switch (cn_l_ks.inc.h)   test_digit_sums_i32 (37-bit sets at 1024, 4096; c3)             matrix cores); the literal form at 16384, on U64
  g  k_mod_switch, k_mod_switch_f64 (not size-templated);     test_gpu_mod_switch ("tiny" .. n16k7), test_gpu_wide_moduli     calls on a level at 2048; U64 / F64 levels at
     the calls above on a level context                       (W60)                                                           8192; F64L at 16384
The issue's reading is confirmed: no call of d - f ran at N = 2048 or on an ArF64 set between 2048 and 8192, and nothing ran at (16384, F64L).  One addition: ArF64
ran nowhere between 2048 and 8192 for families a - c either.
Per launcher with a `case 10 .. 14` switch, the tests here that run it at all five sizes under each policy it is instantiated for: cn_l_rr.inc.h (ntt, intt_tensor,
mul_plain_fused, mul_plain_bcast: 3 policies; square_fused: FP64) - test_a_transforms, test_b_mul_relin_in_every_key_switch_and_squaring_form,
test_d_mul_plain_on_both_plaintext_forms, test_d_rowdot_batch_on_both_plaintext_forms, test_d_pt_transform; cn_l_ks.inc.h (launch: 3 policies) - the test_b,
test_c_rotations and test_f tests; cn_l_diag.hip - test_e_mul_plain_sum_on_both_plaintext_forms (coefficient form; U64 at 16384 has no instantiation: composed);
cn_l_ptn.hip - the same test on the NTT form and test_e_recentring_inside_the_fp64_sum_kernel.  The encryption launchers of cn_l_rr.inc.h are out of scope here.

Modulus switch: the issue asks for 3 -> 2 limbs "with the FP64 form and with the integer form".  A single drop never takes the FP64 form (cn_ms_f64_pair,
cn_l_modswitch.hip: two or more primes), so 3 -> 2 asserts the integer form in every cell and 3 -> 1 runs both forms where the FP64 one exists.
"""
import numpy as np
import pytest

from modswitch_model import switch_residues
from size_policy_sets import CELLS, DIGITS, STEPS, WIDTHS, Cell, edge_words, uniform
from test_digit_sums_i32 import Case
from test_gpu_mul_plain_sum import main_lists, plaintexts, run as run_coeff_sum
from test_gpu_mul_relin_sum import expected as relin_sum_expected, literal as relin_sum_literal, operands as relin_sum_operands, run as run_relin_sum
from test_gpu_ptn import check_transform, run_sum, transformed
from test_gpu_wide_moduli import edges
from test_square_gemm import inputs, res

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ the table, by hand
FP64 = ("f64", "f64l")


def ks_form(policy, n, width, ks_wide):
    """the kernels of one key switch (cn_ks_plan, cn_ks_plan.h; launched by cn_l_ks.inc.h) under "ks_wide" 0, 1, 2"""
    if ks_wide == 1:
        return "k_ks_digit_mac + k_ks_sum_intt"                     # launch_two_phase, a workgroup per digit
    if ks_wide == 2:
        return "k_ks_limb_mac + k_ks_sum_intt"                      # launch_two_phase, a workgroup per source limb
    if n == 16384 and policy in FP64:                               # KS_PAIR14; KsPlan::whole: one digit per limb that covers the limb
        return "k_keyswitch_pair14<WHOLE>" if width == 60 else "k_keyswitch_pair14"
    if n <= 8192 and policy in FP64 and DIGITS[policy][width] >= 12:
        return "k_keyswitch_rr<TWL>"                                # KsPlan::twl: KsFwd<AR, L>::lds and KS_TWL_MIN_DIGITS = 12
    return "k_keyswitch_rr"


def form(family, policy, n, width):
    """(form, the rule it comes from)"""
    if family in ("ntt", "mul_plain", "pt_transform", "mul_relin", "rotate", "mod_switch"):
        return "kernel", "a kernel at every register-radix size and policy (BY_SIZE, cn_l_rr.inc.h; launch, cn_l_ks.inc.h)"
    if family in ("mul_plain_sum", "mul_ptn_sum"):
        if policy == "u64" and n == 16384:
            return "composed", "cn_plain_wide (cn_policy.h) through plain_sum_plan (cn_plain_plan.h): cn_mul_plain per term + k_add_many"
        return "kernel", "k_mul_plain_sum<L, AR> / k_mul_ptn_sum<L, AR, 2, WS, D>"
    if family == "ptn_bcast":
        if policy == "u64" and n == 16384:
            return "composed", "cn_plain_wide (cn_policy.h) through cn_plain_plan (cn_plain_plan.h): k_mul_plain_fused alone on the NTT-form rows"
        return "kernel", "k_mul_plain_bcast<L, AR, true>"
    if family in ("square_gemm", "mul_relin_sum"):
        if policy in FP64 and n <= 8192 and width == 10:
            return "kernel", "square_gemm_ctx_ok (cn_mul_plan.h: FP64 policy, N <= 8192) and digit width <= 30 / 31 bits: one key switch per output"
        return "literal", "square_gemm_ctx_ok / GemmPlan::dig (dbc <= 30) / mul_sum_fused_ok (dbc <= 31; cn_mul_plan.h) fail: cn_mul_relin + GEMM or AddMany"
    raise KeyError(family)


FAMILIES = ("ntt", "mul_plain", "pt_transform", "mul_relin", "rotate", "mod_switch", "mul_plain_sum", "mul_ptn_sum", "ptn_bcast", "square_gemm", "mul_relin_sum")
ALL = [(p, n, w) for p, n in CELLS for w in WIDTHS]
FORM = {(f,) + c: form(f, *c)[0] for f in FAMILIES for c in ALL}
assert len(ALL) == 30 and len(FORM) == 330
# the table's corners, spelt out
assert FORM[("mul_plain_sum", "u64", 16384, 60)] == FORM[("mul_ptn_sum", "u64", 16384, 10)] == FORM[("ptn_bcast", "u64", 16384, 10)] == "composed"
assert FORM[("mul_ptn_sum", "u64", 8192, 10)] == FORM[("mul_plain_sum", "f64l", 16384, 60)] == FORM[("ptn_bcast", "f64", 16384, 60)] == "kernel"
assert [FORM[("square_gemm", "f64", n, 10)] for n in (1024, 2048, 4096, 8192, 16384)] == ["kernel"] * 4 + ["literal"]
assert FORM[("mul_relin_sum", "f64l", 4096, 60)] == FORM[("square_gemm", "u64", 1024, 10)] == "literal" and FORM[("mul_relin_sum", "f64l", 2048, 10)] == "kernel"
assert [ks_form("f64", 4096, w, 0) for w in WIDTHS] == ["k_keyswitch_rr", "k_keyswitch_rr<TWL>"] and ks_form("u64", 4096, 10, 0) == "k_keyswitch_rr"
assert [ks_form("f64l", 16384, w, 0) for w in WIDTHS] == ["k_keyswitch_pair14<WHOLE>", "k_keyswitch_pair14"] and ks_form("u64", 16384, 10, 0) == "k_keyswitch_rr"


@pytest.fixture(scope="module", params=ALL, ids=lambda c: "%s-n%d-w%d" % c)
def cell(request):
    c = Cell(*request.param)
    yield c
    c.close()


def key(c):
    return (c.policy, c.n, c.width)


# ------------------------------------------------------------------ plumbing
class Out:
    """`count` output ciphertexts at index 1 of a handle of count + 2: the first and the last are sentinels"""

    def __init__(self, g, o, count, seed, size=2):
        self.g, self.count, self.size = g, count, size
        self.sentinel = uniform(o, np.random.default_rng(seed), count + 2, size)
        self.h = g.ct_alloc(count + 2, size)
        g.ct_upload(self.h, 0, self.sentinel)

    def words(self):
        got = self.g.ct_download(self.h, 0, self.count + 2, self.size)
        assert np.array_equal(got[0], self.sentinel[0]) and np.array_equal(got[-1], self.sentinel[-1]), "a ciphertext beside the written range changed"
        return got[1:-1]

    def free(self):
        self.g.free(self.h)


def up1(g, cts, size=2):
    """the ciphertexts at index 1 of their handle"""
    h = g.ct_alloc(len(cts) + 1, size)
    g.ct_upload(h, 1, cts)
    return h


class Options:
    """set options for a block, put the earlier values back behind it"""

    def __init__(self, g, **opt):
        self.g, self.opt = g, opt

    def __enter__(self):
        self.old = {k: self.g.get_option(k) for k in self.opt}
        for k, v in self.opt.items():
            self.g.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.g.set_option(k, v)


def delta(g, fn):
    """(result of fn, what stats() moved by)"""
    s0 = g.stats()
    r = fn()
    s1 = g.stats()
    return r, {k: s1[k] - s0[k] for k in s1}


# ------------------------------------------------------------------ a. transforms
def test_a_transforms(cell):
    o, g = cell.o, cell.g
    assert FORM[("ntt",) + key(cell)] == "kernel"
    cts = edge_words(o, np.random.default_rng(0xA0 + cell.n), 2)
    out = Out(g, o, 2, 0xA1)
    g.ct_upload(out.h, 1, cts)
    _, d = delta(g, lambda: g.ct_ntt(out.h, 1, 2))
    exp = np.stack([np.concatenate([o.ntt_fwd(j % o.k, c.reshape(2 * o.k, o.n)[j]) for j in range(2 * o.k)]) for c in cts])
    assert np.array_equal(out.words(), exp)
    assert (d["kernel_launches"], d["ntt_forward_limbs"], d["ntt_inverse_limbs"]) == (1, 2 * 2 * o.k, 0)      # k_ntt_rr<L, AR, false>, one launch
    inv = np.stack([np.concatenate([o.ntt_inv(j % o.k, c.reshape(2 * o.k, o.n)[j]) for j in range(2 * o.k)]) for c in cts])
    g.ct_upload(out.h, 1, cts)
    _, d = delta(g, lambda: g.ct_ntt(out.h, 1, 2, inverse=True))
    assert np.array_equal(out.words(), inv)
    assert (d["kernel_launches"], d["ntt_forward_limbs"], d["ntt_inverse_limbs"]) == (1, 0, 2 * 2 * o.k)
    g.ct_ntt(out.h, 1, 2)                                           # and back
    assert np.array_equal(out.words(), cts)
    out.free()


# ------------------------------------------------------------------ b. products and key switch
def test_b_mul_relin_in_every_key_switch_and_squaring_form(cell):
    """3 products a != b and 3 squarings under "ks_wide" 0, 1, 2; the squarings on k_square_fused (operand parked in the outputs' place / in LDS), on k_square_pipe and
    on the separate transforms ("sq_fused" 0).  Counters: a two-launch key switch is one launch more than the fused one; a fused squaring is two launches fewer
    than the separate transforms (one kernel per base instead of cn_run_ntt + k_intt_tensor) on the FP64 policies and the same sequence on the integer one."""
    o, g = cell.o, cell.g
    assert FORM[("mul_relin",) + key(cell)] == "kernel"
    rng = np.random.default_rng(0xB0 + cell.n)
    A = edge_words(o, rng, 3)
    B = np.concatenate([edges(o)[[8]], A[:2]])                      # the alternating +-Q / 2 of edges() (by CRT), then A shifted by one
    exp_ab, exp_sq = o.mul_relin_batch(A, B), o.mul_relin_batch(A, A)
    ha, hb = up1(g, A), up1(g, B)
    out = Out(g, o, 3, 0xB1)
    launches = {}
    for wide in (0, 1, 2):
        with Options(g, ks_wide=wide):
            _, d = delta(g, lambda: g.mul_relin(ha, 1, hb, 1, out.h, 1, 3))
            assert np.array_equal(out.words(), exp_ab), (wide, ks_form(*key(cell), wide))
            assert (d["Multiplication"], d["Relinarization"], d["ntt_forward_limbs"]) == (3, 3, 3 * 4 * (o.k + o.k + 1) + 3 * cell.tot * o.k)
            launches[("ab", wide)] = d["kernel_launches"]
            for name, opt in (("fused", dict(sq_fused=1, sq_lds=0, sq_pipe=0)), ("lds", dict(sq_fused=1, sq_lds=1, sq_pipe=0)), ("pipe", dict(sq_fused=1, sq_pipe=2)),
                              ("separate", dict(sq_fused=0))):
                with Options(g, **opt):
                    g.ct_upload(out.h, 1, out.sentinel[1:-1])
                    _, d = delta(g, lambda: g.mul_relin(ha, 1, ha, 1, out.h, 1, 3))
                    assert np.array_equal(out.words(), exp_sq), (wide, name)
                    launches[(name, wide)] = d["kernel_launches"]
    for what in ("ab", "fused", "lds", "pipe", "separate"):
        assert launches[(what, 1)] == launches[(what, 2)] == launches[(what, 0)] + 1, (what, launches)
    for wide in (0, 1, 2):
        fewer = 2 if cell.policy in FP64 else 0
        assert [launches[("separate", wide)] - launches[(f, wide)] for f in ("fused", "lds", "pipe")] == [fewer] * 3, launches
    for h in (ha, hb):
        g.free(h)
    out.free()


def test_b_multiply_then_relinearize(cell):
    o, g = cell.o, cell.g
    rng = np.random.default_rng(0xB8 + cell.n)
    A = edge_words(o, rng, 3)
    ha = up1(g, A)
    out3, out2 = Out(g, o, 2, 0xB9, size=3), Out(g, o, 2, 0xBA)
    g.multiply(ha, 1, ha, 2, out3.h, 1, 2)                          # (A0, A1), (A1, A2)
    exp3 = np.stack([o.multiply(A[0], A[1]), o.multiply(A[1], A[2])])
    assert np.array_equal(out3.words(), exp3)
    g.relinearize(out3.h, 1, out2.h, 1, 2)
    assert np.array_equal(out2.words(), np.stack([o.relinearize(c) for c in exp3]))
    g.free(ha)
    out3.free()
    out2.free()


# ------------------------------------------------------------------ c. rotations
def chain8(o, c):
    """SumAllSlots(8): rotate-and-add by -1, -2, -4"""
    for s in (1, 2, 4):
        c = o.add(c, o.rotate_rows(c, -s))
    return c


@pytest.fixture(scope="module")
def rotation_reference(cell):
    """operands and the oracle's words of every rotation of family c, computed once per cell"""
    o = cell.o
    rng = np.random.default_rng(0xC0 + cell.n)
    X, acc = edge_words(o, rng, 3), edge_words(o, rng, 3)[::-1].copy()
    many = [(0, 1), (2, -1), (1, -2)]                                # (input, step)
    return dict(X=X, acc=acc, many=many,
                rows={s: np.stack([o.rotate_rows(c, s) for c in X]) for s in (1, -1)},
                cols=np.stack([o.rotate_columns(c) for c in X]),
                rows_add=np.stack([o.add(a, o.rotate_rows(c, -2)) for a, c in zip(acc, X)]),
                cols_add=np.stack([o.add(a, o.rotate_columns(c)) for a, c in zip(acc, X)]),
                rows_many=np.stack([o.rotate_rows(X[i], s) for i, s in many]),
                slots=np.stack([chain8(o, c) for c in X[:2]]))


@pytest.mark.parametrize("ks_wide", [-1, 0])
def test_c_rotations(cell, rotation_reference, ks_wide):
    """"ks_wide" -1: what the library picks for 3 ciphertexts (the two-launch key switch, the automorphism applied while loading); 0: the fused kernel behind the
    permutation pass - at N = 16384 on the FP64 policies k_keyswitch_pair14, whose links of a SumAllSlots chain hand the next permuted c1 on"""
    o, g, r = cell.o, cell.g, rotation_reference
    assert FORM[("rotate",) + key(cell)] == "kernel" and set(STEPS) >= {1, -1, -2, -4}
    hx, hacc = up1(g, r["X"]), up1(g, r["acc"])
    out = Out(g, o, 3, 0xC1)
    per = cell.tot * o.k                                             # digit transforms of one key switch
    with Options(g, ks_wide=ks_wide):
        for s in (1, -1):
            _, d = delta(g, lambda: g.rotate_rows(hx, 1, s, out.h, 1, 3))
            assert np.array_equal(out.words(), r["rows"][s]), (s, ks_form(*key(cell), max(ks_wide, 0)))
            assert (d["Rotation"], d["ntt_forward_limbs"], d["kernel_launches"]) == (3, 3 * per, 2), d
        _, d = delta(g, lambda: g.rotate_columns(hx, 1, out.h, 1, 3))
        assert np.array_equal(out.words(), r["cols"])
        assert (d["Rotation"], d["ntt_forward_limbs"]) == (3, 3 * per)
        _, d = delta(g, lambda: g.rotate_rows_add(hx, 1, -2, hacc, 1, out.h, 1, 3))
        assert np.array_equal(out.words(), r["rows_add"])
        assert (d["Rotation"], d["Addition"], d["ntt_forward_limbs"], d["kernel_launches"]) == (3, 3, 3 * per, 2), d      # the addition rides in the key switch
        g.rotate_columns_add(hx, 1, hacc, 1, out.h, 1, 3)
        assert np.array_equal(out.words(), r["cols_add"])
        g.ct_upload(out.h, 1, out.sentinel[1:-1])
        _, d = delta(g, lambda: g.rotate_rows_many(hx, [1 + i for i, _ in r["many"]], [s for _, s in r["many"]], out.h, [1, 2, 3]))
        assert np.array_equal(out.words(), r["rows_many"])
        assert (d["Rotation"], d["ntt_forward_limbs"]) == (3, 3 * per)
        g.ct_upload(out.h, 1, r["X"])
        _, d = delta(g, lambda: g.sum_slots(out.h, 1, 2, 8))
        got = out.words()
        assert np.array_equal(got[:2], r["slots"]) and np.array_equal(got[2], r["X"][2])
        assert (d["Rotation"], d["Addition"], d["ntt_forward_limbs"]) == (6, 6, 6 * per)
    assert np.array_equal(g.ct_download(hx, 1, 3), r["X"]) and np.array_equal(g.ct_download(hacc, 1, 3), r["acc"])
    for h in (hx, hacc):
        g.free(h)
    out.free()


# ------------------------------------------------------------------ d. plaintext products
def test_d_mul_plain_on_both_plaintext_forms(cell):
    o, g = cell.o, cell.g
    assert FORM[("mul_plain",) + key(cell)] == "kernel"
    rng = np.random.default_rng(0xD0 + cell.n)
    pts, cts = plaintexts(o, rng, 3), edge_words(o, rng, 3)
    hp, hn = transformed(g, pts)                                    # coefficient form at 1, NTT form at 2
    ha = up1(g, cts)
    out = Out(g, o, 3, 0xD1)
    for stride in (1, 0):
        exp = np.stack([o.multiply_plain(c, pts[i * stride]) for i, c in enumerate(cts)])
        _, d = delta(g, lambda: g.mul_plain(ha, 1, hp, 1, out.h, 1, 3, pt_stride=stride))
        assert np.array_equal(out.words(), exp), stride
        npt = 3 if stride else 1
        assert (d["kernel_launches"], d["ntt_forward_limbs"], d["PlainMultiplication"]) == (2, npt * o.k + 3 * 2 * o.k, 3), d      # k_lift_ntt + k_mul_plain_fused
        g.ct_upload(out.h, 1, out.sentinel[1:-1])
        _, d = delta(g, lambda: g.mul_plain(ha, 1, hn, 2, out.h, 1, 3, pt_stride=stride))
        assert np.array_equal(out.words(), exp), stride
        assert (d["kernel_launches"], d["ntt_forward_limbs"], d["PlainMultiplication"]) == (1, 3 * 2 * o.k, 3), d                  # k_mul_plain_fused alone
    for h in (hp, hn, ha):
        g.free(h)
    out.free()


@pytest.mark.parametrize("ks_wide", [-1, 0])
def test_d_rowdot_batch_on_both_plaintext_forms(cell, ks_wide):
    """5 rows of length 8 against one ciphertext: the broadcast product kernel on coefficient rows and on NTT-form rows, then the rotate-and-add chain.  Under
    "ks_wide" 0 at N = 16384 (FP64 policies) the product kernel hands the chain its first permuted c1.  "ptn_bcast" moves exactly where cn_plain_wide holds."""
    o, g = cell.o, cell.g
    rng = np.random.default_rng(0xD8 + cell.n)
    rows = 5
    pts = plaintexts(o, rng, rows)
    v = edge_words(o, rng, 3)[2]
    exp = np.stack([chain8(o, o.multiply_plain(v, p)) for p in pts])
    hp, hn = transformed(g, pts)
    hv = up1(g, v[None, :])
    out, out2 = Out(g, o, rows, 0xD9), Out(g, o, rows, 0xDA)
    with Options(g, ks_wide=ks_wide):
        b0 = g.get_option("ptn_bcast")
        _, d = delta(g, lambda: g.rowdot_batch(hv, 1, hn, 2, rows, 8, out.h, 1))
        step = g.get_option("ptn_bcast") - b0
        _, dc = delta(g, lambda: g.rowdot_batch(hv, 1, hp, 1, rows, 8, out2.h, 1))
        assert g.get_option("ptn_bcast") - b0 == step                # coefficient rows never count
    got = out.words()
    assert np.array_equal(got, exp) and np.array_equal(out2.words(), got)
    kernel = FORM[("ptn_bcast",) + key(cell)] == "kernel"
    assert step == (1 if kernel else 0), (step, form("ptn_bcast", *key(cell)))
    chain = 3 * rows * cell.tot * o.k                                # the digit transforms of the three links
    # NTT rows: the ciphertext once (broadcast kernel) or once per row (k_mul_plain_fused alone); coefficient rows: the ciphertext once and every row in both blocks
    assert d["ntt_forward_limbs"] - chain == (2 * o.k if kernel else rows * 2 * o.k), d
    assert dc["ntt_forward_limbs"] - chain == 2 * o.k + rows * 2 * o.k, dc
    assert np.array_equal(g.ct_download(hv, 1, 1)[0], v)
    for h in (hp, hn, hv):
        g.free(h)
    out.free()
    out2.free()


def test_d_pt_transform(cell):
    assert FORM[("pt_transform",) + key(cell)] == "kernel"
    check_transform(cell.o, cell.g, 4, 0xDE0 + cell.n)              # 4 plaintexts and an all-zero one; k ntt_forward_limbs each, sentinels, the zero flag


# ------------------------------------------------------------------ e. cn_mul_plain_sum
def test_e_mul_plain_sum_on_both_plaintext_forms(cell):
    """G = 3 groups of 1, 5 and 17 terms over 6 ciphertexts (main_lists): coefficient-form plaintexts (k_mul_plain_sum) and NTT-form ones (k_mul_ptn_sum; run_sum
    also compares the two forms with each other).  The integer policy at N = 16384 composes cn_mul_plain per term and k_add_many."""
    o, g = cell.o, cell.g
    grp_off, idx = main_lists(0xE0 + cell.n)
    E, D = grp_off[-1], len(set(int(i) for i in idx))
    kernel = FORM[("mul_plain_sum",) + key(cell)] == "kernel"
    assert kernel == (FORM[("mul_ptn_sum",) + key(cell)] == "kernel")
    b0 = g.get_option("ptn_sum")
    _, d = delta(g, lambda: run_coeff_sum(o, g, grp_off, idx, 6, 0xE100 + cell.n))
    assert g.get_option("ptn_sum") == b0
    # kernel: the distinct ciphertexts and every plaintext, both polynomials' blocks; composed: per term the plaintext once and the ciphertext
    assert d["ntt_forward_limbs"] == (D * 2 * o.k + E * 2 * o.k if kernel else E * 3 * o.k), (d, form("mul_plain_sum", *key(cell)))
    assert (d["PlainMultiplication"], d["AddMany"], d["AddManyItemCount"]) == (E, 3, E)
    run_sum(o, g, grp_off, idx, 6, 0xE200 + cell.n, kernel=kernel)   # asserts "ptn_sum" + 1 and D 2 k forward limbs (kernel) / no step and E 2 k (composed)


def test_e_recentring_inside_the_fp64_sum_kernel(cell):
    """One group of interval + 2 terms of chosen NTT words, built like test_gpu_ptn.test_sum_of_chosen_words_across_three_recentrings: more than a whole
    interval of the word (q - 1) / 2 against the constant ciphertext q - 1 - every term -(q - 1) / 2 mod q, the residue of largest magnitude, all of one sign -
    then one term of words drawn from {0, 1, (q - 1) / 2, (q + 1) / 2, q - 1} against a uniform ciphertext.  The interval is recomputed from the derivation
    (cn_policy.h): on the ArF64 cells it is 11, so a recentring happens inside the kernel; the other policies run the same group (U64: no lazy accumulators)."""
    o, g, q = cell.o, cell.g, cell.q
    qmax = max(q)
    bound = qmax // 2 + 1 + -((-3 * qmax * qmax) >> 53)
    interval = min((2 ** 52 - 1) // bound, 1 << 16)
    if cell.policy != "u64":
        assert g.get_option("ptn_sum_interval") == interval
    if cell.policy == "f64":
        assert interval == 11
    E = (interval if cell.policy == "f64" else 11) + 2
    rng = np.random.default_rng(0xE300 + cell.n)
    cts = inputs(o, 4, 0xE301)                                       # 0 .. 2 carry edge residues, 3 is uniform
    const = np.zeros((2, o.k, o.n), dtype=np.uint64)
    for j in range(o.k):
        const[:, j, 0] = q[j] - 1
    cts[0] = const.reshape(-1)
    idx = np.zeros(E, dtype=np.uint32)
    idx[-1] = 3
    words = np.empty((E, o.k, o.n), dtype=np.uint64)
    words[:] = np.array([(m - 1) // 2 for m in q], dtype=np.uint64)[None, :, None]
    for j in range(o.k):
        choice = np.array([0, 1, (q[j] - 1) // 2, (q[j] + 1) // 2, q[j] - 1], dtype=np.uint64)
        words[-1, j] = choice[rng.integers(0, 5, size=o.n)]
    last = cts[3].reshape(2, o.k, o.n)
    exp = np.empty((2, o.k, o.n), dtype=np.uint64)
    for p in range(2):
        for j in range(o.k):
            m = q[j]
            head = (E - 1) * (m - 1) * ((m - 1) // 2) % m            # NTT(q - 1 constant) = q - 1 at every position
            tail = o.ntt_fwd(j, last[p, j]).astype(object) * words[-1, j].astype(object)
            exp[p, j] = o.ntt_inv(j, np.array([(head + int(x)) % m for x in tail], dtype=np.uint64))
    hc, hn = up1(g, cts), g.ptn_alloc(E + 1)
    out = Out(g, o, 1, 0xE302)
    g.ptn_upload(hn, 1, words)
    b0 = g.get_option("ptn_sum")
    g.mul_plain_sum(hc, 1, hn, 1, [0, E], idx, out.h, 1)
    assert np.array_equal(out.words()[0], exp.reshape(-1))
    assert g.get_option("ptn_sum") - b0 == (1 if FORM[("mul_ptn_sum",) + key(cell)] == "kernel" else 0)
    for h in (hc, hn):
        g.free(h)
    out.free()


# ------------------------------------------------------------------ f. one key switch per output
@pytest.fixture(scope="module")
def squares(cell):
    """4 inputs (inputs(): q - 1 everywhere, zero, q / 2 in c0, uniform) and their oracle squarings, shared by the cn_square_gemm cases of a cell"""
    c = Case(None, 4, 0xF00 + cell.n, shared=(cell.o, cell.g))
    yield c
    cell.g.free(c.h)


@pytest.mark.parametrize("M", [2, 16])
def test_f_square_gemm(cell, squares, M):
    """K = 3 inputs, M = 2 outputs (the FP64 tile of the digit GEMM) and 16 (the matrix-core tile, where the moduli allow the int8 GEMM: <= 46 bits), under the
    library's own choice of key switch and the fused one.  Literal cells run cn_mul_relin + the plan's GEMM inside the call."""
    o, g, c = cell.o, cell.g, squares
    fused = FORM[("square_gemm",) + key(cell)] == "kernel"
    rng = np.random.default_rng(0xF10 + M)
    W = rng.integers(-32768, 32769, size=(M, 3))                     # every residue of t = 65537 is a small weight: 3 x 2^15 x 1023 < q_min / 2 (36 bits)
    W[W == 0] = 1
    W[0, :] = 32768
    W[-1, :] = -32768
    Wr = res(W, o.t)
    idx = np.tile(np.array([0, 2, 3], dtype=np.int32), (M, 1))       # K = 3 of the 4 inputs: all but the zero ciphertext
    exp = c.expected(Wr, idx)
    for wide in (-1, 0):
        got, info = c.run(Wr, idx, i32=1, ks_wide=wide)
        assert np.array_equal(got, exp), (wide, info)
        assert (info["square_gemm_fused"], info["ks_digits_i32"]) == ((1, 1) if fused else (0, 0)), (info, form("square_gemm", *key(cell)))
        assert info["digit_gemm_mfma"] == (1 if fused and M == 16 and cell.policy == "f64l" else 0), info
    if fused:                                                        # digit sums as doubles: the same words
        ref, info = c.run(Wr, idx, i32=0, ks_wide=-1)
        assert np.array_equal(ref, exp) and (info["square_gemm_fused"], info["ks_digits_i32"]) == (1, 0)
    # inputs and outputs at an offset, sentinels beside the outputs
    hx = up1(g, c.X)
    out = Out(g, o, M, 0xF11)
    plan = g.gemm_plan(Wr, idx=idx)
    g.square_gemm(plan, hx, 1, out.h, 1)
    assert np.array_equal(out.words(), exp)
    assert np.array_equal(g.ct_download(hx, 1, 4), c.X)
    for h in (hx, plan):
        g.free(h)
    out.free()


@pytest.mark.parametrize("K,count,b_stride", [(2, 1, 0), (5, 2, 1)])
def test_f_mul_relin_sum(cell, K, count, b_stride):
    o, g = cell.o, cell.g
    fused = FORM[("mul_relin_sum",) + key(cell)] == "kernel"
    i0 = g.get_option("ks_digits_i32")
    run_relin_sum(g, o, K, count, b_stride, 0xF20 + K, fused=fused)   # the oracle's words, the literal sequence's words, the step of "mul_sum_fused"
    assert g.get_option("ks_digits_i32") - i0 == (1 if fused else 0), form("mul_relin_sum", *key(cell))
    # every operand at an offset, sentinels beside the outputs
    A, B = relin_sum_operands(o, K, count, b_stride, 0xF30 + K)
    pad = uniform(o, np.random.default_rng(5), 2)
    ha = [up1(g, A[k]) for k in range(K)]
    hb_all = g.ct_alloc(2 + K * B.shape[1])
    g.ct_upload(hb_all, 0, np.concatenate([pad, B.reshape(K * B.shape[1], -1)]))
    hb, ib = [hb_all] * K, [2 + k * B.shape[1] for k in range(K)]
    out = Out(g, o, count, 0xF31)
    b0 = g.get_option("mul_sum_fused")
    g.mul_relin_sum(ha, [1] * K, hb, ib, b_stride, out.h, 1, count)
    assert g.get_option("mul_sum_fused") - b0 == (1 if fused else 0)
    got = out.words()
    assert np.array_equal(got, relin_sum_expected(o, A, B, b_stride))
    assert np.array_equal(got, relin_sum_literal(g, ha, [1] * K, hb, ib, b_stride, count))
    for h in ha + [hb_all]:
        g.free(h)
    out.free()


# ------------------------------------------------------------------ g. modulus switch and the level context
def test_g_mod_switch_and_calls_on_the_level(cell):
    """3 -> 2 limbs: one drop, the integer kernel in every cell (cn_ms_f64_pair: the FP64 form takes two or more primes); 3 -> 1: the FP64 form on the FP64
    policies, the integer one under "f64" 0 and on the 60-bit set - the model's words each time.  Then cn_mul_plain_sum and cn_rotate_rows on the two-limb level
    against an oracle over the prefix with the sliced keys."""
    o, g, q, n = cell.o, cell.g, cell.q, cell.n
    assert FORM[("mod_switch",) + key(cell)] == "kernel"
    lo, lv = cell.level(2)
    l1 = g.level(1)
    rng = np.random.default_rng(0x600 + n)
    src = np.concatenate([edge_words(o, rng, 3), edges(o)[[3]]])
    m = len(src)
    h = up1(g, src)
    out2, out1 = Out(lv, lo, m, 0x601), Out(l1, type("Q", (), dict(q=q[:1], n=n, k=1))(), m, 0x602)
    try:
        g.mod_switch(h, 1, m, lv, out2.h, 1)
        got2 = out2.words()
        assert np.array_equal(got2, switch_residues(src, q, n, 2).reshape(m, -1))
        assert g.get_option("mod_switch_f64") == 0 and lv.get_option("mod_switch_f64") == 0
        exp1 = switch_residues(src, q, n, 1).reshape(m, -1)
        g.mod_switch(h, 1, m, l1, out1.h, 1)
        assert np.array_equal(out1.words(), exp1)
        assert g.get_option("mod_switch_f64") == (1 if cell.policy in FP64 else 0)
        with Options(g, f64=0):
            l1.ct_upload(out1.h, 1, out1.sentinel[1:-1])
            g.mod_switch(h, 1, m, l1, out1.h, 1)
            assert np.array_equal(out1.words(), exp1) and g.get_option("mod_switch_f64") == 0
        assert np.array_equal(g.ct_download(h, 1, m), src)
        # the level: k = 2, the same policy (60 / 60, 49 / 49, 44 / 40 bits)
        kernel = FORM[("mul_plain_sum",) + key(cell)] == "kernel"
        _, d = delta(lv, lambda: run_coeff_sum(lo, lv, [0, 2, 5], np.array([0, 1, 1, 2, 0], dtype=np.uint32), 3, 0x610 + n))
        assert d["ntt_forward_limbs"] == (3 * 2 * 2 + 5 * 2 * 2 if kernel else 5 * 3 * 2), d
        rot = Out(lv, lo, m, 0x603)
        _, d = delta(lv, lambda: lv.rotate_rows(out2.h, 1, 1, rot.h, 1, m))
        assert np.array_equal(rot.words(), np.stack([lo.rotate_rows(c, 1) for c in got2]))
        tot2 = sum(-(-x.bit_length() // cell.width) for x in q[:2])
        assert (d["Rotation"], d["ntt_forward_limbs"]) == (m, m * tot2 * 2)
        rot.free()
    finally:
        g.set_option("f64", 1)
    g.free(h)
    out2.free()
    out1.free()
