"""GPU: the per-context tunables of cn_set_option / cn_get_option (the option table of cn_options.h, documented in include/cnhip.h) - the
documented defaults, every allowed value read back, out-of-range values refused without a change, retired names refused, and a level context
that takes its parent's values - and the values cn_get_option reads beside them: every counter and read-only name readable, zero / unchanged
by a refused cn_set_option, and the step one small call gives its counters.  Fresh contexts only (never the shared ones of conftest.get_gpu):
the tests change every switch."""
import numpy as np
import pytest

from conftest import PARAMS
from test_options import COUNTERS, READ_ONLY

pytestmark = pytest.mark.gpu

# flags: default at c3; any value is accepted and read back as value != 0
FLAGS = {"f64": 1, "legacy_ntt": 0, "ks_perm_fused": 1, "sq_fused": 1, "sq_lds": 1, "fold_zero": 1, "gemm_mfma": 1, "gemm_pair": 1,
         "mp_fused": 1, "ks_split14": 1, "ks_pair14": 1, "ks_chain": 1, "mp_bcast": 1, "mul_sum": 1, "digit_mfma": 1, "digit_i32": 1, "defer_square_gemm": 0}
# enumerated switches: (default at c3, lowest, highest allowed value)
ENUMS = {"gemm_order": (1, 0, 1), "ks_xcd": (2, 0, 2), "sq_pipe": (1, 0, 2), "sq_halves": (1, 0, 2), "enc_fused": (2, 0, 2), "ks_wide": (-1, -1, 2),
         "sg_prefloor": (1, 0, 2), "ptn_order": (0, 0, 1)}
RETIRED = ("defer_stagger", "sq_overlap", "ks_tight")
CN_ERR_ARG = -1


def fresh(name):
    from cryptonets_amd._native import Context
    p = PARAMS[name]
    return Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)


def refused(call):
    from cryptonets_amd._native import CnError
    with pytest.raises(CnError) as e:
        call()
    assert e.value.code == CN_ERR_ARG
    return str(e.value)


def test_defaults():
    g = fresh("c3")
    try:
        for name, default in FLAGS.items():
            assert g.get_option(name) == default, name
        for name, (default, _, _) in ENUMS.items():
            assert g.get_option(name) == default, name
    finally:
        g.close()
    g = fresh("n16k7")
    try:
        assert g.get_option("ks_xcd") == 1                      # N = 16384: the limbs of a ciphertext on one XCD
    finally:
        g.close()


def test_every_allowed_value_round_trips():
    g = fresh("c3")
    try:
        for name in FLAGS:
            for v, back in ((0, 0), (1, 1), (7, 1), (-1, 1), (0, 0)):
                g.set_option(name, v)
                assert g.get_option(name) == back, (name, v)
        for name, (_, lo, hi) in ENUMS.items():
            for v in list(range(lo, hi + 1)) + [lo]:
                g.set_option(name, v)
                assert g.get_option(name) == v, (name, v)
    finally:
        g.close()


def test_out_of_range_values_are_refused_and_change_nothing():
    g = fresh("c3")
    try:
        for name, (default, lo, hi) in ENUMS.items():
            kept = hi if default != hi else lo                   # a value other than the default, so that "unchanged" means something
            g.set_option(name, kept)
            for bad in (lo - 1, hi + 1, -1000, 1000):
                refused(lambda: g.set_option(name, bad))
                assert g.get_option(name) == kept, (name, bad)
    finally:
        g.close()


def test_retired_names_are_unknown():
    g = fresh("c3")
    try:
        for name in RETIRED:
            assert "unknown option" in refused(lambda: g.set_option(name, 1))
            assert "unknown option" in refused(lambda: g.get_option(name))
    finally:
        g.close()


def test_level_context_takes_every_value_of_its_parent():
    g = fresh("c3")
    lv = None
    try:
        want = {name: 1 - default for name, default in FLAGS.items()}
        want.update({name: (hi if default != hi else lo) for name, (default, lo, hi) in ENUMS.items()})
        for name, v in want.items():
            g.set_option(name, v)
        lv = g.level(2)
        for name, v in want.items():
            assert lv.get_option(name) == v, name
    finally:
        if lv is not None:
            lv.close()
        g.close()


def test_counters_and_read_only_values_are_readable_and_refuse_a_set():
    g = fresh("c3")
    try:
        assert [n for n in COUNTERS if g.get_option(n) != 0] == []
        for name in COUNTERS + READ_ONLY:
            before = g.get_option(name)
            assert "unknown option" in refused(lambda: g.set_option(name, before + 1)), name
            assert g.get_option(name) == before, name
        for name in ("defer", "ks_xi", "record_steps"):              # the three settable names outside the table
            assert g.get_option(name) == 0, name
            g.set_option(name, 1)
            assert g.get_option(name) == 1, name
            g.set_option(name, 0)
        assert "defer: 0, 1 or 2" in refused(lambda: g.set_option("defer", 3))
    finally:
        g.close()


def test_one_small_call_per_counter_family_moves_its_counters():
    """One call of each family that runs at a small shape on the CryptoNets ring, keys and ciphertexts made on the device (the words are other tests' business).  The
    steps are those of the library before the counters moved into one struct (profiles/options_table_refactor.md).  "mul_relin_pipelined" (batches of >= 512
    ciphertexts) and "defer_square_gemm_fused" (a queued layer) have no small call: tests/test_gpu_mul_relin_paths.py and tests/test_deferred_square_gemm.py read them."""
    g = fresh("c3")
    try:
        t, K, O = PARAMS["c3"]["t"], 40, 16
        g.keygen(42, galois=False)
        ph, x = g.pt_alloc(K), g.ct_alloc(K)
        g.encode_batch(np.arange(1, 3 * K + 1, dtype=np.uint64).reshape(K, 3), ph, 0)
        g.encrypt(ph, 0, x, 0, K, seed=7)

        def steps(call, names=COUNTERS):
            before = [g.get_option(n) for n in names]
            call()
            return {n: g.get_option(n) - b for n, b in zip(names, before) if g.get_option(n) != b}

        # cn_square_gemm, 16 outputs of 40 terms, |w| <= 1000, in the pre-floor form: matrix-core digit GEMM, int32 digit sums
        W = np.random.default_rng(0x0C).integers(-1000, 1001, size=(O, K))
        plan, out = g.gemm_plan(np.mod(W, t).astype(np.uint64)), g.ct_alloc(O)
        g.set_option("sg_prefloor", 2)
        assert steps(lambda: g.square_gemm(plan, x, 0, out, 0)) == {"square_gemm_fused": 1, "square_gemm_prefloor": 1, "digit_gemm_mfma": 1, "ks_digits_i32": 1}
        g.set_option("sg_prefloor", 1)
        assert steps(lambda: g.square_gemm(plan, x, 0, out, 0)) == {"square_gemm_fused": 1, "digit_gemm_mfma": 1, "ks_digits_i32": 1}      # K below "sg_prefloor_min_k"
        # cn_mul_relin_sum of three terms
        assert steps(lambda: g.mul_relin_sum([x] * 3, [0, 1, 2], [x] * 3, [3, 4, 5], 1, out, 0, 2)) == {"mul_sum_fused": 1, "ks_digits_i32": 1}
        assert g.get_option("mul_sum_groups") == 1
        # NTT-form plaintexts: a sum of products in two groups, a row-dot batch of four rows without rotations
        pn = g.ptn_alloc(6)
        g.pt_transform(ph, 0, 6, pn, 0)
        assert steps(lambda: g.mul_plain_sum(x, 0, pn, 0, [0, 3, 6], [0, 1, 0, 2, 3, 1], out, 0)) == {"ptn_sum": 1}
        assert steps(lambda: g.rowdot_batch(x, 0, pn, 0, 4, 1, out, 0)) == {"ptn_bcast": 1}
        # a diagonal plan of a 3 x 5 matrix: the scan, then two terms encoded
        rows, dg = g.pt_alloc(3), g.pt_alloc(2)
        g.encode_batch(np.arange(1, 16, dtype=np.uint64).reshape(3, 5), rows, 0)
        assert steps(lambda: g.diag_scan(rows, 0, 3, 5)) == {"diag_scan": 1}
        assert steps(lambda: g.diag_encode(rows, 0, 3, 5, [(0, 0, 0), (0, 0, 1)], dg, 0)) == {"diag_encode": 1}
        # a queued encryption of zero that only one queued scalar product reads: folded
        g.set_option("defer", 1)

        def fold():
            z, d = g.ct_alloc(1), g.ct_alloc(1)
            g.encrypt(0, 0, z, 0, 1, seed=203)
            g.scalar_dot([x, z], np.zeros(2, dtype=np.uint32), np.array([5, 7], dtype=np.uint64), d, 0)
            g.free(z)
            g.sync()
        assert steps(fold) == {"folded_zero_encryptions": 1}
        g.set_option("defer", 0)
    finally:
        g.close()
