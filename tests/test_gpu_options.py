"""GPU: the per-context tunables of cn_set_option / cn_get_option (the option table of cn_api.hip, documented in include/cnhip.h) - the
documented defaults, every allowed value read back, out-of-range values refused without a change, retired names refused, and a level context
that takes its parent's values.  Fresh contexts only (never the shared ones of conftest.get_gpu): the tests change every switch."""
import pytest

from conftest import PARAMS

pytestmark = pytest.mark.gpu

# flags: default at c3; any value is accepted and read back as value != 0
FLAGS = {"f64": 1, "legacy_ntt": 0, "ks_perm_fused": 1, "sq_fused": 1, "sq_lds": 1, "fold_zero": 1, "gemm_mfma": 1, "gemm_pair": 1,
         "mp_fused": 1, "ks_split14": 1, "ks_pair14": 1, "ks_chain": 1, "mp_bcast": 1}
# enumerated switches: (default at c3, lowest, highest allowed value)
ENUMS = {"gemm_order": (1, 0, 1), "ks_xcd": (2, 0, 2), "sq_pipe": (1, 0, 2), "sq_halves": (1, 0, 2), "enc_fused": (2, 0, 2), "ks_wide": (-1, -1, 2)}
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
