"""The automatic key-switch thresholds ("ks_wide" -1) at N = 16384, word for word against the CPU oracle.

test_gpu_mul_relin_paths runs the automatic choice at N <= 8192 ("tiny", c3); at N = 16384 only forced "ks_wide" values ran.  The rules differ there
(cn_ks_plan.h): up to 160 (ciphertext, limb) blocks a key switch is two launches with a workgroup per DIGIT - there is no per-source-limb form, 1024-thread
workgroups cannot hold two accumulator sets - and above them it is ONE launch: k_keyswitch_pair14 when the key is FP64 words, the 1024-thread k_keyswitch_rr
when it is not.  Two cells of size_policy_sets, ("f64", 16384) and ("u64", 16384) at one digit per limb (k = 3): the counts 3, 4, 53, 54 sit on both sides of
10 // 3 and 160 // 3.

Launch counts, from the code: a Multiply has the same launches at every count (one per step of do_multiply), so cn_mul_relin at 3, 4 and 53 ciphertexts
(two-launch key switch) takes one launch more than at 54 (one launch).  A one-hop rotation is two launches on every side: the two-launch forms apply the
automorphism while they load ("ks_perm_fused"), pair14 has k_galois_limbs permute c1 ahead, the 1024-thread kernel a k_galois_lds pass."""
import numpy as np
import pytest

from size_policy_sets import Cell, edge_words
from test_gpu_mul_relin_paths import KS_DIGIT_MAX_BLOCKS, KS_WIDE_MAX_BLOCKS
from test_gpu_size_policy_matrix import delta, up1

pytestmark = pytest.mark.gpu

N, K = 16384, 3
COUNTS = (KS_DIGIT_MAX_BLOCKS // K, KS_DIGIT_MAX_BLOCKS // K + 1, KS_WIDE_MAX_BLOCKS // K, KS_WIDE_MAX_BLOCKS // K + 1)
assert COUNTS == (3, 4, 53, 54)
M = max(COUNTS)


def expected(o):
    """operands and the oracle's words for the largest count; the results for n ciphertexts are the first n rows"""
    rng = np.random.default_rng(0x16384)
    X, Y = edge_words(o, rng, M), edge_words(o, rng, M)
    return X, Y, {"square": o.mul_relin_batch(X, X), "product": o.mul_relin_batch(X, Y), "rows": np.stack([o.rotate_rows(c, 1) for c in X])}


@pytest.mark.parametrize("policy", ("f64", "u64"))
def test_automatic_forms_on_both_sides_of_the_thresholds(policy):
    cell = Cell(policy, N, 60)
    try:
        o, g = cell.o, cell.g
        assert o.k == K and cell.tot == K and g.get_option("ks_wide") == -1
        X, Y, exp = expected(o)
        hx, hy, ho = up1(g, X), up1(g, Y), g.ct_alloc(M + 2)
        fill = np.full((M + 2, 2 * K * N), 7, dtype=np.uint64)
        launches = {}
        for n in COUNTS:
            for what, call in (("square", lambda: g.mul_relin(hx, 1, hx, 1, ho, 1, n)), ("product", lambda: g.mul_relin(hx, 1, hy, 1, ho, 1, n)),
                               ("rows", lambda: g.rotate_rows(hx, 1, 1, ho, 1, n))):
                g.ct_upload(ho, 0, fill)
                _, d = delta(g, call)
                got = g.ct_download(ho, 0, M + 2)
                assert np.array_equal(got[1:1 + n], exp[what][:n]), (what, n)
                assert np.array_equal(got[0], fill[0]) and np.array_equal(got[1 + n:], fill[1 + n:]), (what, n, "written beside the range")
                launches[(what, n)] = d["kernel_launches"]
        for what in ("square", "product"):
            assert launches[(what, 3)] == launches[(what, 4)] == launches[(what, 53)] == launches[(what, 54)] + 1, (what, launches)
        assert [launches[("rows", n)] for n in COUNTS] == [2, 2, 2, 2], launches      # 54 under "f64": k_galois_limbs + k_keyswitch_pair14
        assert np.array_equal(g.ct_download(hx, 1, M), X) and np.array_equal(g.ct_download(hy, 1, M), Y)      # operands intact
    finally:
        cell.close()
