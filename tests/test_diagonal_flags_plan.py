"""A diagonal plan from the non-zero flags of the generalized diagonals alone (diagonal.plan_from_flags - what hewrapper.DEVICE_DIAGONAL_PLAN builds from
cn_diag_scan), without a GPU: the scan formula of include/cnhip.h as a numpy model against `pre_rotated_rows(...).any(axis=1)` over every structural candidate, the
plan against build_plan's, its term list against the rows build_plan emits, and the slot model against W v."""
import numpy as np
import pytest

from cryptonets_amd import diagonal
import diag_helpers as dh

N, T = dh.N, 12289
M = N // 2


def banded(seed):
    """300 x 900, non-zero exactly where (r - x) % 7 == 0: the kept diagonals are neither all baby steps nor all groups"""
    W = np.random.default_rng(seed).integers(1, T, size=(300, 900))
    r, x = np.indices(W.shape)
    W[(r - x) % 7 != 0] = 0
    return W


def three_rows(seed):
    """3 x 1000, non-zero except on the two diagonals (1, 510) and (1, 511) - which only rows 1 and 2 reach, in columns 512 and 513"""
    W = np.random.default_rng(seed).integers(1, T, size=(3, 1000))
    W[2, 512] = W[1, 512] = W[2, 513] = 0
    return W


def full(R, dim, seed):
    W = np.random.default_rng(seed).integers(0, T, size=(R, dim))
    W[0, 0] = T - 1                                                  # (1 x 1: not the zero matrix)
    return W


CASES = {"%dx%d" % s: (lambda s=s: full(s[0], s[1], s[0] + s[1])) for s in dh.SHAPES + [(600, 1024), (1, 1)]}
CASES["banded300x900"] = lambda: banded(3)
CASES["3x1000"] = lambda: three_rows(4)
CASES["signed37x700"] = lambda: dh.weights(37, 700, 1) % T


def scan_model(W, n):
    """include/cnhip.h, cn_diag_scan: every non-zero W[h_r m + p_r, h_c m + x] sets flag (h_r ^ h_c, (x - p_r) mod m)"""
    m = n // 2
    out = np.zeros((2, m), dtype=bool)
    r, x = np.nonzero(W)
    out[(r // m) ^ (x // m), (x % m - r % m) % m] = True
    return out


def candidates(R, dim, n):
    mask = diagonal.structural_diagonals(R, dim, n)
    B = diagonal.choose_baby_steps(mask)
    return mask, B, [(c, j * B, b) for j in range((n // 2) // B) for c in (0, 1) for b in range(B) if mask[c, j * B + b]]


def host_plan(W, n, B=None):
    rows = []
    plan = diagonal.build_plan(W, n, lambda first, part: rows.extend(part), B=B)
    return plan, np.stack(rows)


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    W = CASES[request.param]()
    return request.param, W, scan_model(W, N)


def test_scan_formula_equals_the_rows_of_every_structural_candidate(case):
    name, W, nz = case
    mask, B, cand = candidates(W.shape[0], W.shape[1], N)
    want = np.zeros((2, M), dtype=bool)
    for k0 in range(0, len(cand), 256):
        part = cand[k0:k0 + 256]
        hit = diagonal.pre_rotated_rows(W, N, part).any(axis=1)
        for (c, J, b), z in zip(part, hit):
            want[c, J + b] = z
    assert np.array_equal(nz, want)
    assert not (nz & ~mask).any(), "a flag outside the structural diagonals"
    if name == "banded300x900":
        assert (len(cand), int(nz.sum())) == (1024, 214)
    if name == "3x1000":
        assert (len(cand), int(nz.sum())) == (1002, 1000)


def test_plan_from_flags_is_the_plan_of_build_plan_and_its_terms_are_the_emitted_rows(case):
    name, W, nz = case
    R, dim = W.shape
    for B in (None, 8):
        want, rows = host_plan(W, N, B)
        plan, terms = diagonal.plan_from_flags(nz, N, R, dim, B=B)
        for attr in ("n", "m", "R", "Dim", "B", "Gs", "babies", "groups", "grp_off", "ct_idx"):
            assert getattr(plan, attr) == getattr(want, attr), attr
        assert len(terms) == plan.terms and all(J % plan.B == 0 and b < plan.B for (_, J, b) in terms)
        assert np.array_equal(diagonal.pre_rotated_rows(W, N, terms), rows)


def test_rows_rebuilt_from_the_terms_evaluate_to_the_product(case):
    name, W, nz = case
    R, dim = W.shape
    plan, terms = diagonal.plan_from_flags(nz, N, R, dim)
    v = np.zeros(N, dtype=np.int64)
    v[:dim] = np.random.default_rng(11).integers(0, T, size=dim)
    got = diagonal.evaluate_on_slots(plan, diagonal.pre_rotated_rows(W, N, terms), v, T)
    want = np.zeros(N, dtype=object)
    want[:R] = (W.astype(object) @ v[:dim].astype(object)) % T
    assert [int(x) for x in got] == [int(x) for x in want]


def test_a_zero_matrix_raises_like_build_plan():
    with pytest.raises(ValueError, match="the matrix is zero"):
        diagonal.plan_from_flags(np.zeros((2, M), dtype=bool), N, 37, 700)
    with pytest.raises(ValueError, match="the matrix is zero"):
        diagonal.build_plan(np.zeros((37, 700), dtype=np.int64), N, lambda first, part: None)
    with pytest.raises(ValueError, match="power of two"):
        diagonal.plan_from_flags(np.ones((2, M), dtype=bool), N, 37, 700, B=3)


def test_binding_switch_and_header():
    from cryptonets_amd import _native, hewrapper
    from oracle_backend import OracleBackend
    assert len(_native.SIGNATURES["cn_diag_scan"][1]) == 6 and len(_native.SIGNATURES["cn_diag_encode"][1]) == 9
    assert callable(_native.Context.diag_scan) and callable(_native.Context.diag_encode)
    assert hewrapper.DEVICE_DIAGONAL_PLAN is False
    assert not hasattr(OracleBackend, "diag_scan")                   # the CPU backend keeps the host route
    header = open(_native.os.path.join(_native._ROOT, "include", "cnhip.h")).read()
    assert "int cn_diag_scan(cn_ctx *ctx, cn_handle rows, uint32_t ri, uint32_t R, uint32_t dim, uint8_t *nonzero" in header
    assert "int cn_diag_encode(cn_ctx *ctx, cn_handle rows, uint32_t ri, uint32_t R, uint32_t dim, const uint32_t *terms" in header
