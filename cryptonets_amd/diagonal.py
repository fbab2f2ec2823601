"""Generalized-diagonal (Halevi-Shoup) matrix-vector products with baby-step giant-step rotations: the planner of hewrapper.DIAGONAL_DENSE.

Slot geometry: the N slots of a BFV plaintext are the group Z_m x Z_2, m = N / 2, slot s = h m + p.  RotateRows(+i) gives out[h, p] = in[h, (p + i) mod m],
RotateColumns swaps h.  For g = (c, i) the generalized diagonal of a weight matrix W (R rows, Dim columns, zero elsewhere) is

    diag_g[h, p] = W[h m + p, (h ^ c) m + (p + i) mod m]                              and        W v = sum_g diag_g * rho_g(v)

(* = slot-wise product, rho_(c,i) = RotateColumns^c RotateRows(i)): the result has row r in slot r and zeros at R and above - the dense vector the default
path builds with one product per row, a 14-link SumAllSlots chain on each and a one-hot mask.  With i = j B + b (B baby steps, Gs = m / B giant steps)

    W v = sum_c kappa^c ( sum_j rho_(jB)( u_(c,j) ) ),       u_(c,j) = sum_b pre_(c,j,b) * rho_b(v),       pre_(c,j,b) = kappa^c rho_(-jB) (diag_(c, jB + b))

so the input is rotated B - 1 times, the 2 Gs sums u are ONE cn_mul_plain_sum call, and the sums are rotated 2 (Gs - 1) + 1 times.  Written out:

    pre_(c,j,b)[h, p] = W[(h ^ c) m + (p - jB) mod m,  h m + (p + b) mod m]

Everything here is host-side integer bookkeeping (numpy): no device, no ciphertext.
"""
import numpy as np


def ks_digits(q, dbc):
    """digit polynomials of one key switch: sum over the coefficient moduli of ceil(bits(q_l) / dbc)"""
    return sum(-(-int(ql).bit_length() // int(dbc)) for ql in q)


def structural_diagonals(R, Dim, n):
    """bool [2, m]: may diag_(c, i) of an R x Dim matrix hold a non-zero?  Rows h m + p with p < P_h, columns (h ^ c) m + x with x < L_(h ^ c): some p < P_h has
    (p + i) mod m < L  <=>  i < L or i > m - P_h"""
    m = n // 2
    if not (0 < R <= n and 0 < Dim <= n):
        raise ValueError("the matrix does not fit the %d slots" % n)
    P = (min(R, m), max(0, R - m))
    L = (min(Dim, m), max(0, Dim - m))
    i = np.arange(m)
    out = np.zeros((2, m), dtype=bool)
    for c in (0, 1):
        for h in (0, 1):
            if P[h] and L[h ^ c]:
                out[c] |= (i < L[h ^ c]) | (i > m - P[h])
    return out


def _rotation_counts(mask, B):
    """(distinct baby steps, groups (c, j) with a diagonal, key switches) of the diagonals in `mask` [2, m] under B baby steps: the baby steps by doubling when all B are
    needed (B - 1 single-hop rotations) and one rotation each otherwise, the giant steps by folding when every group of the column classes in use exists (Gs - 1 per
    class) and one rotation per group with j > 0 otherwise, one column rotation when a diagonal with c = 1 exists"""
    m = mask.shape[1]
    Gs = m // B
    g = mask.reshape(2, Gs, B)
    babies = int(g.any(axis=(0, 1)).sum())
    groups = g.any(axis=2)                                            # [2, Gs]
    ngroups = int(groups.sum())
    classes = int(groups.any(axis=1).sum())
    ks = max(babies - (1 if g[:, :, 0].any() else 0), 0)
    ks += classes * (Gs - 1) if ngroups == classes * Gs else int(groups[:, 1:].sum())
    ks += 1 if groups[1].any() else 0
    return babies, ngroups, ks


def choose_baby_steps(mask):
    """the power of two B <= m with the fewest key switches for the diagonals in `mask` (ties: the smaller B - fewer resident rotated inputs)"""
    m = mask.shape[1]
    best = None
    B = 1
    while B <= m:
        ks = _rotation_counts(mask, B)[2]
        if best is None or ks < best[0]:
            best = (ks, B)
        B *= 2
    return best[1]


def dense_path_counts(R, Dim, n, k, digits, length=None, B=None, ntt_weights=False, hoisted=False, summed=False):
    """Limb transforms (one N-point transform of one limb) of the two ways to compute the dense product of an R x Dim plaintext matrix with one packed ciphertext on a
    ring of n slots with k coefficient moduli and `digits` digit polynomials per key switch (ks_digits of the Galois decomposition bit count):

      a key switch              digits k forward + 2 k inverse transforms
      default (cn_rowdot_batch, one-hot masks, cn_add_many)
                                R x links key switches (links: the SumAllSlots chain over `length` slots, None = all), 2 k forward for the ciphertext, 2 k forward +
                                2 k inverse per row product, and k + 2 k forward + 2 k inverse per mask product
      diagonal (cn_mul_plain_sum between baby and giant steps)
                                the key switches of _rotation_counts, 2 k forward per distinct rotated input, 2 k forward per diagonal (a workgroup per polynomial
                                transforms the plaintext itself) and 2 k inverse per group

    ntt_weights: the row plaintexts / the diagonals are resident in NTT form (hewrapper.NTT_WEIGHTS, cn_pt_transform) - their transforms drop out of both counts:
    2 k per row on the default path, 2 k per diagonal on the diagonal path.

    hoisted: the baby steps are ONE hoisted call (hewrapper.HOISTED_ROTATIONS, cn_rotate_rows_hoisted: every baby step with its own key) - their key switches share
    the digits k forward transforms of the input and cost 2 k inverse transforms each, instead of digits k + 2 k each.  The default path does not change.

    summed: the giant steps are ONE summed call (hewrapper.SUMMED_ROTATIONS, cn_rotate_rows_sum: one key switch per group with j > 0, priced with its own key as
    the folding links are) - every one keeps its digits k forward transforms, and the 2 k inverse transforms are paid once per column class with such a group
    instead of once per key switch.  The default path does not change.

    Weights are taken as dense inside R x Dim (structural_diagonals).  Returns a dict with the two totals, their parts and "choice": "diagonal" if and only if its
    total is lower."""
    m = n // 2
    per_ks = digits * k + 2 * k
    ln = n if length is None else int(length)
    links = 0
    if ln >= m:
        links, ln = 1, m
    links += max(ln - 1, 0).bit_length()
    d_ks = R * links
    d_plain = 2 * k + R * (2 if ntt_weights else 4) * k + R * 7 * k
    mask = structural_diagonals(R, Dim, n)
    if B is None:
        B = choose_baby_steps(mask)
    babies, ngroups, g_ks = _rotation_counts(mask, B)
    terms = int(mask.sum())
    g_plain = babies * 2 * k + (0 if ntt_weights else terms * 2 * k) + ngroups * 2 * k
    default, diagonal = d_ks * per_ks + d_plain, g_ks * per_ks + g_plain
    baby_ks = max(babies - (1 if mask.reshape(2, -1, B)[:, :, 0].any() else 0), 0)
    if hoisted and baby_ks:
        diagonal -= baby_ks * per_ks - (digits * k + baby_ks * 2 * k)
    if summed:
        far = mask.reshape(2, -1, B).any(axis=2)[:, 1:]              # groups (c, j) with j > 0: the same number of key switches by folding and by one rotation each
        diagonal -= (int(far.sum()) - int(far.any(axis=1).sum())) * 2 * k
    return {"default": default, "diagonal": diagonal, "choice": "diagonal" if diagonal < default else "default", "B": B,
            "default_key_switches": d_ks, "diagonal_key_switches": g_ks, "default_plain_transforms": d_plain, "diagonal_plain_transforms": g_plain,
            "diagonals": terms, "babies": babies, "groups": ngroups}


class DiagonalPlan:
    """What one (matrix, plaintext prime) needs to run: B, Gs, the baby steps `babies` (ascending, babies[0] = 0 always), the groups (j, c) in ascending order of
    (j, c) - index len(classes) j + position of c in `classes` when every group of the column classes in use exists - and the lists of cn_mul_plain_sum: grp_off [groups + 1], ct_idx [terms] (positions in `babies`).  Term e multiplies
    rho_(babies[ct_idx[e]])(v) by the plaintext whose slots are row e of the matrices handed to `emit` while the plan was built."""

    def __init__(self, n, R, Dim, B):
        self.n, self.m, self.R, self.Dim, self.B, self.Gs = n, n // 2, R, Dim, B, (n // 2) // B
        self.babies, self.groups, self.grp_off, self.ct_idx = [0], [], [0], []

    @property
    def terms(self):
        return len(self.ct_idx)

    @property
    def babies_by_doubling(self):
        return self.babies == list(range(self.B))

    @property
    def classes(self):
        """the column classes c with a diagonal: [0], [1] or [0, 1]"""
        return sorted({c for (_, c) in self.groups})

    @property
    def giants_by_folding(self):
        return len(self.groups) == len(self.classes) * self.Gs

    def key_switches(self):
        ks = self.B - 1 if self.babies_by_doubling else len(self.babies) - 1
        ks += len(self.classes) * (self.Gs - 1) if self.giants_by_folding else sum(1 for (j, c) in self.groups if j)
        return ks + (1 if any(c for (_, c) in self.groups) else 0)


def pre_rotated_rows(W, n, terms):
    """slot values [len(terms), n] of pre_(c,j,b) for terms = [(c, jB, b)]: W is the R x Dim integer matrix (any integer dtype), zero outside"""
    W = np.asarray(W)
    R, Dim = W.shape
    m = n // 2
    t = np.asarray(terms, dtype=np.int64).reshape(-1, 3)
    s = np.arange(n, dtype=np.int64)
    h, p = s // m, s % m
    rows = (h[None, :] ^ t[:, 0:1]) * m + (p[None, :] - t[:, 1:2]) % m
    cols = h[None, :] * m + (p[None, :] + t[:, 2:3]) % m
    ok = (rows < R) & (cols < Dim)
    out = np.zeros(rows.shape, dtype=W.dtype)
    out[ok] = W[rows[ok], cols[ok]]
    return out


def plan_from_flags(nz, n, R, Dim, B=None):
    """(DiagonalPlan, terms) from the non-zero flags of the generalized diagonals alone: nz bool [2, m], nz[c, i] = diag_(c,i) of the R x Dim matrix has a non-zero
    (what `pre_rotated_rows(...).any(axis=1)` says of every structural candidate, or Context.diag_scan on the device).  The plan build_plan returns for a matrix with
    those diagonals; terms = [(c, j B, b)] in term order - the rows pre_rotated_rows / Context.diag_encode make of them are the plan's plaintexts."""
    m = n // 2
    mask = structural_diagonals(R, Dim, n)
    nz = np.asarray(nz, dtype=bool).reshape(2, m)
    if B is None:
        B = choose_baby_steps(mask)
    if B < 1 or B & (B - 1) or m % B:
        raise ValueError("B must be a power of two that divides %d" % m)
    plan = DiagonalPlan(n, R, Dim, B)
    keep = (nz & mask).reshape(2, m // B, B)
    kept = [(int(j), int(c), int(b)) for (j, c, b) in np.argwhere(keep.transpose(1, 0, 2))]      # ascending (j, c, b): the terms of a group are neighbours
    if not kept:
        raise ValueError("the matrix is zero")
    plan.babies = sorted({0} | {b for (_, _, b) in kept})
    pos = {b: i for i, b in enumerate(plan.babies)}
    for (j, c, b) in kept:
        if not plan.groups or plan.groups[-1] != (j, c):
            if plan.groups:
                plan.grp_off.append(len(plan.ct_idx))
            plan.groups.append((j, c))
        plan.ct_idx.append(pos[b])
    plan.grp_off.append(len(plan.ct_idx))
    return plan, [(c, j * B, b) for (j, c, b) in kept]


def build_plan(W, n, emit, B=None, chunk=256):
    """Plan the product with the integer matrix W (R x Dim residues mod t) on n slots.  All-zero diagonals are dropped; the slot values of the kept plaintexts, already
    rotated, are handed to emit(first_term, rows[count, n]) in term order, at most `chunk` candidates at a time (the caller encodes them and forgets them: at
    CIFAR shapes they are 2 GiB per prime).  B: baby steps (a power of two dividing m; None = choose_baby_steps on the structural diagonals)."""
    W = np.asarray(W)
    R, Dim = W.shape
    m = n // 2
    mask = structural_diagonals(R, Dim, n)
    if B is None:
        B = choose_baby_steps(mask)
    if B < 1 or B & (B - 1) or m % B:
        raise ValueError("B must be a power of two that divides %d" % m)
    plan = DiagonalPlan(n, R, Dim, B)
    cand = [(c, j, b) for j in range(m // B) for c in (0, 1) for b in range(B) if mask[c, j * B + b]]
    kept = []                                                        # (j, c, b) of the diagonals with a non-zero
    for k0 in range(0, len(cand), chunk):
        part = cand[k0:k0 + chunk]
        rows = pre_rotated_rows(W, n, [(c, j * B, b) for (c, j, b) in part])
        nz = rows.any(axis=1)
        if nz.any():
            emit(len(kept), rows[nz])
            kept.extend((j, c, b) for (c, j, b), z in zip(part, nz) if z)
    plan.babies = sorted({0} | {b for (_, _, b) in kept})
    pos = {b: i for i, b in enumerate(plan.babies)}
    for (j, c, b) in kept:                                           # (cand is ordered by (j, c, b): the terms of a group are neighbours)
        if not plan.groups or plan.groups[-1] != (j, c):
            if plan.groups:
                plan.grp_off.append(len(plan.ct_idx))
            plan.groups.append((j, c))
        plan.ct_idx.append(pos[b])
    plan.grp_off.append(len(plan.ct_idx))
    if not kept:
        raise ValueError("the matrix is zero")
    return plan


def rot_slots(x, i):
    """RotateRows(+i) on slot values"""
    m = x.shape[-1] // 2
    return np.roll(x.reshape(x.shape[:-1] + (2, m)), -int(i), axis=-1).reshape(x.shape)


def swap_slots(x):
    """RotateColumns on slot values"""
    m = x.shape[-1] // 2
    return x.reshape(x.shape[:-1] + (2, m))[..., ::-1, :].reshape(x.shape)


def evaluate_on_slots(plan, rows, v, t):
    """the plan's evaluation order in plain slot arithmetic mod t (Python integers): rows = the emitted plaintext slots [terms, n], v = the n input slots.  What the
    ciphertext path computes slot by slot - the model tests/test_diagonal_plan.py holds against W v."""
    n = plan.n
    kind = np.int64 if int(t) < 2 ** 31 else object                  # (products of two residues below 2^62 fit int64)
    v = np.asarray(v, dtype=object) % t
    v = v.astype(kind)
    bab = [rot_slots(v, b) for b in plan.babies]
    u = []
    for g in range(len(plan.groups)):
        acc = np.zeros(n, dtype=kind)
        for e in range(plan.grp_off[g], plan.grp_off[g + 1]):
            acc = (acc + np.asarray(rows[e]).astype(kind) * bab[plan.ct_idx[e]]) % t
        u.append(acc)
    if plan.giants_by_folding:
        nc, half = len(plan.classes), plan.Gs // 2
        while half >= 1:
            for x in range(nc * half):
                u[x] = (u[x] + rot_slots(u[nc * half + x], half * plan.B)) % t
            half //= 2
        tot = [None, None]
        for x, c in enumerate(plan.classes):
            tot[c] = u[x]
    else:
        tot = [None, None]
        for g, (j, c) in enumerate(plan.groups):
            x = rot_slots(u[g], j * plan.B) if j else u[g]
            tot[c] = x if tot[c] is None else (tot[c] + x) % t
    if tot[1] is None:
        return tot[0]
    return swap_slots(tot[1]) if tot[0] is None else (tot[0] + swap_slots(tot[1])) % t
