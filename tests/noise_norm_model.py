"""Python model of k_noise_norm (cryptonets_amd/csrc/cn_k_noise.hip.h), word for word: the K-word CRT composition, the FP64 estimate of
the quotient with its one correction, the centring and the K-word comparison.  An estimate forced off by one runs both corrections of the
kernel's exactness argument."""
MASK = (1 << 64) - 1


def words(x, k):
    return [(x >> (64 * i)) & MASK for i in range(k)]


def value(ws):
    return sum(int(w) << (64 * i) for i, w in enumerate(ws))


def prod(q):
    Q = 1
    for m in q:
        Q *= int(m)
    return Q


def less(a, b):
    """a < b as K-word integers, scanned like nn_less: the highest differing word decides"""
    lt = False
    for x, y in zip(a, b):
        lt = x < y or (x == y and lt)
    return lt


def y_of(X, q):
    """the kernel's per-limb inputs for the noise value X: y_j = [x_j (Q/q_j)^-1]_{q_j}, x_j = X mod q_j"""
    Q = prod(q)
    return [(X % m) * pow((Q // m) % m, -1, m) % m for m in map(int, q)]


def norm_words(y, q, a=None):
    """centred |[sum_j y_j Q/q_j]_Q| as K words, as k_noise_norm computes it; `a`: the quotient estimate to use instead of the FP64 one"""
    q = [int(m) for m in q]
    K, Q = len(q), prod(q)
    Qw = words(Q, K)
    if K == 1:
        X = [y[0]]
    else:
        X, s = [0] * K, 0.0
        for j, m in enumerate(q):
            qh = words(Q // m, K)
            assert qh[K - 1] == 0                                  # q/q_j < 2^(61 (K - 1)): K - 1 words
            s += float(y[j]) * (1.0 / m)                           # (the kernel fuses this into one FMA)
            carry = 0
            for w in range(K - 1):
                p = y[j] * qh[w] + X[w] + carry
                X[w], carry = p & MASK, p >> 64
            X[K - 1] += carry
            assert X[K - 1] <= MASK                                # S < K q < 2^(64 K)
        a = int(s) if a is None else a
        mc = br = 0
        for w in range(K):
            p = a * Qw[w] + mc
            sub, mc = p & MASK, p >> 64
            d = (X[w] - sub) & MASK
            b1 = X[w] < sub
            X[w] = (d - br) & MASK
            br = int(b1 or d < br)
        assert mc == 0                                             # a q < 2^(64 K)
        if br:
            cy = 0
            for w in range(K):
                u = (X[w] + Qw[w]) & MASK
                c1 = u < X[w]
                X[w] = (u + cy) & MASK
                cy = int(c1 or X[w] < u)
        elif not less(X, Qw):
            bw = 0
            for w in range(K):
                d = (X[w] - Qw[w]) & MASK
                b1 = X[w] < Qw[w]
                X[w] = (d - bw) & MASK
                bw = int(b1 or d < bw)
    D, bw = [], 0
    for w in range(K):
        d = (Qw[w] - X[w]) & MASK
        b1 = Qw[w] < X[w]
        D.append((d - bw) & MASK)
        bw = int(b1 or d < bw)
    return D if less(D, X) else X


def centred(X, Q):
    """the host's centring: X if 2X <= Q, else Q - X"""
    return X if 2 * X <= Q else Q - X
