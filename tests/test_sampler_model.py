"""CPU: the model of the device samplers, keygen and encryption (tests/sampler_model.py) against the documented distribution.

* the thresholds the library computes (cn_noise_table.h, long double erf; printed by tests/cpp/noise_table.cpp) against the exact ones (mpmath, 256 bits);
* the structure of the draws: value ranges, the redraw of an all-3 ternary word, no two blocks of a key generation and two encryptions share a counter;
* the distribution: chi-square of 2^22 noise and 2^22 ternary coefficients per key against the exact probabilities, and the SAME statistic on near misses
  (sigma 3.1 / 3.3, rounding to nearest, thresholds shifted by one index, a sign taken with probability 0.51, a ternary P(0) of 0.34), which it must reject;
* independence of the streams, items and nonces.

The GPU side (tests/test_gpu_sampler_kat.py) holds every word of the device's keys and ciphertexts to this model, so what is shown here about the model's
distribution holds for the device."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import sampler_model as M
import seeded_model as sm
from sampler_cases import CASES, make_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three fixed (key, nonce): the second nonce has a non-zero high word
KEYS = [(bytes(range(32)), 7), (bytes((11 * i + 5) & 0xff for i in range(32)), (0x9e3779b9 << 32) | 0x7f4a7c15), (bytes(32), 1 << 32)]
DRAWS = 1 << 22                     # coefficients per key and distribution: enough for every near miss below (see test_distribution_*)
P_ACCEPT, P_REJECT = 1e-4, 1e-9


# ---------------------------------------------------------------- thresholds
@pytest.fixture(scope="module")
def library_thresholds():
    exe = os.path.join(tempfile.mkdtemp(), "noise_table")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "noise_table.cpp"), "-o", exe])
    return [int(x, 16) for x in subprocess.check_output([exe]).decode().split()]


def test_library_thresholds_are_the_exact_ones(library_thresholds):
    """|library - exact| <= 2^10 units of 2^-63 (about the last place of a plain double; a wrong sigma, clip or index moves a threshold by more than 2^40).
    Measured with g++ long double: the library's value is the exact floor or one above it, maximum difference 1 unit (at i = 6, 7, 10, 14, 16, 17)."""
    exact = M.noise_thresholds()
    assert len(library_thresholds) == len(exact) == 19
    diff = [g - e for g, e in zip(library_thresholds, exact)]
    print("threshold differences (library - exact, units of 2^-63):", diff)
    assert max(abs(d) for d in diff) <= 1 << 10, diff
    for thr in (library_thresholds, exact):
        assert all(a < b for a, b in zip(thr, thr[1:])), "thresholds are not strictly increasing"
        assert 0 < thr[0] and thr[-1] < (1 << 63) - 1
    # the sensitivity the bound relies on: the nearest wrong tables are far away
    for wrong in (M.noise_thresholds(sigma=3.1), M.noise_thresholds(sigma=3.3), M.noise_thresholds(clip=16.0), M.noise_thresholds(nearest=True), M.shifted(exact)):
        assert max(abs(a - b) for a, b in zip(wrong, exact)) > 1 << 40


def test_documented_standard_deviation():
    """sigma 3.2 clipped at 19.2 and truncated towards zero has standard deviation 2.83 (not 3.2)"""
    p = M.noise_probabilities(M.noise_thresholds())
    v = np.arange(-19, 20)
    assert abs(p.sum() - 1) < 1e-12 and abs((p * v).sum()) < 1e-12
    assert abs(float(np.sqrt((p * v * v).sum())) - 2.8283) < 1e-3


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize("key,nonce", KEYS, ids=["key%d" % i for i in range(len(KEYS))])
def test_value_ranges_and_layout(key, nonce):
    n = 1024
    t = M.sample_ternary(key, nonce, 0, 3, n)
    e = M.sample_noise(key, nonce, 1, 3, n)
    assert t.shape == e.shape == (n,) and set(np.unique(t)) <= {-1, 0, 1} and int(np.abs(e).max()) <= 19
    # coefficient c of block blk: word c of the block (ternary), the word pair (2c, 2c + 1) (noise) - by hand, with Python integers
    thr = M.noise_thresholds()
    for blk in (0, 5, n // 16 - 1):
        w = sm.chacha20_block(key, sm.rng_counter(3, 0, 0, blk), nonce)[0]
        for c in range(16):
            pairs = [(int(w[c]) >> b) & 3 for b in range(0, 32, 2)]
            assert int(t[16 * blk + c]) == next(p for p in pairs if p != 3) - 1
        w = sm.chacha20_block(key, sm.rng_counter(3, 1, 0, blk), nonce)[0]
        for c in range(8):
            v = (int(w[2 * c]) << 32) | int(w[2 * c + 1])
            k = sum(1 for x in thr if x <= v & ((1 << 63) - 1))
            assert int(e[8 * blk + c]) == (-k if v >> 63 else k)
    # the nonce enters with all 64 bits, the streams and items differ
    assert not np.array_equal(e, M.sample_noise(key, nonce ^ (1 << 40), 1, 3, n))
    assert not np.array_equal(e, M.sample_noise(key, nonce, 2, 3, n)) and not np.array_equal(e, M.sample_noise(key, nonce, 1, 4, n))


def test_ternary_redraw_takes_the_word_of_the_next_trial():
    """a word whose sixteen pairs are all 3 has probability 2^-32: the 3 * 2^22 words of test_distribution_ternary hold none (it prints the count), so the path
    is forced here through a generator whose trial-0 block has such words - the model then takes word c of the block of trial 1 (and of trial 2 where that one
    is all-3 again), for the pending coefficients only"""
    key, nonce = KEYS[0]
    calls = []

    def rigged(k, nc, stream, items, blks, trial=0):
        w = M.blocks(k, nc, stream, items, blks, trial).copy()
        calls.append((trial, [int(b) for b in np.atleast_1d(blks)]))
        if trial == 0:
            w[2, 5] = w[2, 9] = w[4, 0] = 0xffffffff           # block 2 words 5, 9; block 4 word 0
        if trial == 1 and list(np.atleast_1d(blks)) == [2]:
            w[0, 9] = 0xffffffff                               # ... and word 9 of block 2 once more
        return w
    got, redrawn = M.sample_ternary_items(key, nonce, 0, [6], 128, block_fn=rigged)
    plain = M.sample_ternary(key, nonce, 0, 6, 128)
    want = plain.copy()
    for blk, c, trial in ((2, 5, 1), (2, 9, 2), (4, 0, 1)):
        w = int(sm.chacha20_block(key, sm.rng_counter(6, 0, trial, blk), nonce)[0][c])
        want[16 * blk + c] = next(p for p in ((w >> b) & 3 for b in range(0, 32, 2)) if p != 3) - 1
    assert redrawn == 3 and np.array_equal(got[0], want)
    assert sorted(calls) == [(0, list(range(8))), (1, [2]), (1, [4]), (2, [2])]


def test_no_two_blocks_share_a_counter(monkeypatch):
    """every generator block of a whole key generation (Galois keys included) and of two encryptions behind it, at the largest case of the GPU test (N = 16384:
    2048 blocks per limb), redraws included: the counters (item, stream, trial, blk) are pairwise distinct per nonce"""
    seen = {}
    real = sm.chacha20_block

    def recording(key, counter, nonce):
        seen.setdefault(int(nonce), []).append(np.atleast_1d(np.asarray(counter, dtype=np.uint64)).copy())
        return real(key, counter, nonce)
    monkeypatch.setattr(sm, "chacha20_block", recording)
    case = CASES["E"]
    o = make_oracle(case)
    key, seed = KEYS[1]
    K = M.keygen_model(o, key, seed, galois=True)
    plains = [None, None, None]
    M.encrypt_model(o, key, seed, K["items"], K["pk"], plains)
    M.encrypt_model(o, key, seed, K["items"] + len(plains), K["pk"], plains[:2])
    M.encrypt_model(o, key, seed + 1, 0, K["pk"], plains[:1])                     # another nonce: its own space
    entries = sum(M.digit_counts(o.q, o.dbc)) + len(M.default_galois_elts(o.n)) * sum(M.digit_counts(o.q, o.gdbc))
    assert K["items"] == 3 + 2 * entries
    for nonce, parts in seen.items():
        ctr = np.concatenate(parts)
        assert len(np.unique(ctr)) == len(ctr), "nonce %#x: %d blocks, %d distinct counters" % (nonce, len(ctr), len(np.unique(ctr)))
    n8 = o.n // 8
    assert len(np.concatenate(seen[seed])) >= entries * (o.k * n8 + n8) + 5 * (o.n // 16 + 2 * n8)


# ---------------------------------------------------------------- distribution
def chi_square_p(counts, probs):
    """p-value of Pearson's statistic.  Cells whose expectation is below 5 (the values beyond +-14 at 2^22 draws: P(|x| >= 15) = 2.8e-6) are pooled with their
    neighbours towards the centre, per side - the chi-square approximation needs that; the number of cells left is printed with the result"""
    import mpmath
    counts, expect = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64) * float(np.sum(counts))
    c, e = list(counts), list(expect)
    while len(e) > 2 and e[0] < 5:
        e[1] += e[0]; c[1] += c[0]; del e[0], c[0]
    while len(e) > 2 and e[-1] < 5:
        e[-2] += e[-1]; c[-2] += c[-1]; del e[-1], c[-1]
    c, e = np.array(c), np.array(e)
    stat = float(((c - e) ** 2 / e).sum())
    return float(mpmath.gammainc((len(e) - 1) / 2.0, stat / 2.0, mpmath.inf, regularized=True)), stat, len(e)


@pytest.fixture(scope="module")
def raw_noise_blocks():
    """the generator blocks behind DRAWS noise coefficients per key: stream 1, items 0 .. 7 of 2^16 blocks (8 coefficients each)"""
    return [M.blocks(key, nonce, M.ST_E1, np.arange(DRAWS // 8 >> 16), np.arange(1 << 16)) for key, nonce in KEYS]


def noise_counts(values):
    return np.bincount(values.reshape(-1).astype(np.int64) + 19, minlength=39)


def test_distribution_of_the_noise(raw_noise_blocks):
    """2^22 coefficients per key over the 39 values against the exact probabilities of the mpmath thresholds: p >= 1e-4 for the model on every key, p < 1e-9 for
    every near miss on every key.  2^22 draws suffice for all of them; the weakest is the 0.51 sign (statistic about 1 250 on 30 degrees of freedom, p below
    1e-240).  Measured p of the model on the three keys: 0.92, 0.84, 0.75."""
    mp = M._mp()
    assert mp is not None
    thr = M.noise_thresholds()
    probs = M.noise_probabilities(thr)
    near = {"sigma 3.1": dict(thr=M.noise_thresholds(sigma=3.1)), "sigma 3.3": dict(thr=M.noise_thresholds(sigma=3.3)),
            "rounded to nearest": dict(thr=M.noise_thresholds(nearest=True)), "thresholds shifted by one index": dict(thr=M.shifted(thr)),
            "sign with probability 0.51": dict(thr=thr, sign_p=0.51)}
    for (key, nonce), w in zip(KEYS, raw_noise_blocks):
        assert w.shape[0] * 8 == DRAWS
        values = M.noise_from_blocks(w, thr)
        assert np.array_equal(values[:128].reshape(-1), M.sample_noise(key, nonce, M.ST_E1, 0, 1024))          # the draw of the model, not a relative of it
        p, stat, cells = chi_square_p(noise_counts(values), probs)
        print("noise, nonce %#x: chi-square %.1f over %d cells, p = %.3g; std %.4f" % (nonce, stat, cells, p, values.std()))
        assert p >= P_ACCEPT, (nonce, stat, p)
        for name, kw in near.items():
            pn, statn, _ = chi_square_p(noise_counts(M.noise_from_blocks(w, **kw)), probs)
            print("    near miss %-32s chi-square %10.1f, p = %.3g" % (name, statn, pn))
            assert pn < P_REJECT, (name, nonce, statn, pn)


def test_distribution_of_the_ternary_draw():
    """2^22 coefficients per key over {-1, 0, 1} against 1/3 each: p >= 1e-4 for the model, p < 1e-9 for a draw with P(0) = 0.34 (statistic 770 to 850 on two
    degrees of freedom at 2^22 draws).  Measured p of the model on the three keys: 0.49, 0.80, 0.62.  Prints how many all-3 words (redraws) the 2^22 words held."""
    M._mp()
    third = np.full(3, 1 / 3)
    for key, nonce in KEYS:
        w = M.blocks(key, nonce, M.ST_TERNARY, np.arange(DRAWS // 16 >> 14), np.arange(1 << 14))
        assert w.size == DRAWS
        values = M.ternary_from_words(w)
        assert np.array_equal(values[:64].reshape(-1), M.sample_ternary(key, nonce, M.ST_TERNARY, 0, 1024))
        pending = int((values == 2).sum())
        print("ternary, nonce %#x: %d all-3 words among %d (bounded search for a natural redraw: %s)" % (nonce, pending, w.size, "found" if pending else "none found"))
        values = values[values != 2]
        p, stat, _ = chi_square_p(np.bincount(values.reshape(-1).astype(np.int64) + 1, minlength=3), third)
        print("    chi-square %.2f, p = %.3g" % (stat, p))
        assert p >= P_ACCEPT, (nonce, stat, p)
        pn, statn, _ = chi_square_p(np.bincount(M.ternary_from_words(w, p0=0.34).reshape(-1).astype(np.int64) + 1, minlength=3), third)
        print("    near miss P(0) = 0.34: chi-square %.1f, p = %.3g" % (statn, pn))
        assert pn < P_REJECT, (nonce, statn, pn)


def corr(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    return float(np.corrcoef(a, b)[0, 1])


@pytest.mark.parametrize("key,nonce", KEYS, ids=["key%d" % i for i in range(len(KEYS))])
def test_streams_items_and_nonces_are_independent(key, nonce):
    """sample correlation below 5 / sqrt(samples) (five standard deviations of the correlation of independent samples): e1 against e2 of one item, u of items
    i and i + 1, the noise of stream 1 under the nonces x and x + 1; 2^18 samples each"""
    items, n = np.arange(4, 8), 1 << 16
    samples = len(items) * n
    bound = 5 / np.sqrt(samples)
    e1, e2 = M.sample_noise_items(key, nonce, M.ST_E1, items, n), M.sample_noise_items(key, nonce, M.ST_E2, items, n)
    u, _ = M.sample_ternary_items(key, nonce, M.ST_TERNARY, np.arange(4, 9), n)
    x1 = M.sample_noise_items(key, nonce + 1, M.ST_E1, items, n)
    for name, c in (("e1 ~ e2", corr(e1, e2)), ("u[i] ~ u[i + 1]", corr(u[:-1], u[1:])), ("nonce x ~ x + 1", corr(e1, x1))):
        print("%-16s %+.5f (bound %.5f)" % (name, c, bound))
        assert abs(c) < bound, (name, c)
    assert abs(corr(e1, e1) - 1) < 1e-12                                         # (the statistic sees a shared stream)
