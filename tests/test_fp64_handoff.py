"""The lazy-FP64 hand-off between the tensor kernels and the BEHZ floor (cryptonets_amd/csrc/cn_dev_common.hip.h: lazy_word).

On the FP64 policies k_square_pipe, k_square_fused (operand parked in LDS or in the output's place) and k_intt_tensor store the registers of their
inverse transforms as they are - doubles without the 1/N factor, |x| <= 8.5 p - and k_behz_floor_f64 multiplies them with constants that carry N^-1
(DevConsts::bd.fl_c1n_q, fl_Tn_bsk).  Every step is exact arithmetic modulo the same primes, so a product has the words it always had:

  * GPU: cn_multiply(a, a) and cn_multiply(a, b) for 1, 100 and 845 ciphertexts of the CryptoNets set under every squaring form ("sq_pipe" 0 / 1 / 2,
    "sq_lds" 0 / 1) and with the separate launches - all forms word for word the same in full, and the oracle's words on a sample; the same on five
    primes just below 2^49 (ArF64T<1> on the data side as well: |x| <= 8.5 p under p < 2^49 is where mulmod's 16 p is nearest), on operands at the
    edges of the residue range too; a context with a 50-bit modulus (integer transforms and floor) and one with FP64 transforms beside the integer
    floor keep the canonical u64 words;
  * CPU: the two constant tables, recomputed from Python integers, against what cn_tables.cpp builds (compiled here with the host compiler).
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PARAMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def ntt_primes(bits, n, count, avoid=()):
    """the `count` largest primes below 2^bits that are 1 mod 2n and not in `avoid`, decreasing"""
    out, x = [], ((1 << bits) - 1) // (2 * n) * (2 * n) + 1
    while len(out) < count:
        if x not in avoid and is_prime(x):
            out.append(x)
        x -= 2 * n
    return out


TINY_Q = [0xffffee001, 0xffffc4001, 0x1ffffe0001]
SETS = {
    "c3": dict(PARAMS["c3"]),
    # the five largest NTT primes below 2^49 at N = 8192: the widest moduli cn_build_f64_tables admits, the CryptoNets shapes (k = 5, L = 13: four
    # stages in the last pass of the inverse transform).  The auxiliary base is then the next six such primes: log2 t + 13 + 2 < 49 holds for t = 65537
    "top49": dict(n=8192, t=65537, q=ntt_primes(49, 8192, 5), dbc=60, gdbc=60),
    # one modulus of 50 bits: integer transforms, SEAL's 61-bit auxiliary base, integer floor
    "int50": dict(n=1024, t=12289, q=[TINY_Q[0], ntt_primes(50, 1024, 1)[0]], dbc=60, gdbc=60),
    # two FP64-capable data limbs beside a 54-bit one: the q base as a whole, the 61-bit auxiliary base and the floor take the integer policy
    "mix2048": dict(n=2048, t=12289, q=TINY_Q[:2] + [0x3fffffff000001], dbc=60, gdbc=60),
    # every data modulus below 2^49 but SEAL's 61-bit auxiliary base forced: FP64 q-side tensor kernel, integer Bsk side and integer floor
    "tiny": dict(PARAMS["tiny"]),
}
FORMS = [dict(sq_fused=1, sq_lds=1, sq_pipe=0), dict(sq_fused=1, sq_lds=1, sq_pipe=1), dict(sq_fused=1, sq_lds=1, sq_pipe=2),
         dict(sq_fused=1, sq_lds=0, sq_pipe=0), dict(sq_fused=0, sq_lds=1, sq_pipe=1)]
DEFAULT_FORM = dict(sq_fused=1, sq_lds=1, sq_pipe=1)


def make(name):
    from cryptonets_amd._native import Context
    from oracle.cno import Oracle
    p = SETS[name]
    o = Oracle(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"])
    g = Context(p["n"], p["t"], q=p["q"], dbc=p["dbc"], gdbc=p["gdbc"], device=0)
    return o, g


def words(rng, o, count):
    """uniform ciphertext words (the evaluator is a function of words)"""
    return np.stack([np.concatenate([rng.integers(0, q, size=o.n, dtype=np.uint64) for _ in range(2) for q in o.q]) for _ in range(count)])


def edge_words(o):
    """every coefficient 0, q - 1, floor(q/2), ceil(q/2), alternating +-q/2 (as residues of every q_j), each beside the q/2 pattern and beside itself"""
    Q, n = 1, o.n
    for m in o.q:
        Q *= int(m)
    pats = [[0] * n, [Q - 1] * n, [Q // 2] * n, [Q // 2 + 1] * n, [(Q // 2) if i % 2 else (Q - Q // 2) for i in range(n)]]
    cts = []
    for pa in pats:
        for pb in (pats[2], pa):
            cts.append(np.concatenate([np.array([x % int(qj) for x in poly], dtype=np.uint64) for poly in (pa, pb) for qj in o.q]))
    return np.stack(cts)


def run_forms(g, h, hb, cnt, out3):
    """products of ciphertexts [0, cnt) of h with those of hb under every squaring form; returns the first form's words after comparing all in full"""
    first = None
    try:
        for form in FORMS:
            for k, v in form.items():
                g.set_option(k, v)
            g.multiply(h, 0, hb, 0, out3, 0, cnt)
            got = g.ct_download(out3, 0, cnt, size=3)
            if first is None:
                first = got
            else:
                assert np.array_equal(got, first), form
    finally:
        for k, v in DEFAULT_FORM.items():
            g.set_option(k, v)
    return first


def check_against_oracle(o, got, a, b, sample):
    for i in sample:
        assert np.array_equal(got[i], o.multiply(a[i], b[i])), i


@pytest.mark.gpu
@pytest.mark.parametrize("cnt", [1, 100, 845])
def test_cryptonets_products_keep_their_words(cnt, rng):
    o, g = make("c3")
    assert g.get_option("behz_f64") == 1
    a, b = words(rng, o, cnt), words(rng, o, cnt)
    a[0] = edge_words(o)[1]                                       # every word q_j - 1
    ha, hb, out3 = g.ct_alloc(cnt), g.ct_alloc(cnt), g.ct_alloc(cnt, 3)
    g.ct_upload(ha, 0, a)
    g.ct_upload(hb, 0, b)
    sample = sorted({0, cnt // 2, cnt - 1})
    sq = run_forms(g, ha, ha, cnt, out3)                         # squarings: k_square_fused (LDS / in place), k_square_pipe, separate launches
    check_against_oracle(o, sq, a, a, sample)
    del sq
    ab = run_forms(g, ha, hb, cnt, out3)                         # a != b: k_intt_tensor
    check_against_oracle(o, ab, a, b, sample)
    for x in (ha, hb, out3):
        g.free(x)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cnt", [1, 100])
def test_products_on_primes_just_below_2_to_49(cnt, rng):
    """ArF64T<1> on both bases; the edge operands drive the tensor to its largest magnitudes"""
    o, g = make("top49")
    assert all(int(q).bit_length() == 49 for q in o.q) and g.get_option("behz_f64") == 1
    e = edge_words(o)
    a, b = words(rng, o, cnt), words(rng, o, cnt)
    m = min(cnt, len(e))
    a[:m] = e[:m]
    b[:m] = e[::-1][:m]
    ha, hb, out3 = g.ct_alloc(cnt), g.ct_alloc(cnt), g.ct_alloc(cnt, 3)
    g.ct_upload(ha, 0, a)
    g.ct_upload(hb, 0, b)
    sample = sorted(set(range(m)) | {cnt - 1})
    sq = run_forms(g, ha, ha, cnt, out3)
    check_against_oracle(o, sq, a, a, sample)
    ab = run_forms(g, ha, hb, cnt, out3)
    check_against_oracle(o, ab, a, b, sample)
    for x in (ha, hb, out3):
        g.free(x)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["int50", "mix2048", "tiny"])
def test_integer_floor_keeps_the_canonical_words(name, rng, monkeypatch):
    """a modulus of 50 bits (integer policy throughout), FP64-capable limbs beside a 54-bit one, and - "tiny" under SEAL's 61-bit auxiliary base - the
    FP64 tensor kernels on the q side in front of the INTEGER floor: the tensor limbs stay canonical u64 words"""
    if name == "tiny":
        monkeypatch.setenv("CN_SEAL_AUX", "1")
    o, g = make(name)
    assert g.get_option("behz_f64") == 0
    cnt = 6
    a, b = words(rng, o, cnt), words(rng, o, cnt)
    a[:3] = edge_words(o)[[1, 2, 4]]
    ha, hb, out3 = g.ct_alloc(cnt), g.ct_alloc(cnt), g.ct_alloc(cnt, 3)
    g.ct_upload(ha, 0, a)
    g.ct_upload(hb, 0, b)
    check_against_oracle(o, run_forms(g, ha, ha, cnt, out3), a, a, range(cnt))
    check_against_oracle(o, run_forms(g, ha, hb, cnt, out3), a, b, range(cnt))
    for x in (ha, hb, out3):
        g.free(x)
    g.close()


@pytest.mark.gpu
def test_f64_switched_off_at_run_time_keeps_the_canonical_words(rng):
    """cn_set_option("f64", 0) on a context whose tables admit the FP64 floor: integer tensor kernels, integer floor, the same words"""
    o, g = make("tiny")
    cnt = 4
    a, b = words(rng, o, cnt), words(rng, o, cnt)
    ha, hb, out3 = g.ct_alloc(cnt), g.ct_alloc(cnt), g.ct_alloc(cnt, 3)
    g.ct_upload(ha, 0, a)
    g.ct_upload(hb, 0, b)
    got = {}
    try:
        for f64 in (1, 0, 1):
            g.set_option("f64", f64)
            got[f64] = (run_forms(g, ha, ha, cnt, out3), run_forms(g, ha, hb, cnt, out3))
    finally:
        g.set_option("f64", 1)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    check_against_oracle(o, got[0][0], a, a, range(cnt))
    check_against_oracle(o, got[0][1], a, b, range(cnt))
    for x in (ha, hb, out3):
        g.free(x)
    g.close()


# ------------------------------------------------------------------ the constant tables, without a GPU
PROBE = r"""
#include "cn_internal.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
int main(int argc, char **argv) {
    const uint32_t n = (uint32_t)strtoul(argv[1], nullptr, 0), k = (uint32_t)argc - 3;
    const uint64_t t = strtoull(argv[2], nullptr, 0);
    std::vector<uint64_t> q;
    for (int i = 3; i < argc; i++) q.push_back(strtoull(argv[i], nullptr, 0));
    std::vector<uint64_t> tw((size_t)(2 * k + 3) * 4 * n);
    std::vector<double> twd((size_t)(2 * k + 3) * 2 * n);
    std::vector<uint32_t> map(n);
    static DevConsts c;
    char err[256];
    if (cn_build_consts(&c, n, q.data(), k, t, 60, 60, tw.data(), map.data(), err, sizeof err)) { fprintf(stderr, "%s\n", err); return 1; }
    cn_build_f64_tables(&c, tw.data(), twd.data());
    printf("{\"behz_f64\": %u, \"kb\": %u, \"bsk\": [", c.behz_f64, c.kb);
    for (uint32_t b = 0; b < c.kb; b++) printf("%s%llu", b ? ", " : "", (unsigned long long)c.bsk[b].q);
    printf("], \"fl_c1n_q\": [");
    for (uint32_t j = 0; j < k; j++) printf("%s%.0f", j ? ", " : "", c.bd.fl_c1n_q[j]);
    printf("], \"fl_Tn_bsk\": [");
    for (uint32_t b = 0; b < c.kb; b++) printf("%s%.0f", b ? ", " : "", c.bd.fl_Tn_bsk[b]);
    printf("]}\n");
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler: cn_tables.cpp cannot be compiled for the table check")
    d = tmp_path_factory.mktemp("handoff_probe")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    csrc = os.path.join(ROOT, "cryptonets_amd", "csrc")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-I", csrc, str(src), os.path.join(csrc, "cn_tables.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("name", ["c3", "top49", "tiny", "n16k7"])
def test_handoff_constants_from_big_integers(name, probe):
    """fl_c1n_q[j] = t (q/q_j)^-1 N^-1 mod q_j and fl_Tn_bsk[b] = t q^-1 N^-1 mod b, over the auxiliary base the tables chose"""
    from cryptonets_amd import _native
    p = SETS.get(name) or PARAMS[name]
    n, t = p["n"], p["t"]
    q = [int(x) for x in (p["q"] or _native.default_coeff_modulus(n))]
    got = json.loads(subprocess.check_output([probe, str(n), str(t)] + [str(x) for x in q], env={k: v for k, v in os.environ.items() if k != "CN_SEAL_AUX"}))
    assert got["behz_f64"] == 1 and all(b < (1 << 49) for b in got["bsk"])
    Q = 1
    for m in q:
        Q *= m
    c1n = [t * pow(Q // m, -1, m) * pow(n, -1, m) % m for m in q]
    Tn = [t * pow(Q, -1, b) * pow(n, -1, b) % b for b in got["bsk"]]
    assert got["fl_c1n_q"] == c1n
    assert got["fl_Tn_bsk"] == Tn
