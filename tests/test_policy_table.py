"""The two decisions of cryptonets_amd/csrc/cn_policy.h on the CPU: tests/cpp/policy_table.cpp builds the tables of every parameter set of the suite
(cn_tables.cpp, plain g++) and prints, for both values of the "f64" option, what cn_mod_range and cn_policy answer for the q limbs and their prefixes, the
BEHZ auxiliary base, both together, the plain modulus and every single modulus - beside the moduli it read.  Every answer is recomputed here from those
moduli with Python integers (bit_length, < 2**49, <= 44 bits); the anchors below are the parent's answers, spelt out.  The three policies give the same
words, so the GPU suite cannot tell a wrong pick from a right one: this table can.
A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program."""
import os
import subprocess
import tempfile

import pytest

from conftest import PARAMS
from oracle.cno import COEFF_MODULUS_128
from size_policy_sets import CELLS, NAME, SETS as SIZE_POLICY_SETS      # one set per (policy, ring size) of tests/test_gpu_size_policy_matrix.py
from test_gpu_wide_moduli import SETS                       # the wide-modulus sets and ring sizes (a prime search at import, no device)
from test_oracle_math import is_prime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cryptonets_amd", "csrc")
ALL_SETS = dict(PARAMS, **SETS, **SIZE_POLICY_SETS)
assert len(ALL_SETS) == len(PARAMS) + len(SETS) + len(SIZE_POLICY_SETS) and len(SIZE_POLICY_SETS) == 15


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "policy_table")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "policy_table.cpp"),
                           os.path.join(CSRC, "cn_tables.cpp"), "-o", exe])
    return exe


def run(exe):
    path = os.path.join(tempfile.mkdtemp(), "sets.txt")
    with open(path, "w") as f:
        for name, p in ALL_SETS.items():
            q = p["q"] or []                                # none: the program asks cn_default_coeff_modulus_impl
            f.write("%s %d %d %d %d %d %s\n" % (name, p["n"], p["t"], p["dbc"], p["gdbc"], len(q), " ".join("%x" % x for x in q)))
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def parse(text):
    """{set: (header fields, {(use_f64, base_off, nmod): (f64ok, light, bits, qmax, policy, moduli)})}"""
    out, rows = {}, None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "set":
            rows = {}
            out[w[1]] = (dict(zip(("n", "t", "batching", "k", "kb"), map(int, w[2:]))), rows)
        else:
            assert w[0] == "r" and rows is not None, line
            key = (int(w[1]), int(w[2]), int(w[3]))
            assert key not in rows or key[2] == 1, line     # (single moduli are printed again as ranges of one: q of k = 1, t)
            rows[key] = (int(w[4]), int(w[5]), int(w[6]), int(w[7], 16), w[8], [int(x, 16) for x in w[9:]])
            assert len(rows[key][5]) == key[2], line
    return out


def check(tables):
    """every printed answer against Python integers; returns the number of answers checked"""
    assert sorted(tables) == sorted(ALL_SETS)
    checked = 0
    for name, p in ALL_SETS.items():
        hdr, rows = tables[name]
        n, t = p["n"], p["t"]
        q = list(p["q"] or COEFF_MODULUS_128[n])
        k, kb = len(q), hdr["kb"]                           # (the auxiliary base takes k + 2 primes where k + 1 below 2^49 are too few bits: n16k7, c5)
        batching = int(is_prime(t) and t % (2 * n) == 1)
        assert hdr == dict(n=n, t=t, batching=batching, k=k, kb=kb) and kb in (k + 1, k + 2), (name, hdr)
        both = rows[(1, 0, k + kb)][5]                      # the moduli in table order: q, the auxiliary base, then t
        assert both[:k] == q, name
        aux = both[k:]
        assert len(set(both)) == k + kb and all(is_prime(b) and b % (2 * n) == 1 for b in aux), name
        order = both + [t]
        asked = {(0, j) for j in range(1, k + 1)} | {(k, kb), (0, k + kb), (0, 0)} | {(m, 1) for m in range(k + kb + batching)}
        assert batching or (k + kb, 1) not in asked
        for use_f64 in (0, 1):
            assert {key[1:] for key in rows if key[0] == use_f64} == asked, name
            for off, nmod in asked:
                f64ok, light, bits, qmax, policy, moduli = rows[(use_f64, off, nmod)]
                assert moduli == order[off:off + nmod], (name, off, nmod)
                want_ok = all(m < 2 ** 49 and (i < k + kb or batching) for i, m in enumerate(moduli, off))
                want_light = all(m.bit_length() <= 44 for m in moduli)
                want = "U64" if not (use_f64 and want_ok) else ("F64L" if want_light else "F64")
                assert (f64ok, light, bits, qmax) == (int(want_ok), int(want_light), max(moduli, default=0).bit_length(), max(moduli, default=0)), (name, off, nmod)
                assert policy == want, (name, use_f64, off, nmod, policy, want)
                if not use_f64:
                    assert policy == "U64"
                checked += 1
    return checked


@pytest.fixture(scope="module")
def tables():
    r = run(build())
    assert r.returncode == 0, r
    return parse(r.stdout.decode())


def test_every_answer_matches_python_integers(tables):
    assert check(tables) > 2 * 6 * len(ALL_SETS)


def policy(tables, name, off, nmod, use_f64=1):
    return tables[name][1][(use_f64, off, nmod)][4]


def test_anchors(tables):
    """the parent's picks as literals; k and kb as the tables have them"""
    k = {name: tables[name][0]["k"] for name in tables}
    q = lambda name: policy(tables, name, 0, k[name])
    aux = lambda name: policy(tables, name, k[name], tables[name][0]["kb"])
    assert (k["c3"], tables["c3"][0]["kb"]) == (5, 6) and q("c3") == "F64L" and aux("c3") == "F64"
    assert policy(tables, "c3", 0, 11) == "F64" and policy(tables, "c3", 11, 1) == "F64L"       # q + auxiliary base; t
    for name in ("c5", "n16k7"):
        assert q(name) == "F64" and tables[name][1][(1, 0, k[name])][2] == 49                    # 48-49 bits
        assert min(m.bit_length() for m in tables[name][1][(1, 0, k[name])][5]) == 48
    for name in ("tiny", "default4096"):
        assert q(name) == "F64L" and aux(name) == "F64"
    for name in tables:
        assert all(row[4] == "U64" for key, row in tables[name][1].items() if key[0] == 0), name
    assert q("B44") == "F64L"
    for name in ("B45", "B46", "B47", "B49"):
        assert q(name) == "F64"
    for name in ("B50", "B60", "W60"):
        assert q(name) == "U64"
    assert policy(tables, "MIX2048", 0, 2) == "F64L" and policy(tables, "MIX2048", 0, 3) == "U64"
    assert tables["c3"][1][(1, 0, 0)][:4] == (1, 1, 0, 0)                                        # the empty range: bits 0, no clz of 0


def test_size_policy_cells_take_the_policy_they_are_named_for(tables):
    """the 15 cells of the size x policy matrix: the q range, its two-limb prefix (the level context) and every single limb take the named policy; the BEHZ
    auxiliary base has k + 1 primes, 61-bit ones (U64) beside the 60-bit set and 49-bit ones (F64) beside the other two"""
    want = {"u64": ("U64", "U64"), "f64": ("F64", "F64"), "f64l": ("F64L", "F64")}
    for pol, n in CELLS:
        name = NAME(pol, n)
        hdr = tables[name][0]
        assert (hdr["n"], hdr["k"], hdr["kb"], hdr["batching"]) == (n, 3, 4, 1), name
        assert (policy(tables, name, 0, 3), policy(tables, name, 3, 4)) == want[pol], name
        assert policy(tables, name, 0, 2) == want[pol][0], name
        assert all(row[4] == "U64" for key, row in tables[name][1].items() if key[0] == 0), name
    for n in (1024, 16384):
        assert [policy(tables, NAME("u64", n), j, 1) for j in range(3)] == ["U64"] * 3
        assert [policy(tables, NAME("f64", n), j, 1) for j in range(3)] == ["F64"] * 3
        assert [policy(tables, NAME("f64l", n), j, 1) for j in range(3)] == ["F64L"] * 3


def test_policy_header_is_clean_under_the_sanitizers(tables):
    """-fsanitize=undefined,address with errors fatal over the same sets (N = 16384 included): the same table, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == tables
