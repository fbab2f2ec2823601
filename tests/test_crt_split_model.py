"""The per-value arithmetic of cn_split_encode / cn_split_encrypt on the CPU: tests/cpp/crt_split_model.cpp calls the __host__ __device__ functions of
cryptonets_amd/csrc/cn_k_split.hip.h - scaling and rounding, the range test, the residue of every plaintext prime - that the kernel k_crt_split runs per
value.  Compared with Python's integers and with the numpy expression of EncryptedSealBfvVector.__init__ (rint, the 2^62 test, astype(int64), np.mod).
A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program (the negation of INT64_MIN is what it is for)."""
import os
import random
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from test_crt_join_model import is_prime, primes_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "crt_split_model.cpp")
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def moduli_sets():
    """P = 1 .. 8, 14 to 62 bits, equal moduli allowed (the call does not ask for different ones)"""
    sets = [primes_of(bits, P) for bits in (14, 20, 31, 40, 62) for P in (1, 2, 4, 8)]
    sets.append([primes_of(b, 1)[0] for b in (62, 31, 14, 40, 20, 61, 15, 50)])
    sets.append([12289, 12289, 65537])
    sets.append([557057, 638977])                           # two 20-bit batching primes of N = 8192
    return sets


def f64_inputs(ts, scale, rng):
    xs = [0.0, -0.0]
    for tie in (0.5, 1.5, 2.5):
        xs += [tie, -tie, tie * 3, -tie * 3, tie * 16384, -tie * 16384]
    xs += [0.1, -0.1, 0.7, 1.0 / 3.0, -2.0 / 3.0, 1e-3, 123456.789, -0.49999999999999994, 0.49999999999999994]      # products inexact in double
    for t in ts:
        for m in (t, -t, t - 1, 1 - t, 2 * t, -3 * t, t + 1):
            xs.append(float(m) / scale)                    # (lands on or next to a multiple of t after scaling)
            xs.append(float(m))
    top = np.nextafter(2.0 ** 62, 0.0)                      # the largest double below 2^62
    xs += [top / scale, -top / scale, np.nextafter(top / scale, 0.0), 2.0 ** 61 / scale]
    xs += [rng.uniform(-1, 1) * 10.0 ** rng.randrange(-3, 17) for _ in range(2000)]
    return [float(x) for x in xs]


BAD_F64 = [2.0 ** 62, -(2.0 ** 62), 2.0 ** 63, -(2.0 ** 64), 1e300, float("nan"), float("inf"), float("-inf")]


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "crt_split_model")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def cases():
    """(text of the case file, [(moduli, flags, scale, inputs as Python objects)])"""
    rng = random.Random(20261019)
    groups, lines = [], []
    for ts in moduli_sets():
        for scale in (1.0, 3.0, 16384.0):
            xs = f64_inputs(ts, scale, rng) + [b if scale == 1.0 else b / scale * 1.0000001 for b in BAD_F64]
            groups.append((ts, 0, scale, xs))
            lines.append("%d 0 %x %d %s" % (len(ts), bits_of(scale), len(xs), " ".join("%x" % t for t in ts)))
            lines.extend("%x" % bits_of(x) for x in xs)
        ws = [I64_MIN, I64_MAX, -1, 0, 1, I64_MIN + 1] + [m * t for t in ts for m in (1, -1, 2)] + [t - 1 for t in ts] + \
             [rng.randrange(I64_MIN, I64_MAX + 1) for _ in range(10000)]
        groups.append((ts, 1, 1.0, ws))
        lines.append("%d 1 %x %d %s" % (len(ts), bits_of(0.0), len(ws), " ".join("%x" % t for t in ts)))
        lines.extend("%x" % (w % 2 ** 64) for w in ws)
    return "\n".join(lines) + "\n", groups


def run(exe, text):
    path = os.path.join(tempfile.mkdtemp(), "cases.txt")
    with open(path, "w") as f:
        f.write(text)
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def check(out, groups):
    pos, checked, flagged = 0, 0, 0
    for ts, flags, scale, xs in groups:
        assert all(is_prime(t) for t in ts)
        if flags:
            want_rows = [[w % t for t in ts] for w in xs]                                   # Python integers
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                r = np.rint(np.asarray(xs, dtype=np.float64) * scale)                       # the expression of EncryptedSealBfvVector.__init__
                fits = np.abs(r) < 2.0 ** 62                                                # (False for NaN)
                w = np.where(fits, r, 0.0).astype(np.int64)
                cols = [np.mod(w, np.int64(t)) for t in ts]
            want_rows = [None if not fits[i] else [int(c[i]) for c in cols] for i in range(len(xs))]
            assert not fits[-len(BAD_F64):].any()                                           # 2^62, NaN, the infinities and beyond must be flagged
            if scale == 1.0:                                                                # ... and the largest doubles below 2^62 must not be
                top = float(np.nextafter(2.0 ** 62, 0.0))
                assert fits[xs.index(top)] and fits[xs.index(-top)] and int(w[xs.index(-top)]) == -(2 ** 62 - 2 ** 9)
            for i, x in enumerate(xs):                                                      # ... and Python's own rounding and integers
                if fits[i]:
                    assert want_rows[i] == [round(x * scale) % t for t in ts], (x, scale)
        for x, want in zip(xs, want_rows):
            line = out[pos]
            pos += 1
            if want is None:
                assert line == "bad", (ts, scale, x, line)
                flagged += 1
            else:
                assert [int(v, 16) for v in line.split()] == want, (ts, flags, scale, x, line)
            checked += 1
    return checked, flagged


def test_split_arithmetic_matches_python_and_numpy(cases):
    text, groups = cases
    r = run(build(), text)
    assert r.returncode == 0, r
    checked, flagged = check(r.stdout.decode().split("\n"), groups)
    assert checked > 300000 and flagged >= len(BAD_F64) * 3 * len(moduli_sets())


def test_split_arithmetic_is_clean_under_the_sanitizers(cases):
    """-fsanitize=undefined,address with errors fatal: INT64_MIN, -1 and the doubles next to 2^62 go through the same functions without a report"""
    text, groups = cases
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")), text)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    check(r.stdout.decode().split("\n"), groups)
