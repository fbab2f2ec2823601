"""The per-value arithmetic of cn_decrypt_join on the CPU: tests/cpp/crt_join_model.cpp calls the __host__ __device__ functions of
cryptonets_amd/csrc/cn_k_join.hip.h - Garner's recombination, the sign step, integer -> double with ties to even, the division by the scale - that the
kernel k_crt_join runs per value.  Compared with Python's integers and float(x) / scale: words equal, doubles equal as bit patterns."""
import os
import random
import struct
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [1.0, float(32 * 32 * 16), 3.0]
TIES = [2 ** 53 + 1, 2 ** 53 + 3, 2 ** 60 + 2 ** 7, 2 ** 200 + 2 ** 147]      # exactly half way between two doubles; +-1 falls on either side


def is_prime(n):
    if n < 2:
        return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
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


def primes_of(bits, count):
    """the `count` largest primes of exactly `bits` bits"""
    out, c = [], (1 << bits) - 1
    while len(out) < count:
        if is_prime(c):
            out.append(c)
        c -= 2
    return out


def moduli_sets():
    """P = 1, 2, 4, 8 at every width whose product stays below 2^255, and mixed widths"""
    sets = []
    for bits in (14, 20, 31, 40, 62):
        for P in (1, 2, 4, 8):
            if bits * P < 255:
                sets.append(primes_of(bits, P))
    sets.append([primes_of(b, 1)[0] for b in (14, 62, 20, 40)])
    sets.append([primes_of(b, 1)[0] for b in (62, 31, 14, 40, 20, 62 - 1, 14 + 1, 8 + 3)])
    return sets


def values_for(M, signed, rng):
    xs = [0, 1, M - 1, (M - 1) // 2, (M + 1) // 2] + [rng.randrange(M) for _ in range(2000)]
    for tie in TIES:
        for x in (tie - 1, tie, tie + 1):
            if x < M:
                xs.append(x)
            if signed and 2 * x <= M:
                xs.append(M - x)                     # the residue class of -x: joined to -x under the signed flag
    return xs


@pytest.fixture(scope="module")
def model():
    exe = os.path.join(tempfile.mkdtemp(), "crt_join_model")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", os.path.join(ROOT, "tests", "cpp", "crt_join_model.cpp"), "-o", exe])
    return exe


def test_join_arithmetic_matches_python_integers(model):
    rng = random.Random(20261019)
    groups, lines = [], []
    for ts in moduli_sets():
        M = 1
        for t in ts:
            assert is_prime(t)
            M *= t
        assert M < 2 ** 255
        for signed in (0, 1):
            xs = values_for(M, signed, rng)
            for scale in SCALES:
                groups.append((ts, M, signed, scale, xs))
                lines.append("%d %d %x %d %s" % (len(ts), signed, struct.unpack("<Q", struct.pack("<d", scale))[0], len(xs), " ".join("%x" % t for t in ts)))
                lines.extend(" ".join("%x" % (x % t) for t in ts) for x in xs)
    path = os.path.join(tempfile.mkdtemp(), "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([model, path], stdout=subprocess.PIPE, check=True, timeout=300).stdout.decode().split("\n")
    pos, checked = 0, 0
    for ts, M, signed, scale, xs in groups:
        W = (M.bit_length() + 1 + 63) // 64
        assert out[pos] == "W %d" % W, (ts, out[pos])
        pos += 1
        for x in xs:
            want = x - M if (signed and 2 * x > M) else x
            f = out[pos].split()
            pos += 1
            got = sum(int(w, 16) << (64 * i) for i, w in enumerate(f[:W]))
            assert got == want % (1 << (64 * W)), (ts, signed, x, f)
            bits = struct.unpack("<Q", struct.pack("<d", float(want) / scale))[0]
            assert int(f[W], 16) == bits, (ts, signed, scale, want, f[W], "%016x" % bits)
            checked += 1
    assert checked > 100000


def test_table_refuses_what_the_call_refuses(model):
    """equal moduli and a product of 2^255 or more: the table builder (cnj_build_tab, also cn_join_words' check) refuses"""
    p62 = primes_of(62, 5)
    for ts in ([12289, 12289], p62):
        path = os.path.join(tempfile.mkdtemp(), "cases.txt")
        with open(path, "w") as f:
            f.write("%d 0 %x 0 %s\n" % (len(ts), struct.unpack("<Q", struct.pack("<d", 1.0))[0], " ".join("%x" % t for t in ts)))
        r = subprocess.run([model, path], stdout=subprocess.PIPE, timeout=60)
        assert r.returncode == 4 and r.stdout.decode().strip() == "refused", (ts, r)
