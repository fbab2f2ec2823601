#!/usr/bin/env python
"""The client's reply path, device join (cn_decrypt_join, hewrapper.DEVICE_JOIN = True) against the per-prime path (decrypt, download, decode, join slot by
slot with Python integers; DEVICE_JOIN = False), on one MI355X: both paths alternate in one process, ROUNDS rounds each after one untimed round, wall time around
the synchronising call, clocks as found.

    python tools/reply_probe.py [--rounds 5] [--device-only]        # --device-only: the True path alone (for a kernel trace)

Shapes (factory parameters: networks.FACTORY_PARAMETERS):
  cryptonets   the CryptoNets reply: 10 columns x 8192 slots x 2 primes (N = 8192), EncryptedSealBfvMatrix.Decrypt, and the predicted classes
               (cryptonets_mnist.predict against the arg max over the decrypted matrix)
  lola         the LoLa-MNIST reply: 4 primes, one ciphertext, 10 values (dense vector, N = 8192)
  lola_cifar   the LoLa-CIFAR-shaped sparse reply: 2 primes, N = 16384, 10 ciphertexts (sparse vector)
The ciphertexts are fresh encryptions of random values (what is decrypted does not change the work)."""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cryptonets_amd import cryptonets_mnist as cm                   # noqa: E402
from cryptonets_amd import hewrapper as hw                          # noqa: E402
from cryptonets_amd.networks import FACTORY_PARAMETERS              # noqa: E402


def factory(name):
    return hw.EncryptedSealBfvFactory(galois=False, client_seed=0xBEEF, **FACTORY_PARAMETERS[name])


def columns_in_one_array(F, cols):
    """the columns as views of ONE ciphertext array per plaintext prime: how the batched layers leave a network's output"""
    env = F.AllocateComputationEnv()
    bufs = []
    for i, e in enumerate(env.Environments):
        b = hw._Buf(e.ctx, "ct", len(cols))
        e.ctx.copy_many([c.eVectors[i].encData.h for c in cols], [c.eVectors[i].encData.first for c in cols], b.h, 0)
        bufs.append(b)
    out = []
    for j, c in enumerate(cols):
        atoms = [hw.AtomicSealBfvEncryptedVector._new(Scale=a.Scale, Dim=a.Dim, Format=a.Format, IsSigned=a.IsSigned, encData=bufs[i].view(j, 1))
                 for i, a in enumerate(c.eVectors)]
        out.append(hw.EncryptedSealBfvVector._of(atoms, c.Scale))
    return F.GetMatrix(out, hw.EMatrixFormat.ColumnMajor, CopyVectors=False), bufs


def shapes():
    rng = np.random.default_rng(1)
    F = factory("CryptoNets")
    env = F.AllocateComputationEnv()
    cols = [F.GetEncryptedVector(rng.integers(-(1 << 30), 1 << 30, size=8192).astype(float), hw.EVectorFormat.dense, 1.0) for _ in range(10)]
    for c in cols:
        c.Scale = float(32 * 32 * 16)
    matrix, bufs = columns_in_one_array(F, cols)
    channels = [types.SimpleNamespace(g=e.ctx, h5=b.h) for e, b in zip(env.Environments, bufs)]
    yield "cryptonets matrix.Decrypt 10x8192x2", lambda: matrix.Decrypt(env), lambda a, b: np.array_equal(a.view(np.uint64), b.view(np.uint64))
    yield ("cryptonets predict 10x8192x2", lambda: cm.predict(channels) if hw.DEVICE_JOIN else np.argmax(matrix.Decrypt(env), axis=1).astype(np.int32),
           lambda a, b: np.array_equal(a, b))
    F2 = factory("LoLa")
    env2 = F2.AllocateComputationEnv()
    v = F2.GetEncryptedVector(rng.integers(-(1 << 20), 1 << 20, size=10).astype(float), hw.EVectorFormat.dense, 1.0)
    v.Scale = float(32 * 32 * 16)
    yield "lola vector.Decrypt 1x10x4", lambda: v.Decrypt(env2), lambda a, b: np.array_equal(a.view(np.uint64), b.view(np.uint64))
    F3 = factory("LoLaCifar")
    env3 = F3.AllocateComputationEnv()
    s = F3.GetEncryptedVector(rng.integers(-(1 << 30), 1 << 30, size=10).astype(float), hw.EVectorFormat.sparse, 1.0)
    s.Scale = float(32 * 32 * 16)
    yield "lola_cifar sparse vector.Decrypt 10x1x2 (N = 16384)", lambda: s.Decrypt(env3), lambda a, b: np.array_equal(a.view(np.uint64), b.view(np.uint64))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    print("reply_probe: wall ms around the synchronising call, %d rounds per path, alternating, one untimed round first" % a.rounds)
    for name, fn, same in shapes():
        paths = (True,) if a.device_only else (False, True)
        samples, last = {p: [] for p in paths}, {}
        for rnd in range(a.rounds + 1):
            for p in paths:
                hw.DEVICE_JOIN = p
                ms, last[p] = timed(fn)
                if rnd:
                    samples[p].append(ms)
        hw.DEVICE_JOIN = True
        if not a.device_only:
            assert same(last[True], last[False]), name + ": the two paths disagree"
        for p in paths:
            x = samples[p]
            print("%-52s DEVICE_JOIN=%-5s min %9.3f  median %9.3f  samples %s" % (name, p, min(x), statistics.median(x), " ".join("%.3f" % v for v in x)))
        if not a.device_only:
            print("%-52s ratio of medians (False / True) %.1f" % (name, statistics.median(samples[False]) / statistics.median(samples[True])))


if __name__ == "__main__":
    main()
