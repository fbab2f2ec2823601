#!/usr/bin/env python
"""The client's request path, device split (cn_split_encrypt, hewrapper.DEVICE_SPLIT = True) against the host path (np.rint and one np.mod per prime on the host,
then one encode + encrypt per vector and prime; DEVICE_SPLIT = False), on one MI355X: both paths alternate in one process, ROUNDS rounds each after one untimed
round, wall time around the call (each path ends with its own host wait), clocks as found.

    python tools/request_probe.py [--rounds 5] [--device-only]        # --device-only: the True path alone (for a kernel trace)

Shapes (factory parameters: networks.FACTORY_PARAMETERS):
  cryptonets   the CryptoNets request: 784 columns x 8192 slots x 2 primes (N = 8192), EncryptedSealBfvFactory.GetEncryptedMatrix of the image-major batch
  images       the same request through cryptonets_mnist.encrypt_images into every channel's h_in (host path: the per-column wrapper path above, which is what a
               caller without encrypt_images has)
  lola         a LoLa-MNIST request: 4 primes, one dense vector of 8192 values (N = 8192), EncryptedSealBfvFactory.GetEncryptedVector
What is encrypted does not change the work: MNIST-like synthetic images."""
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


def synced(env, fn):
    """fn(), then every context's stream drained: the host path's last encryptions are asynchronous"""
    r = fn()
    for e in env.Environments:
        e.ctx.sync()
    return r


def shapes():
    images = cm.synthetic_images(8192, seed=2) * cm.NORMALIZATION
    F = factory("CryptoNets")
    env = F.AllocateComputationEnv()

    def matrix():
        m = synced(env, lambda: F.GetEncryptedMatrix(images, hw.EMatrixFormat.ColumnMajor, cm.INPUT_SCALE))
        return m, m.Dispose
    yield "cryptonets GetEncryptedMatrix 784x8192x2", matrix, lambda m: m.Decrypt(env)[:16]

    channels = [types.SimpleNamespace(g=e.ctx, h_in=e.ctx.ct_alloc(784)) for e in env.Environments]

    def request():
        if hw.DEVICE_SPLIT:
            cm.encrypt_images(channels, images, cm.INPUT_SCALE)
            return None, lambda: None
        return matrix()
    yield "cryptonets encrypt_images 784x8192x2", request, None

    F2 = factory("LoLa")
    env2 = F2.AllocateComputationEnv()
    vec = np.random.default_rng(3).integers(-128, 128, size=8192).astype(float) / 16.0

    def vector():
        v = synced(env2, lambda: F2.GetEncryptedVector(vec, hw.EVectorFormat.dense, 16.0))
        return v, v.Dispose
    yield "lola GetEncryptedVector 1x8192x4", vector, lambda v: v.Decrypt(env2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    print("request_probe: wall ms around the call, %d rounds per path, alternating, one untimed round first" % a.rounds)
    shipped = hw.DEVICE_SPLIT
    for name, fn, value in shapes():
        paths = (True,) if a.device_only else (False, True)
        samples, last = {p: [] for p in paths}, {}
        for rnd in range(a.rounds + 1):
            for p in paths:
                hw.DEVICE_SPLIT = p
                t0 = time.perf_counter()
                r, release = fn()
                ms = (time.perf_counter() - t0) * 1e3
                if rnd:
                    samples[p].append(ms)
                if rnd == a.rounds and value is not None:
                    last[p] = value(r)
                release()
        hw.DEVICE_SPLIT = shipped
        if len(last) == 2:
            assert np.array_equal(last[True].view(np.uint64), last[False].view(np.uint64)), name + ": the two paths disagree"
        for p in paths:
            x = samples[p]
            print("%-44s DEVICE_SPLIT=%-5s min %10.3f  median %10.3f  samples %s" % (name, p, min(x), statistics.median(x), " ".join("%.3f" % v for v in x)))
        if not a.device_only:
            print("%-44s ratio of medians (False / True) %.1f   device below host in every sample: %s" %
                  (name, statistics.median(samples[False]) / statistics.median(samples[True]), max(samples[True]) < min(samples[False])))


if __name__ == "__main__":
    main()
