#!/usr/bin/env python
"""Modulus switching on one MI355X: the kernel against its HBM floor, and what a lower level buys downstream (no program's default changes).

    python tools/mod_switch_probe.py [--reps 20]

Prints, one line per figure:
  * cn_mod_switch kernel time (HIP events on the target context's stream, mean of --reps launches after a warm-up) and its ALGORITHMIC bandwidth
    count x size x (k_src + k_dst) x N x 8 bytes / time, also as a fraction of the 8 TB/s HBM peak: C3 (845 ciphertexts, 5 -> 4 and 5 -> 2),
    C5 (128 ciphertexts, 8 -> 1);
  * cn_mul_relin of 845 ciphertexts at C3 on 5 and 3 limbs;
  * cn_rotate_rows of 130 ciphertexts at C4 on 5, 3 and 2 limbs;
  * CryptoNets-MNIST's reply (C3, one output ciphertext per plaintext prime): size and device decryption time at the lowest level whose noise
    budget stays positive after the squared layer;
  * the one-time cost of cn_ctx_create_level (stream selection, tables, key slices).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cryptonets_amd._native import Context  # noqa: E402

PEAK = 8.0e12
C3 = dict(n=8192, t=549764251649, q=None)
C4 = dict(n=8192, t=557057, q=None)
C5 = dict(n=16384, t=957181001729, q=[0xfffffffd8001, 0xfffffffa0001, 0xfffffff00001, 0x1fffffff68001, 0x1fffffff50001,
                                       0x1ffffffee8001, 0x1ffffffea0001, 0x1ffffffe88001], dbc=60, gdbc=60)


def make(p, keys=None):
    g = Context(p["n"], p["t"], q=p["q"], dbc=p.get("dbc", 10), gdbc=p.get("gdbc", 20), device=0)
    if keys is not None:
        g.keygen(7, galois=keys)
    return g


def rand_cts(g, count, rng):
    h = g.ct_alloc(count, 2)
    w = np.stack([np.concatenate([rng.integers(0, m, size=g.n, dtype=np.uint64) for _ in range(2) for m in g.q]) for _ in range(min(count, 16))])
    for s in range(0, count, 16):
        c = min(16, count - s)
        g.ct_upload(h, s, w[:c])
    return h


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.time_begin()
    for _ in range(reps):
        fn()
    return ctx.time_end() / reps


def probe_kernel(name, p, count, kd, reps, rng):
    g = make(p)
    h = rand_cts(g, count, rng)
    lv = g.level(kd)
    out = lv.ct_alloc(count, 2)
    ms = timed(lv, lambda: g.mod_switch(h, 0, count, lv, out, 0), reps)
    nbytes = count * 2 * (g.k + kd) * g.n * 8
    print("mod_switch %s %d cts %d->%d: %.1f us, %.0f GB/s algorithmic = %.2f of 8 TB/s (%.1f MB moved)"
          % (name, count, g.k, kd, ms * 1e3, nbytes / (ms * 1e-3) / 1e9, nbytes / (ms * 1e-3) / PEAK, nbytes / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    probe_kernel("C3", C3, 845, 4, a.reps, rng)
    probe_kernel("C3", C3, 845, 2, a.reps, rng)
    probe_kernel("C5", C5, 128, 1, a.reps, rng)

    g = make(C3, keys=False)
    for limbs in (5, 3):
        c = g if limbs == 5 else g.level(limbs)
        h = rand_cts(c, 845, rng)
        out = c.ct_alloc(845, 2)
        ms = timed(c, lambda: c.mul_relin(h, 0, h, 0, out, 0, 845), max(3, a.reps // 4))
        print("mul_relin C3 845 cts at %d limbs: %.3f ms" % (limbs, ms), flush=True)
    g.close()

    g = make(C4, keys=True)
    for limbs in (5, 3, 2):
        t0 = time.perf_counter()
        c = g if limbs == 5 else g.level(limbs)
        if limbs != 5:
            print("cn_ctx_create_level C4 (relin + %d Galois keys) -> %d limbs: %.1f ms" % (sum(1 for e in range(1, 2 * g.n, 2) if g.has_galois_key(e)), limbs,
                                                                                      (time.perf_counter() - t0) * 1e3), flush=True)
        h = rand_cts(c, 130, rng)
        out = c.ct_alloc(130, 2)
        ms = timed(c, lambda: c.rotate_rows(h, 0, 1, out, 0, 130), max(3, a.reps // 4))
        print("rotate_rows C4 130 cts at %d limbs: %.3f ms" % (limbs, ms), flush=True)
    g.close()

    # CryptoNets-MNIST reply: a squared scalar product (the network's last non-linear layer feeds a dense layer: the output's noise is the
    # square's plus a weighted sum) switched down; the lowest level with a positive budget
    g = make(C3, keys=False)
    pt = g.pt_alloc(3)
    vals = rng.integers(0, 64, size=(3, g.n), dtype=np.uint64)
    g.encode_batch(vals, pt, 0)
    enc = g.ct_alloc(3, 2)
    g.encrypt(pt, 0, enc, 0, 3, seed=5)
    lin, sq, rep = g.ct_alloc(1, 2), g.ct_alloc(1, 2), g.ct_alloc(10, 2)
    g.scalar_gemm(enc, np.array([[3, 1, 2]], dtype=np.uint64), lin, 0)
    g.mul_relin(lin, 0, lin, 0, sq, 0)
    g.scalar_gemm(sq, np.array([[100]], dtype=np.uint64), rep, 0)
    for i in range(1, 10):
        g.copy(rep, 0, rep, i, 1)
    print("CryptoNets reply at 5 limbs: budget %d bits, %d KiB per ciphertext" % (g.invariant_noise_budget(rep, exact_bits=True)[0], 2 * 5 * g.n * 8 // 1024), flush=True)
    dp = g.pt_alloc(10)
    ms5 = timed(g, lambda: g.decrypt(rep, 0, 10, dp, 0), max(3, a.reps // 4))
    best = 5
    for limbs in (4, 3, 2, 1):
        lv = g.level(limbs)
        out = lv.ct_alloc(10, 2)
        g.mod_switch(rep, 0, 10, lv, out, 0)
        b = lv.invariant_noise_budget(out, exact_bits=True)[0]          # SEAL's integer budget: 0 = nothing left
        d = lv.pt_alloc(10)
        ms = timed(lv, lambda: lv.decrypt(out, 0, 10, d, 0), max(3, a.reps // 4))
        print("CryptoNets reply at %d limbs: budget %d bits, %d KiB per ciphertext, decrypt of 10 ciphertexts %.1f us (5 limbs: %.1f us)"
              % (limbs, b, 2 * limbs * g.n * 8 // 1024, ms * 1e3, ms5 * 1e3), flush=True)
        if b >= 1:
            best = limbs
    print("CryptoNets reply: lowest level with a positive budget = %d limbs" % best, flush=True)


if __name__ == "__main__":
    main()
