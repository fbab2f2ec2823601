#!/usr/bin/env python
"""Noise-budget probes on one MI355X: the device-reduced cn_noise_norm against the path it replaced (cn_noise_poly's N k words per
ciphertext to the host, composed there with Python integers - kept below as the baseline), alternating in one run on seeded inputs.

    python tools/noise_budget_probe.py [--reps 3] [--skip-plans]
    python tools/noise_budget_probe.py --kernel-only [--reps 10]        # the new path only: run it under rocprofv3 --kernel-trace --stats
    python tools/noise_budget_probe.py --stats kernel_stats.csv --reps 10    # k_noise_norm time per call from that run

Prints:
  * the integer budgets of 845 C3 ciphertexts (N = 8192, 5 limbs, after one multiply) and of 128 N = 16384 9-limb ciphertexts (fresh):
    host wall time per call of each path (median and range of --reps alternating rounds), and that both give the same budgets;
  * with --stats: the kernel time of k_noise_norm per call against its HBM floor 2 x count x k x N x 8 bytes at 8 TB/s (it reads c0 and
    the decryption accumulator once; an algorithmic floor - no counter pass);
  * levels.plan_levels wall time for CryptoNets-MNIST (C3, one 8192-image batch) and LoLa-MNIST (C4, one image), old path then new, and
    whether the two schedules and budget trails are identical.
"""
import argparse
import contextlib
import csv
import io
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8.0e12
SHAPES = (("C3", 8192, 549764251649, 845), ("C9", 16384, 957181001729, 128))


# ------------------------------------------------------------------ the old path (the baseline)
def old_invariant_noise_budget(ctx, ct, ci=0, count=1, exact_bits=False):
    """Context.invariant_noise_budget before cn_noise_norm: cn_noise_poly's words composed on the host with Python integers"""
    w = ctx.noise_poly(ct, ci, count)
    Q = 1
    for qj in ctx.q:
        Q *= qj
    coef = [(Q // qj) * pow((Q // qj) % qj, -1, qj) for qj in ctx.q]
    out = []
    for c in range(count):
        x = sum(w[c, j].astype(object) * coef[j] for j in range(ctx.k)) % Q
        norm = max(int(v) if 2 * int(v) <= Q else Q - int(v) for v in x)
        if exact_bits:
            out.append(max(0, Q.bit_length() - norm.bit_length() - 1))
        else:
            out.append(math.log2(Q) - (math.log2(norm) if norm else 0.0) - 1.0)
    return out


def old_min_budget(ms, Factory):
    """levels.min_budget before cn_noise_norm: CryptoTracker.TestVectorBudget column by column (one probe per column and prime)"""
    from cryptonets_amd.cryptotracker import CryptoTracker
    from cryptonets_amd.hewrapper import _env_at
    saved, best = CryptoTracker.MinBudgetSoFar, None
    try:
        for m in ms:
            env = _env_at(Factory.AllocateComputationEnv(), m.Limbs)
            for col in m.leVectors:
                CryptoTracker.Reset()
                try:
                    with contextlib.redirect_stdout(io.StringIO()):
                        b = CryptoTracker.TestVectorBudget(col, env)
                except Exception as e:
                    if "budget is zero" not in str(e):
                        raise
                    b = 0
                best = b if best is None else min(best, b)
    finally:
        CryptoTracker.MinBudgetSoFar = saved
    return float(best)


@contextlib.contextmanager
def old_path():
    from cryptonets_amd import _native, levels
    saved = _native.Context.invariant_noise_budget, levels.min_budget
    _native.Context.invariant_noise_budget = old_invariant_noise_budget
    levels.min_budget = old_min_budget
    try:
        yield
    finally:
        _native.Context.invariant_noise_budget, levels.min_budget = saved


# ------------------------------------------------------------------ probe calls
def inputs(name, n, t, count):
    """seeded ciphertexts: C3 after one multiply (the budget a squared layer leaves), C9 fresh"""
    from cryptonets_amd._native import Context
    g = Context(n, t, dbc=60 if n == 16384 else 10, gdbc=60 if n == 16384 else 20, device=0)
    g.keygen(2024, galois=False)
    rng = np.random.default_rng(11)
    pt = g.pt_alloc(count)
    g.encode_batch(rng.integers(0, t, size=(count, n), dtype=np.uint64), pt, 0)
    h = g.ct_alloc(count)
    g.encrypt(pt, 0, h, 0, count, seed=3)
    g.free(pt)
    if name == "C3":
        g.mul_relin(h, 0, h, 0, h, 0, count)
    g.sync()
    return g, h


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def budgets_part(reps):
    print("# budget of every ciphertext (SEAL's integer budget): host wall time per call, median (range) of %d alternating rounds" % reps, flush=True)
    print("%-4s %5s %5s %6s %28s %28s %9s %10s" % ("", "N", "limbs", "count", "old: noise_poly + host ms", "new: noise_norm ms", "old/new",
                                                   "same bits"), flush=True)
    for name, n, t, count in SHAPES:
        g, h = inputs(name, n, t, count)
        g.invariant_noise_budget(h, 0, count, exact_bits=True)                 # warm-up (scratch, code objects)
        old, new, same = [], [], True
        for _ in range(reps):
            to, bo = wall(lambda: old_invariant_noise_budget(g, h, 0, count, exact_bits=True))
            tn, bn = wall(lambda: g.invariant_noise_budget(h, 0, count, exact_bits=True))
            old.append(to)
            new.append(tn)
            same = same and bo == bn
        print("%-4s %5d %5d %6d %12.1f (%.1f-%.1f) %14.2f (%.2f-%.2f) %9.0f %10s   min budget %d bits" % (
            name, n, g.k, count, np.median(old), min(old), max(old), np.median(new), min(new), max(new), np.median(old) / np.median(new),
            same, min(bn)), flush=True)
        g.free(h)
        g.close()


def kernel_only(reps):
    for name, n, t, count in SHAPES:
        g, h = inputs(name, n, t, count)
        for _ in range(reps + 1):                                               # + 1 warm-up
            g.noise_norm(h, 0, count)
        g.free(h)
        g.close()


def stats_part(path, reps):
    """k_noise_norm<K> per call from a rocprofv3 kernel_stats.csv of `--kernel-only --reps reps` (reps + 1 calls per shape)"""
    rows = {r["Name"]: r for r in csv.DictReader(open(path))}
    print("# k_noise_norm kernel time per call (rocprofv3 --kernel-trace --stats of --kernel-only, %d calls per shape; a call of more than"
          " 2^24 / (k N) ciphertexts is several launches)" % (reps + 1), flush=True)
    print("%-4s %5s %6s %8s %10s %10s %10s" % ("", "limbs", "count", "launches", "kernel us", "floor us", "x floor"), flush=True)
    for (name, n, t, count), k in zip(SHAPES, (5, 9)):
        r = next((v for key, v in rows.items() if key.startswith("void k_noise_norm<%d>" % k)), None)
        if r is None:
            print("%-4s k_noise_norm<%d> not in %s" % (name, k, path), flush=True)
            continue
        per_call = float(r["TotalDurationNs"]) / (reps + 1) / 1e3
        floor = 2 * count * k * n * 8 / PEAK * 1e6
        print("%-4s %5d %6d %8.0f %10.1f %10.1f %10.2f" % (name, k, count, int(r["Calls"]) / (reps + 1), per_call, floor, per_call / floor), flush=True)


# ------------------------------------------------------------------ plan_levels
def plan(title, Factory, head_fn, set_input):
    from cryptonets_amd.levels import plan_levels
    net = head_fn()
    set_input(0)
    t0 = time.perf_counter()
    p = plan_levels(net, Factory, records=1, margin_bits=8)
    return time.perf_counter() - t0, p


def plans_part():
    from cryptonets_amd import cryptonets_mnist as cm
    from cryptonets_amd import networks
    from cryptonets_amd.hewrapper import EncryptedSealBfvFactory
    from test_cryptonets_mnist import build_network, synthetic_images
    from test_lola import PRIMES as LOLA_PRIMES, lola

    print("# levels.plan_levels (one calibration record, margin 8 bits): host wall time, the old path first, then the new one", flush=True)
    holder = {}
    batch = synthetic_images(8192, seed=1)
    img = np.where(np.random.default_rng(1).random(784) < 0.81, 0, np.random.default_rng(6).integers(1, 256, size=784)).astype(float)

    def cn(F):
        def head():
            holder["net"], _ = build_network(F, batch)
            return holder["net"]
        return head, lambda i: None

    def lo(F):
        def head():
            holder["lola"] = lola(F, img)
            return holder["lola"]

        def set_input(i):
            list(networks._chain(holder["lola"]))[-1].Features = img / 256.0
        return head, set_input

    for title, primes, galois, make in (("CryptoNets-MNIST, C3, one 8192-image batch", cm.PLAIN_PRIMES, False, cn),
                                        ("LoLa-MNIST, C4, one image", LOLA_PRIMES, True, lo)):
        res = {}
        for which in ("old", "new"):
            F = EncryptedSealBfvFactory(list(primes), 8192, 10, 20, -1, galois=galois, client_seed=99)
            head, set_input = make(F)
            if which == "old":
                with old_path():
                    res[which] = plan(title, F, head, set_input)
            else:
                res[which] = plan(title, F, head, set_input)
        (to, po), (tn, pn) = res["old"], res["new"]
        same = po.schedule == pn.schedule and po.top == pn.top and po.scheduled == pn.scheduled
        print("## %s: planned in %.1f s (old) and %.1f s (new): %.1fx; schedules and budget trails identical: %s" % (title, to, tn, to / tn, same),
              flush=True)
        print(pn, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-plans", action="store_true")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--stats", help="kernel_stats.csv of a --kernel-only run under rocprofv3 (same --reps)")
    a = ap.parse_args()
    if a.kernel_only:
        kernel_only(a.reps)
        return
    if a.stats:
        stats_part(a.stats, a.reps)
        return
    budgets_part(a.reps)
    if not a.skip_plans:
        plans_part()


if __name__ == "__main__":
    main()
