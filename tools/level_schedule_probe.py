#!/usr/bin/env python
"""Modulus-switching schedules on one MI355X: what levels.plan_levels finds for the networks, what the schedules buy, and the switch kernel's
two arithmetic forms against the HBM floor.

    python tools/level_schedule_probe.py [--reps 5] [--skip-cifar]

Prints:
  * cn_mod_switch kernel times, integer (k_mod_switch, "f64" = 0) and exact FP64 (k_mod_switch_f64), for every (KS, KD) pair of a C3 chain
    (845 ciphertexts) and of LoLa-CIFAR's 9-limb chain (128 ciphertexts), as fractions of the HBM floor
    count x 2 x (KS + KD) x N x 8 bytes / 8 TB/s.  The FP64 form runs only where cn_l_mod_switch selects it, so this part runs in a child
    process on an A/B build of the library with CN_MS_F64_ALL=1 (every pair eligible; lib/libcnhip_msf64all.so);
  * for CryptoNets-MNIST (C3, one 8192-image batch), LoLa-MNIST (C4, one image) and the LoLa-CIFAR shapes at 9 limbs (one image, synthetic
    weights): the planned schedule with its budget trail (margin 8 bits, one calibration record), the time per batch / image at the top
    level and as scheduled (wall time with every stream of the top and level contexts synchronised, after one warm-up run; median and
    range of --reps runs) and the reply size at the reply level;
  * whether the reference's own 8-limb CIFAR configuration decrypts the whole network under any schedule.
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK = 8.0e12
C3 = dict(n=8192, t=549764251649)
C9 = dict(n=16384, t=957181001729)


def timed(ctx, fn, reps, rounds=3):
    """HIP events on `ctx`'s stream: mean of `reps` launches after a warm-up, for `rounds` rounds -> (median, min, max) ms"""
    fn()
    ctx.sync()
    out = []
    for _ in range(rounds):
        ctx.time_begin()
        for _ in range(reps):
            fn()
        out.append(ctx.time_end() / reps)
    return float(np.median(out)), min(out), max(out)


def kernels(reps):
    from cryptonets_amd._native import Context, default_coeff_modulus
    rng = np.random.default_rng(1)
    for name, p, count in (("C3", C3, 845), ("C9", C9, 128)):
        q = default_coeff_modulus(p["n"])
        print("# %s: N = %d, %d limbs (%s), %d size-2 ciphertexts" % (name, p["n"], len(q), " ".join("%d" % (m.bit_length()) for m in q), count), flush=True)
        print("%-6s %-8s %22s %22s %8s" % ("pair", "floor us", "integer us (x floor)", "FP64 us (x floor)", "FP64/int"), flush=True)
        for ks in range(2, len(q) + 1):
            ctxs = {}
            for f64 in (0, 1):
                g = Context(p["n"], p["t"], q=q[:ks], dbc=60, gdbc=60, device=0)
                g.set_option("f64", f64)
                h = g.ct_alloc(count, 2)
                w = np.stack([np.concatenate([rng.integers(0, m, size=g.n, dtype=np.uint64) for _ in range(2) for m in g.q]) for _ in range(8)])
                for s in range(0, count, 8):
                    g.ct_upload(h, s, w[:min(8, count - s)])
                ctxs[f64] = (g, h)
            for kd in range(ks - 1, 0, -1):
                row = []
                for f64 in (0, 1):
                    g, h = ctxs[f64]
                    lv = g.level(kd)
                    out = lv.ct_alloc(count, 2)
                    t = timed(lv, lambda: g.mod_switch(h, 0, count, lv, out, 0), reps)
                    assert g.get_option("mod_switch_f64") == f64, "the A/B build must run FP64 for every pair"
                    row.append(t)
                    lv.free(out)
                floor_us = count * 2 * (ks + kd) * p["n"] * 8 / PEAK * 1e6
                print("%d->%d   %8.1f %9.1f-%-6.1f(%.2f) %9.1f-%-6.1f(%.2f) %8.2f" % (
                    ks, kd, floor_us, row[0][1] * 1e3, row[0][2] * 1e3, row[0][0] * 1e3 / floor_us, row[1][1] * 1e3, row[1][2] * 1e3,
                    row[1][0] * 1e3 / floor_us, row[1][0] / row[0][0]), flush=True)
            for g, h in ctxs.values():
                g.free(h)
                g.close()


def sync_all(env):
    for e in env.Environments:
        e.ctx.sync()
        for lv in e._levels.values():
            lv.ctx.sync()


def time_runs(env, run, reps):
    run()
    sync_all(env)
    out = []
    for _ in range(reps):
        sync_all(env)
        t0 = time.perf_counter()
        run()
        sync_all(env)
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), min(out), max(out)


def network(title, Factory, head_fn, set_input, reps, boundaries=None, unit="batch"):
    from cryptonets_amd import networks
    from cryptonets_amd.levels import plan_levels
    env = Factory.AllocateComputationEnv()
    net = head_fn()
    layers = list(networks._chain(net))[::-1]
    set_input(0)
    t0 = time.perf_counter()
    try:
        plan = plan_levels(net, Factory, records=1, margin_bits=8, boundaries=boundaries(layers) if boundaries else None)
    except Exception as ex:                                            # noqa: BLE001 - reported
        print("## %s: no schedule: %s" % (title, ex), flush=True)
        return
    print("## %s (planned in %.1f s)" % (title, time.perf_counter() - t0), flush=True)
    print(plan, flush=True)
    sources = [p.Source for p in layers]

    def run_with(head):
        def run():
            set_input(1)
            out = head.GetNext()
            run.limbs, run.count = out.Limbs, sum(a.encData.count for c in out.leVectors for a in c.eVectors)
            out.Dispose()
        return run
    top = run_with(net)
    t_top = time_runs(env, top, reps)
    head = networks.with_levels(net, plan.schedule)
    sch = run_with(head)
    t_sch = time_runs(env, sch, reps)
    for p, s in zip(layers, sources):
        p.Source = s
    n = env.Environments[0].ctx.n
    print("time per %s: top level %.1f ms (%.1f-%.1f), scheduled %.1f ms (%.1f-%.1f): %.2fx" % (unit, *t_top, *t_sch, t_top[0] / t_sch[0]), flush=True)
    print("reply: %d ciphertexts over the plaintext primes at %d limbs = %.0f KiB (top level, %d limbs: %.0f KiB)" % (
        sch.count, sch.limbs, sch.count * 2 * sch.limbs * n * 8 / 1024, top.limbs, top.count * 2 * top.limbs * n * 8 / 1024), flush=True)


def networks_part(reps, skip_cifar):
    from cryptonets_amd import cryptonets_mnist as cm
    from cryptonets_amd import networks
    from cryptonets_amd.hewrapper import EncryptedSealBfvFactory
    from test_cryptonets_mnist import build_network, synthetic_images
    from test_lola import PRIMES as LOLA_PRIMES, lola
    from test_lola_cifar import PRIMES as CIFAR_PRIMES

    def factory(primes, n, dbc=10, gdbc=20, smc=-1, galois=True):
        return EncryptedSealBfvFactory(list(primes), n, dbc, gdbc, smc, galois=galois, client_seed=99)

    F = factory(cm.PLAIN_PRIMES, cm.N, galois=False)
    batches = [synthetic_images(8192, seed=s) for s in (1, 2)]
    holder = {}

    def cn_head():
        holder["net"], _ = build_network(F, batches[0])
        return holder["net"]

    def cn_input(i):
        list(networks._chain(holder["net"]))[-1].data = batches[i]
    network("CryptoNets-MNIST, C3, one 8192-image batch", F, cn_head, cn_input, reps)

    F = factory(LOLA_PRIMES, 8192)
    imgs = [np.where(np.random.default_rng(s).random(784) < 0.81, 0, np.random.default_rng(s + 5).integers(1, 256, size=784)).astype(float) for s in (1, 2)]

    def lola_head():
        holder["lola"] = lola(F, imgs[0])
        return holder["lola"]

    def lola_input(i):
        list(networks._chain(holder["lola"]))[-1].Features = imgs[i] / 256.0
    network("LoLa-MNIST, C4, one image", F, lola_head, lola_input, reps, unit="image")
    if skip_cifar:
        return
    rng = np.random.default_rng(5)
    w = [np.rint(rng.normal(0, 0.05, 83 * 192) * 256) / 256, np.rint(rng.normal(0, 0.02, 112 * 8300) * 512) / 512,
         np.rint(rng.normal(0, 0.05, 10 * 5488) * 512) / 512]
    b = [np.rint(rng.normal(0, 0.05, 83) * 256) / 256, np.rint(rng.normal(0, 0.05, 112) * 512) / 512, np.rint(rng.normal(0, 0.05, 10) * 512) / 512]
    cimgs = [rng.integers(0, 256, size=3 * 32 * 32).astype(float) for _ in range(2)]
    for limbs in (9, 8):
        F = factory(CIFAR_PRIMES, 16384, 60, 60, limbs)

        def cifar_head():
            holder["cifar_reader"] = networks.cifar_reader(Factory=F)
            return networks.LoLaCifar(F, holder["cifar_reader"], w, b, timing=False)

        def cifar_input(i):
            holder["cifar_reader"].Features = cimgs[i] / 256.0
        network("LoLa-CIFAR shapes, N = 16384, %d limbs, one image" % limbs, F, cifar_head, cifar_input, max(2, reps // 2) if limbs == 9 else 1,
                unit="image")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-cifar", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="(child) the kernel table only, on the library CNHIP_LIB names")
    a = ap.parse_args()
    if a.kernels:
        kernels(20)
        return
    from cryptonets_amd import _native
    lib = os.path.join(_native._PKG, "lib", "libcnhip_msf64all.so")
    _native.build(defines=("CN_MS_F64_ALL=1",), out=lib)
    print("# cn_mod_switch kernels: HIP events on the target context's stream, mean of 20 launches after a warm-up, median (range) of 3 rounds",
          flush=True)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--kernels"], env=dict(os.environ, CNHIP_LIB=lib), timeout=900)
    networks_part(a.reps, a.skip_cifar)


if __name__ == "__main__":
    main()
