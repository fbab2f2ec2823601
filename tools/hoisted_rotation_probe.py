"""n rotations of ONE ciphertext on the three routes the library has, in one process on one MI355X, on the same input ciphertext and the same keys:

    hoisted    cn_rotate_rows_hoisted: the digit transforms of the input once, two launches (k_ks_digit_ntt, k_ks_hoist_mac)
    many       cn_rotate_rows_many with the direct key of every step: one two-launch key switch per piece of rotations, each with its own digit transforms
    doubling   "baby steps by doubling": rho_(b + s) = rho_s(rho_b) for all b < s at once, log2 B dependent cn_rotate_rows calls on 1, 2, 4, .. ciphertexts
               (only where the steps are 1 .. B - 1)

Shapes:
    mnist-dup   the copies of Duplicate(8) at the LoLa-MNIST parameters (N = 8192, the default coefficient modulus, gdbc 20): three steps -1024 i of one source row
    cifar       the baby-step set of the LoLa-CIFAR dense layer (N = 16384, k = 8, gdbc 60): the 127 steps 1 .. 127 (127 direct keys: 2 GiB)
    large       one plaintext prime of LargeLoLa (N = 16384, k = 7, gdbc 60): the B - 1 baby steps of its 2608 x 11952 layer under diagonal.choose_baby_steps
    three       n = 3 at the cifar parameters: where a hoisted call has least to share

Per shape and route: the median wall-clock time of at least five timed rounds after one untimed one (the routes alternate inside every round; the device is
idle before and after every timed call: cn_sync on both sides), and the invariant noise budget (cn_noise_norm) of the deepest copy - the last step of the list -
on a FRESH encryption.  Every timed step runs under its own time limit; a step that passes its limit ends the probe.  No threshold is set in advance: the output
says what was measured.

    timeout -k 10 900 python tools/hoisted_rotation_probe.py [--shapes mnist-dup,three,large,cifar] [--rounds 5] [--limit 120] [--out profiles/hoisted_rotations.md]

Kernel times (which the wall clock cannot give) come from a run of its own: `timeout -k 10 600 rocprofv3 --kernel-trace --stats -f csv -d DIR -- python
tools/hoisted_rotation_probe.py --shapes cifar --rounds 5`; every shape prints the bytes the second launch needs (keys streamed once, digits gathered per
workgroup) to set the traced time of k_ks_hoist_mac against.
"""
import argparse
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from cryptonets_amd import diagonal, networks
from cryptonets_amd._native import Context, default_coeff_modulus


class StepLimit:
    """a time limit for one step that does not need the interpreter: a watchdog thread ends the process (exit status 124) when the step has not come back in time.
    A timed step sits inside a library call (cn_sync waits for the device) - a Python signal handler would run only after that call returned; the library calls
    release the interpreter lock, so the watchdog runs while the main thread waits.  Nothing more is started on the device behind a step that hangs."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _late(self):
        try:
            sys.stderr.write("time limit of %d s passed in: %s\n" % (self.seconds, self.what))
            sys.stderr.flush()
        finally:
            os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._late)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def large_baby_steps():
    p = networks.FACTORY_PARAMETERS["LoLaLarge"]
    mask = diagonal.structural_diagonals(2608, 11952, p["n"])
    return diagonal.choose_baby_steps(mask)


def shapes():
    cifar, large, mnist = networks.FACTORY_PARAMETERS["LoLaCifar"], networks.FACTORY_PARAMETERS["LoLaLarge"], networks.FACTORY_PARAMETERS["LoLa"]
    Bl = large_baby_steps()
    return {
        "mnist-dup": dict(n=mnist["n"], t=mnist["primes"][0], k=None, gdbc=20, steps=[-1024, -2048, -3072], doubling=False),
        "three": dict(n=cifar["n"], t=cifar["primes"][0], k=8, gdbc=60, steps=[1, 2, 3], doubling=False),
        "large": dict(n=large["n"], t=large["primes"][0], k=7, gdbc=60, steps=list(range(1, Bl)), doubling=True),
        "cifar": dict(n=cifar["n"], t=cifar["primes"][0], k=8, gdbc=60, steps=list(range(1, 128)), doubling=True),
    }


def run_shape(name, S, rounds, limit, say):
    n, steps = S["n"], S["steps"]
    q = default_coeff_modulus(n)
    q = q[:S["k"]] if S["k"] else q
    with StepLimit(limit, name + ": context and keys"):
        g = Context(n, S["t"], q=q, dbc=S["gdbc"], gdbc=S["gdbc"], device=0)
        g.keygen(11, galois=False)
        g.keygen_galois(12, [g.galois_elt_from_step(s) for s in steps])
        g.sync()
    nrot = len(steps)
    tot = diagonal.ks_digits(q, S["gdbc"])
    key_bytes = nrot * tot * 2 * len(q) * n * 8
    pt, src, out = g.pt_alloc(1), g.ct_alloc(1), g.ct_alloc(nrot + 1)
    g.pt_upload(pt, 0, np.random.default_rng(3).integers(0, 16, size=n, dtype=np.uint64))
    g.encrypt(pt, 0, src, 0, 1, seed=5)
    g.copy(src, 0, out, 0, 1)
    ois = list(range(1, nrot + 1))

    def hoisted():
        g.rotate_rows_hoisted(src, 0, steps, out, ois)

    def many():
        g.rotate_rows_many(src, [0] * nrot, steps, out, ois)

    def doubling():                                             # out[b] = rho_b(out[0]); out[0] holds the input
        s = 1
        while s <= nrot:
            g.rotate_rows(out, 0, s, out, s, min(s, nrot + 1 - s))
            s *= 2
    routes = [("hoisted", hoisted), ("many", many)] + ([("doubling", doubling)] if S["doubling"] else [])
    times, budgets, stats = {r: [] for r, _ in routes}, {}, {}
    for rnd in range(rounds + 1):                               # round 0 is not timed (arenas grow, kernels load)
        for r, fn in routes:
            with StepLimit(limit, "%s: %s, round %d" % (name, r, rnd)):
                g.sync()
                s0 = g.stats()
                t0 = time.perf_counter()
                fn()
                g.sync()
                dt = time.perf_counter() - t0
                s1 = g.stats()
                if rnd:
                    times[r].append(dt)
                else:
                    stats[r] = {x: s1[x] - s0[x] for x in ("kernel_launches", "ntt_forward_limbs", "ntt_inverse_limbs")}
                    budgets[r] = float(g.invariant_noise_budget(out, nrot, 1)[0])
    fresh = float(g.invariant_noise_budget(src, 0, 1)[0])
    say("")
    say("### %s: N = %d, k = %d, %d digits (gdbc %d), n = %d rotations of one ciphertext, steps %s" %
        (name, n, len(q), tot, S["gdbc"], nrot, steps if nrot <= 4 else "%d .. %d" % (steps[0], steps[-1])))
    say("")
    say("Direct keys of these steps: %.1f MiB.  Fresh input: %.1f bits of budget." % (key_bytes / 2 ** 20, fresh))
    wgs = nrot * len(q) * (2 if n == 16384 else 1)              # k_ks_hoist_mac: a workgroup per (rotation, limb), per component at N = 16384
    say("Bytes of the second launch (k_ks_hoist_mac, %d workgroups): %.1f MiB of keys, each word read once; %.1f MiB of transformed digits gathered in 16-byte pieces "
        "(%d digits x N x 8 per workgroup, out of an array of %.1f MiB); %.1f MiB written." %
        (wgs, key_bytes / 2 ** 20, wgs * tot * n * 8 / 2 ** 20, tot, tot * len(q) * n * 8 / 2 ** 20, nrot * 2 * len(q) * n * 8 / 2 ** 20))
    say("")
    say("| route | median ms | min | max | launches | forward limb transforms | inverse | budget of the deepest copy (bits) |")
    say("|---|---|---|---|---|---|---|---|")
    for r, _ in routes:
        ms = [1e3 * x for x in times[r]]
        say("| %s | %.3f | %.3f | %.3f | %d | %d | %d | %.1f |" % (r, statistics.median(ms), min(ms), max(ms), stats[r]["kernel_launches"], stats[r]["ntt_forward_limbs"],
                                                               stats[r]["ntt_inverse_limbs"], budgets[r]))
    med = {r: statistics.median(times[r]) for r, _ in routes}
    best = min(med, key=med.get)
    say("")
    say("Fastest: %s.  hoisted / many = %.2f%s." % (best, med["hoisted"] / med["many"], ", hoisted / doubling = %.2f" % (med["hoisted"] / med["doubling"]) if "doubling" in med else ""))
    for h in (pt, src, out):
        g.free(h)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mnist-dup,three,large,cifar")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("# Hoisted rotations: cn_rotate_rows_hoisted beside cn_rotate_rows_many and baby steps by doubling")
    say("")
    say("`python tools/hoisted_rotation_probe.py --shapes %s --rounds %d`: one process, one device, wall-clock time of the calls between two cn_sync, median of %d timed "
        "rounds after one untimed round, the routes alternating inside every round on the same fresh ciphertext and keys.  The code of `many` and `doubling` is the "
        "parent commit's." % (a.shapes, a.rounds, a.rounds))
    S = shapes()
    for name in a.shapes.split(","):
        run_shape(name, S[name], max(a.rounds, 5), a.limit, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
