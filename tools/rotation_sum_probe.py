"""Sums of rotations of DIFFERENT ciphertexts on the routes the library has, in one process on one MI355X, on the same ciphertexts and the same keys:

    summed     cn_rotate_rows_sum: the term MAC of every rotated term, one pair of inverse transforms per output limb (k_ks_sum_terms), no rotated term stored
    many+add   the parent commit's route where zero diagonals leave gaps, and Interleave's: cn_rotate_rows_many into a temporary, cn_add_many per output
    folding    the parent commit's giant steps: log2 Gs DEPENDENT cn_rotate_rows_add calls over all column classes (only where the terms are the giant steps
               j B, j < Gs, of every class)

Shapes:
    mnist-interleave   the LoLa-MNIST interleave (N = 8192, the default coefficient modulus, gdbc 20): 13 vectors, vector i by the step -(4096 - i), one output
    cifar-giant        the giant steps of the LoLa-CIFAR dense layer (N = 16384, k = 8, gdbc 60, B = 128): two column classes of 64 groups, 63 of them rotated
    large-giant        one plaintext prime of LargeLoLa (N = 16384, k = 7, gdbc 60): the giant steps of its 2608 x 11952 layer under diagonal.choose_baby_steps
Key sets: `direct` - a key for every step of the shape - and, for the giant steps, `default` - keys for the powers of two only, the other steps run their
non-adjacent-form hops on every route.

Per shape, key set and route: the median / min / max wall-clock time of at least five timed rounds after one untimed one (the routes alternate inside every round;
the device is idle before and after every timed call: cn_sync on both sides), launches, forward and inverse limb transforms, and the invariant noise budget
(cn_noise_norm) of the first output on FRESH encryptions.  Every timed step runs under its own time limit; a step that passes its limit ends the probe.  No ratio is
set in advance: the output says what was measured.  CN_KS_DIGIT_MAX / CN_KS_WIDE_MAX (read once per process) move the thresholds between the granularities of
the first launch (cn_ks_sum_plan).

    timeout -k 10 900 python tools/rotation_sum_probe.py [--shapes mnist-interleave,cifar-giant,large-giant] [--rounds 5] [--limit 120] [--out profiles/rotation_sum.md]

Kernel times (which the wall clock cannot give) come from a run of its own: `timeout -k 10 600 rocprofv3 --kernel-trace --stats -f csv -d DIR -- python
tools/rotation_sum_probe.py --shapes cifar-giant --rounds 5`.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np

from cryptonets_amd import diagonal, networks
from cryptonets_amd._native import Context, default_coeff_modulus
from hoisted_rotation_probe import StepLimit, large_baby_steps


def giant(n, B):
    """(steps of one class, classes): term j of a class is u[nc j + x] rotated by j B"""
    Gs = (n // 2) // B
    return [j * B for j in range(Gs)], 2


def shapes():
    cifar, large, mnist = networks.FACTORY_PARAMETERS["LoLaCifar"], networks.FACTORY_PARAMETERS["LoLaLarge"], networks.FACTORY_PARAMETERS["LoLa"]
    return {
        "mnist-interleave": dict(n=mnist["n"], t=mnist["primes"][0], k=None, gdbc=20, steps=[0] + [-(4096 - i) for i in range(1, 13)], classes=1, giant=False),
        "cifar-giant": dict(n=cifar["n"], t=cifar["primes"][0], k=8, gdbc=60, steps=giant(cifar["n"], 128)[0], classes=2, giant=True),
        "large-giant": dict(n=large["n"], t=large["primes"][0], k=7, gdbc=60, steps=giant(large["n"], large_baby_steps())[0], classes=2, giant=True),
    }


def run_keys(name, S, keys, rounds, limit, say):
    n, steps, nc = S["n"], S["steps"], S["classes"]
    q = default_coeff_modulus(n)
    q = q[:S["k"]] if S["k"] else q
    per = len(steps)
    if keys == "direct":
        key_steps = [s for s in steps if s]
    else:                                                       # the powers of two the non-adjacent forms of the steps need, both signs
        key_steps = sorted({sg * (1 << i) for i in range((n // 4).bit_length()) for sg in (1, -1)})
    with StepLimit(limit, "%s / %s: context and keys" % (name, keys)):
        g = Context(n, S["t"], q=q, dbc=S["gdbc"], gdbc=S["gdbc"], device=0)
        g.keygen(11, galois=False)
        g.keygen_galois(12, sorted({g.galois_elt_from_step(s) for s in key_steps}))
        g.sync()
    tot = diagonal.ks_digits(q, S["gdbc"])
    terms = per * nc
    pt, src, tmp, out, fold = g.pt_alloc(1), g.ct_alloc(terms), g.ct_alloc(terms), g.ct_alloc(nc), g.ct_alloc(terms)
    rng = np.random.default_rng(3)
    for e in range(terms):                                      # term e = nc j + x: group j of class x, as DiagonalDense lays u out
        g.pt_upload(pt, 0, rng.integers(0, 16, size=n, dtype=np.uint64))
        g.encrypt(pt, 0, src, e, 1, seed=5 + e)
    idx = [nc * j + x for x in range(nc) for j in range(per)]
    st = [steps[j] for _ in range(nc) for j in range(per)]
    off = [per * x for x in range(nc + 1)]

    def summed():
        g.rotate_rows_sum(src, idx, st, off, out, 0)

    def many_add():
        g.rotate_rows_many(src, idx, st, tmp, idx)
        for x in range(nc):
            g.add_many(tmp, [nc * j + x for j in range(per)], out, x)

    def folding():                                              # in place on a copy: u[nc j + x] += rho_(half B)(u[nc (j + half) + x])
        g.copy(src, 0, fold, 0, terms)
        half, B = per // 2, steps[1]
        while half >= 1:
            g.rotate_rows_add(fold, nc * half, half * B, fold, 0, fold, 0, nc * half)
            half //= 2
        g.copy(fold, 0, out, 0, nc)
    routes = [("summed", summed), ("many+add", many_add)] + ([("folding", folding)] if S["giant"] and per & (per - 1) == 0 and per > 1 else [])
    times, budgets, stats = {r: [] for r, _ in routes}, {}, {}
    summed0 = g.get_option("ks_summed")
    for rnd in range(rounds + 1):                               # round 0 is not timed (arenas grow, kernels load)
        for r, fn in routes:
            with StepLimit(limit, "%s / %s: %s, round %d" % (name, keys, r, rnd)):
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
                    stats[r] = {x: s1[x] - s0[x] for x in ("kernel_launches", "ntt_forward_limbs", "ntt_inverse_limbs", "Rotation")}
                    budgets[r] = float(g.invariant_noise_budget(out, 0, 1)[0])
    fused = g.get_option("ks_summed") - summed0
    fresh = float(g.invariant_noise_budget(src, 0, 1)[0])
    say("")
    say("### %s, %s keys: N = %d, k = %d, %d digits (gdbc %d), %d output(s) of %d terms, steps %s" %
        (name, keys, n, len(q), tot, S["gdbc"], nc, per, steps if per <= 4 else "%d, %d .. %d" % (steps[0], steps[1], steps[-1])))
    say("")
    say("%d Galois keys: %.1f MiB.  Fresh input: %.1f bits of budget.  The summed call launched the fused form in %d of %d calls (the others composed the literal "
        "sequence)." % (len(key_steps), len(key_steps) * tot * 2 * len(q) * n * 8 / 2 ** 20, fresh, fused, rounds + 1))
    say("")
    say("| route | median ms | min | max | launches | key switches | forward limb transforms | inverse | budget of the first output (bits) |")
    say("|---|---|---|---|---|---|---|---|---|")
    for r, _ in routes:
        ms = [1e3 * x for x in times[r]]
        say("| %s | %.3f | %.3f | %.3f | %d | %d | %d | %d | %.1f |" % (r, statistics.median(ms), min(ms), max(ms), stats[r]["kernel_launches"], stats[r]["Rotation"],
                                                                    stats[r]["ntt_forward_limbs"], stats[r]["ntt_inverse_limbs"], budgets[r]))
    med = {r: statistics.median(times[r]) for r, _ in routes}
    say("")
    say("Fastest: %s.  summed / many+add = %.2f%s." % (min(med, key=med.get), med["summed"] / med["many+add"],
                                                     ", summed / folding = %.2f" % (med["summed"] / med["folding"]) if "folding" in med else ""))
    for h in (pt, src, tmp, out, fold):
        g.free(h)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="mnist-interleave,cifar-giant,large-giant")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    say("# Summed rotations: cn_rotate_rows_sum beside cn_rotate_rows_many + cn_add_many and the folding chain")
    say("")
    say("`python tools/rotation_sum_probe.py --shapes %s --rounds %d`: one process, one device, wall-clock time of the calls between two cn_sync, median of %d timed "
        "rounds after one untimed round, the routes alternating inside every round on the same fresh ciphertexts and keys.  The code of `many+add` and `folding` is "
        "the parent commit's." % (a.shapes, a.rounds, max(a.rounds, 5)))
    S = shapes()
    for name in a.shapes.split(","):
        for keys in (("direct", "default") if S[name]["giant"] else ("direct",)):
            run_keys(name, S[name], keys, max(a.rounds, 5), a.limit, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
