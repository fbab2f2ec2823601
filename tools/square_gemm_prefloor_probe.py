"""cn_square_gemm on the device: one fast floor per dense output for components 0 and 1 ("sg_prefloor" = 2) against one floor per product ("sg_prefloor" = 0) in ONE
process, the same plan, alternating the two forms in rounds, HIP-event time per call (cn_event_time_begin / end), clocks as found.  Shapes: the CryptoNets ring C3
(N = 8192, five limbs), M = 100 outputs, K = 64, 128, 256, 512 and 845 inputs, a repetition = --reps calls between two events, signed weights |w| <= --wmax (44: row sums near the 18 596 of the trained 845 -> 100 layer).
Both forms are checked to give the same words before anything is timed.  Output: markdown on stdout (profiles/square_gemm_prefloor.md keeps it) - per K the median
and spread of both forms and whether the new form's SLOWEST repetition beats the old form's FASTEST: SG_PREFLOOR_MIN_K (cn_mul_plan.h) is the smallest K from which it does.
  --trace: two calls of each form at K = 845 only (for rocprofv3 --kernel-trace, a run of its own)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bench import uniform_ct_words
from cryptonets_amd._native import Context

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=8)
ap.add_argument("--reps", type=int, default=8, help="calls per timed repetition")
ap.add_argument("--wmax", type=int, default=44)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()

N, T, M = 8192, 549764251649, 100
g = Context(N, T)
g.keygen(5, galois=False)
rng = np.random.default_rng(7)
KS = [845] if args.trace else [64, 128, 256, 512, 845]
h, out = g.ct_alloc(max(KS)), g.ct_alloc(M)
for s in range(0, max(KS), 256):
    c = min(256, max(KS) - s)
    g.ct_upload(h, s, uniform_ct_words(rng, g.q, N, c))
bias = np.zeros((M, N), dtype=np.uint64)
bias[:, 0] = rng.integers(1, T, size=M, dtype=np.uint64)
bh = g.pt_alloc(M)
g.pt_upload(bh, 0, bias)


def timed(plan):
    g.sync()
    g.time_begin()
    for _ in range(args.reps):
        g.square_gemm(plan, h, 0, out, 0)
    return g.time_end() / args.reps


if not args.trace:
    print("| K | new ms: median (min .. max) | old ms: median (min .. max) | new / old | new max < old min |")
    print("|---|---|---|---|---|")
for K in KS:
    W = rng.integers(-args.wmax, args.wmax + 1, size=(M, K))
    W[W == 0] = 1
    plan = g.gemm_plan(np.mod(W, T).astype(np.uint64), bias_pt=bh, bias_idx=np.arange(M, dtype=np.int32))
    words = []
    for mode in (2, 0):                                              # warm-up of both forms (arenas, code objects), the counter and the word check
        g.set_option("sg_prefloor", mode)
        before = g.get_option("square_gemm_prefloor")
        g.square_gemm(plan, h, 0, out, 0)
        assert g.get_option("square_gemm_prefloor") - before == (1 if mode else 0), "the form asked for did not run"
        words.append(g.ct_download(out, 0, M))
    assert np.array_equal(words[0], words[1]), "the two forms differ"
    if args.trace:
        for mode in (2, 0, 2, 0):
            g.set_option("sg_prefloor", mode)
            g.square_gemm(plan, h, 0, out, 0)
        g.sync()
        continue
    t = {2: [], 0: []}
    for mode in (2, 0):                                              # one untimed repetition of each form at this shape: clocks and caches as in the rounds
        g.set_option("sg_prefloor", mode)
        timed(plan)
    for r in range(args.rounds):
        for mode in ((2, 0) if r % 2 == 0 else (0, 2)):
            g.set_option("sg_prefloor", mode)
            t[mode].append(timed(plan))
    a, b = t[2], t[0]
    print("| %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.3f | %s |" % (
        K, statistics.median(a), min(a), max(a), statistics.median(b), min(b), max(b), statistics.median(a) / statistics.median(b), "yes" if max(a) < min(b) else "no"), flush=True)
    g.free(plan)
g.set_option("sg_prefloor", 1)
