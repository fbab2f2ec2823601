"""cn_mul_relin_sum on the device: the one-key-switch-per-output form ("mul_sum" = 1) against the literal sequence ("mul_sum" = 0: Multiply + Relinearize per
term into a temporary, AddMany per output - the code path before the call existed) in ONE process, alternating the two forms in rounds, HIP-event time per call
(cn_event_time_begin / end), clocks as found.  Shapes: CryptoNets ring C3 (N = 8192, five limbs) with K = 845 x 1 output, K = 100 x 8 outputs, and K = 2, 3, 4, 8
at 1 and 8 outputs (the routing threshold MUL_SUM_MIN_K).  Per shape: median and spread (min .. max) of both forms, the key switches saved, and the bytes
k_product_sum reads (3 K k N 8 per output) with the time they take at 8 TB/s - the kernel's own duration comes from a kernel trace of `--trace` (a run of its own:
  rocprofv3 --kernel-trace -f csv -d DIR -- python tools/mul_sum_probe.py --trace ; python tools/summarize_trace.py DIR/.../*kernel_trace.csv).
Both forms are checked to give the same words before anything is timed.  Output: markdown on stdout (profiles/mul_relin_sum.md keeps it)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bench import uniform_ct_words
from cryptonets_amd._native import Context

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--trace", action="store_true", help="two fused calls of the two large shapes only (for a kernel trace)")
args = ap.parse_args()

N, T = 8192, 549764251649
g = Context(N, T)
g.keygen(5, galois=False)
rng = np.random.default_rng(1)
SHAPES = [(845, 1), (100, 8)] + ([] if args.trace else [(K, c) for K in (2, 3, 4, 8) for c in (1, 8)])
KMAX, CMAX, AMAX = max(K for K, _ in SHAPES), max(c for _, c in SHAPES), max(K * c for K, c in SHAPES)
# one array of columns (term k of output i at k * count + i) and one of sparse entries: uniform words, the distribution of ciphertext words
ha, hb = g.ct_alloc(AMAX), g.ct_alloc(KMAX)
for h, total in ((ha, AMAX), (hb, KMAX)):
    for s in range(0, total, 256):
        c = min(256, total - s)
        g.ct_upload(h, s, uniform_ct_words(rng, g.q, N, c))
out = g.ct_alloc(CMAX)


def call(K, count):
    g.mul_relin_sum([ha] * K, [k * count for k in range(K)], [hb] * K, list(range(K)), 0, out, 0, count)


def timed(K, count, reps):
    g.sync()
    g.time_begin()
    for _ in range(reps):
        call(K, count)
    return g.time_end() / reps


if args.trace:
    for K, count in SHAPES:
        for _ in range(2):
            call(K, count)
    g.sync()
    sys.exit(0)

print("| K | outputs | fused ms: median (min .. max) | literal ms: median (min .. max) | fused / literal | key switches saved | k_product_sum reads | at 8 TB/s |")
print("|---|---|---|---|---|---|---|---|")
for K, count in SHAPES:
    words = []
    for mode in (1, 0):                                              # warm-up of both forms (arenas, code objects) and the word check
        g.set_option("mul_sum", mode)
        before = g.get_option("mul_sum_fused")
        call(K, count)
        assert g.get_option("mul_sum_fused") - before == mode, "the form asked for did not run"
        words.append(g.ct_download(out, 0, count))
    assert np.array_equal(words[0], words[1]), "the two forms differ"
    reps = 1 if K * count >= 100 else 10
    t = {1: [], 0: []}
    for r in range(args.rounds):
        for mode in ((1, 0) if r % 2 == 0 else (0, 1)):
            g.set_option("mul_sum", mode)
            t[mode].append(timed(K, count, reps))
    f, l = t[1], t[0]
    nbytes = 3 * K * g.k * N * 8 * count
    print("| %d | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.2f | %d | %.1f MB | %.3f ms |" % (
        K, count, statistics.median(f), min(f), max(f), statistics.median(l), min(l), max(l), statistics.median(f) / statistics.median(l),
        (K - 1) * count, nbytes / 1e6, nbytes / 8e12 * 1e3), flush=True)
g.set_option("mul_sum", 1)
