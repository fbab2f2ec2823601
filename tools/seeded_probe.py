#!/usr/bin/env python
"""Measurements of the seeded symmetric ciphertexts on the GPU (profiles/seeded_probe.txt): cn_encrypt_symmetric against cn_encrypt, cn_ct_expand
against the HBM floor of its output and against the same number of inverse transforms, cn_ct_upload_compact against cn_ct_upload from pageable and
pinned host memory, and the budget gain per parameter set.  HIP events on the context stream, clocks as found, both sides in one process.

    python tools/seeded_probe.py [out.txt]
"""
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cryptonets_amd._native import Context, default_coeff_modulus  # noqa: E402

HBM_PEAK = 8.0e12            # bytes per second, MI355X data sheet
SEED_A = bytes(range(1, 33))
C3 = dict(n=8192, t=549764251649, q=None, dbc=10, gdbc=20)
C5 = dict(n=16384, t=957181001729, q=[0xfffffffd8001, 0xfffffffa0001, 0xfffffff00001, 0x1fffffff68001, 0x1fffffff50001, 0x1ffffffee8001, 0x1ffffffea0001,
                                      0x1ffffffe88001], dbc=60, gdbc=60)
BUDGET_SETS = {"tiny": dict(n=1024, t=12289, q=[0xffffee001, 0xffffc4001, 0x1ffffe0001]), "default4096": dict(n=4096, t=40961, q=None),
               "c2": dict(n=8192, t=549764251649, q=[0x7fffffd8001, 0x7fffffc8001]), "c3": C3, "c4": dict(n=8192, t=557057, q=None), "c5": C5}


def ev(g, fn, reps=7):
    fn(); g.sync()
    out = []
    for _ in range(reps):
        g.time_begin(); fn(); out.append(g.time_end() * 1e3)
    return statistics.median(out), min(out), max(out)


def wall(g, fn, reps=5):
    fn(); g.sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); g.sync(); out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def ctx(p):
    q = p["q"] or default_coeff_modulus(p["n"])
    g = Context(p["n"], p["t"], q=q, dbc=p.get("dbc", 10), gdbc=p.get("gdbc", 20), device=0)
    g.keygen(3, galois=False)
    return g


def pinned(shape):
    """a page-locked uint64 host array from the HIP runtime itself (hipHostMalloc); returns (pointer to free, array)"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    ptr, nbytes = ctypes.c_void_p(), int(np.prod(shape)) * 8
    if hip.hipHostMalloc(ctypes.byref(ptr), ctypes.c_size_t(nbytes), ctypes.c_uint(0)) != 0:
        raise RuntimeError("hipHostMalloc failed")
    arr = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint64)), shape=(int(np.prod(shape)),)).reshape(shape)
    return (hip, ptr), arr


def unpin(keep):
    keep[0].hipHostFree(keep[1])


def main(out):
    L = []

    def say(s=""):
        print(s, flush=True); L.append(s)
    say("seeded symmetric ciphertexts: median [min .. max]; kernels in us by HIP events on the context stream, copies in ms wall time; clocks as found")
    for name, p, cnt in (("c3 (N = 8192, k = 5)", C3, 784), ("c5 (N = 16384, k = 8)", C5, 128)):
        g = ctx(p)
        rng = np.random.default_rng(1)
        ph, ca, cb = g.pt_alloc(cnt), g.ct_alloc(cnt), g.ct_alloc(cnt)
        g.encode_batch(rng.integers(0, g.t, size=(cnt, g.n), dtype=np.uint64), ph, 0)
        say("\n%s, %d ciphertexts" % (name, cnt))
        e_pk = ev(g, lambda: g.encrypt(ph, 0, ca, 0, cnt, seed=5))
        e_sy = ev(g, lambda: g.encrypt_symmetric(ph, 0, cb, 0, cnt, seed=5, a_seed=SEED_A))
        e_ex = ev(g, lambda: g.ct_expand(cb, 0, cnt, SEED_A))
        say("  cn_encrypt            %8.1f [%8.1f .. %8.1f] us" % e_pk)
        say("  cn_encrypt_symmetric  %8.1f [%8.1f .. %8.1f] us   (%.2f x cn_encrypt)" % (*e_sy, e_sy[0] / e_pk[0]))
        nbytes = cnt * g.k * g.n * 8
        ptr, _ = g.device_ptr(ca)
        g.ntt_time(ptr, cnt * g.k, 0, True, 2)
        t_ntt = g.ntt_time(ptr, cnt * g.k, 0, True, 10) * 1e3
        say("  cn_ct_expand          %8.1f [%8.1f .. %8.1f] us   output %.1f MB: HBM floor %.1f us (%.2f of it); %d inverse transforms %.1f us (%.2f x)"
            % (*e_ex, nbytes / 1e6, nbytes / HBM_PEAK * 1e6, nbytes / HBM_PEAK * 1e6 / e_ex[0], cnt * g.k, t_ntt, e_ex[0] / t_ntt))
        say("  symmetric encryption = %.2f x expansion: the c0 blocks cost %.1f us beside the c1 blocks" % (e_sy[0] / e_ex[0], e_sy[0] - e_ex[0]))
        full = g.ct_download(cb, 0, cnt)
        c0 = g.ct_download_compact(cb, 0, cnt)
        keep_f, pf = pinned(full.shape); pf[:] = full
        keep_c, pc = pinned(c0.shape); pc[:] = c0
        for label, a, b in (("pageable", full, c0), ("pinned", pf, pc)):
            w_full = wall(g, lambda: g.ct_upload(ca, 0, a))
            w_comp = wall(g, lambda: g.ct_upload_compact(ca, 0, b, SEED_A))
            say("  upload from %-8s  cn_ct_upload %7.2f [%7.2f .. %7.2f] ms (%.1f MB)   cn_ct_upload_compact %7.2f [%7.2f .. %7.2f] ms (%.1f MB)   ratio %.2f"
                % (label, *w_full, a.nbytes / 1e6, *w_comp, b.nbytes / 1e6, w_comp[0] / w_full[0]))
        assert np.array_equal(g.ct_download(ca, 0, cnt), full)
        del pf, pc
        unpin(keep_f); unpin(keep_c)
        g.close()
    say("\nbudget: log2(cn_noise_norm of cn_encrypt) - log2(cn_noise_norm of cn_encrypt_symmetric), 8 ciphertexts per set, min / mean / max bits")
    say("  zero: encryptions of zero (the norm is t |fresh noise|); dense: random slots (the norm carries the term (q mod t) m of the embedding, the same for both routes)")
    for name, p in BUDGET_SETS.items():
        g = ctx(p)
        rng = np.random.default_rng(2)
        ph, ca, cb = g.pt_alloc(8), g.ct_alloc(8), g.ct_alloc(8)
        g.encode_batch(rng.integers(0, g.t, size=(8, g.n), dtype=np.uint64), ph, 0)
        for label, pt in (("zero", 0), ("dense", ph)):
            g.encrypt(pt, 0, ca, 0, 8, seed=7)
            g.encrypt_symmetric(pt, 0, cb, 0, 8, seed=7, a_seed=SEED_A, a_nonce=1 if pt else 0)
            npk, nsy = g.noise_norm(ca, 0, 8), g.noise_norm(cb, 0, 8)
            gain = [math.log2(a) - math.log2(b) for a, b in zip(npk, nsy)]
            say("  %-12s N = %5d k = %d %-5s: %6.2f / %6.2f / %6.2f   fresh budget %d -> %d bits; symmetric norm larger in %d of 8"
                % (name, g.n, g.k, label, min(gain), sum(gain) / 8, max(gain), min(g.invariant_noise_budget(ca, 0, 8, exact_bits=True)),
                   min(g.invariant_noise_budget(cb, 0, 8, exact_bits=True)), sum(1 for a, b in zip(npk, nsy) if b > a)))
        g.close()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write("\n".join(L) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
