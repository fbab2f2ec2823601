#!/usr/bin/env python
"""How a CryptoNets-MNIST batch REACHES the evaluation (config 3: 784 input ciphertexts per plaintext prime, 2 primes, N = 8192, k = 5; synthetic images,
fixed seeds) - writes profiles/ingest_probe.txt.

  P  a build of the PARENT commit (its tree, extracted and built by --build-parent): per batch cn_ct_upload_compact from a numpy array, forward(), download of the logits
  S  this tree: cn_ct_upload_packed instead
  and, each alone: the pinned host-to-device copy of one batch's packed bytes (against the 63 GB/s link spec), forward() with resident inputs.

Every sequence runs in a process of its own (one after the other, alternated P S P S ..., --reps times each) over --batches batches after --warmup; wall
clock around work that ends in a device synchronise.  The logits' SHA-256 must be the same in P and S.

    python tools/ingest_probe.py --build-parent HEAD~1 DIR      # extract that commit into DIR and build its library there (no GPU needed)
    python tools/ingest_probe.py --parent DIR [--out FILE]      # on the GPU
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_A = bytes((11 * i + 5) & 0xff for i in range(32))
LINK_GBS = 63.0


def build_parent(rev, where):
    os.makedirs(where, exist_ok=True)
    tar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, "cryptonets_amd", "include"], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", where], stdin=tar.stdout)
    if tar.wait():
        raise SystemExit("git archive %s failed" % rev)
    subprocess.check_call([sys.executable, "-c", "from cryptonets_amd import _native; _native.build()"], cwd=where)
    print("parent %s built in %s" % (rev, where))


def setup():
    """the two channels with device-made keys and one batch of seeded inputs per prime as c0 words (the same words in every sequence: fixed seeds)"""
    from cryptonets_amd._native import Context
    from cryptonets_amd import cryptonets_mnist as cm
    layers = cm.layer_tables(*cm.synthetic_weights(1))
    x_int = np.rint(cm.synthetic_images(cm.N, seed=1000) * cm.NORMALIZATION * cm.INPUT_SCALE).astype(np.int64)
    chans, c0s = [], []
    for p in cm.PLAIN_PRIMES:
        g = Context(cm.N, p, dbc=10, gdbc=20, device=0)
        g.set_rng_key(bytes(range(32)))
        g.keygen(0xC0FFEE ^ p, galois=False)
        ch = cm.CryptoNetsChannel(g, layers, cm.constant_plaintext(cm.N))
        ph = g.pt_alloc(784)
        g.encode_batch(np.ascontiguousarray(np.mod(x_int, p).astype(np.uint64).T), ph, 0)
        g.encrypt_symmetric(ph, 0, ch.h_in, 0, 784, seed=0xFEED, a_seed=SEED_A, a_nonce=1, a_item0=0)
        g.free(ph)
        c0s.append(g.ct_download_compact(ch.h_in, 0, 784))
        chans.append(ch)
    return cm, chans, c0s


class Desc:
    a_seed, a_nonce, a_item0 = SEED_A, 1, 0


def run_sequence(seq, batches, warmup):
    cm, chans, c0s = setup()
    digest = hashlib.sha256()

    def logits(ch):
        w = ch.g.ct_download(ch.h5, 0, 10)
        digest.update(w.tobytes())
        return w

    def sync():
        for ch in chans:
            ch.g.sync()
    out = {"seq": seq}
    if seq in ("P", "S"):
        if seq == "S":
            data = [ch.g.ct_download_packed(ch.h_in, 0, 784, polys=1) for ch in chans]
        else:
            data = c0s

        def step():
            for ch, d in zip(chans, data):
                if seq == "S":
                    ch.g.ct_upload_packed(ch.h_in, 0, d, polys=1, a_seed=SEED_A, a_nonce=1, a_item0=0)
                else:
                    ch.g.ct_upload_compact(ch.h_in, 0, d, SEED_A, a_nonce=1, a_item0=0)
                ch.forward()
            for ch in chans:
                logits(ch)
        for _ in range(warmup):
            step()
        sync()
        digest = hashlib.sha256()
        t0 = time.perf_counter()
        for _ in range(batches):
            step()
        sync()
        out["ms_per_batch"] = 1e3 * (time.perf_counter() - t0) / batches
        out["bytes_per_batch"] = int(sum(d.nbytes for d in data))
    elif seq == "floors":
        import ctypes as C
        hip = C.CDLL("libamdhip64.so")
        data = [ch.g.ct_download_packed(ch.h_in, 0, 784, polys=1) for ch in chans]
        hostp = []
        for d in data:                                                        # one pinned block per prime
            ptr = C.c_void_p()
            assert hip.hipHostMalloc(C.byref(ptr), C.c_size_t(d.nbytes), C.c_uint(0)) == 0
            C.memmove(ptr, d.ctypes.data, d.nbytes)
            hostp.append(ptr)
        times = []
        for _ in range(2 + 8):
            t0 = time.perf_counter()
            for ch, hp, d in zip(chans, hostp, data):
                dev, _ = ch.g.device_ptr(ch.h1)                               # any device array large enough: h1 is rewritten by forward()
                rc = hip.hipMemcpy(C.c_void_p(dev), hp, C.c_size_t(d.nbytes), C.c_int(1))
                assert rc == 0, rc
            assert hip.hipDeviceSynchronize() == 0
            times.append(time.perf_counter() - t0)
        nbytes = sum(d.nbytes for d in data)
        out["copy_ms"] = [1e3 * t for t in times[2:]]
        out["copy_bytes"] = int(nbytes)
        fw = []
        for _ in range(3):
            sync()
            t0 = time.perf_counter()
            for _ in range(batches):
                for ch in chans:
                    ch.forward()
            sync()
            fw.append(1e3 * (time.perf_counter() - t0) / batches)
        out["forward_ms"] = fw
        for hp in hostp:
            hip.hipHostFree(hp)
    out["sha256"] = digest.hexdigest() if seq != "floors" else None
    print("RESULT " + json.dumps(out), flush=True)


def child(seq, tree, batches, warmup):
    env = dict(os.environ, PYTHONPATH=tree)
    env.pop("CNHIP_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--sequence", seq, "--batches", str(batches), "--warmup", str(warmup)], env=env, cwd=tree,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit("sequence %s failed (exit %d):\n%s" % (seq, p.returncode, p.stdout[-3000:]))


def spread(v):
    return "min %.2f  median %.2f  max %.2f" % (min(v), sorted(v)[len(v) // 2], max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-parent", nargs=2, metavar=("REV", "DIR"))
    ap.add_argument("--parent", help="the extracted and built tree of the parent commit")
    ap.add_argument("--sequence", choices=["P", "S", "floors"])
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_probe.txt"))
    a = ap.parse_args()
    if a.build_parent:
        return build_parent(*a.build_parent)
    if a.sequence:
        sys.path.insert(0, os.getcwd())
        return run_sequence(a.sequence, a.batches, a.warmup)
    if not a.parent:
        raise SystemExit("--parent DIR: the tree --build-parent made")
    res = {"P": [], "S": []}
    for _ in range(a.reps):                       # alternated
        for seq in ("P", "S"):
            res[seq].append(child(seq, os.path.abspath(a.parent) if seq == "P" else ROOT, a.batches, a.warmup))
    fl = child("floors", ROOT, a.batches, a.warmup)
    ms = {s: [r["ms_per_batch"] for r in res[s]] for s in res}
    shas = {s: sorted({r["sha256"] for r in res[s]}) for s in res}
    same = len({x for v in shas.values() for x in v}) == 1
    copy_ms = sorted(fl["copy_ms"])[len(fl["copy_ms"]) // 2]
    fwd_ms = min(fl["forward_ms"])
    gbs = fl["copy_bytes"] / (copy_ms * 1e-3) / 1e9
    lines = [
        "ingest probe: CryptoNets-MNIST config 3 (784 ciphertexts x 2 primes, N = 8192, k = 5), %d batches after %d warm-up, %d runs per sequence, alternated P S" % (a.batches, a.warmup, a.reps),
        "per batch: upload of both primes' inputs, forward() of both, download of the logits; wall clock, ends in a device synchronise; ms per batch",
        "  P  parent build, cn_ct_upload_compact (%d bytes per batch): %s   runs %s" % (res["P"][0]["bytes_per_batch"], spread(ms["P"]), " ".join("%.2f" % x for x in ms["P"])),
        "  S  this tree, cn_ct_upload_packed    (%d bytes per batch): %s   runs %s" % (res["S"][0]["bytes_per_batch"], spread(ms["S"]), " ".join("%.2f" % x for x in ms["S"])),
        "floors, each alone:",
        "  pinned H2D copy of one batch's packed bytes (%d bytes): median %.2f ms (%s) = %.1f GB/s, %.0f %% of the %.0f GB/s link spec" % (
            fl["copy_bytes"], copy_ms, spread(fl["copy_ms"]), gbs, 100 * gbs / LINK_GBS, LINK_GBS),
        "  forward() of both primes, inputs resident: %s ms per batch" % spread(fl["forward_ms"]),
        "S against max(copy alone, forward alone) = %.2f ms: median S %.2f ms = %.2f x" % (max(copy_ms, fwd_ms), sorted(ms["S"])[len(ms["S"]) // 2], sorted(ms["S"])[len(ms["S"]) // 2] / max(copy_ms, fwd_ms)),
        "logits SHA-256: %s" % ("identical in P and S: " + shas["P"][0] if same else "DIFFER: %s" % shas),
        "k_unpack_rows kernel time against its bytes: not measured (needs a rocprofv3 --kernel-trace --stats run of `tools/ingest_probe.py --sequence S`, in a call of its own)",
    ]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
