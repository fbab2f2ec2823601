"""The dense layer of one image on the default path (cn_rowdot_batch + one-hot masks) and on the diagonal path (hewrapper.DIAGONAL_DENSE: cn_mul_plain_sum between
baby and giant steps), in one process on the same input ciphertext: wall-clock time of Mul(..., ForceDenseFormat=True) with the plans and plaintexts resident,
equality of all N decrypted slots, and the invariant noise budget (cn_noise_norm) of both outputs per plaintext prime.

Shapes: the test shape 37 x 700 at N = 1024 (two primes, three 36-37-bit limbs), the LoLa-CIFAR layer 5488 x 16268 (N = 16384, 8 limbs, dbc 60) and the LargeLoLa
layer 2608 x 11952 (N = 16384, 7 limbs).  Weights are synthetic small integers (the reference's blobs are not available); the input is a FRESH encryption of small
integers - in the networks it arrives behind a squaring with most of its budget spent, so the budgets below compare the two paths, they are not the networks'.

"network": the LoLa-CIFAR network of the reference's parameters (8 limbs, two primes, synthetic full-range weights of the reference's shapes) evaluated to the logits
with the flag off and on - time of the 5488 x 16268 layer inside the network (bias add included), the budgets behind the layers that follow, and whether the
decrypted outputs equal the integer model (networks.lola_cifar_dense_model).

    python tools/diag_dense_probe.py [--shapes tiny,cifar,large,network] [--primes 1] [--rounds 3] [--out profiles/diag_dense.md]

--ntt-weights: the diagonal path with its plan in coefficient form and in NTT form (hewrapper.NTT_WEIGHTS, cn_pt_transform: DESIGN 6h), both resident in one
process, timed in alternating rounds on the same input ciphertext after one untimed round each; plan build time and resident bytes of each form; all decrypted
slots compared across the two forms and with W v mod t.  --rowdot adds RowsDotProduct (cn_rowdot_batch over all rows, no masks) with the flag off and on.

    python tools/diag_dense_probe.py --ntt-weights [--rowdot] [--shapes tiny,cifar,large] [--primes 1] [--rounds 5] [--out profiles/ntt_weights.md]

--device-plan: the plan itself built on the host route and on the device route (hewrapper.DEVICE_DIAGONAL_PLAN: cn_diag_scan, cn_diag_encode), alternating
in one process with 1 .. --primes plaintext primes, in coefficient form and in NTT form: "plan built in" of both, equality of every plaintext word of the two arrays,
the layer on either plan, resident bytes, the scratch arena.

    python tools/diag_dense_probe.py --device-plan [--shapes tiny,cifar,large] [--primes 2] [--rounds 3] [--out profiles/diag_device_plan.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from cryptonets_amd import diagonal, hewrapper, networks
from cryptonets_amd.hewrapper import EMatrixFormat, EncryptedSealBfvFactory, EVectorFormat

TINY_Q = [0xffffee001, 0xffffc4001, 0x1ffffe0001]


class TinyContexts:
    """context factory of the N = 1024 test ring (the library's default modulus at 1024 is a single prime: no rotations)"""

    def default_coeff_modulus(self, n):
        return list(TINY_Q)

    def __call__(self, n, t, q, dbc, gdbc):
        from cryptonets_amd._native import Context
        return Context(n, t, q=q, dbc=dbc, gdbc=gdbc, device=0)


def device_client(ctx, t):
    from cryptonets_amd.client import DeviceClient
    return DeviceClient(ctx, seed=1234 ^ t)


SHAPES = {
    "tiny": dict(R=37, Dim=700, parms=dict(primes=(12289, 40961), n=1024, context_factory=TinyContexts(), device_client_factory=device_client), wmax=3, vmax=3),
    "cifar": dict(R=5488, Dim=16268, parms=dict(networks.FACTORY_PARAMETERS["LoLaCifar"], client_seed=7), wmax=10, vmax=50),
    "large": dict(R=2608, Dim=11952, parms=dict(networks.FACTORY_PARAMETERS["LoLaLarge"], client_seed=7), wmax=10, vmax=50),
}


def sync(env):
    for e in env.Environments:
        e.ctx.sync()


def slots_and_budgets(vec, env):
    slots, budgets = [], []
    for a, e in zip(vec.eVectors, env.Environments):
        d, ctx = a.encData, e.ctx
        budgets.append(float(ctx.invariant_noise_budget(d.h, d.first, 1)[0]))
        plain = e.client.decrypt(ctx.ct_download(d.h, d.first, 1)[0])
        pt = ctx.pt_alloc(1)
        ctx.pt_upload(pt, 0, plain)
        slots.append(ctx.decode_batch(pt, 0, 1)[0])
        ctx.free(pt)
    return slots, budgets


def timed(fn, env, rounds):
    out, ms = None, []
    for _ in range(rounds):
        if out is not None:
            out.Dispose()
        sync(env)
        t0 = time.perf_counter()
        out = fn()
        sync(env)
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def probe(name, nprimes, rounds, say):
    s = SHAPES[name]
    parms = dict(s["parms"])
    parms["primes"] = tuple(parms["primes"])[:nprimes]
    R, Dim = s["R"], s["Dim"]
    rng = np.random.default_rng(11)
    W = rng.integers(-s["wmax"], s["wmax"] + 1, size=(R, Dim)).astype(float)
    W[:, 0] = np.where(W.any(axis=1), W[:, 0], 1)
    v = rng.integers(-s["vmax"], s["vmax"] + 1, size=Dim).astype(float)
    F = EncryptedSealBfvFactory(**parms)
    env = F.AllocateComputationEnv()
    ctx0 = env.Environments[0].ctx
    mat = F.GetPlainMatrix(W, EMatrixFormat.RowMajor, 1.0)
    vec = F.GetEncryptedVector(v, EVectorFormat.dense, 1.0)
    counts = mat.DiagonalDenseCounts(vec, env)
    say("### %s: %d x %d, N = %d, k = %d, %d plaintext prime(s) %s" % (name, R, Dim, ctx0.n, len(ctx0.q), len(parms["primes"]), list(parms["primes"])))
    say("")
    say("limb transforms counted (`diagonal.dense_path_counts`): default %d (%d key switches), diagonal %d (%d key switches, %d diagonals, B = %d) -> %s"
        % (counts["default"], counts["default_key_switches"], counts["diagonal"], counts["diagonal_key_switches"], counts["diagonals"], counts["B"], counts["choice"]))
    _, in_budget = slots_and_budgets(vec, env)
    hewrapper.DIAGONAL_DENSE = False
    mat.Mul(vec, env, ForceDenseFormat=True).Dispose()               # untimed: row plaintexts and masks become resident
    base, ms_default = timed(lambda: mat.Mul(vec, env, ForceDenseFormat=True), env, rounds)
    t0 = time.perf_counter()
    plans = [mat._diagonal_plan(i, e)[0] for i, e in enumerate(env.Environments)]
    sync(env)
    plan_s = time.perf_counter() - t0
    mat.DiagonalDense(vec, env).Dispose()                            # untimed: the scratch arena takes its size
    out, ms_diag = timed(lambda: mat.DiagonalDense(vec, env), env, rounds)
    a, ba = slots_and_budgets(base, env)
    b, bb = slots_and_budgets(out, env)
    equal = all(np.array_equal(x, y) for x, y in zip(a, b))
    t = [int(e.ctx.t) for e in env.Environments]
    want = (W.astype(np.int64) @ v.astype(np.int64))
    model = all(np.array_equal(x[:R].astype(np.int64), np.mod(want, ti)) and not x[R:].any() for x, ti in zip(b, t))
    p = plans[0]
    say("")
    say("| | default path | diagonal path |")
    say("|---|---|---|")
    say("| time per layer, ms (min / median of %d) | %.2f / %.2f | %.2f / %.2f |" % (rounds, min(ms_default), statistics.median(ms_default), min(ms_diag), statistics.median(ms_diag)))
    say("| invariant noise budget of the output, bits, per prime (input: %s) | %s | %s |" % (", ".join("%.1f" % x for x in in_budget), ", ".join("%.1f" % x for x in ba),
                                                                                             ", ".join("%.1f" % x for x in bb)))
    say("")
    say("ratio default / diagonal (medians): %.2f.  All %d decrypted slots equal on both paths: %s; equal to W v mod t with zeros at %d and above: %s."
        % (statistics.median(ms_default) / statistics.median(ms_diag), ctx0.n, equal, R, model))
    say("Plan: B = %d, Gs = %d, %d diagonals in %d groups, %d rotated inputs, %d key switches (baby steps by doubling: %s, giant steps by folding: %s); built and encoded once in %.1f s "
        "(host, untimed above); resident diagonal plaintexts %.1f MiB per prime against %.1f MiB of row plaintexts."
        % (p.B, p.Gs, p.terms, len(p.groups), len(p.babies), p.key_switches(), p.babies_by_doubling, p.giants_by_folding, plan_s, p.terms * ctx0.n * 8 / 2 ** 20,
           R * ctx0.n * 8 / 2 ** 20))
    say("")
    for x in (base, out, vec):
        x.Dispose()
    mat.Dispose()
    for e in env.Environments:
        e.ctx.close()
    return equal and model


def probe_ntt(name, nprimes, rounds, rowdot, say):
    """coefficient-form plan against NTT-form plan of the diagonal path, alternating rounds in one process"""
    s = SHAPES[name]
    parms = dict(s["parms"])
    parms["primes"] = tuple(parms["primes"])[:nprimes]
    R, Dim = s["R"], s["Dim"]
    rng = np.random.default_rng(11)
    W = rng.integers(-s["wmax"], s["wmax"] + 1, size=(R, Dim)).astype(float)
    W[:, 0] = np.where(W.any(axis=1), W[:, 0], 1)
    v = rng.integers(-s["vmax"], s["vmax"] + 1, size=Dim).astype(float)
    F = EncryptedSealBfvFactory(**parms)
    env = F.AllocateComputationEnv()
    ctx0 = env.Environments[0].ctx
    k, n = len(ctx0.q), ctx0.n
    mat = F.GetPlainMatrix(W, EMatrixFormat.RowMajor, 1.0)
    vec = F.GetEncryptedVector(v, EVectorFormat.dense, 1.0)
    say("### %s: %d x %d, N = %d, k = %d, %d plaintext prime(s) %s" % (name, R, Dim, n, k, len(parms["primes"]), list(parms["primes"])))
    say("")
    hewrapper.DIAGONAL_DENSE = True
    build, plans = {}, {}
    for flag in (False, True):                                       # plans of both forms become resident (cache keys carry the flag)
        hewrapper.NTT_WEIGHTS = flag
        if flag:
            mat._row_plaintexts(0, env.Environments[0])              # (the rows the plan reads are there already: only the plan itself is timed)
        sync(env)
        t0 = time.perf_counter()
        plans[flag] = [mat._diagonal_plan(i, e)[0] for i, e in enumerate(env.Environments)]
        sync(env)
        build[flag] = time.perf_counter() - t0
        mat.DiagonalDense(vec, env).Dispose()                        # untimed round
    ms, outs = {False: [], True: []}, {False: None, True: None}
    launches0 = [e.ctx.get_option("ptn_sum") for e in env.Environments]
    for _ in range(rounds):
        for flag in (False, True):
            hewrapper.NTT_WEIGHTS = flag
            if outs[flag] is not None:
                outs[flag].Dispose()
            sync(env)
            t0 = time.perf_counter()
            outs[flag] = mat.DiagonalDense(vec, env)
            sync(env)
            ms[flag].append((time.perf_counter() - t0) * 1e3)
    ran = [e.ctx.get_option("ptn_sum") - l for e, l in zip(env.Environments, launches0)]
    a, _ = slots_and_budgets(outs[False], env)
    b, _ = slots_and_budgets(outs[True], env)
    words = all(np.array_equal(e.ctx.ct_download(x.encData.h, x.encData.first, 1), e.ctx.ct_download(y.encData.h, y.encData.first, 1))
                for x, y, e in zip(outs[False].eVectors, outs[True].eVectors, env.Environments))
    equal = all(np.array_equal(x, y) for x, y in zip(a, b))
    t = [int(e.ctx.t) for e in env.Environments]
    want = (W.astype(np.int64) @ v.astype(np.int64))
    model = all(np.array_equal(x[:R].astype(np.int64), np.mod(want, ti)) and not x[R:].any() for x, ti in zip(b, t))
    p = plans[True][0]
    say("| diagonal path | coefficient-form plan | NTT-form plan |")
    say("|---|---|---|")
    say("| time per layer, ms (min / median of %d, alternating) | %.2f / %.2f | %.2f / %.2f |"
        % (rounds, min(ms[False]), statistics.median(ms[False]), min(ms[True]), statistics.median(ms[True])))
    say("| plan built in, s (all primes; host rotation + encode%s) | %.2f | %.2f |" % (", + cn_pt_transform per chunk", build[False], build[True]))
    say("| resident plan plaintexts per prime, MiB | %.1f | %.1f |" % (p.terms * n * 8 / 2 ** 20, p.terms * k * n * 8 / 2 ** 20))
    say("")
    say("ratio coefficient / NTT form (medians): %.2f.  %d diagonals, %d rotated inputs, %d groups; `k_mul_ptn_sum` launches in the timed rounds per prime: %s.  "
        "Ciphertext words equal: %s; all %d decrypted slots equal across the two forms: %s; equal to W v mod t with zeros at %d and above: %s."
        % (statistics.median(ms[False]) / statistics.median(ms[True]), p.terms, len(p.babies), len(p.groups), ran, words, n, equal, R, model))
    say("")
    ok = words and equal and model
    for x in outs.values():
        x.Dispose()
    if rowdot:
        hewrapper.DIAGONAL_DENSE = False
        rms, rout = {False: [], True: []}, {}
        for flag in (False, True):
            hewrapper.NTT_WEIGHTS = flag
            for x in mat.RowsDotProduct(vec, env):                   # untimed: the rows (and their NTT form) become resident
                x.Dispose()
        for _ in range(rounds):
            for flag in (False, True):
                hewrapper.NTT_WEIGHTS = flag
                for x in rout.get(flag, []):
                    x.Dispose()
                sync(env)
                t0 = time.perf_counter()
                rout[flag] = mat.RowsDotProduct(vec, env)
                sync(env)
                rms[flag].append((time.perf_counter() - t0) * 1e3)
        same = all(np.array_equal(e.ctx.ct_download(rout[False][0].eVectors[i].encData.buf.h, 0, R), e.ctx.ct_download(rout[True][0].eVectors[i].encData.buf.h, 0, R))
                   for i, e in enumerate(env.Environments))
        say("`RowsDotProduct` (cn_rowdot_batch, %d rows, all slots), ms, min / median of %d alternating rounds: coefficient-form rows %.2f / %.2f, NTT-form rows %.2f / %.2f "
            "(resident rows %.1f against %.1f MiB per prime); all ciphertext words equal: %s."
            % (R, rounds, min(rms[False]), statistics.median(rms[False]), min(rms[True]), statistics.median(rms[True]), R * n * 8 / 2 ** 20, R * k * n * 8 / 2 ** 20, same))
        say("")
        ok = ok and same
        for outs_ in rout.values():
            for x in outs_:
                x.Dispose()
    hewrapper.DIAGONAL_DENSE = hewrapper.NTT_WEIGHTS = False
    vec.Dispose()
    mat.Dispose()
    for e in env.Environments:
        e.ctx.close()
    return ok


def probe_device_plan(name, nprimes, rounds, say):
    """the plan of the diagonal path built on the host route (decode_batch, numpy, encode_batch per chunk: hewrapper.DEVICE_DIAGONAL_PLAN = False) and on the device
    route (cn_diag_scan, diagonal.plan_from_flags, one cn_diag_encode), alternating in one process, for the coefficient form and the NTT form"""
    s = SHAPES[name]
    parms = dict(s["parms"])
    parms["primes"] = tuple(parms["primes"])[:nprimes]
    R, Dim = s["R"], s["Dim"]
    rng = np.random.default_rng(11)
    W = rng.integers(-s["wmax"], s["wmax"] + 1, size=(R, Dim)).astype(float)
    W[:, 0] = np.where(W.any(axis=1), W[:, 0], 1)
    v = rng.integers(-s["vmax"], s["vmax"] + 1, size=Dim).astype(float)
    F = EncryptedSealBfvFactory(**parms)
    env = F.AllocateComputationEnv()
    ctx0 = env.Environments[0].ctx
    k, n = len(ctx0.q), ctx0.n
    mat = F.GetPlainMatrix(W, EMatrixFormat.RowMajor, 1.0)
    vec = F.GetEncryptedVector(v, EVectorFormat.dense, 1.0)
    say("### %s: %d x %d, N = %d, k = %d, %d plaintext prime(s) %s" % (name, R, Dim, n, k, len(parms["primes"]), list(parms["primes"])))
    say("")
    hewrapper.DIAGONAL_DENSE = True
    for i, e in enumerate(env.Environments):
        mat._row_plaintexts(i, e)                                    # (the rows both routes read are resident: only the plan itself is timed)

    def drop():
        for (_, pts) in mat.__dict__.pop("_diagplan", {}).values():
            pts.release()

    def build(dev):
        hewrapper.DEVICE_DIAGONAL_PLAN = dev
        sync(env)
        t0 = time.perf_counter()
        got = [mat._diagonal_plan(i, e) for i, e in enumerate(env.Environments)]
        sync(env)
        return time.perf_counter() - t0, got

    def same_words(ctx, a, b, count, ntt):
        item = (k if ntt else 1) * n * 8
        step = max(1, (256 << 20) // item)
        down = ctx.ptn_download if ntt else ctx.pt_download
        return all(np.array_equal(down(a.h, a.first + c, min(step, count - c)), down(b.h, b.first + c, min(step, count - c))) for c in range(0, count, step))
    ok = True
    say("| plan form | plan built in, s, host route (all primes; %d alternating builds) | device route | ratio of the medians | every plaintext word equal | layer on the host-built / device-built plan, ms (median of %d) "
        "| resident plan plaintexts per prime, MiB, host / device route | scratch arena per context after the device build, MiB |" % (rounds, rounds))
    say("|---|---|---|---|---|---|---|---|")
    for ntt in (False, True):
        hewrapper.NTT_WEIGHTS = ntt
        for dev in (False, True):                                    # one untimed build of each
            build(dev)
            drop()
        secs = {False: [], True: []}
        for r in range(rounds):
            plans = {}
            for dev in (False, True):
                dt, plans[dev] = build(dev)
                secs[dev].append(dt)
            if r + 1 < rounds:
                drop()
        equal = all(hp.terms == dp.terms and hp.grp_off == dp.grp_off and hp.ct_idx == dp.ct_idx and hp.babies == dp.babies and hp.groups == dp.groups
                    and same_words(e.ctx, hb, db, hp.terms, ntt) for (hp, hb), (dp, db), e in zip(plans[False], plans[True], env.Environments))
        ms, outs = {False: [], True: []}, {}
        for dev in (False, True):
            hewrapper.DEVICE_DIAGONAL_PLAN = dev
            mat.DiagonalDense(vec, env).Dispose()                    # untimed
        for _ in range(rounds):
            for dev in (False, True):
                hewrapper.DEVICE_DIAGONAL_PLAN = dev
                if dev in outs:
                    outs[dev].Dispose()
                sync(env)
                t0 = time.perf_counter()
                outs[dev] = mat.DiagonalDense(vec, env)
                sync(env)
                ms[dev].append((time.perf_counter() - t0) * 1e3)
        words = all(np.array_equal(e.ctx.ct_download(x.encData.h, x.encData.first, 1), e.ctx.ct_download(y.encData.h, y.encData.first, 1))
                    for x, y, e in zip(outs[False].eVectors, outs[True].eVectors, env.Environments))
        item = (k if ntt else 1) * n * 8 / 2 ** 20
        say("| %s | %s (median %.2f) | %s (median %.3f) | %.0f | %s | %.2f / %.2f (ciphertext words equal: %s) | %.1f / %.1f | %.1f |"
            % ("NTT" if ntt else "coefficient", ", ".join("%.2f" % x for x in secs[False]), statistics.median(secs[False]), ", ".join("%.3f" % x for x in secs[True]),
               statistics.median(secs[True]), statistics.median(secs[False]) / statistics.median(secs[True]), equal, statistics.median(ms[False]), statistics.median(ms[True]), words,
               plans[False][0][1].buf.count * item, plans[True][0][1].buf.count * item, ctx0.get_option("scratch_mib")))
        ok = ok and equal and words
        for x in outs.values():
            x.Dispose()
        drop()
    p = plans[True][0][0]
    say("")
    say("%d diagonals kept of %d structural candidates, B = %d, %d groups; `k_diag_scan` / `k_diag_gather` launches per context: %d / %d."
        % (p.terms, int(diagonal.structural_diagonals(R, Dim, n).sum()), p.B, len(p.groups), ctx0.get_option("diag_scan"), ctx0.get_option("diag_encode")))
    say("")
    hewrapper.DIAGONAL_DENSE = hewrapper.NTT_WEIGHTS = hewrapper.DEVICE_DIAGONAL_PLAN = False
    vec.Dispose()
    mat.Dispose()
    for e in env.Environments:
        e.ctx.close()
    return ok


def mulmod(a, b, p):
    b = np.asarray(b, dtype=np.uint64)
    hi = (a * (b >> np.uint64(20))) % p
    return (hi * np.uint64(1 << 20) + a * (b & np.uint64(0xFFFFF))) % p


def network(say):
    """LoLa-CIFAR, 8 limbs (LolaCifarCryptoNet.cs:35,58-131), one image, flag off and on"""
    say("### network: LoLa-CIFAR at the reference's parameters (N = 16384, 8 limbs, two primes), one image, synthetic weights of the reference's shapes")
    say("")
    say("| `DIAGONAL_DENSE` | dense 5488 x 16268 layer in the network, ms (three runs) | its outputs exact | budget per prime, bits: input of the layer / its output / behind the second square / logits | logits exact |")
    say("|---|---|---|---|---|")
    ok = True
    for flag in (False, True):
        hewrapper.DIAGONAL_DENSE = flag
        rng = np.random.default_rng(5)
        F = EncryptedSealBfvFactory(**dict(networks.FACTORY_PARAMETERS["LoLaCifar"], client_seed=7))
        env = F.AllocateComputationEnv()
        img = rng.integers(0, 256, size=3 * 32 * 32).astype(float)
        q = lambda a, sc: np.rint(a * sc) / sc
        w = [q(rng.normal(0, 0.05, 83 * 192), 256), q(rng.normal(0, 0.02, 112 * 8300), 512), q(rng.normal(0, 0.05, 10 * 5488), 512)]
        b = [q(rng.normal(0, 0.05, 83), 256), q(rng.normal(0, 0.05, 112), 512), q(rng.normal(0, 0.05, 10), 512)]
        reader = networks.cifar_reader(Factory=F)
        reader.Features = img / 256.0
        d6 = networks.LoLaCifar(F, reader, w, b, timing=False)
        a5 = d6.Source
        d4 = a5.Source
        a3 = d4.Source
        c1 = a3.Source.Source
        d6.PrepareNetwork()
        x3 = a3.GetNext()
        d4.Apply(x3).Dispose()                                       # untimed: plans and plaintexts become resident
        ms, out4 = [], None
        for _ in range(3):
            if out4 is not None:
                out4.Dispose()
            sync(env)
            t0 = time.perf_counter()
            out4 = d4.Apply(x3)
            sync(env)
            ms.append((time.perf_counter() - t0) * 1e3)

        def budgets(m):
            return ", ".join("%.1f" % float(e.ctx.invariant_noise_budget(a.encData.h, a.encData.first, 1)[0]) for a, e in zip(m.GetColumn(0).eVectors, env.Environments))
        a5v = a5.Apply(out4)
        out = d6.Apply(a5v)
        trail = " / ".join(budgets(m) for m in (x3, out4, a5v, out))
        W2i = np.rint(w[2].reshape(10, 5488) * 512).astype(np.int64)
        s2 = ((8 * 256) ** 2 * 512) ** 2
        B2i = [int(round(float(x) * s2 * 512)) for x in b[2]]
        ok4, ok6 = True, True
        for i, e in enumerate(env.Environments):
            p = np.uint64(e.plainmodulusValue)
            a2 = networks.lola_cifar_dense_model(reader, c1, w, b, img, int(p))
            ok4 = ok4 and [int(v) for v in out4.GetColumn(0).eVectors[i]._decrypt_ints(e)] == [int(v) for v in a2]
            a2 = mulmod(a2, a2, p)
            W2p = np.mod(W2i, int(p)).astype(np.uint64)
            lg = np.zeros(10, dtype=np.uint64)
            for c0 in range(0, 5488, 512):
                lg = (lg + (mulmod(W2p[:, c0:c0 + 512], a2[None, c0:c0 + 512], p) % p).sum(axis=1) % p) % p
            lg = (lg + np.array([x % int(p) for x in B2i], dtype=np.uint64)) % p
            ok6 = ok6 and [int(v) for v in out.GetColumn(0).eVectors[i]._decrypt_ints(e)] == [int(v) for v in lg]
        say("| %s | %s | %s | %s | %s |" % (flag, ", ".join("%.1f" % x for x in ms), ok4, trail, ok6))
        ok = ok and ok4
        for e in env.Environments:
            e.ctx.close()
    hewrapper.DIAGONAL_DENSE = False
    say("")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="tiny,cifar,large")
    ap.add_argument("--primes", type=int, default=None, help="plaintext primes of the N = 16384 shapes, default 1 (the tiny shape always takes its two); --device-plan: 1 .. primes, default 2")
    ap.add_argument("--rounds", type=int, default=None, help="timed rounds (default 3; 5 with --ntt-weights)")
    ap.add_argument("--ntt-weights", action="store_true", help="coefficient-form plan against NTT-form plan of the diagonal path, alternating rounds")
    ap.add_argument("--rowdot", action="store_true", help="with --ntt-weights: RowsDotProduct with the flag off and on as well")
    ap.add_argument("--device-plan", action="store_true", help="the plan built on the host route against the device route (hewrapper.DEVICE_DIAGONAL_PLAN), with 1 .. --primes primes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.primes = a.primes or (2 if a.device_plan else 1)
    a.rounds = a.rounds or (5 if a.ntt_weights else 3)
    a.out = a.out or os.path.join(ROOT, "profiles", "diag_device_plan.md" if a.device_plan else ("ntt_weights.md" if a.ntt_weights else "diag_dense.md"))
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)
    ok = True
    if a.device_plan:
        say("# Diagonal plans built on the device: `tools/diag_dense_probe.py --device-plan`")
        say("")
        say("One MI355X, one process; the plan of the diagonal path (`_diagonal_plan`: every plaintext prime, rows resident) built on the host route - the parent's code, unchanged -")
        say("and on the device route (`hewrapper.DEVICE_DIAGONAL_PLAN`), alternating after one untimed build of each, wall clock around the builds and a host wait on every context,")
        say("clocks as found.  Synthetic integer weights (every structural diagonal holds a non-zero).")
        say("")
        for name in a.shapes.split(","):
            for np_ in ([2] if name == "tiny" else range(1, a.primes + 1)):
                ok = probe_device_plan(name, np_, a.rounds, say) and ok
    elif a.ntt_weights:
        say("# NTT-form weight plaintexts: `tools/diag_dense_probe.py --ntt-weights`, %d plaintext prime(s) at N = 16384" % a.primes)
        say("")
        say("One MI355X, one process, one image; the diagonal path with its plan in coefficient form and in NTT form (`hewrapper.NTT_WEIGHTS`), both resident, alternating")
        say("rounds on the same input ciphertext after an untimed round each, wall clock around `DiagonalDense` and a host wait on every context, clocks as found.")
        say("")
        for name in a.shapes.split(","):
            ok = probe_ntt(name, 2 if name == "tiny" else a.primes, a.rounds, a.rowdot, say) and ok
    else:
        say("# Dense layers by generalized diagonals: `tools/diag_dense_probe.py`")
        say("")
        say("One MI355X, one process, one image; both paths on the same input ciphertext, plans and plaintexts resident, wall clock around `Mul(..., ForceDenseFormat=True)` and a")
        say("host wait on every context.  Synthetic integer weights, a fresh input encryption (see the tool's docstring).")
        say("")
        for name in a.shapes.split(","):
            ok = (network(say) if name == "network" else probe(name, 2 if name == "tiny" else a.primes, a.rounds, say)) and ok
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
