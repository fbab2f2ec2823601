"""The clipped + residual weight form of the matrix-core GEMM plans (gemm_residual_form, cryptonets_amd/csrc/cn_gemm_plan.h) on the CPU:
tests/cpp/gemm_residual_plan.cpp plans every case below and prints the layout and the whole image; here every table is decoded by the layout the kernels document
(cn_k_gemm.hip.h).  For a plan in the form: every weight is c + r with c = clamp(w, -127, 127) in plane 0 and r in plane 1; the K slots of a gather row are a
permutation of the caller's list, applied alike to the index row and to both fragment planes, with every input that has a residual in front and the order otherwise
kept; the table kres behind the fragments covers every r != 0 and passes the gate's share of the K steps; the i32 bounds of the gate hold; nothing else is set.  A
plan outside the gate (max |w| <= 127 or > 254, too many steps with a residual, CN_GEMM_RESIDUAL=0) is packed in base-256 planes with its rows as given.
Every case is planned three times: by default (GEMM_RES_SHARE kres <= K steps, share 8: where the kernels' kres extra steps still pay), under CN_GEMM_RESIDUAL=2
(2 kres <= K steps: the form wherever it is correct and not plainly more work - the setting the device test runs layers of two to four K steps under) and under
CN_GEMM_RESIDUAL=0.  check() derives what the planner must decide from the weights and the mode; the cases' own `res` says it again for mode 2.
The i32 head-room (128 R, and 192 R for the digit GEMM) cannot fail for a plan that reaches it: 3 K < 2^17 and |w| <= 254 give R <= 43690 * 254 = 11 097 260,
192 R < 2^31.  It is asserted on every plan in the form; no case can be built beyond it.
A second build of the program runs under -fsanitize=address,undefined: host code in a stand-alone program."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import PARAMS
from size_policy_sets import Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 65537
N = 1024
CASES = []


def case(name, W, idx=None, kind="index", t=T, n=N, q=None, dbc=10, res=None, P=None):
    """W [O][K] signed weights; idx [O][K] (None: the identity); res / P: what the planner must decide under CN_GEMM_RESIDUAL=2"""
    W = [list(map(int, r)) for r in W]
    CASES.append(dict(name=name, kind=kind, W=W, idx=idx, t=t, n=n, q=list(q or Q["f64l"]), dbc=dbc, O=len(W), K=len(W[0]), res=res, P=P))


def rows(O, K, seed, big=(), lo=-20, hi=20):
    """weights mostly |w| <= 20; big: (o, k, w) planted"""
    r = np.random.default_rng(seed).integers(lo, hi + 1, size=(O, K))
    r[r == 0] = 1
    for o, k, w in big:
        r[o, k] = w
    return r.tolist()


def handful(O, K, seed, count):
    """`count` weights in 128..254 of both signs at random places"""
    rng = np.random.default_rng(1000 + seed)
    return [(int(rng.integers(O)), int(rng.integers(K)), int(rng.integers(128, 255)) * (1 if i & 1 else -1)) for i in range(count)]


def device_weights(M, K):
    """the weights tests/test_gpu_gemm_residual.py runs on the device, planned here as well: mostly |w| <= 20, a handful in 128..254 of both signs at random places,
    one in the last K slot, and row 2 with a residual in EVERY input that has one - at K = 100 forty inputs (kres = 2 of 4 steps), otherwise the handful's
    (kres = 1 of 2 / 3).  (A row with a residual in all K inputs cannot be in the form: kres would be every step, and even CN_GEMM_RESIDUAL=2 stops at half.)
    Planned here with the device test's own ring parameters: the plan the device builds."""
    big = handful(M, K, M + K, 5) + [(1, K - 1, 200)] + ([(5 + k % 7, 2 * k, 130 + k) for k in range(40)] if K == 100 else [])
    cols = sorted({k for _, k, _ in big})
    return rows(M, K, M + K, big + [(2, k, -254 + i) for i, k in enumerate(cols)])


DEVICE_SHAPES = [(M, K) for M in (16, 33, 40) for K in (33, 70, 100)]
TINY = dict(t=PARAMS["tiny"]["t"], n=PARAMS["tiny"]["n"], q=PARAMS["tiny"]["q"], dbc=PARAMS["tiny"]["dbc"])
for M, K in DEVICE_SHAPES:
    case("device-M%d-K%d" % (M, K), device_weights(M, K), res=True, P=1, **TINY)
# two gather lists over the device test's 100 inputs: the one with a padded tap has every residual (kres = 1), the other none (kres = 0)
DA = [k if k != 5 else -1 for k in range(70)]
DB = [30 + k for k in range(70)]
DEVICE_LISTS = [DA if o % 2 == 0 else DB for o in range(40)]
DEVICE_LISTS_W = rows(40, 70, 8, [(0, 69, 254), (2, 3, -128), (4, 5, 250), (6, 40, 131)])
case("device-two-lists", DEVICE_LISTS_W, idx=DEVICE_LISTS, res=True, P=1, **TINY)
# the default gate's edge: 8 K steps, 32 inputs with a residual (kres = 1) and 33 (kres = 2)
case("share-at", rows(16, 256, 11, [(k % 16, 3 * k, 140 + k) for k in range(32)]), res=True, P=1)
case("share-above", rows(16, 256, 11, [(k % 16, 3 * k, 140 + k) for k in range(33)]), res=True, P=1)
for top in (127, 128, 254, 255):
    case("edge-%d" % top, rows(16, 70, top, [(3, 7, top), (9, 69, -top)]), res=127 < top <= 254, P=1 if top <= 254 else 2)
case("one-step", rows(16, 32, 5, [(0, 0, 130)]), res=False, P=2)                                  # one K step: kres = 1 is more than half
case("half", rows(16, 128, 6, [(o % 16, k, 150) for o, k in enumerate(range(0, 128, 2))]), res=True, P=1)      # 64 inputs: kres = 2 of 4 steps
case("more-than-half", rows(16, 128, 6, [(o % 16, k, 150) for o, k in enumerate(list(range(0, 128, 2)) + [1])]), res=False, P=2)      # 65 inputs: kres = 3 of 4
case("all-residual-row", rows(33, 70, 7, [(32, k, -129 - k) for k in range(32)]), res=True, P=1)
LA = [k if k != 5 else -1 for k in range(70)]                                                      # a padded tap inside the first K step
LB = [100 + k for k in range(70)]
case("two-lists", rows(40, 70, 8, [(0, 69, 254), (2, 3, -128), (4, 5, 250), (6, 40, 131)]), idx=[LA if o % 2 == 0 else LB for o in range(40)], res=True, P=1)
case("padded-tap-only", rows(16, 70, 9, [(4, 5, 250)]), idx=[LA] * 16, res=True, P=1)             # the weight of a padded tap counts for max |w| (as for P) and for nothing else
# dbc = 15: no matrix-core digit GEMM - the plan's FP64 digit table must follow the permuted gather rows
case("digit-f64-table", rows(33, 70, 12, [(3, 69, 254), (32, 7, -200), (0, 40, 129)]), dbc=15, res=True, P=1)
BASE = 0x7f0000000000
case("addresses", rows(16, 70, 10, [(3, 69, 254), (5, 0, -200)]), idx=[[BASE + 256 * (3 * k + 1) for k in range(70)]] * 16, kind="addr", res=True, P=1)


def trained():
    from cryptonets_amd import cryptonets_mnist as cm
    L = cm.layer_tables(*cm.reference_weights())[1]
    return [list(map(int, r)) for r in L["W"]], [list(map(int, r)) for r in L["idx"]], cm.PLAIN_PRIMES[0]


TW, TIDX, TT = trained()
case("trained-845-100", TW, idx=TIDX, t=TT, n=8192, res=True, P=1)


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "gemm_residual_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "gemm_residual_plan.cpp"), "-o", exe])
    return exe


def run(exe, switch=None):
    path = os.path.join(tempfile.mkdtemp(), "cases.txt")
    flat = lambda m: " ".join(str(x) for r in m for x in r)
    with open(path, "w") as f:
        for c in CASES:
            t, q = c["t"], c["q"]
            f.write("case %s %d %d %d %d %s 1 1 1 1 1\n" % (c["name"], t, c["n"], c["dbc"], len(q), " ".join(map(str, q))))
            res = [[w % t for w in r] for r in c["W"]]
            if c["kind"] == "index":
                f.write("index %d %d %d\n%s\n%s\n" % (c["O"], c["K"], c["idx"] is not None, flat(c["idx"] or []), flat(res)))
            else:
                f.write("addr %d %d\n%s\n%s\n%s\n" % (c["O"], c["K"], flat(c["idx"]), flat(res), " ".join(str(BASE + 256 * (1000 + o)) for o in range(c["O"]))))
    env = {k: v for k, v in os.environ.items() if k != "CN_GEMM_RESIDUAL"}
    if switch is not None:
        env["CN_GEMM_RESIDUAL"] = switch
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)


LAYOUT = "K Kp G M mfma P res mtiles ksteps dig dig_mfma off_oidx off_bidx off_w off_dw sum_abs_w entry".split()


def parse(text):
    out, cur = {}, None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            cur = out[w[1]] = {}
        elif w[0] == "layout":
            assert len(w) == len(LAYOUT) + 1
            cur["layout"] = dict(zip(LAYOUT, map(int, w[1:])))
        else:
            assert w[0] == "image" and len(w[2]) == 2 * int(w[1]), line[:80]
            cur["image"] = np.frombuffer(bytes.fromhex(w[2]), dtype=np.uint8)
    return out


@pytest.fixture(scope="module")
def exe():
    return build()


@pytest.fixture(scope="module")
def plans(exe):
    """under CN_GEMM_RESIDUAL=2"""
    r = run(exe, "2")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


@pytest.fixture(scope="module")
def default_plans(exe):
    r = run(exe)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


SHARE = {0: None, 1: 8, 2: 2}                                      # CN_GEMM_RESIDUAL -> the gate is SHARE kres[g] <= K steps (GEMM_RES_SHARE; 0: never)


def check(c, p, mode):
    """decodes the whole plan of case c made under CN_GEMM_RESIDUAL = mode; returns (in the form?, the kres of every group)"""
    L, image = p["layout"], p["image"]
    W, K, O = c["W"], c["K"], c["O"]
    pad = -1 if L["entry"] == 4 else 0
    entry = np.int32 if L["entry"] == 4 else np.uint64
    lists = c["idx"] or [list(range(K))] * O
    groups = sorted(((key, [o for o in range(O) if tuple(lists[o]) == key]) for key in set(map(tuple, lists))), key=lambda kv: kv[0])
    G, M = len(groups), max(len(outs) for _, outs in groups)
    ksteps, mtiles, Kp = (K + 31) // 32, (M + 31) // 32, (K + 31) // 32 * 32
    amax = max(abs(w) for r in W for w in r)
    assert L["mfma"] and (L["G"], L["M"], L["K"], L["Kp"], L["mtiles"], L["ksteps"]) == (G, M, K, Kp, mtiles, ksteps), c["name"]
    need = [(sum(any(key[kk] > pad and abs(W[o][kk]) > 127 for o in outs) for kk in range(K)) + 31) // 32 for key, outs in groups]
    expect_res = bool(SHARE[mode]) and 127 < amax <= 254 and all(SHARE[mode] * kr <= ksteps for kr in need)
    assert L["res"] == int(expect_res) and L["P"] == (1 if expect_res or amax <= 127 else 2), (c["name"], L)
    gather = image[:L["off_oidx"]].view(entry).copy()
    members = image[L["off_oidx"]:L["off_bidx"]].view(entry).copy()
    planes = 2 if L["res"] else L["P"]
    frags = G * planes * mtiles * ksteps * 1024
    raw = image[L["off_w"]:L["off_dw"]].copy()
    tab = raw[:frags].view(np.int8)
    kres = raw[frags:frags + 4 * G].view(np.uint32).tolist() if L["res"] else [0] * G
    assert len(raw) == (frags + (4 * G if L["res"] else 0) + 255) // 256 * 256 and not raw[frags + (4 * G if L["res"] else 0):].any()
    at = lambda g, pl, m, s: ((((g * planes + pl) * mtiles + m // 32) * ksteps + s // 32) * 1024) + ((s % 32) // 16 * 32 + m % 32) * 16 + s % 16
    R = 0
    dtab = image[L["off_dw"]:].copy().view(np.float64)                                     # the FP64 digit table [g][tile of 10][slot < rows][m]: only without dig_mfma
    dtile, drows = (10 if M > 2 else 2), ((K + 7) & ~7) + 8
    assert len(dtab) == (G * -(-M // dtile) * drows * dtile if L["dig"] and not L["dig_mfma"] else 0)
    for g, (key, outs) in enumerate(groups):
        row = gather[g * Kp:(g + 1) * Kp].tolist()
        assert row[K:] == [pad] * (Kp - K), (c["name"], g)
        assert members[g * M:(g + 1) * M].tolist() == [o if pad else BASE + 256 * (1000 + o) for o in outs] + [pad] * (M - len(outs))
        taps = [a for a in key if a > pad]
        assert len(set(taps)) == len(taps)                                                  # (the cases gather every input once: a slot names its term)
        if not L["res"]:
            assert row[:K] == list(key), (c["name"], g)                                     # the rows as given
            src = list(range(K))
        else:
            assert sorted(row[:K]) == sorted(key), (c["name"], g)                           # a permutation of the caller's list ...
            where = {a: kk for kk, a in enumerate(key) if a > pad}
            pads = [kk for kk, a in enumerate(key) if a <= pad]
            src = [where[a] if a > pad else pads.pop(0) for a in row[:K]]
            assert sorted(src) == list(range(K))                                            # ... a bijection of the K slots
            big = [any(key[kk] > pad and abs(W[o][kk]) > 127 for o in outs) for kk in range(K)]
            want = [kk for kk in range(K) if big[kk]] + [kk for kk in range(K) if not big[kk]]
            assert [kk for kk in src if key[kk] > pad] == [kk for kk in want if key[kk] > pad], (c["name"], g)      # residual inputs first, the order kept
            assert kres[g] == (sum(big) + 31) // 32 == need[g] and SHARE[mode] * kres[g] <= ksteps, (c["name"], g, kres[g])
        for m, o in enumerate(outs):
            ws = [W[o][src[s]] if key[src[s]] > pad else 0 for s in range(K)]               # the fragments follow the same permutation
            R = max(R, sum(abs(w) for w in ws))
            for s, w in enumerate(ws if len(dtab) else ()):                                 # the digit table follows the permuted rows too (GemmGroups::term)
                i = ((g * -(-M // dtile) + m // dtile) * drows + s) * dtile + m % dtile
                assert dtab[i] == float(w), (c["name"], g, m, s)
                dtab[i] = 0.0
            for s, w in enumerate(ws):
                if L["res"]:
                    cc, rr = int(tab[at(g, 0, m, s)]), int(tab[at(g, 1, m, s)])
                    assert cc + rr == w and cc == max(-127, min(127, w)) and abs(rr) <= 127, (c["name"], g, m, s, w, cc, rr)
                    assert not rr or s < 32 * kres[g], (c["name"], g, m, s)                 # kres covers every r != 0
                    tab[at(g, 0, m, s)] = tab[at(g, 1, m, s)] = 0
                else:
                    for pl in range(planes):
                        d = ((w + 128) & 255) - 128
                        w = (w - d) >> 8
                        assert tab[at(g, pl, m, s)] == d
                        tab[at(g, pl, m, s)] = 0
                    assert w == 0
    assert not dtab.view(np.uint64).any()
    assert not tab.any()                                                                    # padded rows / terms / taps: zero in every plane
    if L["res"]:
        assert 128 * R < 2 ** 31 and (not L["dig_mfma"] or (128 + 64) * R < 2 ** 31)      # the gate's i32 head-room
    if L["dig"]:
        assert L["sum_abs_w"] == R
    return bool(L["res"]), kres


def test_residual_plans_up_to_half_the_steps(plans):
    assert sorted(plans) == sorted(c["name"] for c in CASES)
    for c in CASES:
        assert check(c, plans[c["name"]], 2)[0] == c["res"], c["name"]


def test_residual_plans_under_the_default_gate(default_plans):
    """a residual step costs a whole one-plane step, so by default the form stops at one step in eight"""
    got = {c["name"]: check(c, default_plans[c["name"]], 1) for c in CASES}
    assert got["trained-845-100"] == (True, [1]) and got["share-at"] == (True, [1]) and got["padded-tap-only"] == (True, [0])
    assert not got["share-above"][0] and not got["half"][0] and not got["edge-128"][0] and not any(got["device-M%d-K%d" % s][0] for s in DEVICE_SHAPES)
    assert default_plans["share-above"]["layout"]["P"] == 2


def test_anchors(plans):
    """a few plans spelled out"""
    L = lambda name: plans[name]["layout"]
    by = {c["name"]: c for c in CASES}
    assert [(L("edge-%d" % w)["res"], L("edge-%d" % w)["P"]) for w in (127, 128, 254, 255)] == [(0, 1), (1, 1), (1, 1), (0, 2)]
    kres = lambda name: check(by[name], plans[name], 2)[1]
    assert [(kres("device-M%d-K%d" % s), L("device-M%d-K%d" % s)["ksteps"]) for s in DEVICE_SHAPES] == [([1], 2), ([1], 3), ([2], 4)] * 3
    assert (L("half")["res"], kres("half"), L("half")["ksteps"]) == (1, [2], 4) and (L("more-than-half")["res"], L("more-than-half")["P"]) == (0, 2)
    assert (L("one-step")["res"], L("one-step")["P"]) == (0, 2) and (L("padded-tap-only")["res"], kres("padded-tap-only")) == (1, [0])
    assert kres("two-lists") == [1, 0] and kres("device-two-lists") == [1, 0]             # the list with the padded tap has every residual; the other none
    assert kres("all-residual-row") == [1] and kres("share-at") == [1] and kres("share-above") == [2]
    assert all(L(n)["dig_mfma"] for n in plans if n not in ("addresses", "digit-f64-table"))
    assert L("digit-f64-table")["res"] and L("digit-f64-table")["dig"] and not L("digit-f64-table")["dig_mfma"]
    # the trained dense layer: 48 weights beyond 127 in 31 of 845 inputs, max |w| = 165 - one K step of 27
    W = np.array(by["trained-845-100"]["W"])
    assert np.abs(W).max() == 165 and (np.abs(W) > 127).sum() == 48 and (np.abs(W) > 127).any(axis=0).sum() == 31
    assert (L("trained-845-100")["res"], kres("trained-845-100"), L("trained-845-100")["ksteps"], L("trained-845-100")["P"]) == (1, [1], 27, 1)


def test_switched_off(exe):
    """CN_GEMM_RESIDUAL=0: every plan in base-256 planes, its rows as given"""
    r = run(exe, "0")
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    off = parse(r.stdout.decode())
    for c in CASES:
        assert check(c, off[c["name"]], 0) == (False, [0] * off[c["name"]]["layout"]["G"])


def test_residual_planner_is_clean_under_the_sanitizers(plans):
    """-fsanitize=address,undefined with errors fatal over the same cases: the same plans, no report"""
    r = run(build(("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")), "2")
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    again = parse(r.stdout.decode())
    assert sorted(again) == sorted(plans)
    for name, p in plans.items():
        assert p["layout"] == again[name]["layout"] and np.array_equal(p["image"], again[name]["image"]), name
