"""The scalar GEMM planner of cryptonets_amd/csrc/cn_gemm_plan.h on the CPU: tests/cpp/gemm_plan.cpp plans every case below - over indices as cn_scalar_gemm,
cn_gemm_plan_create and the cached plans of deferred square + dense layers do, over device addresses as a flush of the deferred queue does - and prints the
layout and the whole image.  Here the scalars are recomputed from the rules the header states, and every table is decoded by the layout its kernel documents
(cn_k_gemm.hip.h): each output must give back exactly its gather list and its signed weights, and every entry that belongs to no term is 0 (-1 in the index tables).
A second build of the same program runs under -fsanitize=address,undefined: host code in a stand-alone program."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from size_policy_sets import Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 65537
BIG_T = 4206593                                  # a 23-bit plain modulus: the only way to a weight of 2^20 and more
N = 1024
ON = dict(f64=1, gemm_mfma=1, gemm_pair=1, digit_mfma=1, digit_i32=1)
al = lambda b: (b + 255) & ~255
f64_rows = lambda K: ((K + 15) & ~15) + 16        # gemm_f64_rows
digit_rows = lambda K: ((K + 7) & ~7) + 8         # digit_gemm_rows
CASES = []


def index_case(name, W, idx=None, bias=None, bias_count=0, policy="f64l", dbc=10, t=T, want=None, refused=None, **sw):
    """W [O][K] signed weights; idx [O][K] or None (identity); want: (gather lists, signed weights) per output after pairing, where they differ"""
    W = [list(r) for r in W]
    O, K = len(W), len(W[0]) if W else 0
    CASES.append(dict(kind="index", name=name, W=W, idx=idx, bias=bias, bias_count=bias_count, policy=policy, dbc=dbc, t=t, O=O, K=K, sw=dict(ON, **sw),
                      want=want, refused=refused))


def addr_case(name, A, W, out, bias, rel_on=1, policy="f64l", dbc=10, expect_abs=False, **sw):
    CASES.append(dict(kind="addr", name=name, A=A, W=[list(r) for r in W], out=out, bias=bias, rel_on=rel_on, policy=policy, dbc=dbc, t=T, O=len(W), K=len(W[0]),
                      sw=dict(ON, **sw), expect_abs=expect_abs))


def rows(O, K, seed, lo=-9, hi=9):
    r = np.random.default_rng(seed).integers(lo, hi + 1, size=(O, K))
    r[r == 0] = 1
    return r.tolist()


# ---- the cases
index_case("dense", rows(3, 5, 1))
SHARED = [[0, 1, -1, 2], [3, -1, 4, 5]]
index_case("shared", rows(6, 4, 2), idx=[SHARED[o & 1] for o in range(6)], bias=[5, 4, 3, 2, 1, 0], bias_count=6)
index_case("uneven", rows(4, 4, 3), idx=[SHARED[0], SHARED[1], SHARED[0], SHARED[0]])
for M in (1, 2, 3, 8, 16, 21):
    for K in (1, 15, 16, 17):
        index_case("tile-f64-M%d-K%d" % (M, K), rows(M, K, 10 * M + K), gemm_mfma=0)                       # FP64 tiles 1 / 5 / 10 / 20, digit tiles 2 / 10
        index_case("tile-int-M%d-K%d" % (M, K), rows(M, K, 10 * M + K), policy="u64")                      # integer tiles 1 / 5 / 10
LA, LB = [0, 1, 2, 3, 4, 5], [2, 3, 4, 5, 6, 7]
PW = rows(4, 6, 4)
PAIRED = ([list(range(8))] * 4, [PW[0] + [0, 0], [0, 0] + PW[1], PW[2] + [0, 0], [0, 0] + PW[3]])
index_case("pair", PW, idx=[LA, LB, LA, LB], want=PAIRED)
index_case("pair-off", PW, idx=[LA, LB, LA, LB], gemm_pair=0)
index_case("pair-repeated-input", PW, idx=[[0, 1, 2, 3, 4, 4], LB, [0, 1, 2, 3, 4, 4], LB])
index_case("pair-six-outputs", rows(8, 6, 5), idx=[LA] * 6 + [LB] * 2)
index_case("pair-integer-form", PW, idx=[LA, LB, LA, LB], policy="u64")                                    # only the FP64 kernels pair
for P, top in ((1, 127), (2, 32639), (3, 32768)):
    w = rows(16, 33, 6 + P, -100, 100)
    w[3][7], w[9][32] = top, -top
    index_case("mfma-P%d" % P, w, idx=[[k if k != 5 else -1 for k in range(33)]] * 16)                     # a padded tap inside the first K step
index_case("mfma-P3-wide", [[(1 << 20) - 1 if (o, k) == (2, 2) else 1 for k in range(33)] for o in range(16)], t=BIG_T)
index_case("mfma-M15", rows(15, 33, 9))
index_case("mfma-off", rows(16, 33, 9), gemm_mfma=0)
index_case("mfma-dbc15", rows(16, 33, 9), dbc=15)                                                          # FP64 digit table, no dig_mfma
index_case("mfma-digit-mfma-off", rows(16, 33, 9), digit_mfma=0)
index_case("big-weight", [[1 << 20, 3, -(1 << 20) - 7], [2, -5, 1]], t=BIG_T)                            # integer form, lifted per limb
index_case("f64-off", rows(3, 5, 1), f64=0)
for pol in ("f64l", "f64"):
    room = (1 << 53) // max(Q[pol])
    fill = lambda total: [min(32768, max(0, total - 32768 * i)) for i in range(-(-total // 32768))]
    index_case("one-limb-at-%s" % pol, [fill(room - 1), [1] * len(fill(room - 1))], policy=pol)
    index_case("one-limb-above-%s" % pol, [fill(room), [1] * len(fill(room))], policy=pol)
LIM = min((min(Q["f64l"]) - 1) // 2, (1 << 52) - 1) // 1023
FILL = lambda total: [(-1) ** i * min(32768, total - 32768 * i) for i in range(-(-total // 32768))]
index_case("digit-at-lim", [FILL(LIM)])
index_case("digit-above-lim", [FILL(LIM + 1)])
I32 = (2 ** 31 - 1) // 1023
index_case("digit-i32-at", [FILL(I32), [1] * len(FILL(I32))])
index_case("digit-i32-above", [FILL(I32 + 1), [1] * len(FILL(I32 + 1))])
index_case("digit-i32-off", [FILL(I32)], digit_i32=0)
index_case("digit-dbc60", rows(3, 5, 1), dbc=60)
BASE = 0x7f0000000000
AD = lambda i: BASE + 256 * i if i >= 0 else 0
for bias_name, bias in (("all", lambda o: AD(200 + 3 * o)), ("none", lambda o: 0), ("some", lambda o: AD(200 + o) if o != 1 else 0)):
    addr_case("addr-shared-bias-" + bias_name, [[AD(9 * i) for i in SHARED[o & 1]] for o in range(6)], rows(6, 4, 2), [AD(100 + 5 * o) for o in range(6)],
              [bias(o) for o in range(6)], expect_abs=bias_name == "some")
    addr_case("addr-uneven-bias-" + bias_name, [[AD(9 * i) for i in SHARED[o]] for o in (0, 1, 0, 0)], rows(4, 4, 3), [AD(100 + 5 * o) for o in range(4)],
              [bias(o) for o in range(4)], expect_abs=bias_name == "some", policy="u64")
addr_case("addr-far", [[AD(1), AD(2) + (1 << 39)], [AD(1), AD(2) + (1 << 39)]], rows(2, 2, 7), [AD(50), AD(60)], [0, 0], expect_abs=True)
addr_case("addr-near", [[AD(1), AD(2) + (1 << 38)], [AD(1), AD(2) + (1 << 38)]], rows(2, 2, 7), [AD(50), AD(60)], [0, 0])
addr_case("addr-unaligned", [[AD(1), AD(2) + 128]], rows(1, 2, 7), [AD(50)], [0], expect_abs=True)
addr_case("addr-rel-off", [[AD(1), AD(2)]], rows(1, 2, 7), [AD(50)], [0], rel_on=0, expect_abs=True)
addr_case("addr-mfma", [[AD(k) for k in range(33)]] * 16, rows(16, 33, 9), [AD(100 + o) for o in range(16)], [AD(300)] * 16)
index_case("refuse-weight", [[1, T]], refused="weight >= plain modulus")
index_case("refuse-zero-row", [[1, 2], [0, 5]], idx=[[0, 1], [0, -1]], refused="output 1 has no non-zero term (AddMany of nothing)")
index_case("refuse-bias", [[1, 2]], bias=[2], bias_count=2, refused="bias index out of range")
index_case("refuse-empty", [], refused="empty scalar GEMM")


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "gemm_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "gemm_plan.cpp"), "-o", exe])
    return exe


def run(exe):
    path = os.path.join(tempfile.mkdtemp(), "cases.txt")
    flat = lambda m: " ".join(str(x) for r in m for x in r)
    with open(path, "w") as f:
        for c in CASES:
            q, sw, t = Q[c["policy"]], c["sw"], c["t"]
            f.write("case %s %d %d %d %d %s %d %d %d %d %d\n" % (c["name"], t, N, c["dbc"], len(q), " ".join(map(str, q)), sw["f64"], sw["gemm_mfma"], sw["gemm_pair"],
                                                                   sw["digit_mfma"], sw["digit_i32"]))
            res = [[w % t if w != t else t for w in r] for r in c["W"]]                     # (w = t: the refusal case)
            if c["kind"] == "index":
                f.write("index %d %d %d %d %d\n" % (c["O"], c["K"], c["idx"] is not None, c["bias"] is not None, c["bias_count"]))
                f.write("%s\n%s\n%s\n" % (flat(c["idx"] or []), flat(res), " ".join(map(str, c["bias"] or []))))
            else:
                f.write("addr %d %d %d\n%s\n%s\n%s\n%s\n" % (c["O"], c["K"], c["rel_on"], flat(c["A"]), flat(res), " ".join(map(str, c["out"])), " ".join(map(str, c["bias"]))))
    env = {k: v for k, v in os.environ.items() if k != "CN_GEMM_ONE_LIMB"}
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)


LAYOUT = ("K Kp G M MT lazy small two one mfma P mtiles ksteps dig dig_mfma dig_i32 dMT dKw off_oidx off_bidx off_w off_dw").split()


def parse(text):
    out, cur = {}, None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            cur = out[w[1]] = {}
        elif w[0] == "refused":
            cur["refused"] = (int(w[1]), " ".join(w[2:]))
        elif w[0] == "layout":
            cur["layout"] = dict(zip(LAYOUT, map(int, w[1:])))
            assert len(w) == len(LAYOUT) + 1
        elif w[0] == "plan":
            cur["max_in"], cur["nnz"] = int(w[1]), int(w[2])
        elif w[0] == "form":
            cur["form"] = dict(zip("abs any_bias ibase obase bbase some_input".split(), map(int, w[1:])))
        else:
            assert w[0] == "image" and len(w[2]) == 2 * int(w[1]), line[:80]
            cur["image"] = np.frombuffer(bytes.fromhex(w[2]), dtype=np.uint8)
    return out


@pytest.fixture(scope="module")
def plans():
    r = run(build())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


def expected_scalars(c, lists, W, M, G, K, pad):
    """the layout's scalars by the rules of cn_gemm_plan.h; lists / W: gather lists and signed weights per output as planned (after pairing)"""
    q, sw, t, dbc = Q[c["policy"]], c["sw"], c["t"], c["dbc"]
    bits, qmax = max(q).bit_length(), max(q)
    gathered = [[abs(w) for w, a in zip(W[o], lists[o]) if a > pad] for o in range(len(W))]
    small = all(abs(w) < (1 << 20) for r in c["W"] for w in r) and bool(sw["f64"]) and bits <= 49
    two = qmax >> 44 == 0
    lazy = (1024 if two else 32768) if small else (1 if 2 * bits >= 127 else min(1 << 20, 1 << (127 - 2 * bits)))
    mfma = bool(sw["gemm_mfma"]) and small and bits <= 46 and M >= 16 and 3 * K < (1 << 17) and N % 32 == 0
    e = dict(K=K, G=G, M=M, small=small, two=two, lazy=lazy, mfma=mfma, Kp=(K + 31) // 32 * 32 if mfma else ((K + 15) & ~15) + 16)
    amax = max(abs(w) for r in W for w in r)
    e["P"], e["mtiles"], e["ksteps"] = ((1 if amax <= 127 else 2 if amax <= 32639 else 3), (M + 31) // 32, (K + 31) // 32) if mfma else (0, 0, 0)
    e["MT"] = 0 if mfma else ((20 if M >= 16 else 10 if M >= 8 else 5 if M >= 3 else 1) if small else (10 if M >= 8 else 5 if M >= 3 else 1))
    e["one"] = (not mfma) and small and K <= lazy and all(sum(g) + 1 <= (1 << 53) // qmax for g in gathered)
    dig = c["kind"] == "index" and small and len(q) >= 2 and 1 <= dbc <= 30
    if dig:
        lim = min((min(q) - 1) // 2, (1 << 52) - 1) // ((1 << dbc) - 1)
        dig = all(sum(g) <= lim for g in gathered)
    e["dig"] = dig
    e["dig_mfma"] = dig and mfma and bool(sw["digit_mfma"]) and dbc <= 14 and N % 256 == 0
    e["dig_i32"] = dig and bool(sw["digit_i32"]) and max(sum(g) for g in gathered) * ((1 << dbc) - 1) <= 2 ** 31 - 1
    e["dMT"], e["dKw"] = ((10 if M > 2 else 2), digit_rows(K)) if dig and not e["dig_mfma"] else (0, 0)
    return e


def take(tab, index, want, what):
    assert tab[index] == want, (what, index, tab[index], want)
    tab[index] = 0


def decode_weights(c, L, image, groups, W, tap):
    """reads every (group, member, term) out of the weight tables by their documented index and leaves zeros: nothing else may be set"""
    q, t = Q[c["policy"]], c["t"]
    G, M, K = L["G"], L["M"], L["K"]
    raw = image[L["off_w"]:L["off_dw"]].copy()
    terms = [(g, m, o, kk, W[o][kk] if tap(g, kk) else 0) for g, (_, outs) in enumerate(groups) for m, o in enumerate(outs) for kk in range(K)]

    def f64_table(tab, tile, nrows):
        mt = -(-M // tile)
        assert len(tab) >= G * mt * nrows * tile
        for g, m, o, kk, w in terms:
            take(tab, ((g * mt + m // tile) * nrows + kk) * tile + m % tile, float(w), "f64 tile")
        assert not tab.view(np.uint64).any()                                                 # (+0.0 everywhere else, not -0.0)
    if L["mfma"]:
        tab = raw.view(np.int8)
        mtiles, ksteps, P = L["mtiles"], L["ksteps"], L["P"]
        assert len(tab) == al(G * P * mtiles * ksteps * 1024)
        for g, m, o, kk, w in terms:
            for p in range(P):
                d = ((w + 128) & 255) - 128
                w = (w - d) >> 8
                take(tab, ((((g * P + p) * mtiles + m // 32) * ksteps + kk // 32) * 1024) + ((kk % 32) // 16 * 32 + m % 32) * 16 + kk % 16, d, "fragment")
            assert w == 0
        assert not tab.any()
    elif L["small"]:
        f64_table(raw.view(np.float64), L["MT"], f64_rows(K))
    else:
        tab, MT = raw.view(np.uint64), L["MT"]
        mt = -(-M // MT)
        assert len(tab) == al(8 * len(q) * G * mt * K * MT) // 8
        for j, qj in enumerate(q):
            for g, m, o, kk, w in terms:
                take(tab, (((j * G + g) * mt + m // MT) * K + kk) * MT + m % MT, (w + qj if w < 0 else w), "lifted weight")
        assert not tab.any()
    if L["dig"] and not L["dig_mfma"]:
        assert len(image) - L["off_dw"] == al(8 * G * -(-M // L["dMT"]) * L["dKw"] * L["dMT"])
        f64_table(image[L["off_dw"]:].copy().view(np.float64), L["dMT"], L["dKw"])
    else:
        assert len(image) == L["off_dw"]


def check_tables(c, p, lists, W, outs_of, bias_of, entry, pad):
    """groups in the order of the gather lists; entry: dtype of the index / address tables; pad: their 'padded tap / no output' value"""
    L, image = p["layout"], p["image"]
    groups = sorted(((key, [o for o in range(len(W)) if tuple(lists[o]) == key]) for key in set(map(tuple, lists))), key=lambda kv: kv[0])
    G, M, K = len(groups), max(len(outs) for _, outs in groups), len(lists[0])
    want = expected_scalars(c, lists, W, M, G, K, pad)
    assert {k: L[k] for k in want} == {k: int(v) for k, v in want.items()}, c["name"]
    Kp, size = L["Kp"], np.dtype(entry).itemsize
    assert (L["off_oidx"], L["off_bidx"], L["off_w"]) == (al(G * Kp * size), al(G * Kp * size) + al(G * M * size), al(G * Kp * size) + 2 * al(G * M * size))
    gather = image[:L["off_oidx"]].view(entry).copy()
    members = image[L["off_oidx"]:L["off_bidx"]].view(entry).copy()
    biases = image[L["off_bidx"]:L["off_w"]].view(entry).copy()
    for g, (key, outs) in enumerate(groups):
        assert gather[g * Kp:(g + 1) * Kp].tolist() == list(key) + [pad] * (Kp - K), (c["name"], g)
        assert members[g * M:(g + 1) * M].tolist() == [outs_of(o) for o in outs] + [pad] * (M - len(outs)), (c["name"], g)
        assert biases[g * M:(g + 1) * M].tolist() == [bias_of(o) for o in outs] + [0] * (M - len(outs)), (c["name"], g)
    assert not gather[G * Kp:].any() and not members[G * M:].any() and not biases[G * M:].any()       # the 256-byte padding
    decode_weights(c, L, image, groups, W, lambda g, kk: groups[g][0][kk] > pad)
    return groups


def test_index_plans(plans):
    assert sorted(plans) == sorted(c["name"] for c in CASES)
    for c in CASES:
        if c["kind"] != "index":
            continue
        p = plans[c["name"]]
        if c["refused"]:
            assert p == {"refused": (-1, c["refused"])}, c["name"]
            continue
        lists, W = c["want"] or (c["idx"] or [list(range(c["K"]))] * c["O"], c["W"])
        bias = c["bias"]
        check_tables(c, p, lists, W, lambda o: o, lambda o: bias[o] if bias else 0, np.int32, -1)
        given = c["idx"] or [list(range(c["K"]))] * c["O"]
        assert p["max_in"] == 1 + max(a for r in given for a in r)
        assert p["nnz"] == sum(1 for r, ws in zip(given, c["W"]) for a, w in zip(r, ws) if a >= 0 and w)


def test_address_plans(plans):
    for c in CASES:
        if c["kind"] != "addr":
            continue
        p = plans[c["name"]]
        form, A = p["form"], c["A"]
        assert form["abs"] == c["expect_abs"] and form["any_bias"] == any(c["bias"]), c["name"]
        if form["abs"]:
            groups = check_tables(c, p, A, c["W"], lambda o: c["out"][o], lambda o: c["bias"][o], np.uint64, 0)
            assert form["some_input"] == next(a for a in groups[0][0] if a)
            continue
        ibase, obase = min(a for r in A for a in r if a), min(c["out"])
        bbase = min([b for b in c["bias"] if b], default=2 ** 64 - 1)
        assert (form["ibase"], form["obase"], form["bbase"]) == (ibase, obase, bbase), c["name"]
        rel = [[(a - ibase) >> 8 if a else -1 for a in r] for r in A]
        # (address -> offset is monotonic, 0 -> -1 included: the rows sort as the address rows do, which is the order the groups keep)
        check_tables(c, p, rel, c["W"], lambda o: (c["out"][o] - obase) >> 8, lambda o: (c["bias"][o] - bbase) >> 8 if c["bias"][o] else 0, np.int32, -1)


def test_anchors(plans):
    """a few plans spelled out"""
    L = lambda name: plans[name]["layout"]
    assert [L("tile-f64-M%d-K16" % M)["MT"] for M in (1, 2, 3, 8, 16, 21)] == [1, 1, 5, 10, 20, 20]
    assert [L("tile-int-M%d-K16" % M)["MT"] for M in (1, 2, 3, 8, 16, 21)] == [1, 1, 5, 10, 10, 10]
    assert [L("tile-f64-M%d-K16" % M)["dMT"] for M in (1, 2, 3, 8, 16, 21)] == [2, 2, 10, 10, 10, 10]
    assert [(L("tile-f64-M3-K%d" % K)["Kp"], L("tile-f64-M3-K%d" % K)["dKw"]) for K in (1, 15, 16, 17)] == [(32, 16), (32, 24), (32, 24), (48, 32)]
    assert all(not L("tile-int-M%d-K%d" % (M, K))["small"] and not L("tile-int-M%d-K%d" % (M, K))["dig"] for M in (1, 21) for K in (1, 17))
    assert (L("pair")["G"], L("pair")["K"], L("pair")["M"]) == (1, 8, 4) and (L("pair-off")["G"], L("pair-off")["K"]) == (2, 6)
    assert all(L(n)["G"] == 2 and L(n)["K"] == 6 for n in ("pair-repeated-input", "pair-six-outputs", "pair-integer-form"))
    assert [L("mfma-P%d" % P)["P"] for P in (1, 2, 3)] == [1, 2, 3] and L("mfma-P3-wide")["P"] == 3
    assert all(L("mfma-P%d" % P)["mfma"] and L("mfma-P%d" % P)["ksteps"] == 2 and L("mfma-P%d" % P)["Kp"] == 64 and L("mfma-P%d" % P)["dig_mfma"] for P in (1, 2, 3))
    assert not L("mfma-M15")["mfma"] and L("mfma-M15")["MT"] == 10 and not L("mfma-off")["mfma"] and L("mfma-off")["MT"] == 20
    assert L("mfma-dbc15")["mfma"] and L("mfma-dbc15")["dig"] and not L("mfma-dbc15")["dig_mfma"] and L("mfma-dbc15")["dMT"] == 10
    assert L("mfma-digit-mfma-off")["dig"] and not L("mfma-digit-mfma-off")["dig_mfma"]
    assert not L("big-weight")["small"] and L("big-weight")["MT"] == 1 and not L("f64-off")["small"]
    for pol in ("f64l", "f64"):
        assert L("one-limb-at-" + pol)["one"] and not L("one-limb-above-" + pol)["one"] and L("one-limb-above-" + pol)["small"]
    assert L("digit-at-lim")["dig"] and not L("digit-above-lim")["dig"] and not L("digit-at-lim")["dig_i32"]
    assert L("digit-i32-at")["dig_i32"] and L("digit-i32-above")["dig"] and not L("digit-i32-above")["dig_i32"] and not L("digit-i32-off")["dig_i32"]
    assert not L("digit-dbc60")["dig"] and L("dense")["dig"] and (L("dense")["G"], L("dense")["M"]) == (1, 3)
    assert (L("uneven")["G"], L("uneven")["M"]) == (2, 3) and (L("shared")["G"], L("shared")["M"]) == (2, 3)
    assert L("addr-mfma")["mfma"] and not plans["addr-mfma"]["form"]["abs"] and not L("addr-mfma")["dig"]


def test_gemm_plan_header_is_clean_under_the_sanitizers(plans):
    """-fsanitize=address,undefined with errors fatal over the same cases: the same plans, no report"""
    r = run(build(("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    again = parse(r.stdout.decode())
    assert sorted(again) == sorted(plans)
    for name, p in plans.items():
        assert {k: v for k, v in p.items() if k != "image"} == {k: v for k, v in again[name].items() if k != "image"}, name
        assert ("image" in p) == ("image" in again[name]) and ("image" not in p or np.array_equal(p["image"], again[name]["image"])), name
