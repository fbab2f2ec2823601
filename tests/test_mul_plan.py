"""The multiply planner of cryptonets_amd/csrc/cn_mul_plan.h on the CPU: tests/cpp/mul_plan.cpp builds the tables of every parameter set of the suite (cn_tables.cpp,
plain g++) and prints, over a grid of switches, counts and scratch limits, the plan of a product chain, the batches of the six chunking sites, the groups of
cn_mul_relin_sum, the three gates, the parts of a pipelined batch and the scratch of the deferred square + dense form.  Every line is recomputed here from the moduli with
Python integers, from the rules as the code BEFORE the planner spelt them: do_multiply with square_fused_ok / run_intt_tensor / cn_behz_lazy and its salloc sequence,
l_square_fused's kernel pick, mul_scratch_per_ct and chunk_for with the per-site expressions of cn_multiply, mul_relin_body, park_squarings, flush_mulrelin_group,
cn_square_gemm and cn_mul_relin_sum, sg_scratch, square_gemm_ctx_ok, mul_sum_fused_ok, halves_pipeline_ok and pipeline_cuts - an independent second statement, like
test_ks_plan.  A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program.

Two anchors differ from what the issue that asked for this test supposed; both are what the code before the planner does, and the planner may not move them:
 * "tiny" with "f64" off runs k_intt_tensor under the integer policy (not lazy, integer floor), as every integer-policy set does; the element-wise k_tensor is
   "legacy_ntt" (no register-radix kernels) alone.  tests/test_gpu_mul_chunks.py pins 9 launches per chain for the integer-policy set: k_tensor would make 11.
 * c3 under a 40 MiB limit squares 9 ciphertexts per chunk of cn_mul_relin and multiplies 8 per chunk of cn_multiply; the "chunks of 3" in the docstring of
   test_small_scratch_and_no_pool date from an earlier scratch layout.
"""
import itertools
import os
import subprocess
import tempfile

import pytest

from test_ks_plan import planned_mode
from test_policy_table import ALL_SETS, CSRC, ROOT

COUNTS = (1, 3, 4, 127, 128, 255, 256, 511, 512, 513, 700, 845)
SITES = ("multiply", "mul_relin", "park", "deferred", "square_gemm", "sum_group")
SQ_HALVES_MIN, MUL_SUM_MIN_K, MAX_DIGITS = 512, 2, 8
# a limb of more than MAX_DIGITS digits: tiny's 36- and 37-bit moduli at 4 bits per digit
EXTRA = {"tiny-dbc4": dict(ALL_SETS["tiny"], dbc=4)}
SETS = dict(ALL_SETS, **EXTRA)


def al(b):
    return (b + 255) & ~255


def digits(q, w):
    return [(m.bit_length() + w - 1) // w for m in q]


def term_counts(p):
    """K on both sides of every bound of the product sum that a 32-bit K can reach, beside the small ones"""
    if not p["q"]:
        return [1, 2, 9]
    d = (1 << p["dbc"]) - 1
    ks = {1, 2, 3, 9, 845}
    for bound in (1 << 52, min(p["q"]) // 2):                       # K d < bound
        ks |= {-(-bound // d) - 1, -(-bound // d)}
    ks |= {((1 << 64) - 1) // (max(p["q"]) - 1), ((1 << 64) - 1) // (max(p["q"]) - 1) + 1}      # K (q_max - 1) < 2^64
    ks |= {((1 << 31) - 1) // d, ((1 << 31) - 1) // d + 1}          # K d <= 2^31 - 1: the last K of int32 digit sums and the first of doubles
    return sorted(k for k in ks if 1 <= k < 1 << 32)


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "mul_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "mul_plan.cpp"),
                           os.path.join(CSRC, "cn_tables.cpp"), "-o", exe])
    return exe


def run(exe):
    path = os.path.join(tempfile.mkdtemp(), "sets.txt")
    with open(path, "w") as f:
        for name, p in SETS.items():
            q, ks = p["q"] or [], term_counts(p)
            f.write("%s %d %d %d %d %d %s %d %s\n" % (name, p["n"], p["t"], p["dbc"], p["gdbc"], len(q), " ".join("%x" % x for x in q), len(ks), " ".join(map(str, ks))))
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)


def parse(text):
    """({set: {"hdr": header, line type: {key: value}}}, {c: cuts}, constants)"""
    out, cuts, consts, cur = {}, {}, None, None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "set":
            hdr = dict(zip(("n", "logn", "k", "kb", "rl_tot", "dbc", "behz_f64", "f64ok_q", "f64ok_bsk", "max_dig"), map(int, w[2:12])))
            bar = w.index("|")
            hdr["q"], hdr["bsk"] = [int(x, 16) for x in w[12:bar]], [int(x, 16) for x in w[bar + 1:]]
            cur = out[w[1]] = {"hdr": hdr, "p": {}, "b": {}, "u": {}, "c": {}, "k": {}, "h": {}, "g": {}}
        elif w[0] == "x":
            cuts[int(w[1])] = tuple(map(int, w[4:]))
        elif w[0] == "const":
            consts = tuple(map(int, w[1:]))
        else:
            colon = w.index(":")
            key, val = tuple(map(int, w[1:colon])), tuple(int(x) if x.lstrip("-").isdigit() else x for x in w[colon + 1:])
            assert key not in cur[w[0]], line
            cur[w[0]][key] = val
    return out, cuts, consts


# ---- the rules, restated from the code before the planner
def policy(mods, f64):
    return "U64" if not (f64 and all(m < 1 << 49 for m in mods)) else ("F64L" if max(mods) < 1 << 44 else "F64")


def expected_plan(S, square, cnt, f64, fused, pipe, lds, rr, cus):
    k, kb, n, q, bsk = S["k"], S["kb"], S["n"], S["q"], S["bsk"]
    behz = bool(S["behz_f64"] and f64)                               # launch_extend, launch_floor and cn_behz_lazy
    sq_ok = lambda mods: bool(fused and f64 and rr and all(m < 1 << 49 for m in mods))      # square_fused_ok
    lazy = behz
    if square and S["behz_f64"] and sq_ok(q) and sq_ok(bsk):       # do_multiply
        form = "SQUARE_FUSED"
    elif all(rr and not (lazy and policy(m, f64) == "U64") for m in (q, bsk)):      # run_intt_tensor of both bases (BY_SIZE has every register-radix size)
        form = "INTT_TENSOR"
    else:
        form, lazy = "ELEMENTWISE", False

    def kernel(Lm):                                                  # l_square_fused
        if form == "SQUARE_FUSED" and S["logn"] <= 13:
            per_limb = min(max(1, cus) // Lm, cnt)
            if per_limb >= 1 and (pipe == 2 or (pipe and cnt >= 4 * per_limb)):
                return ("PIPE", per_limb)
            if lds:
                return ("LDS", 0)
        return ("PLAIN", 0)
    arrays = ([] if form == "SQUARE_FUSED" else [("aq", cnt * 2 * k * n * 8)]) + [("ab", cnt * 2 * kb * n * 8)]      # the salloc sequence
    if not square:
        arrays += [("bq", cnt * 2 * k * n * 8), ("bb", cnt * 2 * kb * n * 8)]
    arrays += [("dq", cnt * 3 * k * n * 8), ("db", cnt * 3 * kb * n * 8)]
    return (form, int(lazy), int(behz), policy(q, f64)) + kernel(k) + (policy(bsk, f64),) + kernel(kb) + tuple("%s:%d" % a for a in arrays)


def per_ct(S, square):
    """mul_scratch_per_ct"""
    kk = S["k"] + S["kb"]
    return al(((1 if square else 2) * 2 * kk * S["n"] + 3 * kk * S["n"]) * 8) + 1024


def chunk_for(smax, per, count):
    return min(max(1, smax // per), count)


def expected_batch(S, site, square, count, smax, outputs, s32):
    """(per, fixed, chunk, fits, bytes ensured for a full chunk, for a chunk of one)"""
    kn, n, tot, sw = S["k"] * S["n"], S["n"], S["rl_tot"], 4 if s32 else 8
    per = per_ct(S, square)
    if site == "multiply":                                           # cn_multiply
        ensure = lambda c: per * c + 4096
    elif site == "mul_relin":                                        # mul_relin_body
        per += al(3 * kn * 8)
        ensure = lambda c: per * c + 8192
    elif site == "park":                                             # park_squarings
        per += 8 + 64
        ensure = lambda c: per * c + al(c * 8) + 8192
    elif site == "deferred":                                         # flush_mulrelin_group
        per += al(3 * kn * 8) + 3 * 8 + 64
        ensure = lambda c: per * c + 3 * al(c * 8) + 8192
    elif site == "square_gemm":                                      # cn_square_gemm
        fixed = al(count * 3 * kn * 8) + al(outputs * tot * n * sw) + 8192
        fits = not fixed + per > smax
        ch = min(count, (smax - fixed) // per) if fits else 0
        return (per, fixed, ch, int(fits), fixed + per * ch + 4096, fixed + per + 4096)
    else:                                                            # a group of cn_mul_relin_sum: count products, `outputs` outputs
        fixed = al(count * 3 * kn * 8) + al(outputs * tot * n * sw) + 2 * al(count * 8) + 8192
        ch = min(count, max(1, (smax - min(smax, fixed)) // per))
        return (per, fixed, ch, 1, fixed + per * ch + 4096, fixed + per + 4096)
    ch = chunk_for(smax, per, count)
    return (per, 0, ch, 1, ensure(ch), ensure(1))


def expected_groups(S, K, count, smax, digit_i32):
    """cn_mul_relin_sum: (S as int32 words, outputs per group)"""
    kn, d = S["k"] * S["n"], (1 << S["dbc"]) - 1
    s32 = bool(digit_i32 and 1 <= S["dbc"] <= 31 and K * d <= (1 << 31) - 1)
    per, slack = per_ct(S, False), 4 * 256 + 8192
    per_out = K * 3 * kn * 8 + S["rl_tot"] * S["n"] * (4 if s32 else 8) + K * 16
    g_fit = (smax - per - slack) // per_out if smax > per + slack else 0
    return (int(s32), min(count, g_fit))


def ctx_ok(S, f64, rr13, xi, key_f64):
    """square_gemm_ctx_ok"""
    return bool(f64 and rr13 and not xi and key_f64 and all(m < 1 << 49 for m in S["q"]))


def expected_sum_ok(S, K, mul_sum):
    """mul_sum_fused_ok on a context with its defaults"""
    f64ok = all(m < 1 << 49 for m in S["q"])
    if not (mul_sum and K >= MUL_SUM_MIN_K and ctx_ok(S, 1, 10 <= S["logn"] <= 13, 0, f64ok)):
        return 0
    if not 1 <= S["dbc"] <= 31:
        return 0
    s = K * ((1 << S["dbc"]) - 1)
    if s >= 1 << 52 or any(s >= m // 2 for m in S["q"]) or any(d > MAX_DIGITS for d in digits(S["q"], S["dbc"])):
        return 0
    return int(K * (max(S["q"]) - 1) < 1 << 64 and S["n"] % 512 == 0)


def cuts_of(c):
    """pipeline_cuts"""
    P = min(3, max(1, c // 128))
    up8 = lambda x: (x + 7) & ~7
    return (P, 0) + {1: (), 2: (up8(c // 2),), 3: (up8(c * 3 // 10), up8(c * 7 // 10))}[P] + (c,)


def expected_parts(S, halves, capturing, minimum, c, wide, smax):
    """halves_pipeline_ok before its stream: 0 or the parts and their cuts"""
    if halves < minimum or S["logn"] > 13 or c < SQ_HALVES_MIN or capturing:
        return (0,)
    cuts = cuts_of(c)
    rr = 10 <= S["logn"] <= 14
    ks = dict(S, gk_tot=0, ctw2=2 * S["k"] * S["n"])
    if any(planned_mode(ks, wide, rr, smax, cuts[i + 2] - cuts[i + 1], 0) for i in range(cuts[0])):      # ks_writes_arena: up to N = 8192 the two-launch forms alone
        return (0,)
    return cuts if cuts[0] >= 2 else (0,)


def smax_list(S):
    return (24 << 30, 40 << 20, int(0.00224 * float(1 << 30)), 3 * S["k"] * S["n"] * 8 - 1)


def check(tables):
    sets, cuts, consts = tables
    assert sorted(sets) == sorted(SETS) and consts == (MUL_SUM_MIN_K, SQ_HALVES_MIN, MAX_DIGITS)
    checked = 0
    for name, T in sets.items():
        p, S = SETS[name], dict(T["hdr"])
        if p["q"]:
            assert S["q"] == list(p["q"]), name
        q, bsk = S["q"], S["bsk"]
        assert (S["n"], S["logn"], S["k"], S["kb"], S["dbc"]) == (p["n"], p["n"].bit_length() - 1, len(q), len(bsk), p["dbc"]), name
        assert S["rl_tot"] == sum(digits(q, p["dbc"])) and S["max_dig"] == max(digits(q, p["dbc"])), name
        assert S["f64ok_q"] == int(all(m < 1 << 49 for m in q)) and S["f64ok_bsk"] == int(all(m < 1 << 49 for m in bsk)) and S["behz_f64"] == (S["f64ok_q"] & S["f64ok_bsk"]), name
        smaxs = smax_list(S)
        want = set()
        for key in itertools.product((0, 1), COUNTS, (0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1), (1, 64, 256)):
            assert T["p"][key] == expected_plan(S, *key), (name, key, T["p"][key], expected_plan(S, *key))
            want.add(key)
        assert set(T["p"]) == want, name
        checked += len(want)
        want = set()
        for site, square, count, s, outputs, s32 in itertools.product(range(6), (0, 1), COUNTS, range(4), (0, 1, 10, 100), (0, 1)):
            if site < 4 and (outputs or s32):
                continue
            key = (site, square, count, s, outputs, s32)
            exp = expected_batch(S, SITES[site], square, count, smaxs[s], outputs, s32)
            assert T["b"][key] == exp, (name, key, T["b"][key], exp)
            want.add(key)
        assert set(T["b"]) == want, name
        checked += len(want)
        ks = term_counts(p) if p["q"] else [1, 2, 9]
        for K, count, s, i32 in itertools.product(ks, (1, 6, 100), range(4), (0, 1)):
            assert T["u"][(K, count, s, i32)] == expected_groups(S, K, count, smaxs[s], i32), (name, K, count, s, i32)
        assert len(T["u"]) == len(ks) * 24
        for key in itertools.product((0, 1), repeat=4):
            ok = int(ctx_ok(S, *key))
            assert T["c"][key] == (ok, ok, 0, ok, 0, 0), (name, key, T["c"][key])
        assert len(T["c"]) == 16
        for K, ms in itertools.product(ks, (0, 1)):
            assert T["k"][(K, ms)] == (expected_sum_ok(S, K, ms),), (name, K, ms, T["k"][(K, ms)])
        assert len(T["k"]) == len(ks) * 2
        want = set()
        for key in itertools.product((0, 1, 2), (0, 1), (1, 2), COUNTS, (-1, 0, 1, 2), range(4)):
            exp = expected_parts(S, *key[:5], smaxs[key[5]])
            assert T["h"][key] == exp, (name, key, T["h"][key], exp)
            want.add(key)
        assert set(T["h"]) == want, name
        for key in itertools.product((1, 10, 100), (1, 3), (8, 848), (2, 32), (0, 1)):
            O, G, Kp, M, i32 = key
            exp = al(O * 2 * S["k"] * S["n"] * 8) + al(O * S["rl_tot"] * S["n"] * (4 if i32 else 8)) + al(G * Kp * 4) + al(G * M * 4) + al(O * 8) + 8192      # sg_scratch
            assert T["g"][key] == (exp,), (name, key)
        checked += len(ks) * 26 + 16 + len(want) + 48
    for c, got in cuts.items():
        assert got == cuts_of(c)[1:] and len(got) == cuts_of(c)[0] + 1, c
    return checked


@pytest.fixture(scope="module")
def tables():
    r = run(build())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


def test_every_line_matches_the_rules_restated(tables):
    assert check(tables) > 5000 * len(SETS)


def test_the_product_sum_bounds_have_both_sides(tables):
    """Python integers on both sides of each bound: the last K that passes and the first that does not.  "tiny": 36-bit moduli and 10-bit digits put the q_j / 2
    bound at 2^25 terms, within a 32-bit K (c3's 44-bit moduli do not)"""
    sets = tables[0]
    S, p = sets["tiny"]["hdr"], SETS["tiny"]
    d, half = (1 << p["dbc"]) - 1, min(S["q"]) // 2
    last = -(-half // d) - 1                                         # the q_j / 2 bound is the tight one: far below 2^52
    assert last * d < half <= (last + 1) * d and half < 1 << 52 and last + 1 < 1 << 32
    assert sets["tiny"]["k"][(last, 1)] == (1,) and sets["tiny"]["k"][(last + 1, 1)] == (0,) and sets["tiny"]["k"][(last, 0)] == (0,)
    assert sets["c3"]["k"][(1, 1)] == (0,) and sets["c3"]["k"][(2, 1)] == (1,)      # MUL_SUM_MIN_K
    i32 = ((1 << 31) - 1) // d                                       # digit sums as int32 words: K d <= 2^31 - 1 < (K + 1) d
    assert i32 * d <= (1 << 31) - 1 < (i32 + 1) * d
    assert sets["tiny"]["u"][(i32, 1, 0, 1)][0] == 1 and sets["tiny"]["u"][(i32 + 1, 1, 0, 1)][0] == 0 and sets["tiny"]["u"][(i32, 1, 0, 0)][0] == 0
    # a limb of ten 4-bit digits: never the fused form, though every other bound holds at K = 2
    assert sets["tiny-dbc4"]["hdr"]["max_dig"] == 10 > MAX_DIGITS and sets["tiny"]["hdr"]["max_dig"] == 4
    assert sets["tiny-dbc4"]["k"][(2, 1)] == (0,) and sets["tiny"]["k"][(2, 1)] == (1,)
    # K (q_max - 1) < 2^64 is reachable with a 32-bit K from 33-bit moduli on; the sets' digit bounds fail first wherever it is
    for name, T in sets.items():
        qmax = max(T["hdr"]["q"])
        k64 = ((1 << 64) - 1) // (qmax - 1)
        if (k64 + 1, 1) in T["k"]:
            assert k64 * (qmax - 1) < 1 << 64 <= (k64 + 1) * (qmax - 1)
            assert T["k"][(k64 + 1, 1)] == (0,), name


def plan(tables, name, square, cnt, f64=1, fused=1, pipe=1, lds=1, rr=1, cus=256):
    return tables[0][name]["p"][(square, cnt, f64, fused, pipe, lds, rr, cus)]


def test_anchors(tables):
    """what the code before the planner did for the workloads, as literals"""
    sets, cuts, _ = tables
    assert cuts[845] == (0, 256, 592, 845) and cuts[512] == (0, 160, 360, 512) and cuts[255] == (0, 255) and cuts[256] == (0, 128, 256)
    c3 = sets["c3"]["hdr"]
    assert (c3["k"], c3["kb"], c3["n"], c3["behz_f64"]) == (5, 6, 8192, 1)
    # CryptoNets: the squaring of 845 is the fused kernel on both bases, lazy words into the FP64 floor, the pipelined resident kernel with 256 / 5 and 256 / 6
    # workgroups per modulus; no MUL_AQ
    kn8 = 8192 * 8
    assert plan(tables, "c3", 1, 845) == ("SQUARE_FUSED", 1, 1, "F64L", "PIPE", 51, "F64", "PIPE", 42,
                                          "ab:%d" % (845 * 2 * 6 * kn8), "dq:%d" % (845 * 3 * 5 * kn8), "db:%d" % (845 * 3 * 6 * kn8))
    assert plan(tables, "c3", 1, 3)[4:9] == ("LDS", 0, "F64", "LDS", 0)            # 3 < 4 x 3 blocks per resident workgroup: the parked-in-LDS kernel
    assert plan(tables, "c3", 1, 3, lds=0)[4] == "PLAIN" and plan(tables, "c3", 1, 3, pipe=2)[4:6] == ("PIPE", 3)
    assert plan(tables, "c3", 0, 845)[:5] == ("INTT_TENSOR", 1, 1, "F64L", "PLAIN") and len(plan(tables, "c3", 0, 845)) == 9 + 6
    # "f64" off: k_intt_tensor under the integer policy, canonical words into the integer floor (see the module docstring); "legacy_ntt": k_tensor
    assert plan(tables, "tiny", 0, 3, f64=0)[:4] == plan(tables, "tiny", 1, 3, f64=0)[:4] == ("INTT_TENSOR", 0, 0, "U64")
    assert plan(tables, "tiny", 1, 3, rr=0)[:4] == ("ELEMENTWISE", 0, 1, "F64L") and plan(tables, "tiny", 1, 3, f64=0, rr=0)[:4] == ("ELEMENTWISE", 0, 0, "U64")
    assert plan(tables, "sp-u64-n1024", 1, 3)[:4] == ("INTT_TENSOR", 0, 0, "U64")
    # c3 under 40 MiB: 9 squarings per chunk of cn_mul_relin, 8 products per chunk of cn_multiply (3 605 504 + 983 040 and 5 047 296 bytes each)
    b = sets["c3"]["b"]
    assert b[(1, 1, 845, 1, 0, 0)][:3] == (3605504 + 983040, 0, 9) and b[(0, 0, 845, 1, 0, 0)][:3] == (5047296, 0, 8)
    assert b[(1, 1, 3, 1, 0, 0)][2] == 3 and b[(1, 1, 845, 0, 0, 0)][2] == 845
    # K = 9, count = 6 on "tiny" at 0.00224 GiB: two outputs per group, three groups (test_outputs_run_in_groups_when_the_scratch_limit_is_small)
    assert sets["tiny"]["u"][(9, 6, 2, 1)] == (1, 2) and sets["tiny"]["k"][(9, 1)] == (1,)
    assert sets["tiny"]["u"][(9, 6, 3, 1)] == (1, 0)                # less than one product: the literal sequence
    # the pipeline: 845 and 512 squarings of c3 in three parts (fused key switch in every part), not while capturing, not at "ks_wide" 1, queued calls at 2 only
    h = sets["c3"]["h"]
    assert h[(1, 0, 1, 845, -1, 0)] == (3, 0, 256, 592, 845) and h[(1, 0, 1, 512, -1, 0)] == (3, 0, 160, 360, 512)
    assert h[(1, 0, 1, 511, -1, 0)] == h[(1, 1, 1, 845, -1, 0)] == h[(1, 0, 1, 845, 1, 0)] == h[(1, 0, 2, 845, -1, 0)] == h[(0, 0, 1, 845, -1, 0)] == (0,)
    assert h[(2, 0, 2, 845, -1, 0)][0] == 3 and sets["c5"]["h"][(1, 0, 1, 845, -1, 0)] == (0,)      # N = 16384: never


def test_mul_plan_header_is_clean_under_the_sanitizers(tables):
    """-fsanitize=undefined,address with errors fatal over the same sets: the same table, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == tables
