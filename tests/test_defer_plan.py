"""The flush planner of the deferred queue (cryptonets_amd/csrc/cn_defer_plan.h) on the CPU: tests/cpp/defer_plan.cpp pushes text programs of queued calls over
synthetic addresses through defer_admit / defer_record and, at every flush, through the planner as cn_defer_flush drives it, and prints the rewritten calls, the
decision about pending products and the ordered steps.  Checked here: anchors - what the code BEFORE the planner did for the patterns that matter, as literals; an
independent oracle for random programs - the steps are interpreted on a toy algebra (every array a residue mod 2^61 - 1) and must leave every array the caller still
holds with the value the calls give one by one in issue order; and the same program under -fsanitize=undefined,address (host code in a stand-alone program)."""
import hashlib
import os
import random
import subprocess
import tempfile

import pytest

from test_policy_table import CSRC, ROOT

P = 2 ** 61 - 1
N, CTW2 = 1024, 4096                                        # ring size, words of a size-2 ciphertext (k = 2)
CT = CTW2 * 8
X0, PT0 = 0x10000000, 0x90000000                            # ciphertext arrays, plaintext polynomials
KINDS = ("gemm", "add", "sub", "addplain", "subplain", "mulrelin", "enc", "copy", "mulplain", "rot", "rotadd", "cols", "colsadd", "sumslots")


def al(x):
    return (x + 255) & ~255


def ct(i):
    return X0 + i * CT


def pt(j):
    return PT0 + j * N * 8


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "defer_plan")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "cpp", "defer_plan.cpp"), "-I" + CSRC, "-o", exe])
    return exe


def header(name, device=1, fold_zero=1, merge=1, flush_min=64, max_ops=32768, few_rot=0, square=1, park_max=64 * CTW2 * 12, t_half=6144):
    return "program %s %d %d %d %d %d %d %d %d %d %d %d" % (name, device, N, CTW2, t_half, park_max, fold_zero, merge, flush_min, max_ops, few_rot, square)


def stmt(kind, *args):
    """gemm: (out, [(addr, w), ...]); every other kind: addresses in hex, trailing integers (argument, item, bytes) in decimal"""
    if kind == "gemm":
        return "gemm %x %s" % (args[0], " ".join("%x:%d" % t for t in args[1]))
    n_int = {"enc": 1, "rot": 1, "rotadd": 1, "sumslots": 1, "free": 1}.get(kind, 0)
    head, tail = args[:len(args) - n_int], args[len(args) - n_int:]
    return " ".join([kind] + ["%x" % a for a in head] + ["%d" % a for a in tail])


def run(exe, programs):
    path = os.path.join(tempfile.mkdtemp(), "programs.txt")
    with open(path, "w") as f:
        for head, body in programs:
            f.write("\n".join([head] + body + ["end"]) + "\n")
    return subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def kv(words):
    return dict(w.split("=", 1) for w in words if "=" in w)


def parse(text):
    """{program: dict(admits=[...], flushes=[dict(boundary, ops, folds, pending, groups, steps, end)])}"""
    out, prog, fl = {}, None, None
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "program":
            prog = out[w[1]] = dict(admits=[], flushes=[])
        elif w[0] == "admit":
            d = kv(w)
            prog["admits"].append((int(w[1]), w[2], int(d["level"]), int(d["hd"]), int(d["flush"])))
        elif w[0] == "flush":
            fl = dict(boundary=int(kv(w)["boundary"]), ops=[], folds=[], pending=None, groups=[], steps=[], end=None)
            prog["flushes"].append(fl)
        elif w[0] == "op":
            d = kv(w)
            first, count = d["folds"].split("+")
            terms = [(int(t.split(":")[0], 16), int(t.split(":")[1])) for t in w[w.index("terms") + 1:]]
            fl["ops"].append(dict(kind=w[2], level=int(d["level"]), dead=int(d["dead"]), out=int(d["out"], 16), a=int(d["a"], 16), b=int(d["b"], 16), bias=int(d["bias"], 16),
                                  arg=int(d["arg"]), item=int(d["item"]), fold_first=int(first), fold_count=int(count), terms=terms))
        elif w[0] == "fold":
            d = kv(w)
            fl["folds"].append((int(d["enc"]), int(d["w"])))
        elif w[0] == "pending":
            d = kv(w)
            fl["pending"] = dict(count=int(w[1]), pure=int(d["pure"]), fused=int(d["fused"]), need=[int(x) for x in w[w.index("need") + 1:]])
        elif w[0] == "group":
            d = kv(w)
            r, s, c = w.index("rows"), w.index("slot_of"), w.index("cidx")
            fl["groups"].append(dict(level=int(d["level"]), K=int(d["K"]), bias_ok=int(d["bias_ok"]), rows=[int(x) for x in w[r + 1:s]], slot_of=[int(x) for x in w[s + 1:c]],
                                     cidx=[int(x) for x in w[c + 1:]]))
        elif w[0] == "step":
            d = kv(w)
            fl["steps"].append(dict(level=int(d["level"]), kind=w[2], type=w[3], key=int(d["key"]), park=int(d["park"]), ops=[int(x) for x in w[w.index("ops") + 1:]], can_park=None, staged=None))
        elif w[0] == "park":
            fl["steps"][-1]["can_park"] = int(w[2])
        elif w[0] == "staged":
            d = kv(w)
            fl["steps"][-1]["staged"] = dict(same_a=int(d["same_a"]), direct=d["direct"], consistent=int(d["consistent"]), off=[int(x) for x in d["off"].split(",")], total=int(d["total"]))
        elif w[0] == "endflush":
            fl["end"] = {k: int(v) for k, v in kv(w).items()}
        else:
            assert w[0] == "end", line
    return out


def steps_of(fl):
    return [(s["level"], s["kind"], s["type"], s["key"], s["ops"]) for s in fl["steps"]]


# ---------------------------------------------------------------- anchors: the parent's answers, read off its code
BIAS = [pt(j) for j in range(8)]


def pool_layer(release_all, blocked=False):
    """PoolLayer.Apply with padded taps: zero vectors z0, z1 (calls 0, 1), three windows of 3 terms (one reads z0, one reads z1 and a null tap), one of 2 terms, each
    followed by its AddPlain and the release of the intermediate"""
    x, z, t, r = [ct(i) for i in range(4)], [ct(10), ct(11)], [ct(20 + i) for i in range(5)], [ct(30 + i) for i in range(4)]
    body = [stmt("enc", z[0], 0, 100), stmt("enc", z[1], 0, 101)]
    windows = [[(x[0], 3), (x[1], 5), (x[2], 7)], [(x[1], 2), (x[2], 4), (z[0], 6)], [(x[2], 1), (z[1], 9), (0, 0)], [(x[0], 1), (x[3], 2)]]
    for i, terms in enumerate(windows):
        body += [stmt("gemm", t[i], terms), stmt("addplain", r[i], t[i], BIAS[i]), stmt("free", t[i], CT)]
    if blocked:                                             # a fifth window without a bias whose input is overwritten afterwards: it cannot wait for the deeper level
        body += [stmt("gemm", t[4], [(x[0], 1), (x[1], 1), (x[3], 1)]), stmt("sub", x[3], x[3], x[0])]
    body += [stmt("free", z[0], CT)] + ([stmt("free", z[1], CT)] if release_all else [])
    return body, x, z, t, r


@pytest.fixture(scope="module")
def exe():
    return build()


def one(exe, head, body):
    r = run(exe, [(head, body)])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())[head.split()[1]]


def test_pool_layer_pattern_with_every_zero_vector_released(exe):
    body, x, z, t, r = pool_layer(True)
    (fl,) = one(exe, header("pool"), body)["flushes"]
    ops = fl["ops"]
    # calls: 0, 1 the zero encryptions; 2 / 3, 4 / 5, 6 / 7, 8 / 9 scalar product / AddPlain
    assert [o["dead"] for o in ops] == [2, 2, 0, 1, 0, 1, 0, 1, 0, 1]
    assert [(ops[g]["out"], ops[g]["bias"]) for g in (2, 4, 6, 8)] == [(r[i], BIAS[i]) for i in range(4)]      # every AddPlain folded into its own scalar product
    assert fl["folds"] == [(0, 6), (1, 9)]
    assert [(ops[g]["fold_first"], ops[g]["fold_count"]) for g in (2, 4, 6, 8)] == [(-1, 0), (0, 1), (1, 1), (-1, 0)]
    assert ops[4]["terms"] == [(x[1], 2), (x[2], 4), (0, 0)] and ops[6]["terms"] == [(x[2], 1), (0, 0), (0, 0)]
    # one scalar-product step per term count: the three-term windows wait for the deepest of them (level 2), the fold follows their launch
    assert steps_of(fl) == [(1, "GEMM", "gemm", 2, [8]), (2, "GEMM", "gemm", 3, [2, 4, 6]), (2, "ZERO_FOLD", "gemm", 0, [4, 6])]
    assert fl["end"] == dict(bias_folds=4, zero_folds=2, merged=1, parked=0, fused=0, materialised=0)


def test_pool_layer_pattern_with_one_zero_vector_held(exe):
    body, x, z, t, r = pool_layer(False, blocked=True)
    (fl,) = one(exe, header("held"), body)["flushes"]
    ops = fl["ops"]
    # all or nothing: no zero encryption is folded.  The AddPlain of the two-term window is not folded either: x[3], an input of its scalar product, is overwritten behind it
    assert [o["dead"] for o in ops] == [0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0] and fl["folds"] == []
    assert ops[4]["terms"] == [(x[1], 2), (x[2], 4), (z[0], 6)] and (ops[8]["out"], ops[8]["bias"]) == (t[3], 0)
    # the first window joins the two on level 2; the fifth stays on level 0: x[3] is overwritten on level 1
    assert steps_of(fl) == [(0, "GEMM", "gemm", 2, [8]), (0, "GEMM", "gemm", 3, [10]), (0, "ENCRYPT", "enc", 0, [0, 1]), (1, "ELEMENTWISE", "sub", 0, [11]),
                            (1, "ELEMENTWISE", "addplain", 0, [9]), (2, "GEMM", "gemm", 3, [2, 4, 6])]
    assert fl["end"]["merged"] == 1 and fl["end"]["zero_folds"] == 0


def test_reused_output_handle_is_not_folded_across(exe):
    """GEMM1 -> tmp, AddPlain(tmp) -> r1, GEMM2 -> tmp, AddPlain(tmp) -> r2, free(tmp) (tests/test_deferred.py: test_bias_fold_with_a_reused_output_handle)"""
    x, tmp, r1, r2 = [ct(i) for i in range(5)], ct(20), ct(30), ct(31)
    body = [stmt("gemm", tmp, [(a, 3 + i) for i, a in enumerate(x)]), stmt("addplain", r1, tmp, BIAS[0]), stmt("gemm", tmp, [(a, 7 + i) for i, a in enumerate(x)]),
            stmt("addplain", r2, tmp, BIAS[1]), stmt("free", tmp, CT)]
    p = one(exe, header("reused"), body)
    assert [a[2] for a in p["admits"]] == [0, 1, 2, 3]
    (fl,) = p["flushes"]
    ops = fl["ops"]
    assert [o["dead"] for o in ops] == [0, 0, 0, 1]
    assert (ops[0]["out"], ops[0]["bias"], ops[0]["level"]) == (tmp, 0, 0) and (ops[2]["out"], ops[2]["bias"], ops[2]["level"]) == (r2, BIAS[1], 3)
    assert steps_of(fl) == [(0, "GEMM", "gemm", 5, [0]), (1, "ELEMENTWISE", "addplain", 0, [1]), (3, "GEMM", "gemm", 5, [2])]


def test_blocked_rewrites(exe):
    x, z, e, o = [ct(i) for i in range(4)], ct(10), ct(11), [ct(20 + i) for i in range(3)]
    # a zero encryption read by two scalar products
    (fl,) = one(exe, header("twice"), [stmt("enc", z, 0, 5), stmt("gemm", o[0], [(x[0], 3), (x[1], 2), (z, 9)]), stmt("gemm", o[1], [(x[1], 3), (x[2], 2), (z, 9)]),
                                      stmt("free", z, CT)])["flushes"]
    assert [q["dead"] for q in fl["ops"]] == [0, 0, 0] and fl["folds"] == [] and steps_of(fl) == [(0, "ENCRYPT", "enc", 0, [0]), (1, "GEMM", "gemm", 3, [1, 2])]
    # an input written on a deeper level / an output read on a deeper level: the scalar product stays on its level
    deeper = [stmt("enc", e, pt(4), 6), stmt("gemm", o[0], [(x[0], 5), (x[1], 7)]), stmt("gemm", o[1], [(x[0], 5), (e, 7)])]
    (fl,) = one(exe, header("input"), deeper + [stmt("add", x[0], x[2], x[3])])["flushes"]
    assert steps_of(fl) == [(0, "GEMM", "gemm", 2, [1]), (0, "ENCRYPT", "enc", 0, [0]), (1, "GEMM", "gemm", 2, [2]), (2, "ELEMENTWISE", "add", 0, [3])]
    (fl,) = one(exe, header("output"), deeper + [stmt("add", o[2], o[0], x[3])])["flushes"]
    assert steps_of(fl) == [(0, "GEMM", "gemm", 2, [1]), (0, "ENCRYPT", "enc", 0, [0]), (1, "GEMM", "gemm", 2, [2]), (1, "ELEMENTWISE", "add", 0, [3])]
    (fl,) = one(exe, header("written"), deeper + [stmt("copy", o[0], x[3])])["flushes"]      # ... or written
    assert steps_of(fl)[0] == (0, "GEMM", "gemm", 2, [1]) and fl["end"]["merged"] == 0
    (fl,) = one(exe, header("free"), deeper)["flushes"]                                      # nothing in the way: one launch
    assert steps_of(fl) == [(0, "ENCRYPT", "enc", 0, [0]), (1, "GEMM", "gemm", 2, [1, 2])] and fl["end"]["merged"] == 1
    (fl,) = one(exe, header("off", merge=0), deeper)["flushes"]                              # CN_DEFER_MERGE_GEMM=0
    assert fl["end"]["merged"] == 0


def squares_then_dense(held=(), add_reads=None, written=None, rows=((1, 2, 3, 4), (5, 6, 7, 8)), read=(0, 1, 2, 3)):
    x, s, d = [ct(i) for i in range(4)], [ct(10 + i) for i in range(4)], [ct(20 + i) for i in range(4)]
    body = [stmt("mulrelin", s[i], x[i], x[i]) for i in range(4)] + ["flush boundary"]
    body += [stmt("gemm", d[j], [(s[i], w[i]) for i in read]) for j, w in enumerate(rows)]
    if add_reads is not None:
        body.append(stmt("add", d[2], s[add_reads], x[0]))
    if written is not None:
        body.append(stmt("copy", s[written], x[0]))
    body += [stmt("free", s[i], CT) for i in range(4) if i not in held]
    return body


def test_pending_squarings_feed_the_dense_layer(exe):
    for device in (1, 0):
        first, second = one(exe, header("dense%d" % device, device=device), squares_then_dense())["flushes"]
        assert steps_of(first) == [(0, "MULRELIN", "mulrelin", 1, [0, 1, 2, 3])] and first["steps"][0]["park"] == 1 and first["steps"][0]["can_park"] == 1
        assert second["pending"] == dict(count=4, pure=1, fused=device, need=[1, 1, 1, 1])
        if device:
            assert second["groups"] == [dict(level=0, K=4, bias_ok=1, rows=[0, 1], slot_of=[0, 1, 2, 3], cidx=[0, 1, 2, 3, 0, 1, 2, 3])]
            assert steps_of(second) == [(0, "FUSED", "gemm", 0, [0, 1])] and second["end"]["fused"] == 1
        else:
            assert steps_of(second) == [(0, "GEMM", "gemm", 4, [0, 1])] and second["end"]["materialised"] == 4
    # rows sorted by their weights, slots renumbered by first appearance: the key does not depend on the order of the calls
    _, fl = one(exe, header("order"), squares_then_dense(rows=((5, 6, 7, 8), (1, 2, 3, 4)), read=(2, 0, 3, 1)))["flushes"]
    assert fl["groups"][0]["rows"] == [1, 0] and fl["groups"][0]["slot_of"] == [2, 0, 3, 1] and fl["groups"][0]["cidx"] == [0, 1, 2, 3, 0, 1, 2, 3]
    # a demand flush does not park; neither does "defer_square_gemm" off
    (fl,) = one(exe, header("demand"), squares_then_dense()[:4])["flushes"]
    assert fl["steps"][0]["park"] == 0 and fl["end"]["parked"] == 0
    fl = one(exe, header("optoff", square=0), squares_then_dense())["flushes"][0]
    assert fl["steps"][0]["park"] == 0
    # the products must fit a quarter of the scratch limit: three products' bytes hold no four
    fl = one(exe, header("small", park_max=3 * CTW2 * 12), squares_then_dense())["flushes"][0]
    assert fl["steps"][0]["park"] == 1 and fl["steps"][0]["can_park"] == 0


def test_pending_squarings_that_must_be_materialised(exe):
    need = lambda **k: one(exe, header("m"), squares_then_dense(**k))["flushes"][1]["pending"]
    assert need(read=(0, 1), held=(3,)) == dict(count=4, pure=0, fused=0, need=[1, 1, 0, 1])                 # (a) one array still held; slot 2 released and unread
    assert need(read=(0, 1), add_reads=2) == dict(count=4, pure=0, fused=0, need=[1, 1, 1, 0])               # (b) an Add reads a pending array
    assert need(read=(0, 1), written=3) == dict(count=4, pure=0, fused=0, need=[1, 1, 0, 0])                 # (d) a queued call writes a pending array
    assert need(read=(0, 1)) == dict(count=4, pure=1, fused=1, need=[1, 1, 0, 0])
    x9 = ct(9)                                                                                              # (c) a gathered term that is no pending array
    body = squares_then_dense(read=(0, 1))
    body.insert(5, stmt("gemm", ct(25), [(ct(10), 1), (x9, 2)]))
    assert one(exe, header("c"), body)["flushes"][1]["pending"] == dict(count=4, pure=0, fused=0, need=[1, 1, 0, 0])
    # a squaring whose output somebody reads, or which the caller has released, or which is not the last writer of its output, is not parked (nor are the others of its level)
    x, s = [ct(i) for i in range(4)], [ct(10 + i) for i in range(4)]
    sq = [stmt("mulrelin", s[i], x[i], x[i]) for i in range(3)]
    for extra, want in (([stmt("add", ct(20), s[0], x[0])], [0]), ([stmt("free", s[1], CT)], [0]), ([stmt("mulrelin", s[2], x[3], x[3])], [0, 1])):      # (level 0, level 1)
        fl = one(exe, header("nopark"), sq + extra + ["flush boundary"])["flushes"][0]
        assert [st["can_park"] for st in fl["steps"] if st["kind"] == "MULRELIN" and st["park"]] == want, extra


def staged_total(cnt, has_b, has_p, in_place):
    tabs, ctb = al(3 * cnt * 16) + al(cnt * 16), al(cnt * CTW2 * 8)
    off_o = tabs if in_place else tabs + ctb * (2 if has_b else 1)
    return dict(off=[0, 2 * cnt * 16, al(3 * cnt * 16), tabs, tabs + ctb if has_b else 0, off_o, off_o + ctb if has_p else 0],
                total=tabs + ctb * (1 + has_b + (0 if in_place else 1)) + (al(cnt * N * 8) if has_p else 0))


def test_staged_layouts(exe):
    v = ct(0)
    # thirteen MultiplyPlain of one ciphertext (the rows of a dense layer): the broadcast form, nothing gathered; scattered results are scattered back
    (fl,) = one(exe, header("rows"), [stmt("mulplain", ct(10 + 2 * i), v, pt(i)) for i in range(13)])["flushes"]
    (st,) = fl["steps"]
    assert (st["kind"], st["type"], len(st["ops"])) == ("STAGED", "mulplain", 13)
    assert st["staged"] == dict(same_a=1, direct="1010", consistent=1, **staged_total(13, 0, 1, 0))
    assert st["staged"]["total"] == al(39 * 16) + al(13 * 16) + 2 * 13 * CT + 13 * N * 8
    # equally spaced operands and results are used in place, scattered ones gathered; one call is always in place
    (fl,) = one(exe, header("rot"), [stmt("rot", ct(20 + i), ct(i), 3) for i in range(3)] + [stmt("rot", ct(30 + 2 * i), ct(5 + 2 * i), -1) for i in range(3)]
                + [stmt("rot", ct(40), ct(9), 7)])["flushes"]
    assert [(s["kind"], s["key"], s["staged"]["direct"]) for s in fl["steps"]] == [("STAGED", -1, "0000"), ("STAGED", 3, "1001"), ("STAGED", 7, "1001")]
    assert fl["steps"][0]["staged"] == dict(same_a=0, direct="0000", consistent=1, **staged_total(3, 0, 0, 0))
    (fl,) = one(exe, header("few", few_rot=7), [stmt("rot", ct(20 + i), ct(i), i + 1) for i in range(7)])["flushes"]      # few rotations: one chain per hop round
    assert steps_of(fl) == [(0, "ROT_JOBS", "rot", 0, list(range(7)))]
    (fl,) = one(exe, header("many", few_rot=6), [stmt("rot", ct(20 + i), ct(i), 1 + i % 2) for i in range(7)])["flushes"]
    assert [(s["kind"], s["key"], s["ops"]) for s in fl["steps"]] == [("STAGED", 1, [0, 2, 4, 6]), ("STAGED", 2, [1, 3, 5])]
    # RotateRowsAndAdd with the accumulators scattered, SumAllSlots in place (operands and results are the same arrays: both direct or both gathered)
    (fl,) = one(exe, header("acc"), [stmt("rotadd", ct(20 + i), ct(i), ct(30 + 3 * i), 2) for i in range(2)] + [stmt("sumslots", ct(40 + i), 8) for i in range(2)]
                + [stmt("sumslots", ct(50 + 2 * i), 16) for i in range(2)] + [stmt("copy", ct(60), ct(1)), stmt("colsadd", ct(61), ct(2), ct(3))])["flushes"]
    got = {(s["type"], s["key"]): s for s in fl["steps"]}
    assert [(s["kind"], s["type"]) for s in fl["steps"]] == [("COPY", "copy"), ("STAGED", "rotadd"), ("STAGED", "colsadd"), ("STAGED", "sumslots"), ("STAGED", "sumslots")]
    assert got["rotadd", 2]["staged"] == dict(same_a=0, direct="1001", consistent=1, **staged_total(2, 1, 0, 0))
    assert got["sumslots", 8]["staged"] == dict(same_a=0, direct="1001", consistent=1, **staged_total(2, 0, 0, 1))
    assert got["sumslots", 16]["staged"] == dict(same_a=0, direct="0000", consistent=1, **staged_total(2, 0, 0, 1))
    assert got["colsadd", 0]["staged"] == dict(same_a=0, direct="1101", consistent=1, **staged_total(1, 1, 0, 0))


def test_admission_levels_heavy_depth_and_the_boundary_rule(exe):
    x = [ct(i) for i in range(4)]
    body = [stmt("enc", ct(10), 0, 1), stmt("gemm", ct(11), [(x[0], 1), (ct(10), 2)]), stmt("addplain", ct(12), ct(11), BIAS[0]), stmt("rot", ct(13), ct(12), 1),
            stmt("mulrelin", ct(14), ct(13), ct(13)), stmt("add", ct(11), x[1], x[2])]
    p = one(exe, header("admit", flush_min=5), body)
    # (index, kind, level, heavy depth, flush): the squaring reads a value of heavy depth 1 with five calls queued - a layer boundary; two calls follow the flush
    assert p["admits"] == [(0, "enc", 0, 0, 0), (1, "gemm", 1, 1, 0), (2, "addplain", 2, 1, 0), (3, "rot", 3, 1, 0), (4, "mulrelin", 4, 2, 0), (5, "add", 3, 0, 0)]
    p = one(exe, header("admit4", flush_min=4), body)
    assert p["admits"][4:] == [(0, "mulrelin", 0, 1, 1), (1, "add", 0, 0, 0)] and [f["boundary"] for f in p["flushes"]] == [1, 0]
    p = one(exe, header("full", max_ops=3), body)
    assert [a[4] for a in p["admits"]] == [0, 0, 0, 2, 0, 0] and [f["boundary"] for f in p["flushes"]] == [0, 0]


# ---------------------------------------------------------------- the oracle: a toy algebra
def H(tag, x):
    return int.from_bytes(hashlib.blake2b(("%s:%d" % (tag, x)).encode(), digest_size=8).digest(), "little") % P


def affine(tag, arg, v):
    return ((H(tag + "m", arg) % (P - 1) + 1) * v + H(tag + "c", arg)) % P


def apply_call(kind, a, b, pt_b, arg, item):
    """the value one call gives: a, b the values of its ciphertext operands, pt_b of its plaintext operand"""
    if kind == "add":
        return (a + b) % P
    if kind == "sub":
        return (a - b) % P
    if kind == "addplain":
        return (a + pt_b) % P
    if kind == "subplain":
        return (a - pt_b) % P
    if kind == "mulrelin":
        return a * b % P
    if kind == "mulplain":
        return a * pt_b % P
    if kind == "copy":
        return a
    if kind == "rot":
        return affine("rot", arg, a)
    if kind == "rotadd":
        return (affine("rot", arg, a) + b) % P
    if kind == "cols":
        return affine("cols", 0, a)
    if kind == "colsadd":
        return (affine("cols", 0, a) + b) % P
    if kind == "sumslots":
        return affine("sum", arg, a)
    raise AssertionError(kind)


class Values(dict):
    def __missing__(self, addr):
        return H("ct", addr)


def issue_order(calls):
    """the calls one by one, as the caller issued them"""
    val, freed = Values(), []
    for c in calls:
        k = c[0]
        if k == "free":
            freed.append((c[1], c[2]))
        elif k == "gemm":
            val[c[1]] = sum(w * val[a] for a, w in c[2] if a) % P
        elif k == "enc":
            val[c[1]] = (H("enc", c[3]) + (H("pt", c[2]) if c[2] else 0)) % P
        elif k == "sumslots":
            val[c[1]] = apply_call(k, val[c[1]], 0, 0, c[2], 0)
        elif k in ("addplain", "subplain", "mulplain"):
            val[c[1]] = apply_call(k, val[c[2]], 0, H("pt", c[3]), 0, 0)
        elif k in ("copy", "cols"):
            val[c[1]] = apply_call(k, val[c[2]], 0, 0, 0, 0)
        elif k == "rot":
            val[c[1]] = apply_call(k, val[c[2]], 0, 0, c[3], 0)
        elif k == "rotadd":
            val[c[1]] = apply_call(k, val[c[2]], val[c[3]], 0, c[4], 0)
        elif k != "flush":
            val[c[1]] = apply_call(k, val[c[2]], val[c[3]], 0, 0, 0)
    return val, freed


def scheduled(flushes):
    """the steps of every flush in order, parked products carried from one flush to the next"""
    val, parked = Values(), []                              # parked: (output array, product) by slot
    for fl in flushes:
        ops, old = fl["ops"], dict(parked)
        if parked:
            pend = fl["pending"]
            assert pend["count"] == len(parked)
            if not pend["fused"]:
                for (out, v), need in zip(parked, pend["need"]):
                    if need:
                        val[out] = v
            parked = []
        for st in fl["steps"]:
            new = {}
            for i in st["ops"]:
                o = ops[i]
                assert not o["dead"]
                if st["kind"] in ("GEMM", "FUSED"):
                    src = old if st["kind"] == "FUSED" else val
                    new[o["out"]] = (sum(w * src[a] for a, w in o["terms"] if a) + (H("pt", o["bias"]) if o["bias"] else 0)) % P
                elif st["kind"] == "ZERO_FOLD":
                    fs = fl["folds"][o["fold_first"]:o["fold_first"] + o["fold_count"]]
                    new[o["out"]] = (val[o["out"]] + sum(w * H("enc", ops[e]["item"]) for e, w in fs)) % P
                elif st["kind"] == "ENCRYPT":
                    new[o["out"]] = (H("enc", o["item"]) + (H("pt", o["a"]) if o["a"] else 0)) % P
                else:
                    plain = o["kind"] in ("addplain", "subplain", "mulplain")
                    v = apply_call(o["kind"], val[o["a"]], 0 if plain or not o["b"] else val[o["b"]], H("pt", o["b"]) if plain else 0, o["arg"], 0)
                    if st["kind"] == "MULRELIN" and st["can_park"]:
                        parked.append((o["out"], v))
                    else:
                        new[o["out"]] = v
            val.update(new)                                 # a step is one batched launch: every call reads what stood before it
    assert not parked
    return val


def random_program(seed):
    rng = random.Random(seed)
    calls, live, nxt, item = [], [ct(i) for i in range(6)], [100], [1]

    def fresh():
        nxt[0] += rng.choice((1, 1, 2))
        return ct(nxt[0])

    def noise():
        k = rng.choice(("add", "add", "sub", "inplace", "addplain", "subplain", "general", "rot", "rot", "rotadd", "cols", "colsadd", "sumslots", "copy", "mulplain", "mulplain", "enc",
                        "gemm", "free", "overwrite"))
        a, b = rng.choice(live), rng.choice(live)
        if k in ("add", "sub"):
            calls.append((k, fresh(), a, b))
        elif k == "inplace":
            calls.append(("sub", a, a, b))
        elif k == "overwrite" and a != b:
            calls.append(("copy", a, b))
        elif k in ("addplain", "subplain", "mulplain"):
            calls.append((k, fresh(), a, pt(rng.randrange(8))))
        elif k == "general" and a != b:
            calls.append(("mulrelin", b, a, b))
        elif k == "rot":
            calls.append(("rot", fresh(), a, rng.choice((1, 2, -3))))
        elif k == "rotadd":
            calls.append(("rotadd", fresh(), a, b, rng.choice((1, 2))))
        elif k in ("cols", "copy"):
            calls.append((k, fresh(), a))
        elif k == "colsadd":
            calls.append((k, fresh(), a, b))
        elif k == "sumslots":
            calls.append((k, a, rng.choice((4, 8))))
        elif k == "enc":
            calls.append(("enc", fresh(), pt(rng.randrange(8)), item[0]))
            item[0] += 1
        elif k == "gemm":
            terms = [(x, rng.randrange(1, 40)) for x in rng.sample(live, rng.randrange(2, 5))]
            if rng.random() < 0.3:
                terms[-1] = (0, 0)
            calls.append(("gemm", fresh(), terms))
        elif k == "free" and len(live) > 6:
            live.remove(a)
            calls.append(("free", a, CT))
            return
        else:
            return
        if calls[-1][1] not in live:
            live.append(calls[-1][1])

    def pool():
        """PoolLayer: zero vectors for the padded taps, windows of one or two term counts, bias, releases (now and then one zero vector stays, or is read twice)"""
        zs = []
        for _ in range(rng.randrange(1, 4)):
            zs.append(fresh())
            calls.append(("enc", zs[-1], 0, item[0]))
            item[0] += 1
        twice = rng.random() < 0.15
        for j in range(rng.randrange(3, 7)):
            K = rng.choice((3, 3, 4))
            terms = [(x, rng.randrange(1, 40)) for x in rng.sample(live, K - 1)]
            if j < len(zs) or (twice and j == len(zs)):
                terms.append((zs[min(j, len(zs) - 1)], rng.randrange(0, 9)))
            else:
                terms.append(rng.choice(((0, 0), (rng.choice(live), 0))))
            t, r = fresh(), fresh()
            calls.extend([("gemm", t, terms), ("addplain", r, t, pt(rng.randrange(8))), ("free", t, CT)])
            live.append(r)
            if rng.random() < 0.2:
                noise()
        for z in zs[:len(zs) - (rng.random() < 0.2)]:
            calls.append(("free", z, CT))

    def square_dense():
        """SquareActivation, a layer boundary, a dense layer over the squares, their release (now and then one is held, read by an Add or overwritten)"""
        xs = rng.sample(live, rng.randrange(3, 6))
        ss = [fresh() for _ in xs]
        calls.extend(("mulrelin", s, x, x) for s, x in zip(ss, xs))
        calls.append(("flush", "boundary"))
        mishap = rng.choice((None, None, None, "held", "add", "write", "other"))
        bias = rng.random() < 0.5
        for _ in range(rng.randrange(2, 4)):
            terms = [(s, rng.randrange(1, 40)) for s in ss]
            if rng.random() < 0.3:
                terms[rng.randrange(len(terms))] = (0, 0)
            if mishap == "other":
                terms[0] = (rng.choice(live), 3)
            d = fresh()
            if bias:
                t = fresh()
                calls.extend([("gemm", t, terms), ("addplain", d, t, pt(rng.randrange(8))), ("free", t, CT)])
            else:
                calls.append(("gemm", d, terms))
            live.append(d)
        if mishap == "add":
            calls.append(("add", fresh(), ss[0], rng.choice(live)))
            live.append(calls[-1][1])
        if mishap == "write":
            calls.append(("copy", ss[-1], rng.choice(live)))
        for s in ss[1 if mishap == "held" else 0:]:
            calls.append(("free", s, CT))
        if mishap == "held":
            live.append(ss[0])
        if rng.random() < 0.5:
            calls.append(("flush", "demand"))

    while sum(c[0] not in ("free", "flush") for c in calls) < 30:
        rng.choice((pool, pool, square_dense, square_dense, noise))()
        for _ in range(rng.randrange(0, 5)):
            noise()
    head = header("r%d" % seed, device=rng.randrange(2), flush_min=rng.choice((8, 64)), few_rot=rng.choice((0, 2)))
    return head, calls


def as_text(calls):
    return [("flush " + c[1]) if c[0] == "flush" else stmt(*c) for c in calls]


SEEDS = range(300)


def check_random(tables, programs):
    did = dict(bias_folds=0, zero_folds=0, merged=0, parked=0, fused=0, materialised=0)
    for head, calls in programs:
        p = tables[head.split()[1]]
        assert len(p["admits"]) == sum(c[0] not in ("free", "flush") for c in calls)
        want, freed = issue_order(calls)
        got = scheduled(p["flushes"])
        for addr in set(want) | set(got):
            if not any(base <= addr < base + size for base, size in freed):
                assert got[addr] == want[addr], (head, hex(addr))
        for k in did:
            did[k] += any(fl["end"][k] for fl in p["flushes"])
    return did


@pytest.fixture(scope="module")
def randoms(exe):
    programs = [random_program(s) for s in SEEDS]
    r = run(exe, [(h, as_text(c)) for h, c in programs])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return programs, r.stdout.decode()


def test_random_programs_leave_the_values_of_the_calls_in_issue_order(randoms):
    programs, text = randoms
    assert all(30 <= sum(c[0] not in ("free", "flush") for c in calls) for _, calls in programs)
    did = check_random(parse(text), programs)
    print(did)
    # every rewrite, parking, fusing and materialising occurs in at least a tenth of the programs: the oracle is not passed by programs in which nothing is rewritten
    assert all(v * 10 >= len(programs) for v in did.values()), did


def test_the_oracle_notices_a_wrong_schedule(randoms):
    """the check above is not vacuous: a schedule that runs a folded scalar product on the level it was queued on, or drops a fold, gives other values"""
    programs, text = randoms
    tables = parse(text)
    caught = 0
    for head, calls in programs[:60]:
        p = tables[head.split()[1]]
        for fl in p["flushes"]:
            if fl["folds"]:
                fl["folds"][0] = (fl["folds"][0][0], fl["folds"][0][1] + 1)
                want, freed = issue_order(calls)
                got = scheduled(p["flushes"])
                caught += any(got[a] != want[a] for a in want if not any(b <= a < b + s for b, s in freed))
                break
    assert caught >= 5


def test_defer_plan_header_is_clean_under_the_sanitizers(randoms):
    """-fsanitize=undefined,address with errors fatal over the same programs: the same output, no report"""
    programs, text = randoms
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")), [(h, as_text(c)) for h, c in programs])
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert r.stdout.decode() == text
