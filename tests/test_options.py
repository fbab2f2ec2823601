"""The option and counter tables of cryptonets_amd/csrc/cn_options.h on the CPU, compiled: tests/cpp/options.cpp (plain g++) prints the option table, the counter
names, what the environment reader makes of a fixed environment and what set-by-name answers at the edges of every range.  Checked here: every member of CnTunables
has exactly one table row; range, default and environment name of every row are those of its row in include/cnhip.h, and every name cn_get_option reads is
documented there; the retired switches are gone from the library and its package; the environment rule, the refusal rule and the rows that drop plans, restated in
Python.  A second build of the same program runs under -fsanitize=undefined,address: host code in a stand-alone program."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETIRED = ("defer_stagger", "sq_overlap", "ks_tight", "CN_DEFER_STAGGER", "CN_SQ_OVERLAP", "CN_KS_TIGHT", "CN_DEFER_PAIR", "CN_SQ_PARTS", "CN_SQ_SPLIT")
MEMBERS = 25
# what cn_set_option takes beside the table (their own code in cn_api.hip), and what cn_get_option reads beside the table and the counters
STATE = ("defer", "ks_xi", "record_steps")
READ_ONLY = ("pin_laps", "ready_handles", "sg_prefloor_min_k", "mul_sum_groups", "mul_sum_min_k", "defer_pending_products", "scratch_mib", "ptn_sum_interval",
             "packed_bad_residues", "behz_small_base", "behz_f64", "mod_switch_f64", "aux_primes", "pending_calls", "pool_arrays", "stream_tries")
COUNTERS = ("folded_zero_encryptions", "mul_relin_pipelined", "square_gemm_fused", "square_gemm_prefloor", "defer_square_gemm_fused", "digit_gemm_mfma",
            "mul_sum_fused", "ks_digits_i32", "ptn_sum", "ptn_bcast", "diag_scan", "diag_encode")
REPLAN = ("f64", "gemm_mfma", "gemm_pair", "digit_mfma", "digit_i32")
ENV_TEXTS = ("0", "1", "-5", "9")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def build(extra=()):
    exe = os.path.join(tempfile.mkdtemp(), "options")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", *extra, os.path.join(ROOT, "tests", "cpp", "options.cpp"), "-o", exe])
    return exe


def run(exe):
    return subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def parse(text):
    out = {"options": {}, "counters": [], "env": {}, "set": {}, "unknown": {}, "get": {}}
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "sizeof":
            out["sizeof"] = (int(w[1]), int(w[2]))
        elif w[0] == "o":
            assert w[1] not in out["options"], line
            out["options"][w[1]] = dict(index=int(w[2]), flag=int(w[3]), lo=int(w[4]), hi=int(w[5]), env=None if w[6] == "-" else w[6], d13=int(w[7]), d14=int(w[8]),
                                        replan=int(w[9]))
        elif w[0] == "c":
            out["counters"].append(w[1])
        elif w[0] == "e":
            assert w[3] == ":" and (w[1], w[2]) not in out["env"], line
            out["env"][(w[1], w[2])] = list(map(int, w[4:]))
        elif w[0] == "s":
            assert w[3] == ":" and (w[1], int(w[2])) not in out["set"], line
            out["set"][(w[1], int(w[2]))] = (int(w[4]), int(w[5]))
        elif w[0] == "u":
            out["unknown"][w[1]] = int(w[3])
        else:
            assert w[0] == "g" and w[2] == ":", line
            out["get"][w[1]] = (int(w[3]), int(w[4]))
    return out


@pytest.fixture(scope="module")
def tables():
    r = run(build())
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return parse(r.stdout.decode())


def header_options():
    """{name: (values, default at N <= 8192, default at N = 16384, environment)} of cn_set_option's list in include/cnhip.h"""
    lines = read("include", "cnhip.h").split("\n")
    first = next(i for i, l in enumerate(lines) if re.match(r" \*   name\s+values\s+default\s+environment\s+what it selects", l))
    rows = {}
    for i in range(first + 1, len(lines)):
        if not lines[i].startswith(" *  "):
            break                                                        # the list ends at the first line that is no row and no continuation
        m = re.match(r' \*   "(\w+)"\s+(flag|-?\d+\.\.-?\d+)\s+(\S.*?)\s{2,}(\S.*?)\s{2,}\S', lines[i])
        if not m:
            continue
        name, values, default, env = m.groups()
        assert name not in rows, name
        d13 = d14 = int(default.split()[0])
        if default != str(d13):                                          # a default by ring size: "2 (N <= 8192)," above "1 (N = 16384)" in the same column
            below = re.match(r"(-?\d+) \(N = 16384\)", lines[i + 1][m.start(3):])
            assert default == "%d (N <= 8192)," % d13 and below, lines[i]
            d14 = int(below.group(1))
        rows[name] = (values, d13, d14, env)
    return rows


def test_every_tunable_has_a_table_entry(tables):
    assert tables["sizeof"] == (MEMBERS * 4, 4) and MEMBERS == 25                # sizeof(CnTunables) == 25 * sizeof(int): a new switch goes through the table
    assert sorted(o["index"] for o in tables["options"].values()) == list(range(25))
    assert all(len(v) == 25 for v in tables["env"].values())
    assert tuple(tables["counters"]) == COUNTERS and len(set(COUNTERS)) == 12
    assert not (set(tables["options"]) | set(STATE)) & (set(COUNTERS) | set(READ_ONLY)) and not set(COUNTERS) & set(READ_ONLY)


def test_every_option_name_is_documented(tables):
    doc = header_options()
    assert sorted(doc) == sorted(list(tables["options"]) + list(STATE))
    for name, o in tables["options"].items():
        values, d13, d14, env = doc[name]
        assert values == ("flag" if o["flag"] else "%d..%d" % (o["lo"], o["hi"])), name
        assert (d13, d14) == (o["d13"], o["d14"]), name
        assert env == ("CN_NO_F64=1: 0" if name == "f64" else o["env"] or "-"), name
        assert not o["flag"] or (o["lo"], o["hi"]) == (0, 1), name
    assert [n for n, o in tables["options"].items() if o["d13"] != o["d14"]] == ["ks_xcd"]
    header = read("include", "cnhip.h")
    assert [n for n in COUNTERS + READ_ONLY if '"%s"' % n not in header] == []
    # cn_get_option's own list names nothing else
    start = header.index("reads back every option of cn_set_option's list")
    listed = re.findall(r'"(\w+)"', "\n".join(re.findall(r'^ \*   ("\w+"(?:, "\w+")*)\s', header[start:header.index("int cn_get_option(", start)], re.M)))
    assert len(listed) > 20 and [n for n in listed if n not in COUNTERS + READ_ONLY] == []


def test_retired_switches_are_gone(tables):
    found = []
    for top in ("include", "cryptonets_amd"):
        for dirpath, dirnames, files in os.walk(os.path.join(ROOT, top)):
            dirnames[:] = [d for d in dirnames if d not in ("lib", "__pycache__")]      # (build products)
            for f in files:
                with open(os.path.join(dirpath, f), "rb") as fh:
                    data = fh.read()
                found += ["%s: %s" % (os.path.relpath(os.path.join(dirpath, f), ROOT), r) for r in RETIRED if r.encode() in data]
    assert found == []
    assert tables["unknown"] == {"square_gemm_prefloor": 0, "defer": 0, "sq_overlap": 0, "ks_tight": 0, "-": 0}      # no switch: counters, state, retired names
    assert tables["get"]["defer"] == tables["get"]["stream_tries"] == tables["get"]["defer_stagger"] == (0, -99)


def test_environment_rule(tables):
    """a flag is text != 0, an enumerated switch is clamped into its range, CN_NO_F64 is inverted; a switch without an environment name keeps its default"""
    opts = tables["options"]
    assert sorted(tables["env"]) == sorted([("-", "-"), ("-", "0"), ("-", "1")] + [(t, n) for t in ENV_TEXTS for n in ("0", "1")])
    for (text, no_f64), got in tables["env"].items():
        for name, o in opts.items():
            want = o["d13"]
            if o["env"] and text != "-":
                want = int(int(text) != 0) if o["flag"] else max(o["lo"], min(o["hi"], int(text)))
            if name == "f64":
                want = 0 if no_f64 == "1" else 1
            assert got[o["index"]] == want, (text, no_f64, name)
    assert sum(1 for o in opts.values() if o["env"]) == 15 and opts["ptn_order"]["env"] == "CN_PTN_ORDER"
    assert tables["env"][("9", "0")][opts["ptn_order"]["index"]] == 1                 # clamped, like every enumerated switch


def test_out_of_range_values_are_refused_and_flags_normalise(tables):
    for name, o in tables["options"].items():
        kept = o["hi"] if o["d13"] != o["hi"] else o["lo"]
        if o["flag"]:
            assert [tables["set"][(name, v)] for v in (0, 1, 7, -1)] == [(0, 0), (0, 1), (0, 1), (0, 1)], name
        else:
            lo, hi = o["lo"], o["hi"]
            assert [tables["set"][(name, v)] for v in (lo - 1, lo, hi, hi + 1)] == [(1, kept), (0, lo), (0, hi), (1, kept)], name
    assert len(tables["set"]) == 4 * 25
    # get by name: every switch reads its default, every counter its count, saturated
    for name, o in tables["options"].items():
        assert tables["get"][name] == (1, o["d13"]), name
    assert [tables["get"][n] for n in COUNTERS] == [(1, i + 1) for i in range(11)] + [(1, 0x7fffffff)]


def test_the_rows_that_drop_plans(tables):
    assert sorted(n for n, o in tables["options"].items() if o["replan"]) == sorted(REPLAN)


def test_option_tables_are_clean_under_the_sanitizers(tables):
    """-fsanitize=undefined,address with errors fatal: the same output, no report"""
    r = run(build(("-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-g")))
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    assert parse(r.stdout.decode()) == tables
