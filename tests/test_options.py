"""The option table of cn_api.hip against its documentation and its struct: every tunable of CnTunables has a table entry, every option name
cn_set_option / cn_get_option accepts is documented in include/cnhip.h, and the retired switches are gone from the library and its package."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cryptonets_amd", "csrc")
RETIRED = ("defer_stagger", "sq_overlap", "ks_tight", "CN_DEFER_STAGGER", "CN_SQ_OVERLAP", "CN_KS_TIGHT", "CN_DEFER_PAIR", "CN_SQ_PARTS", "CN_SQ_SPLIT")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def table():
    """{option name: CnTunables member} of the option table"""
    return dict(re.findall(r'\{"(\w+)",\s*&CnTunables::(\w+),', read("cryptonets_amd", "csrc", "cn_api.hip")))


def option_function(name):
    src = read("cryptonets_amd", "csrc", "cn_api.hip")
    start = src.index('extern "C" int %s(' % name)
    return src[start:src.index("API_END }", start)]


def test_every_tunable_has_a_table_entry():
    struct = re.search(r"struct CnTunables \{(.*?)\n\};", read("cryptonets_amd", "csrc", "cn_runtime.h"), re.S).group(1)
    members = re.findall(r"^\s*int (\w+) = ", struct, re.M)
    assert len(members) == 19
    assert sorted(table().values()) == sorted(members)


def test_every_option_name_is_documented():
    names = set(table())
    for fn in ("cn_set_option", "cn_get_option"):
        names |= set(re.findall(r'strcmp\(name, "(\w+)"\)', option_function(fn)))
    assert {"defer", "ks_xi", "pending_calls", "mul_relin_pipelined", "stream_tries"} <= names
    header = read("include", "cnhip.h")
    assert [n for n in sorted(names) if '"%s"' % n not in header] == []


def test_retired_switches_are_gone():
    found = []
    for top in ("include", "cryptonets_amd"):
        for dirpath, dirnames, files in os.walk(os.path.join(ROOT, top)):
            dirnames[:] = [d for d in dirnames if d not in ("lib", "__pycache__")]      # (build products)
            for f in files:
                with open(os.path.join(dirpath, f), "rb") as fh:
                    data = fh.read()
                found += ["%s: %s" % (os.path.relpath(os.path.join(dirpath, f), ROOT), r) for r in RETIRED if r.encode() in data]
    assert found == []
