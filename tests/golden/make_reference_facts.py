"""Regenerates tests/golden/reference_facts.json: the facts tests/test_integration_cs.py checks about the reference's C# sources, taken from a
checkout of the reference so that the tests need none (data, not code: member names and the text a manifest pattern matched, no source lines).

  wrapper_members : every member the unchanged wrapper files (HE Wrapper/EncryptedSealBfvVector.cs, EncryptedSealBfvMatrix.cs, IFactory.cs,
                    CryptoTracker.cs) apply to the atomic classes
  cited_uses      : for every integration/SEALNET_MANIFEST.json entry with a `reference_use` ("file:line"), the entry's `reference_pattern` and
                    the text it matches on the cited line (the script fails if it matches nothing there)

    python tests/golden/make_reference_facts.py REFERENCE_CHECKOUT     # rewrites the JSON next to this file
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WRAPPER_FILES = ("EncryptedSealBfvVector.cs", "EncryptedSealBfvMatrix.cs", "IFactory.cs", "CryptoTracker.cs")
MEMBER_PATTERNS = (r"eVectors\[[a-z0-9]*\]\.([A-Za-z]+)", r"AtomicSealBfvEncryptedVector\.([A-Za-z]+)", r"Environments\[[a-z0-9]*\]\.([A-Za-z]+)",
                   r"envs\[i\]\.([A-Za-z]+)")


def wrapper_members(ref):
    found = set()
    for f in WRAPPER_FILES:
        txt = open(os.path.join(ref, "HE Wrapper", f), encoding="utf-8-sig").read()
        for p in MEMBER_PATTERNS:
            found |= set(re.findall(p, txt))
    return sorted(found)


def cited_uses(ref):
    out = {}
    for m in json.load(open(os.path.join(ROOT, "integration", "SEALNET_MANIFEST.json")))["members"]:
        if "reference_use" not in m:
            continue
        f, line = m["reference_use"].rsplit(":", 1)
        text = open(os.path.join(ref, f), encoding="utf-8-sig").read().splitlines()[int(line) - 1]
        hit = re.search(m["reference_pattern"], text)
        assert hit, (m["type"], m["member"], m["reference_use"])
        out.setdefault(m["reference_use"], {})[m["reference_pattern"]] = hit.group(0)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    facts = {"wrapper_members": wrapper_members(sys.argv[1]), "cited_uses": cited_uses(sys.argv[1])}
    with open(os.path.join(HERE, "reference_facts.json"), "w") as fh:
        json.dump(facts, fh, indent=1, sort_keys=True)
        fh.write("\n")
