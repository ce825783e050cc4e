#!/usr/bin/env python3
"""Record what the code-plane entry points refuse, and in which words: tests/golden/code_plane_refusals.json.

    python tools/make_golden_refusals.py [--lib libcodon_hip.so] [--commit REV] [--out FILE]

For each of the eleven entries of tests/code_plane_calls.py: the status and the full message of every single violation (the tool's
own refusal list and the unaligned-pointer cases) and of every pair of two, which pins the ORDER of the checks.  No GPU is needed
and none is touched: every call is refused on the host, over addresses that are never dereferenced; a call that is not refused
stops the tool.  Run it on the library of the commit whose behaviour is to be kept (--lib, --commit name it), commit the file,
and tests/test_code_plane_abi_cpu.py holds every later library to it.  The messages go through one string table."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=None, help="the library to record (default: the tree's own)")
    ap.add_argument("--commit", default="HEAD", help="the revision the library was built from, for the provenance")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "code_plane_refusals.json"))
    a = ap.parse_args(argv)
    if a.lib:
        os.environ["CODON_AMD_LIB"] = os.path.abspath(a.lib)
    from codon_amd import _lib as L
    from tests import code_plane_calls as calls
    lib = L.load()
    strings, index, entries = [], {}, {}
    for entry, violations in calls.VIOLATIONS.items():
        got = []
        for kw in calls.cases(violations):
            st, msg = calls.call(lib, entry, kw)
            if st == 0 or not msg.startswith(entry + ": "):
                raise SystemExit(f"{entry}{kw}: status {st}, {msg!r}: not a refusal of this entry")
            key = (st, msg)
            if key not in index:
                index[key] = len(strings)
                strings.append([st, msg])
            got.append(index[key])
        n = len(violations)
        entries[entry] = {"violations": violations, "single": got[:n], "pairs": got[n:]}
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", a.commit], check=True, capture_output=True, text=True).stdout.strip()
    doc = {"provenance": {"commit": commit, "library_source_hash": lib.codon_build_source_hash().decode(),
                          "abi_version": lib.codon_abi_version()},
           "strings": strings, "entries": entries}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    calls = sum(len(e["single"]) + len(e["pairs"]) for e in entries.values())
    print(f"{a.out}: {calls} calls, {len(strings)} distinct refusals, {os.path.getsize(a.out)} bytes")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
