#!/usr/bin/env python3
"""Records what a library answers to the table of tests/_list_checks.py: (status, bad_index, ore_last_error(NULL)) per
case, into tests/golden/list_check_messages.json.  The recording pins the order of the image-list checks' rules and
the text of their messages, so it is made by the library whose behaviour is to be KEPT: run this with ORE_LIB pointing
at a libore.so built from the commit before a change to the checks, never at the changed one.  Host only, no GPU.
usage: ORE_LIB=/path/to/parent/libore.so python tools/record_list_checks.py [--out FILE]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "onnx-rusty-inference-engine_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "list_check_messages.json"))
    a = ap.parse_args()
    if not os.environ.get("ORE_LIB"):
        sys.exit("record_list_checks.py: set ORE_LIB to the library whose answers are to be recorded")
    import ore
    from _list_checks import cases
    L = ore.load()
    rec = {name: call(L) for name, call in cases()}
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in rec.items()) + "\n}\n")
    print(f"{len(rec)} cases from {os.environ['ORE_LIB']} -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
