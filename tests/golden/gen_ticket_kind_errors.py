#!/usr/bin/env python3
"""Record tests/golden/ticket_kind_errors.json: the return code and npow_last_error() message of each of the 13 ticket
calls on a search's, a sweep job's and a best job's ticket, from the libnanopow.so that is built in the tree (needs
an MI355X).  The calls, their arguments and their order are those of tests/test_gpu_ticket_kinds.py (calls()), which
compares a build against this file: record it at the commit whose behaviour is to be kept.

Usage:
  python3 tests/golden/gen_ticket_kind_errors.py [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
import conftest  # noqa: E402,F401  (the tests' import paths)
import nanopow  # noqa: E402
import test_gpu_ticket_kinds as kinds  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ticket_kind_errors.json")
    got, _ = kinds.calls(nanopow.engine())
    doc = {"about": "return code and npow_last_error() of every ticket call on a ticket of every kind "
                    "(tests/golden/gen_ticket_kind_errors.py; tests/test_gpu_ticket_kinds.py)",
           "version": nanopow.engine().version(),
           "kinds": {k: {c: got[k][c] for c in kinds.CALLS} for k in kinds.KINDS}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["kinds"]))


if __name__ == "__main__":
    main()
