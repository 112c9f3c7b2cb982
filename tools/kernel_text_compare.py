#!/usr/bin/env python3
"""Compare kernels of two builds of libnanopow.so instruction by instruction (CPU only).

For each kernel name given (default: the two unbounded search kernels) prints one JSON line with
tools/kernel_loop_census.py's census of the loop in each library and one with the instruction text of both,
addresses stripped: the instruction counts and every differing instruction.  A difference is "allowed" only when it
is the 32-bit pc-relative displacement to a noinline callee (the s_add_u32 / s_addc_u32 after an s_getpc_b64), i.e. an
address.  Exit status 1 if any other instruction differs.

    python tools/kernel_text_compare.py PARENT_LIB BUILD_LIB [--kernel SUBSTRING ...]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kernel_loop_census as census  # noqa: E402


def text(lib, kernel):
    with tempfile.TemporaryDirectory() as tmp:
        name, base, insts = census.disassemble(census.code_object(lib, tmp), kernel)
    out = []
    for _, op, args in insts:
        args = re.sub(r"\s+", " ", args).strip()
        args = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<label>", args)  # branch targets: compared by position below
        out.append((op + " " + args).strip())
    return name, out


def branch_free(line):
    # a branch's encoded offset moves with nothing but the code between: the label was stripped, the immediate too
    return re.sub(r"^(s_cbranch_\w+|s_branch) \d+", r"\1", line)


def pc_relative(i, a, b, lines):
    if not (a.startswith(("s_add_u32", "s_addc_u32")) and b.split(",")[:2] == a.split(",")[:2]):
        return False
    return any(ln.startswith("s_getpc_b64") for ln in lines[max(0, i - 3):i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("build")
    ap.add_argument("--kernel", action="append")
    a = ap.parse_args()
    kernels = a.kernel or ["npow_pool_kernel_ls2<false>", "npow_pool_kernel_ls2_arg<false>"]
    bad = 0
    for k in kernels:
        for arm, lib in (("parent", a.parent), ("build", a.build)):
            r = subprocess.run([sys.executable, os.path.join(HERE, "kernel_loop_census.py"), "--json", "--kernel", k,
                                "--lib", lib], check=True, capture_output=True, text=True)
            print(json.dumps({"record": "census", "arm": arm, **json.loads(r.stdout)}))
        _, p = text(a.parent, k)
        _, b = text(a.build, k)
        diff = []
        for i in range(min(len(p), len(b))):
            if branch_free(p[i]) != branch_free(b[i]):
                ok = pc_relative(i, p[i], b[i], p)
                diff.append({"index": i, "parent": p[i], "build": b[i], "pc_relative": ok})
                bad += 0 if ok else 1
        if len(p) != len(b):
            bad += 1
        print(json.dumps({"record": "instruction_text", "kernel": k, "instructions": [len(p), len(b)],
                          "differing": diff,
                          "note": "allowed: the 32-bit pc-relative displacements (s_getpc_b64 + s_add_u32) to the "
                                  "noinline callees, i.e. addresses"}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
