"""Best jobs leave the search kernels' hot paths as they were (CPU test, no GPU).

The best entry's code lives in the rare `hits != 0` branch of the BOUNDED pool kernels only.  This reads the gfx950
code object inside the built libnanopow.so with the project's own tools (tests/test_kernel_resources.py's metadata
reader, tools/kernel_loop_census.py, tools/kernel_text_compare.py) and compares with the figures recorded from the
commit before best jobs (tests/golden/best_kernel_census.json):

* the unbounded search kernels (npow_pool_kernel_ls2<false>, npow_pool_kernel_ls2_arg<false>) are instruction for
  instruction that commit's: the same number of instructions and the same digest of their text, addresses and the
  pc-relative displacements to the noinline callees left out (what kernel_text_compare.py allows to differ);
* the BOUNDED kernels keep at most 64 VGPRs, no AGPRs and no scratch: 8 waves per SIMD;
* the hash loop of the BOUNDED kernels -- the per-iteration path; the rare branches lie outside it -- has no more
  VALU, vector-memory, scalar-memory or LDS instructions than that commit's.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_kernel_resources import LIB, LLVM, kernel_metadata

sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_text_compare as ktc  # noqa: E402

UNBOUNDED = ("npow_pool_kernel_ls2<false>", "npow_pool_kernel_ls2_arg<false>")
BOUNDED = ("npow_pool_kernel_ls2<true>", "npow_pool_kernel_ls2_arg<true>")
PER_ITERATION = ("valu", "vmem", "smem", "lds")

pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(f"{LLVM}/clang-offload-bundler")),
                                reason="libnanopow.so not built or no ROCm LLVM tools")


def census(lib, kernel):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_loop_census.py"), "--json", "--kernel",
                        kernel, "--lib", lib], check=True, capture_output=True, text=True)
    return json.loads(r.stdout)


def text_digest(lib, kernel):
    """(instructions, sha256 of the kernel's instruction text) with what may differ between two builds of unchanged
    source left out: branch offsets and the displacements to noinline callees (kernel_text_compare.py's rule)."""
    _, lines = ktc.text(lib, kernel)
    out = []
    for i, ln in enumerate(lines):
        ln = ktc.branch_free(ln)
        if ktc.pc_relative(i, ln, ln, lines):
            ln = ",".join(ln.split(",")[:2])
        out.append(ln)
    return len(out), hashlib.sha256("\n".join(out).encode()).hexdigest()


def record(lib):
    """The golden file's content for a library (how tests/golden/best_kernel_census.json was made)."""
    out = {"unbounded": {}, "bounded_loop": {}}
    for k in UNBOUNDED:
        n, d = text_digest(lib, k)
        out["unbounded"][k] = {"instructions": n, "sha256": d}
    for k in BOUNDED:
        out["bounded_loop"][k] = census(lib, k)["by_class"]
    return out


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "best_kernel_census.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("kernel", UNBOUNDED)
def test_unbounded_search_kernels_are_the_parents(parent, kernel):
    n, digest = text_digest(LIB, kernel)
    assert (n, digest) == (parent["unbounded"][kernel]["instructions"], parent["unbounded"][kernel]["sha256"])


def test_bounded_kernels_fit_eight_waves_per_simd_without_scratch(tmp_path):
    kernels = {n: m for n, m in kernel_metadata(tmp_path).items() if "npow_pool_kernel_ls2" in n and "Lb1E" in n}
    assert len(kernels) == 2, sorted(kernels)
    for name, m in kernels.items():
        assert m["vgpr_count"] <= 64 and m["agpr_count"] == 0, (name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)


@pytest.mark.parametrize("kernel", BOUNDED)
def test_bounded_hash_loop_gains_no_valu_and_no_memory_instruction(parent, kernel):
    got = census(LIB, kernel)["by_class"]
    print(json.dumps({"kernel": kernel, "loop": got, "parent": parent["bounded_loop"][kernel]}))
    assert got["s_barrier"] == 1 and got["s_setprio"] == parent["bounded_loop"][kernel]["s_setprio"]  # the hash loop
    for c in PER_ITERATION:
        assert got.get(c, 0) <= parent["bounded_loop"][kernel].get(c, 0), (c, got, parent["bounded_loop"][kernel])


def test_the_best_entry_is_read_in_the_rare_branch_only():
    """The flag is tested where the collecting entry's flags are re-read (ls2_collect), not in the loop."""
    src = open(os.path.join(ROOT, "nano-dpow_amd", "csrc", "npow_kernel.hip")).read()
    assert src.count("kEntryBest") >= 2 and "c.bounded & kEntryBest" not in src
    assert "if (flags & kEntryBest) return ls2_best(" in src
