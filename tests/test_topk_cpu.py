"""Host side of the top-K selection (no GPU): ``Result.top`` — the pure-Python
reference of ``Engine.top_k`` — and the C ABI's entry points.

Top K of a table = the min(K, n) rows first under (count descending, row
position ascending), in that order, with the whole table's ``total``.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

ops = pytest.importorskip("cuda_mapreduce_amd.ops")

HIPCC = "/opt/rocm/bin/hipcc"


def hand_made():
    words = [b"a", b"b", b"c", b"d", b"e", b"f"]
    counts = np.array([3, 5, 3, 1, 5, 3], np.uint64)
    first = np.array([0, 2, 4, 6, 8, 10], np.uint64)
    return ops.Result(words, counts, first, int(counts.sum()))


def rows_of(res):
    return list(zip(res.words, res.counts.tolist(), res.first_off.tolist()))


def test_result_top_hand_made():
    res = hand_made()
    full = rows_of(res)
    top4 = res.top(4)
    assert rows_of(top4) == [full[i] for i in (1, 4, 0, 2)]
    assert top4.total == res.total == 20
    assert top4.counts.dtype == np.uint64 and top4.first_off.dtype == np.uint64
    top0 = res.top(0)
    assert len(top0) == 0 and top0.total == 20
    by_count = [full[i] for i in (1, 4, 0, 2, 5, 3)]
    assert rows_of(res.top(6)) == by_count
    assert rows_of(res.top(99)) == by_count
    assert res.top(99).total == 20
    assert rows_of(res) == full  # the source table is left as it was


def test_result_top_matches_format_output():
    text = ops.synth_host(64 << 10, seed=4, vocab=500)
    res = ops.cpu_count(text)
    n = len(res)
    assert n > 100
    head = b"Input Data:\n" + b"-" * 26 + b"\n"
    for k in range(1, n):
        out = ops.format_output(res, top_k=k)
        assert out.startswith(head)
        listed = out[len(head):].split(b"-" * 26)[0].split(b"\n")[:-1]
        top = res.top(k)
        assert listed == [w + b"\t" + str(c).encode() for w, c in top.rows()], k
        assert top.total == res.total


def test_top_k_symbols_exported():
    lib = ctypes.CDLL(ops.LIB_PATH)
    for name in ("wc_engine_top_k", "wc_debug_top_k"):
        assert hasattr(lib, name), f"{name} is not exported by libwc.so"


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")
def test_topk_kernels_use_no_scratch(tmp_path):
    """Every ``wc_topk_*`` kernel keeps its per-lane arrays (the pick's bins, the
    compaction's 16 counts) in registers: the compiler's resource report for
    gfx950 shows no scratch."""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
         "-I" + os.path.join(ROOT, "src"), "-I/opt/rocm/include", "-c",
         os.path.join(ROOT, "src", "kernels", "topk.hip"), "-o", str(tmp_path / "topk.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    name, found = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "wc_topk_" in name:
            found[name] = int(m.group(1))
    assert len(found) >= 12, f"expected every wc_topk kernel in the resource report, got {sorted(found)}"
    assert all(v == 0 for v in found.values()), f"wc_topk kernels spill to scratch: {found}"
