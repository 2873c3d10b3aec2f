"""Host side of the word order (no GPU): ``Result.by_word`` — the pure-Python
reference of ``Engine.result(order="word")`` — and the CLI's ``--sort word`` on
the host paths (CPU oracle, reference emulation, checkpointed runs).

Word order = plain bytewise order of the words, as ``sorted()`` on ``bytes``:
bytes compare unsigned, a proper prefix comes first.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import byte_cases as bc
import word_cases as wcs
from conftest import ROOT

ops = pytest.importorskip("cuda_mapreduce_amd.ops")

EXE = os.path.join(ROOT, "wordcount")
HIPCC = "/opt/rocm/bin/hipcc"


def rows_of(res):
    return list(zip(res.words, res.counts.tolist(), res.first_off.tolist()))


def hand_made(words, seed):
    rng = np.random.default_rng(seed)
    words = list(words)
    rng.shuffle(words)
    counts = rng.integers(1, 1000, len(words)).astype(np.uint64)
    first = np.cumsum([len(w) + 1 for w in words]).astype(np.uint64)
    return ops.Result(words, counts, first, int(counts.sum()) + 7)


@pytest.mark.parametrize("name,words", [("nul-ladder", wcs.NUL_LADDER), ("nul-words", wcs.NUL_WORDS),
                                        ("high-bytes", wcs.HIGH_BYTES), ("a-chain", wcs.A_CHAIN),
                                        ("all", wcs.ladders())])
def test_result_by_word_equals_sorted(name, words):
    res = hand_made(words, len(words))
    full = rows_of(res)
    got = res.by_word()
    assert got.words == sorted(words)
    assert rows_of(got) == sorted(full, key=lambda r: r[0])  # counts and first offsets travel with their words
    assert got.total == res.total
    assert got.counts.dtype == np.uint64 and got.first_off.dtype == np.uint64
    assert rows_of(res) == full  # the source table is left as it was


def test_result_by_word_known_order():
    res = ops.Result([b"ab\x01", b"ab\0\0", b"\xff", b"ab", b"\x80", b"ab\0", b"b", b"a"], np.arange(8, dtype=np.uint64),
                     np.arange(8, dtype=np.uint64) * 3, 99)
    got = res.by_word()
    assert got.words == [b"a", b"ab", b"ab\0", b"ab\0\0", b"ab\x01", b"b", b"\x80", b"\xff"]
    assert got.counts.tolist() == [7, 3, 5, 1, 0, 6, 4, 2]
    assert got.first_off.tolist() == [21, 9, 15, 3, 0, 18, 12, 6]
    assert got.total == 99
    empty = ops.Result().by_word()
    assert len(empty) == 0 and empty.total == 0


def test_word_order_symbols_exported():
    lib = ctypes.CDLL(ops.LIB_PATH)
    for name in ("wc_engine_result_by_word", "wc_debug_word_order"):
        assert hasattr(lib, name), f"{name} is not exported by libwc.so"


def test_engine_result_rejects_unknown_order():
    """The order is checked before the engine is touched."""
    e = object.__new__(ops.Engine)
    e._p = None
    with pytest.raises(ValueError):
        ops.Engine.result(e, order="count")


def cli(args, cwd, ok=True):
    out = subprocess.run([EXE, *args], cwd=cwd, capture_output=True, timeout=120)
    if ok:
        assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out


@pytest.fixture(scope="module")
def ladder_text():
    return bc.family_text(5, 20_000) + b" " + b" ".join(wcs.ladders() + wcs.ladders()[::3]) + b"\n"


def test_cli_cpu_sort_word(tmp_path, ladder_text):
    (tmp_path / "t.txt").write_bytes(ladder_text)
    want = ops.cpu_count(ladder_text)
    got = cli(["t.txt", "--cpu", "--no-echo", "--sort", "word"], tmp_path).stdout
    assert got == ops.format_output(want.by_word())
    assert want.by_word().words == sorted(bc.py_table(ladder_text)[0])
    # the default order, spelled out, is today's output
    plain = cli(["t.txt", "--cpu", "--no-echo"], tmp_path).stdout
    assert cli(["t.txt", "--cpu", "--no-echo", "--sort", "first"], tmp_path).stdout == plain
    assert plain == ops.format_output(want)
    # nothing is listed: nothing to sort
    assert cli(["t.txt", "--cpu", "--no-echo", "--no-list", "--sort", "word"], tmp_path).stdout == \
        ops.format_output(want, list_rows=False)


def test_cli_compat_sort_word(tmp_path, golden_text):
    (tmp_path / "test.txt").write_bytes(golden_text)
    got = cli(["--compat=reference", "--no-echo", "--sort", "word"], tmp_path).stdout
    assert got == ops.format_output(ops.cpu_count_compat(golden_text).by_word())
    assert got == (b"Input Data:\n" + b"-" * 26 + b"\nEveryOne\t1\nGood\t2\nHello\t2\nMorning\t1\nNews\t1\nWorld\t2\n" +
                   b"-" * 26 + b"\nTotal Count:9\n")
    # with the echo, the framing around the rows is unchanged
    echoed = cli(["--compat=reference", "--sort", "word"], tmp_path).stdout
    first = cli(["--compat=reference"], tmp_path).stdout
    assert echoed.split(b"-" * 26)[0] == first.split(b"-" * 26)[0]
    assert echoed.split(b"-" * 26)[1:] == got.split(b"-" * 26)[1:]


def test_cli_checkpointed_sort_word(tmp_path, ladder_text):
    (tmp_path / "t.txt").write_bytes(ladder_text)
    want = cli(["t.txt", "--cpu", "--no-echo", "--sort", "word"], tmp_path).stdout
    got = cli(["t.txt", "--cpu", "--no-echo", "--sort", "word", "--checkpoint", "ck.bin", "--checkpoint-every", "3000"],
              tmp_path).stdout
    assert got == want


def test_cli_rejects_sort_word_with_top(tmp_path, golden_text):
    (tmp_path / "test.txt").write_bytes(golden_text)
    out = cli(["--cpu", "--sort", "word", "--top", "3"], tmp_path, ok=False)
    assert out.returncode != 0 and out.stdout == b""
    assert b"--sort word cannot be combined with --top" in out.stderr
    # --top 0 lists everything: allowed
    assert cli(["--cpu", "--no-echo", "--sort", "word", "--top", "0"], tmp_path).stdout == \
        cli(["--cpu", "--no-echo", "--sort", "word"], tmp_path).stdout


def test_cli_rejects_unknown_sort(tmp_path, golden_text):
    (tmp_path / "test.txt").write_bytes(golden_text)
    out = cli(["--cpu", "--sort", "bogus"], tmp_path, ok=False)
    assert out.returncode != 0 and out.stdout == b""
    assert b"--sort expects first or word, got bogus" in out.stderr
    bogus_merge = cli(["--cpu", "--merge", "bogus"], tmp_path, ok=False)
    assert bogus_merge.returncode == out.returncode


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="hipcc not installed")
def test_word_order_kernels_use_no_scratch(tmp_path):
    """Every ``wc_word_*`` kernel keeps its per-lane state (the compaction's
    flags and slots of four rounds) in registers: the compiler's resource
    report for gfx950 shows no scratch."""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    out = subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
         "-I" + os.path.join(ROOT, "src"), "-I/opt/rocm/include", "-c",
         os.path.join(ROOT, "src", "kernels", "wordorder.hip"), "-o", str(tmp_path / "wordorder.o"),
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
        if m and name and "wc_word_" in name:
            found[name] = int(m.group(1))
    assert len(found) >= 9, f"expected every wc_word kernel in the resource report, got {sorted(found)}"
    assert all(v == 0 for v in found.values()), f"wc_word kernels spill to scratch: {found}"
