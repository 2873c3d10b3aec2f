"""The byte map on the host: the builder's tables, the validity check, the CPU
twin of the mapped count and the CLI flags (no GPU needed; the same map on the
GPU paths: test_gpu_byte_map.py).

The reference of every count is byte_cases.py py_table of
``text.translate(M)`` — pure Python, it knows nothing of the engine."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import byte_cases as bc
from conftest import ROOT

ops = pytest.importorskip("cuda_mapreduce_amd.ops")

from cuda_mapreduce_amd.ops._lib import WcError, lib  # noqa: E402

EXE = os.path.join(ROOT, "wordcount")
PUNCT = set(range(0x21, 0x30)) | set(range(0x3A, 0x41)) | set(range(0x5B, 0x61)) | set(range(0x7B, 0x7F))
FLAG_SETS = [dict(), dict(fold_case=True), dict(split_punct=True), dict(split=b"\t;a\x80\xff"),
             dict(fold_case=True, split_punct=True), dict(fold_case=True, split=b"\t;a\x80\xff", split_punct=True)]


def expected_entry(b, fold_case=False, split=b"", split_punct=False):
    """What byte b maps to, from the flags' descriptions alone."""
    if b in bc.DELIMS:
        return b
    if fold_case and ord("A") <= b <= ord("Z"):
        b += 32  # then split like the lower-case letter it now is
    if b in split or (split_punct and b in PUNCT):
        return 0x20
    return b


def native_map(fold_case=False, split=b"", split_punct=False):
    out = (ctypes.c_uint8 * 256)()
    buf = (ctypes.c_uint8 * max(len(split), 1)).from_buffer_copy(split or b"\0")
    assert lib.wc_byte_map_build(int(fold_case), buf, len(split), int(split_punct), out) == 0
    return bytes(out)


@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "+".join(sorted(f)) or "identity")
def test_builder_tables(flags):
    m = ops.byte_map(**flags)
    assert isinstance(m, bytes) and len(m) == 256
    for b in range(256):
        assert m[b] == expected_entry(b, **flags), hex(b)
    ops.check_byte_map(m)  # valid by construction
    assert native_map(**flags) == m  # the native builder is its twin


def test_builder_details():
    assert ops.byte_map() == bytes(range(256))
    fold = ops.byte_map(fold_case=True)
    assert fold[ord("A")] == ord("a") and fold[ord("Z")] == ord("z") and fold[ord("@")] == ord("@")
    assert fold[ord("[")] == ord("[") and fold[0xC0] == 0xC0 and fold[0xDE] == 0xDE  # ASCII only
    punct = ops.byte_map(split_punct=True)
    assert [b for b in range(256) if punct[b] != b] == sorted(PUNCT)
    assert all(punct[b] == 0x20 for b in PUNCT) and punct[0x7F] == 0x7F and punct[ord("0")] == ord("0")
    # listing a delimiter changes nothing; a split lower-case letter takes its capital with it under the fold
    assert ops.byte_map(split=b" \r\n") == bytes(range(256))
    m = ops.byte_map(fold_case=True, split=b"q")
    assert m[ord("q")] == 0x20 and m[ord("Q")] == 0x20
    ops.check_byte_map(m)


def test_validator_rejects_and_names_the_byte():
    moved = bytearray(range(256))
    moved[0x0A] = ord("x")
    with pytest.raises(WcError, match="0x0A"):
        ops.check_byte_map(bytes(moved))
    for d in (0x20, 0x0D):
        moved = bytearray(range(256))
        moved[d] = 0x0A
        with pytest.raises(WcError, match="0x%02X" % d):
            ops.check_byte_map(bytes(moved))
    chain = bytearray(range(256))
    chain[ord("a")], chain[ord("b")] = ord("b"), ord("c")
    with pytest.raises(WcError, match="idempotent.*0x61"):
        ops.check_byte_map(bytes(chain))
    with pytest.raises(WcError, match="0x61"):
        ops.cpu_count(b"a b c", byte_map=bytes(chain))
    short = bytes(range(255))
    for call in (lambda: ops.check_byte_map(short), lambda: ops.cpu_count(b"a", byte_map=short),
                 lambda: ops.default_options(byte_map=short), lambda: ops.default_options(byte_map="x" * 256)):
        with pytest.raises(ValueError, match="256"):
            call()


def test_options_carry_the_map():
    o = ops.default_options()
    assert bytes(o.byte_map) == bytes(range(256)) and o.byte_map_on == 0
    m = ops.byte_map(fold_case=True, split_punct=True)
    o = ops.default_options(byte_map=m, chunk_bytes=1 << 20)
    assert bytes(o.byte_map) == m and o.byte_map_on == 1 and o.chunk_bytes == 1 << 20


@pytest.mark.parametrize("flags", FLAG_SETS[1:], ids=lambda f: "+".join(sorted(f)))
@pytest.mark.parametrize("p", [1 / 3, 1 / 40])
def test_cpu_count_all_bytes(flags, p):
    text = bc.random_bytes_text(21, 200_000, p)
    assert len(set(text)) == 256
    m = ops.byte_map(**flags)
    for base in (0, 2**40 + 7):
        bc.assert_table(ops.cpu_count(text, base, byte_map=m), bc.py_table(text.translate(m), base))
    bc.assert_table(ops.cpu_count(text), bc.py_table(text))  # no map: as before
    bc.assert_table(ops.cpu_count(text, byte_map=bytes(range(256))), bc.py_table(text))


COLLAPSE = b"  Word other word, x WORD.\r\n(word) other tab\tbed tail"


def test_variants_collapse_to_one_key():
    m = ops.byte_map(fold_case=True, split_punct=True)
    got = ops.cpu_count(COLLAPSE, 1000, byte_map=m)
    want = bc.py_table(COLLAPSE.translate(m), 1000)
    bc.assert_table(got, want)
    i = got.words.index(b"word")
    assert int(got.counts[i]) == 4 and int(got.first_off[i]) == 1000 + COLLAPSE.index(b"Word")
    assert b"Word" not in got.words and b"word," not in got.words
    top = got.top(2)
    assert top.words == [b"word", b"other"] and top.counts.tolist() == [4, 2] and top.total == got.total
    order = sorted(range(len(want[0])), key=lambda j: (-want[1][j], j))[:2]
    assert top.first_off.tolist() == [want[2][j] for j in order]
    by = got.by_word()
    order = sorted(range(len(want[0])), key=want[0].__getitem__)
    assert by.words == [want[0][j] for j in order] and by.words == sorted(want[0])
    assert by.counts.tolist() == [want[1][j] for j in order] and by.first_off.tolist() == [want[2][j] for j in order]


def run_cli(args, cwd):
    return subprocess.run([EXE] + args, cwd=cwd, capture_output=True, timeout=60)


def oracle_output(text, m, **kw):
    words, counts, first = bc.py_table(text.translate(m))
    res = ops.Result(words, np.array(counts, np.uint64), np.array(first, np.uint64), sum(counts))
    return ops.format_output(res, **kw)


def test_cli_cpu_flags(tmp_path):
    text = COLLAPSE + b"\n" + bc.random_bytes_text(22, 50_000, 1 / 6)
    (tmp_path / "in.txt").write_bytes(text)
    out = run_cli(["in.txt", "--cpu", "--fold-case", "--split-punct", "--no-echo"], tmp_path)
    assert out.returncode == 0, out.stderr
    assert out.stdout == oracle_output(text, ops.byte_map(fold_case=True, split_punct=True))
    # the echo is the raw input
    out = run_cli(["in.txt", "--cpu", "--fold-case"], tmp_path)
    assert out.returncode == 0 and out.stdout == oracle_output(text, ops.byte_map(fold_case=True), echo=text)
    # --split reads C escapes and combines with the other flags and with itself
    for args, split in ((["--split", "\\t;"], b"\t;"), (["--split", "\\x41\\\\", "--split", "z\\n"], b"A\\z"),
                        (["--split", "\\xfF\\0"], b"\xff\x00")):
        out = run_cli(["in.txt", "--cpu", "--no-echo"] + args, tmp_path)
        assert out.returncode == 0, out.stderr
        assert out.stdout == oracle_output(text, ops.byte_map(split=split)), args
    out = run_cli(["in.txt", "--cpu", "--no-echo", "--split", ".", "--fold-case", "--sort", "word"], tmp_path)
    m = ops.byte_map(fold_case=True, split=b".")
    assert out.returncode == 0 and out.stdout == ops.format_output(ops.cpu_count(text, byte_map=m).by_word())


@pytest.mark.parametrize("args,word", [(["--fold-case", "--compat=reference"], b"--compat=reference"),
                                        (["--split-punct", "--compat=reference"], b"--compat=reference"),
                                        (["--fold-case", "--checkpoint", "ck"], b"--checkpoint"),
                                        (["--cpu", "--split", ",", "--checkpoint", "ck"], b"--checkpoint"),
                                        (["--cpu", "--split", "\\q"], b"escape"),
                                        (["--cpu", "--split", "\\x4"], b"hex")])
def test_cli_rejects(tmp_path, args, word):
    (tmp_path / "in.txt").write_bytes(COLLAPSE)
    out = run_cli(["in.txt"] + args, tmp_path)
    assert out.returncode == 1 and out.stdout == b""
    assert word in out.stderr and out.stderr.startswith(b"wordcount: ")
    assert not (tmp_path / "ck").exists()


HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_translate_kernel_uses_no_scratch(tmp_path):
    """The compiler's resource report of wc_translate for gfx950: a streaming
    kernel with a 256-byte LDS table has no reason to touch scratch."""
    import re

    out = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
         "-I" + os.path.join(ROOT, "src"), "-I/opt/rocm/include", "-c",
         os.path.join(ROOT, "src", "kernels", "translate.hip"), "-o", str(tmp_path / "translate.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    report = out.stderr[out.stderr.index("wc_translate"):]
    assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", report).group(1)) == 0
    assert int(re.search(r"VGPRs Spill: (\d+)", report).group(1)) == 0
    assert int(re.search(r"LDS Size \[bytes/block\]: (\d+)", report).group(1)) == 256


def test_distributed_cpu_rank_translates_on_the_host(tmp_path):
    from cuda_mapreduce_amd.parallel.dist import DistEnv, DistributedWordCount

    m = ops.byte_map(fold_case=True, split_punct=True)
    text = COLLAPSE + b"\n" + bc.random_bytes_text(23, 30_000, 1 / 6)
    want = bc.py_table(text.translate(m))
    job = DistributedWordCount(DistEnv(), use_gpu=False, byte_map=m)
    bc.assert_table(job.count_bytes(text), want)
    p = tmp_path / "in.bin"
    p.write_bytes(text)
    bc.assert_table(job.count_file(str(p)), want)
    with pytest.raises(ValueError, match="checkpoint"):
        job.count_file(str(p), checkpoint=str(tmp_path / "ck"))
    job.close()
