"""Differential test against the reference program itself.

The reference is a CUDA program and cannot be compiled for a GPU here, so
`tools/record_reference_golden.py` builds a HOST EMULATION of it (a shim
`cuda_runtime.h` on host memory, the two `<<< >>>` launches rewritten into
serial loops over the grid: exact, as mapKernel threads write disjoint records
and reduceKernel works on thread 0 only) and records, in
`tests/golden/reference_diff.json`, the bytes it writes to stdout for each of
this module's inputs.  Nothing of the reference is copied into this
repository; the golden file holds inputs and recorded output only, so the test
runs wherever the repository does.

Random inputs were drawn (fixed seeds) inside the reference's safe envelope
(<= 9 lines, <= 20 tokens per line, tokens <= 19 bytes, <= 10 distinct words,
trailing LF) and the emulated reference's stdout is compared byte for byte with
  * `wordcount --compat=reference` (quirks mode: prefix compare, fgets records),
  * `wordcount --cpu` (clean semantics) when no word is a prefix of another
    and the input has single spaces only — where the two semantics coincide.
"""
import json
import os
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "wordcount")


@pytest.fixture(scope="module")
def ref_cases():
    """Test name -> [(input text, the reference's stdout, row)], all bytes."""
    with open(os.path.join(ROOT, "tests", "golden", "reference_diff.json")) as f:
        golden = json.load(f)
    return {name: [(r["input"].encode("latin-1"), r["stdout"].encode("latin-1"), r) for r in rows]
            for name, rows in golden.items()}


def run_in(cwd, argv, text):
    with open(os.path.join(cwd, "test.txt"), "wb") as f:
        f.write(text)
    out = subprocess.run(argv, cwd=cwd, capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_golden_matches_reference(ref_cases, tmp_path, golden_text):
    (text, want, _), = ref_cases["golden"]
    assert text == golden_text
    assert run_in(tmp_path, [EXE, "--cpu"], golden_text) == want
    assert run_in(tmp_path, [EXE, "--compat=reference"], golden_text) == want


def test_compat_mode_matches_reference_with_prefix_words(ref_cases, tmp_path):
    """Prefix words ('Go' / 'Good'), TABs and CRLF exercise the reference's quirks."""
    cases = ref_cases["prefix_words"]
    assert len(cases) == 40 and any(b"\r\n" in t for t, _, _ in cases)
    for t, want, _ in cases:
        assert run_in(tmp_path, [EXE, "--compat=reference"], t) == want, t


def test_clean_mode_matches_reference_inside_envelope(ref_cases, tmp_path):
    cases = ref_cases["clean_envelope"]
    assert len(cases) == 40
    for t, want, _ in cases:
        assert run_in(tmp_path, [EXE, "--cpu"], t) == want, t


def test_compat_mode_echo_stops_at_blank_line(ref_cases, tmp_path):
    """A blank line ends the reference's input: the echo stops there too."""
    cases = ref_cases["blank_line"]
    assert len(cases) == 20
    for t, want, row in cases:
        head, tail = row["head"].encode("latin-1"), row["tail"].encode("latin-1")
        assert t == head + b"\n" + tail  # the blank line hides `tail` from the reference
        got = run_in(tmp_path, [EXE, "--compat=reference"], t)
        assert got == want, t
        assert tail not in got.split(b"-" * 26)[0][len(b"Input Data:\n") + len(head):]
