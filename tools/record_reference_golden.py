#!/usr/bin/env python3
"""Records tests/golden/reference_diff.json: what the reference program prints
for the inputs of tests/test_reference_diff.py.

    python tools/record_reference_golden.py PATH/TO/main.cu

The reference is a CUDA program and cannot be compiled for a GPU here, so this
builds a HOST EMULATION of it in a temp dir: a shim `cuda_runtime.h` maps
cudaMalloc/Memcpy/Memset/Free to host memory (calloc = the zero-filled device
memory the reference relies on) and the two `<<< >>>`
launch lines are rewritten into loops running every thread of the grid
serially (exact: mapKernel threads write disjoint records and reduceKernel
works on thread 0 only).  Nothing of the reference is copied into this
repository: the golden file holds the test inputs (drawn here, inside the
reference's safe envelope: <= 9 lines, <= 20 tokens per line, tokens <= 19
bytes, <= 10 distinct words, trailing LF) and the bytes the emulated reference
wrote to stdout for each.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_diff.json")

SHIM = r"""
#pragma once
#include <cstdlib>
#include <cstring>
#define __global__
#define __device__
#define __host__
typedef int cudaError_t;
enum cudaMemcpyKind { cudaMemcpyHostToDevice = 1, cudaMemcpyDeviceToHost = 2 };
template <class T> inline cudaError_t cudaMalloc(T** p, size_t n) { *p = (T*)calloc(1, n); return 0; }
inline cudaError_t cudaFree(void* p) { free(p); return 0; }
inline cudaError_t cudaMemcpy(void* d, const void* s, size_t n, cudaMemcpyKind) { memcpy(d, s, n); return 0; }
inline cudaError_t cudaMemset(void* p, int v, size_t n) { memset(p, v, n); return 0; }
struct wc_dim { unsigned x; };
static wc_dim threadIdx, blockIdx, blockDim, gridDim;
#define WC_LAUNCH(kernel, g, b, ...)                                         \
  for (unsigned wc_b = 0; wc_b < (unsigned)(g); ++wc_b)                     \
    for (unsigned wc_t = 0; wc_t < (unsigned)(b); ++wc_t) {                 \
      blockIdx.x = wc_b; threadIdx.x = wc_t; blockDim.x = (b); gridDim.x = (g); \
      kernel(__VA_ARGS__);                                                  \
    }
"""


def build_emulation(ref_src: str, d: str) -> str:
    src = open(ref_src, encoding="latin-1").read()
    src, n = re.subn(r"(\w+)\s*<<\s*<\s*(\w+)\s*,\s*(\w+)\s*>>\s*>\s*\((.*?)\);", r"WC_LAUNCH(\1, \2, \3, \4);", src)
    assert n == 2, "expected the two kernel launches of the reference"
    with open(os.path.join(d, "cuda_runtime.h"), "w") as f:
        f.write(SHIM)
    with open(os.path.join(d, "main.cpp"), "w", encoding="latin-1") as f:
        f.write(src)
    exe = os.path.join(d, "ref")
    subprocess.run(["g++", "-O1", "-w", "-I", d, "-o", exe, os.path.join(d, "main.cpp")], check=True, timeout=120)
    return exe


def envelope_text(rng, vocab, max_lines=9, max_words=6):
    lines = []
    for _ in range(int(rng.integers(1, max_lines + 1))):
        words = [vocab[i] for i in rng.integers(0, len(vocab), int(rng.integers(1, max_words + 1)))]
        lines.append(b" ".join(words) + b"\n")
    return b"".join(lines)


def inputs():
    """Test name -> its input texts (fixed seeds)."""
    out = {}
    with open(os.path.join(ROOT, "tests", "data", "test.txt"), "rb") as f:
        out["golden"] = [f.read()]

    # prefix words ('Go' / 'Good'), TABs and CRLF exercise the reference's quirks
    rng = np.random.default_rng(7)
    vocab = [b"Go", b"Good", b"a", b"ab", b"abc", b"b\tc", b"x", b"Hello", b"hello,", b"W"]
    out["prefix_words"] = []
    for _ in range(40):
        t = envelope_text(rng, vocab)
        if rng.integers(0, 4) == 0:
            t = t.replace(b"\n", b"\r\n")
        out["prefix_words"].append(t)

    # no word a prefix of another, single spaces: clean and reference semantics coincide
    rng = np.random.default_rng(11)
    vocab = [b"alpha", b"beta", b"gamma", b"delta", b"eps", b"zeta", b"Eta", b"theta,", b"iota!", b"kappa\t1"]
    out["clean_envelope"] = [envelope_text(rng, vocab) for _ in range(40)]

    # a blank line ends the reference's input: head + blank line + tail
    rng = np.random.default_rng(23)
    vocab = [b"one", b"two", b"three", b"four", b"Go", b"Good"]
    out["blank_line"] = []
    for _ in range(20):
        head = envelope_text(rng, vocab, max_lines=4)
        tail = envelope_text(rng, vocab, max_lines=4)
        out["blank_line"].append((head, tail))
    return out


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    with tempfile.TemporaryDirectory() as d:
        exe = build_emulation(sys.argv[1], d)

        def ref(text: bytes) -> str:
            with open(os.path.join(d, "test.txt"), "wb") as f:
                f.write(text)
            p = subprocess.run([exe], cwd=d, capture_output=True, timeout=60, check=True)
            return p.stdout.decode("latin-1")

        golden = {}
        for name, texts in inputs().items():
            rows = []
            for t in texts:
                row = {}
                if isinstance(t, tuple):
                    row["head"], row["tail"] = (x.decode("latin-1") for x in t)
                    t = t[0] + b"\n" + t[1]
                row["input"] = t.decode("latin-1")
                row["stdout"] = ref(t)
                rows.append(row)
            golden[name] = rows
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {sum(len(v) for v in golden.values())} cases")
    return 0


if __name__ == "__main__":
    sys.exit(main())
