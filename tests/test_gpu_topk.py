"""Top-K selection on the GPU (src/kernels/topk.hip, ``Engine.top_k``, ``--top``).

Top K = the min(K, n) rows first under (count descending, row position
ascending), in that order, with the whole table's total.  The kernel hook is
checked against a stable argsort; the engine against ``Result.top`` of the CPU
oracle (exact words, counts, first offsets and total).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ops = pytest.importorskip("cuda_mapreduce_amd.ops")

U64_MAX = np.uint64(2**64 - 1)
SIZES = [1, 2, 63, 64, 65, 1023, 1025, 4097, 100_000, 1_000_003]
DISTS = ["equal", "zipf", "two", "wide", "ascending", "descending"]
TWO_T = 7  # the two-valued column: T and T + 1 interleaved


def make_counts(dist, n):
    rng = np.random.default_rng(1000 + n)
    if dist == "equal":
        return np.full(n, 5, np.uint64)
    if dist == "zipf":  # a few large counts, then runs of equal small ones; three quarters of the rows are 1
        c = np.maximum(1, max(n // 8, 1) // np.arange(1, n + 1)).astype(np.uint64)
        rng.shuffle(c)
        return c
    if dist == "two":
        c = np.full(n, TWO_T, np.uint64)
        c[1::2] += np.uint64(1)
        return c
    if dist == "wide":
        c = rng.integers(1, 2**40, n, dtype=np.uint64)
        planted = np.array([2**32 - 1, 2**32, 2**32 + 1, 2**48], np.uint64)[:n]
        c[rng.choice(n, len(planted), replace=False)] = planted
        return c
    if dist == "ascending":
        return np.arange(1, n + 1, dtype=np.uint64)
    if dist == "descending":
        return np.arange(n, 0, -1).astype(np.uint64)
    raise AssertionError(dist)


def ks_for(dist, n, counts):
    ks = {1, 2, 20, 64, 65, 1000, n - 1, n, n + 5}
    if dist == "zipf":
        ks.add(n // 2)  # inside the run of ones
    if dist == "two":
        n_gt = int((counts > np.uint64(TWO_T)).sum())
        ks |= {n_gt - 1, n_gt, n_gt + 1}
    return sorted(k for k in ks if k > 0)


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("n", SIZES)
def test_kernel_hook(n, dist):
    counts = make_counts(dist, n)
    order = np.argsort(U64_MAX - counts, kind="stable")
    total = int(counts.sum(dtype=np.uint64))
    for k in ks_for(dist, n, counts):
        rows, s = ops.debug_top_k(counts, k)
        assert len(rows) == min(k, n), (n, dist, k)
        assert np.array_equal(rows, order[:k].astype(np.uint32)), (n, dist, k)
        assert s == total, (n, dist, k)


def test_kernel_hook_k_zero():
    counts = make_counts("wide", 4097)
    rows, s = ops.debug_top_k(counts, 0)
    assert len(rows) == 0
    assert s == int(counts.sum(dtype=np.uint64))


def test_kernel_hook_full_width_counts():
    """Counts that differ only in their lowest bits under a set top bit: every
    refinement pass of the threshold search runs."""
    rng = np.random.default_rng(9)
    counts = (np.uint64(1) << np.uint64(63)) + rng.integers(0, 3000, 5000, dtype=np.uint64)
    order = np.argsort(U64_MAX - counts, kind="stable")
    for k in (1, 700, 2500, 5000):
        rows, s = ops.debug_top_k(counts, k)
        assert np.array_equal(rows, order[:k].astype(np.uint32)), k
        assert s == int(counts.sum(dtype=np.uint64))


def assert_same(got, want):
    assert got.total == want.total
    assert len(got) == len(want)
    assert got.words == want.words
    assert np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.first_off, want.first_off)


@pytest.fixture(scope="module")
def text4m():
    return ops.synth_host(4 << 20, seed=5, vocab=3000, zipf_s=0.6)


@pytest.fixture(scope="module")
def want4m(text4m):
    return ops.cpu_count(text4m)


@pytest.mark.parametrize("resident", [False, True])
def test_engine_top_k(text4m, want4m, resident):
    want = want4m
    with ops.Engine(device=0, chunk_bytes=1 << 20) as e:
        def count():
            e.reset()
            if resident:  # the speculative finalize
                e.synth_device(4 << 20, seed=5, vocab=3000, zipf_s=0.6)
                e.count_resident()
            else:  # four chunks, the synchronous finalize
                e.count_bytes(text4m)

        for k in (1, 20, 1000, len(want), len(want) + 10):
            count()
            assert_same(e.top_k(k), want.top(k))
        assert_same(e.result(), want)
        assert_same(e.top_k(20), want.top(20))
        empty = e.top_k(0)
        assert len(empty) == 0 and empty.total == want.total
        e.reset()
        small = ops.synth_host(1 << 18, seed=8, vocab=400)
        e.count_bytes(small)
        assert_same(e.top_k(7), ops.cpu_count(small).top(7))


def test_engine_deep_tie_boundary():
    text = ops.synth_host(16 << 20, seed=3, vocab=60000, zipf_s=0.6)
    want = ops.cpu_count(text)
    by_count = np.sort(want.counts)[::-1]
    edges = np.flatnonzero(np.diff(by_count)) + 1  # starts of the runs of equal counts
    starts = np.concatenate(([0], edges))
    lens = np.diff(np.concatenate((starts, [len(by_count)])))
    run = int(np.argmax(lens))
    assert lens[run] > 100
    k = int(starts[run] + lens[run] // 2)
    with ops.Engine(device=0) as e:
        e.count_bytes(text)
        assert_same(e.top_k(k), want.top(k))


def test_engine_word_classes():
    """Inline keys (7 and 15 bytes), hashed keys (16, 40, 257 bytes) and a
    70 000-byte word among the top rows: the arena gather returns every byte."""
    rng = np.random.default_rng(12)
    special = [(b"sevenby", 50), (b"fifteen-bytes-w", 40), (b"sixteen-bytes-wo", 30), (b"f" * 39 + b"!", 20),
               (bytes(rng.integers(97, 123, 257, dtype=np.uint8)), 10),
               (bytes(rng.integers(97, 123, 70_000, dtype=np.uint8)), 2)]
    assert [len(w) for w, _ in special] == [7, 15, 16, 40, 257, 70_000]
    toks = [b"w%d" % i for i in range(3000)]
    for w, c in special:
        for p in rng.integers(0, len(toks), c):
            toks.insert(int(p), w)
    text = b" ".join(toks) + b"\n"
    want = ops.cpu_count(text)
    with ops.Engine(device=0, chunk_bytes=1 << 22) as e:
        e.count_bytes(text)
        got = e.top_k(8)
        assert_same(got, want.top(8))
        assert got.words[:6] == [w for w, _ in special]
        assert got.counts.tolist()[:6] == [c for _, c in special]
        assert_same(e.result(), want)


def test_rccl_world1_top_k():
    uid = ops.Comm.unique_id()
    comm = ops.Comm(uid, 0, 1, 0)
    with ops.Engine(device=0, chunk_bytes=1 << 20) as e:
        text = ops.synth_host(1 << 18, seed=1, vocab=500)
        e.count_bytes(text)
        got = e.top_k(20, comm)
    comm.close()
    assert_same(got, ops.cpu_count(text).top(20))


@pytest.mark.parametrize("merge_mode", [0, 1])
def test_rccl_merge_protocol_world1_top_k(merge_mode):
    """top_k behind the full merge protocol on one rank (WC_MERGE_ALWAYS, in a
    child process so the switch does not leak): the selection runs on the
    merged columns, with and without all_ranks."""
    code = (
        "from cuda_mapreduce_amd import ops\n"
        "uid = ops.Comm.unique_id(); comm = ops.Comm(uid, 0, 1, 0)\n"
        f"e = ops.Engine(device=0, chunk_bytes=1 << 20, merge_mode={merge_mode})\n"
        "text = ops.synth_host(3 << 18, seed=2, vocab=3000, zipf_s=0.8)\n"
        "e.count_bytes(text)\n"
        "want = ops.cpu_count(text)\n"
        "for all_ranks in (False, True):\n"
        "    for k in (20, 2500):\n"
        "        got, w = e.top_k(k, comm, all_ranks=all_ranks), want.top(k)\n"
        "        assert got.words == w.words and got.counts.tolist() == w.counts.tolist(), 'rows'\n"
        "        assert got.first_off.tolist() == w.first_off.tolist() and got.total == w.total, 'offsets'\n"
        "assert e.stats()['device_ms']['merge'] > 0\n"
        "e.close(); comm.close(); print('ok')\n"
    )
    env = dict(os.environ, WC_MERGE_ALWAYS="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, timeout=120)
    assert out.returncode == 0 and b"ok" in out.stdout, out.stderr.decode()[-2000:]


@pytest.fixture(scope="module")
def cli_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("topk") / "text.txt"
    path.write_bytes(ops.synth_host(1 << 20, seed=6, vocab=2000))
    return str(path)


def cli(*args):
    out = subprocess.run([os.path.join(ROOT, "wordcount"), *args], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out.stdout


@pytest.mark.parametrize("extra", [("--top", "7"), ("--top", "5000"), ("--virtual-ranks", "3", "--top", "7"),
                                   ("--no-list",)])
def test_cli_top_matches_cpu(cli_file, extra, tmp_path):
    top = [a for a in extra if a != "--virtual-ranks" and a != "3"]
    gpu_json, cpu_json = str(tmp_path / "gpu.json"), str(tmp_path / "cpu.json")
    got = cli(cli_file, "--no-echo", *extra, "--bench-json", gpu_json)
    want = cli(cli_file, "--cpu", "--no-echo", *top, "--bench-json", cpu_json)
    assert got == want
    g, c = json.load(open(gpu_json)), json.load(open(cpu_json))
    assert g["keys"] == c["keys"] and g["tokens"] == c["tokens"]
