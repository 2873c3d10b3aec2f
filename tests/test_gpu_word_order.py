"""Word order on the GPU (src/kernels/wordorder.hip, ``Engine.result(order="word")``,
``--sort word``).

Word order = plain bytewise order of the words, as ``sorted()`` on ``bytes``:
bytes compare unsigned, a proper prefix comes first.  The kernel hook is checked
against ``sorted`` on crafted word sets; the engine against ``Result.by_word``
of the CPU oracle (exact words, counts, first offsets and total).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import byte_cases as bc
import word_cases as wcs
from conftest import ROOT

pytestmark = pytest.mark.gpu

ops = pytest.importorskip("cuda_mapreduce_amd.ops")

SIZES = [1, 2, 63, 64, 65, 1023, 1025, 4097, 100_000]
ALPHABET = np.array([0x00, 0x61, 0x62, 0xFF], np.uint8)


def check_hook(words):
    perm, levels = ops.debug_word_order(words)
    assert len(perm) == len(words)
    assert np.array_equal(perm, np.array(wcs.want_perm(words), np.uint32))
    return levels


def random_words(n, seed):
    """n distinct words over ALPHABET, lengths 1..24: shared prefixes and ties
    between NUL bytes and zero padding are dense."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n:
        k = max(2 * (n - len(out)), 64)
        lens = rng.integers(1, 25, k)
        raw = ALPHABET[rng.integers(0, 4, (k, 24))]
        for i in range(k):
            w = raw[i, :lens[i]].tobytes()
            if w not in seen:
                seen.add(w)
                out.append(w)
                if len(out) == n:
                    break
    return out


@pytest.mark.parametrize("n", SIZES)
def test_kernel_hook_random_sets(n):
    words = random_words(n, 100 + n)
    rng = np.random.default_rng(n)
    by_word = sorted(words)
    shuffled = list(by_word)
    rng.shuffle(shuffled)
    for order in (by_word, by_word[::-1], shuffled):
        levels = check_hook(order)
        assert levels >= 1


def test_kernel_hook_large():
    """About a million words of up to 6 lowercase bytes: the large-n path of
    level 0, every row resolved by its first chunk."""
    rng = np.random.default_rng(77)
    short = [bytes(97 + (i // 26 ** j) % 26 for j in range(L)) for L in (1, 2, 3) for i in range(26 ** L)]
    v = np.unique(rng.integers(0, 26 ** 6, 1_100_000))
    rng.shuffle(v)
    v = v[:1_000_003 - len(short)]
    digits = np.stack([(v // 26 ** i) % 26 for i in range(6)], axis=1).astype(np.uint8) + 97
    words = short + np.ascontiguousarray(digits).view("S6").ravel().tolist()
    assert len(words) == 1_000_003
    order = rng.permutation(len(words))
    words = [words[i] for i in order]
    perm, levels = ops.debug_word_order(words)
    assert np.array_equal(perm, np.array(wcs.want_perm(words), np.uint32))
    assert levels == 1


def test_kernel_hook_ladders():
    words = wcs.ladders()
    np.random.default_rng(4).shuffle(words)
    check_hook(words)


@pytest.mark.parametrize("P", [7, 8, 9, 14, 15, 16, 17, 23, 24, 25, 31])
def test_kernel_hook_key_class_edges(P):
    """64 words equal in their first P bytes, differing after, suffixes of 1..12
    bytes over all byte values: the chunk and key-class boundaries."""
    rng = np.random.default_rng(P)
    prefix = bytes(rng.integers(1, 256, P, dtype=np.uint8))
    words = set()
    while len(words) < 64:
        words.add(prefix + bytes(rng.integers(0, 256, int(rng.integers(1, 13)), dtype=np.uint8)))
    words = sorted(words)
    rng.shuffle(words)
    check_hook(words)


def test_kernel_hook_byte_case_words():
    words = [w for w, _ in bc.family_words()] + bc.long_tail_words(3) + [w for cls in bc.twin_classes() for w in cls]
    words = list(dict.fromkeys(words))
    np.random.default_rng(5).shuffle(words)
    check_hook(words)


def test_kernel_hook_url_like():
    rng = np.random.default_rng(6)
    prefix = b"https://www.example.org/a/path/"
    assert len(prefix) == 31
    words = set()
    while len(words) < 5000:
        words.add(prefix + bytes(rng.integers(33, 127, int(rng.integers(1, 13)), dtype=np.uint8)))
    words = list(words)
    rng.shuffle(words)
    levels = check_hook(words)
    assert levels <= 16


def test_kernel_hook_deep_prefixes():
    """The level count does not grow with the length of a shared prefix: two
    70 000-byte words differing in their last byte (8 750 chunks) and their
    common prefix as a third word order in a handful of levels."""
    rng = np.random.default_rng(7)
    big = bytes(rng.integers(97, 123, 70_000, dtype=np.uint8))
    stem = bytes(rng.integers(97, 123, 250, dtype=np.uint8))
    mid = set()
    while len(mid) < 200:
        mid.add(stem + bytes(rng.integers(97, 123, 7, dtype=np.uint8)))
    words = [big[:-1] + b"x", big[:-1] + b"y", big[:-1]] + sorted(mid) + [b"f%d" % i for i in range(3000)]
    assert len(set(words)) == len(words)
    rng.shuffle(words)
    levels = check_hook(words)
    assert levels <= 16


@pytest.mark.parametrize("word", [b"ab", b"ab\0\0\0\0\0\0", b"nine-byte", b"sixteen-bytes-wo", b"q" * 300])
def test_kernel_hook_duplicate_word_fails(word):
    """Words of a finalized table are distinct: two rows holding one word fail
    the order naming both rows, at whichever level the word ends."""
    words = [b"f%d" % i for i in range(500)] + [b"q" * 299, b"ab\0", b"sixteen-bytes-wO"]
    words.insert(17, word)
    words.insert(401, word)
    with pytest.raises(ops.WcError) as err:
        ops.debug_word_order(words)
    msg = str(err.value)
    assert "hold the same word" in msg
    assert {"17", "401"} <= set(msg.replace(",", " ").split())
    rest = words[:401] + words[402:]  # the device is usable afterwards
    perm, _ = ops.debug_word_order(rest)
    assert [rest[i] for i in perm] == sorted(rest)


def assert_same(got, want):
    assert got.total == want.total
    assert len(got) == len(want)
    assert got.words == want.words
    assert np.array_equal(got.counts, want.counts)
    assert np.array_equal(got.first_off, want.first_off)


def check_engine(e, want):
    by_word = want.by_word()
    got = e.result(order="word")
    assert_same(got, by_word)
    assert got.words == sorted(want.words)
    assert e.stats()["word_order"]["levels"] >= 1
    assert_same(e.result(), want)  # the first-occurrence table is untouched
    assert_same(e.top_k(20), want.top(20))
    assert_same(e.result(order="word"), by_word)
    assert_same(e.result(order="first"), want)


@pytest.mark.parametrize("name", ["family-one-hot", "long-tail", "uniform-1/8"])
def test_engine_streamed(name):
    text = bc.text(name)
    want = ops.cpu_count(text)
    with ops.Engine(device=0, chunk_bytes=1 << 20) as e:
        e.count_bytes(text)
        check_engine(e, want)
        with pytest.raises(ValueError):
            e.result(order="count")


def test_engine_resident():
    want = ops.cpu_count(bc.text("synthetic"))
    with ops.Engine(device=0) as e:
        e.synth_device(bc.SYNTH["nbytes"], seed=bc.SYNTH["seed"], vocab=bc.SYNTH["vocab"])
        e.count_resident()
        check_engine(e, want)
        st = e.stats()
        assert st["host_ms"]["word_order"] > 0
        assert 0 <= st["word_order"]["unresolved"] <= len(want)


def test_engine_delimiters_only():
    with ops.Engine(device=0) as e:
        e.count_bytes(b" \n\r\n   \r ")
        got = e.result(order="word")
        assert len(got) == 0 and got.total == 0


def test_engine_offsets_above_4g():
    base = 2 ** 32 + 12345
    text = bc.text("long-tail")
    want = ops.cpu_count(text, global_base=base)
    assert int(want.first_off.min()) >= base
    with ops.Engine(device=0, chunk_bytes=1 << 20) as e:
        e.count_bytes(text, global_base=base)
        assert_same(e.result(order="word"), want.by_word())


def test_engine_word_classes():
    """Inline keys (7 and 15 bytes), hashed keys (16, 40, 257 bytes) and a
    70 000-byte word: every byte comes back, in word order."""
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
        got = e.result(order="word")
        assert_same(got, want.by_word())
        for w, c in special:
            assert got.counts[got.words.index(w)] == c
        assert_same(e.result(), want)


@pytest.mark.parametrize("merge_mode", [0, 1])
def test_rccl_merge_protocol_world1_word_order(merge_mode):
    """The word order behind the full merge protocol on one rank (WC_MERGE_ALWAYS,
    in a child process so the switch does not leak): it runs on the merged
    columns, with and without all_ranks."""
    code = (
        "from cuda_mapreduce_amd import ops\n"
        "uid = ops.Comm.unique_id(); comm = ops.Comm(uid, 0, 1, 0)\n"
        f"e = ops.Engine(device=0, chunk_bytes=1 << 20, merge_mode={merge_mode})\n"
        "text = ops.synth_host(3 << 18, seed=2, vocab=3000, zipf_s=0.8, long_frac=0.2)\n"
        "e.count_bytes(text)\n"
        "want = ops.cpu_count(text)\n"
        "w = want.by_word()\n"
        "assert w.words == sorted(want.words)\n"
        "for all_ranks in (False, True):\n"
        "    got = e.result(comm, all_ranks=all_ranks, order='word')\n"
        "    assert got.words == w.words and got.counts.tolist() == w.counts.tolist(), 'rows'\n"
        "    assert got.first_off.tolist() == w.first_off.tolist() and got.total == w.total, 'offsets'\n"
        "    first = e.result(comm, all_ranks=all_ranks)\n"
        "    assert first.words == want.words and first.counts.tolist() == want.counts.tolist(), 'first order'\n"
        "assert e.stats()['device_ms']['merge'] > 0\n"
        "e.close(); comm.close(); print('ok')\n"
    )
    env = dict(os.environ, WC_MERGE_ALWAYS="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, timeout=120)
    assert out.returncode == 0 and b"ok" in out.stdout, out.stderr.decode()[-2000:]


@pytest.fixture(scope="module")
def cli_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("wordorder") / "text.txt"
    path.write_bytes(ops.synth_host(1 << 20, seed=6, vocab=2000, long_frac=0.1) + b" ".join(wcs.ladders()) + b"\n")
    return str(path)


def cli(*args):
    out = subprocess.run([os.path.join(ROOT, "wordcount"), *args], capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return out.stdout


@pytest.mark.parametrize("extra", [(), ("--virtual-ranks", "3")])
def test_cli_sort_word_matches_cpu(cli_file, extra, tmp_path):
    gpu_json, cpu_json = str(tmp_path / "gpu.json"), str(tmp_path / "cpu.json")
    got = cli(cli_file, "--no-echo", "--sort", "word", *extra, "--bench-json", gpu_json)
    want = cli(cli_file, "--cpu", "--no-echo", "--sort", "word", "--bench-json", cpu_json)
    assert got == want
    g, c = json.load(open(gpu_json)), json.load(open(cpu_json))
    assert g["keys"] == c["keys"] and g["tokens"] == c["tokens"]
