"""The engine on all 256 byte values, on the edges of the key classes and on
first offsets above 2^32 (inputs and reference: byte_cases.py; the same inputs
against the CPU oracle: test_byte_inputs_cpu.py).

Every comparison is exact — words, their order, counts, first offsets, total —
against byte_cases.py py_table, a pure-Python table that knows nothing of the
key scheme."""
import pytest

import byte_cases as bc

pytestmark = pytest.mark.gpu

ops = pytest.importorskip("cuda_mapreduce_amd.ops")


def run(e, text, base=0):
    e.reset()
    e.count_bytes(text, global_base=base)
    return e.result()


# ------------------------------------------------------------- key classes --
@pytest.mark.parametrize("chunk", [32 << 10, 4 << 20])
@pytest.mark.parametrize("name", ["family-one-hot", "family-both-hot"])
def test_key_class_families(name, chunk):
    """Every word length at a class edge with NUL / 0xFF last bytes, all-NUL and
    all-0xFF words, words of one hot-table signature (one twin hot and one cold,
    or both hot), 16-byte-record edges and the delimiters' neighbours: through
    the hot table and as records (both asserted), in small and large chunks, on
    a fresh engine and on one reused after reset()."""
    text, want = bc.text(name), bc.table(name)
    with ops.Engine(device=0, chunk_bytes=chunk) as e:
        for job in range(2):
            bc.assert_table(run(e, text), want)
            st = e.stats()
            assert 0 < st["records"] < st["tokens"]  # hot-table hits and misses both happened
            assert st["long_tokens"] > 0


# -------------------------------------------------------------- LONG tails --
@pytest.mark.parametrize("bits", [1, 62])
def test_long_tail_lengths(bits, monkeypatch):
    """LONG words of lengths 0, 1 and 7 mod 8 and around the hot table's 64-byte
    limit, 40 per length sharing their first 8 bytes (with 1 hash bit they also
    share keys): the partial last chunk of the map's key and byte compares, the
    reduce's and both merges' byte compares, in both LONG-record layouts."""
    text, want = bc.text("long-tail"), bc.table("long-tail")
    with ops.Engine(device=0, k1_hash_bits=bits) as e:
        for job in range(2):
            bc.assert_table(run(e, text), want)
            st = e.stats()
            assert st["long_direct"] == job  # the second job takes the layout the first one's LONG share chose
            assert st["long_tokens"] > 0
    monkeypatch.setenv("WC_MERGE_ROOT_ROWS", "0")  # the owner exchange, not the root gather
    for merge_mode in (0, 1):
        got = ops.loopback_count(text, 3, merge_mode=merge_mode, k1_hash_bits=bits, chunk_bytes=1 << 20)
        bc.assert_table(got, want)


# ----------------------------------------------------------- uniform bytes --
UNIFORM = {1 / 3: "uniform-1/3", 1 / 8: "uniform-1/8", 1 / 40: "uniform-1/40"}


MODES = {"one-chunk": dict(chunk_bytes=4 << 20), "chunks-32k": dict(chunk_bytes=32 << 10),
         "table-splits": dict(chunk_bytes=1 << 20, log2_rec_buckets=1, log2_tab_buckets=1), "ranks-2": 2, "ranks-5": 5}
UNIFORM_CASES = ([(n, 1 / 8, "chunks-32k") for n in (1, 31, 32, 33, 2047, 2048, 2049, 70_001)] +
                 [(2 << 20, p, mode) for p in sorted(UNIFORM) for mode in MODES])


@pytest.mark.parametrize("n,p,mode", UNIFORM_CASES, ids=[f"{n}-1/{round(1 / p)}-{mode}" for n, p, mode in UNIFORM_CASES])
def test_uniform_bytes(n, p, mode):
    """Uniform bytes 0..255 with a share p of delimiters: sizes around the map's
    lane (32 bytes) and unit (2 KiB) and over two chunks, and 2 MiB at three
    densities (mostly words of <= 7 bytes; half of them longer; mostly LONG
    words up to ~300 bytes) in one chunk, in 32 KiB chunks, into a 2-bucket
    table that has to split, and merged at 2 and 5 ranks in both merge modes."""
    if n == 2 << 20:
        text, want = bc.text(UNIFORM[p]), bc.table(UNIFORM[p])
    else:
        text = bc.random_bytes_text(n, n, p)
        want = bc.py_table(text)
    if mode.startswith("ranks"):
        for merge_mode in (0, 1):
            got = ops.loopback_count(text, MODES[mode], merge_mode=merge_mode, chunk_bytes=1 << 20)
            bc.assert_table(got, want)
        return
    with ops.Engine(device=0, **MODES[mode]) as e:
        bc.assert_table(run(e, text), want)
        st = e.stats()
    if mode == "table-splits":
        assert st["table_splits"] >= 1


# ---------------------------------------------------- offsets above 32 bits --
def bases(n):
    return {"straddle": 2**32 - n // 2, "above": 2**32 + 1, "far": 2**40 + 12345}


# WC_FIRST_ORDER=bitmap sizes the bitmap from the job's absolute end offset (one
# bit per two bytes below it: Engine::Impl::ensure_bitmap), not from the text's
# length: 256 MiB at 2^32, zeroed once and then touched only where keys are —
# it would be 64 GiB at 2^40, so the forced bitmap runs at the two bases near
# 2^32 only.
ORDER_CASES = [(order, where) for order in (None, "radix", "bitmap") for where in ("straddle", "above", "far")
               if not (order == "bitmap" and where == "far")]
# Stats()["order_path"] (test_gpu_order.py).  With no order forced the engine
# takes the sample sort up to 400k keys.  Its bins are unions of whole log bins
# (keys.hpp fo_logbin: 2^M per octave, M = fo_mbits = 9 for 33..40-bit keys), so
# at 2^32 a log bin is 8 MiB of offsets wide (4 MiB just below it) and at 2^40
# 2 GiB: the 50k / 207k first offsets of a 4 / 2 MiB job lie in one or two of
# them, a sort bin holds 8192 rows (FO_BLOCK_CAP), so the sample sort has to
# overflow and the radix sort redoes the order — path 3, on every job.  (At
# base 0 the same texts take path 1: the bins below 2^22 are 1..8 KiB wide.)
# The family text's 1114 keys fit one bin: there the sample sort itself must
# deliver the order at these offsets (1; 4 = job 1's hint was outgrown first).
ORDER_PATHS = {None: (3,), "radix": (2,), "bitmap": (5,)}
ORDER_PATHS_FEW_KEYS = {None: (1, 4), "radix": (2,), "bitmap": (5,)}


@pytest.mark.parametrize("order,where", ORDER_CASES)
def test_offsets_above_32_bits(order, where, monkeypatch):
    """First offsets are 64-bit end to end: a job that straddles 2^32, one just
    above it and one at 2^40, streamed in 1 MiB chunks and counted from resident
    text (the speculative finalize), under every first-occurrence order."""
    if order:
        monkeypatch.setenv("WC_FIRST_ORDER", order)  # read at engine creation
    for name, paths in (("synthetic", ORDER_PATHS), ("uniform-1/8", ORDER_PATHS), ("family-one-hot", ORDER_PATHS_FEW_KEYS)):
        text = bc.text(name)
        base = bases(len(text))[where]
        with ops.Engine(device=0, chunk_bytes=1 << 20) as e:
            bc.assert_table(run(e, text, base), bc.table(name, base))
            assert e.stats()["order_path"] in paths[order]
    n = bc.SYNTH["nbytes"]
    base = bases(n)[where]
    want = bc.table("synthetic", base)
    with ops.Engine(device=0) as e:
        e.synth_device(n, seed=bc.SYNTH["seed"], vocab=bc.SYNTH["vocab"])
        e.reset()
        e.count_resident(n, global_base=base)
        bc.assert_table(e.result(), want)
        assert e.stats()["order_path"] in ORDER_PATHS[order]
        for _ in range(2):
            assert e.job_resident(n, global_base=base) == len(want[0])
            bc.assert_table(e.result(), want)
            assert e.stats()["order_path"] in ORDER_PATHS[order]


@pytest.mark.parametrize("resident", [False, True], ids=["streamed", "resident"])
@pytest.mark.parametrize("where", ["straddle", "far"])
@pytest.mark.parametrize("ranks", [2, 4])
def test_offsets_above_32_bits_merged(ranks, where, resident, monkeypatch):
    """The same through the cross-rank merge (the shuffle's owner merge and the
    dense mode's minimum over first offsets), every shard counted at the job's
    base + its begin."""
    monkeypatch.setenv("WC_MERGE_ROOT_ROWS", "0")
    for name in ("synthetic", "uniform-1/8"):
        text = bc.text(name)
        base = bases(len(text))[where]
        for merge_mode in (0, 1):
            got = ops.loopback_count(text, ranks, merge_mode=merge_mode, resident=resident, chunk_bytes=1 << 20,
                                     global_base=base)
            bc.assert_table(got, bc.table(name, base))
