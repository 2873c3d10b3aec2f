"""Cost of the output stage: result() + host selection against Engine.top_k.

A resident 1 GiB Zipf(1.0) job per vocabulary (100k and 1M words by default),
after a warm-up job that runs every call once.  Each repetition counts the
text again, drains the device, then times ONE output call with a host clock;
every call ends in a stream synchronise inside the engine.  All calls run the
same finalize first (its time alone is the first row), so the rows differ by
what follows it:

  result() + Result.top(20)   today's path: the whole table to the host (native:
                              D2H of six columns + the word arena, one
                              std::string per word), its export into Python, a
                              host sort
  top_k(K)                    selection, order and gather on the GPU, K rows copied

Per row: the median and the min-max spread of `reps` repetitions in ms, and
the bytes copied to the host (Stats::download_bytes).

usage: python tools/topk_cost.py [--reps 5] [--bytes 1073741824] [vocab ...]   (markdown on stdout)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mapreduce_amd import ops  # noqa: E402
from cuda_mapreduce_amd.ops._lib import check_ptr, lib  # noqa: E402


def ms(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def fmt(ts):
    return f"{statistics.median(ts):.3f} | {min(ts):.3f}-{max(ts):.3f}"


def measure(e, nbytes, reps):
    def job():
        e.reset()
        e.count_resident(nbytes)
        e.sync()

    job()
    n = len(e.result())  # warm-up: every call once
    ks = [("top_k(20)", 20), ("top_k(1000)", 1000), (f"top_k(n = {n})", n)]
    for _, k in ks:
        e.top_k(k)
    rows = []
    ts = []
    for _ in range(reps):
        job()
        ts.append(ms(e.finalize_device)[0])
    rows.append(("finalize_device() alone", fmt(ts), 0))
    native, export, top, whole = [], [], [], []
    want20 = None
    for _ in range(reps):
        job()
        t_native, p = ms(lambda: check_ptr(lib.wc_engine_result(e._p, None, 0)))
        nbytes_down = e.stats()["download_bytes"]
        t_export, res = ms(lambda: ops.Result._from_native(p))
        t_top, want20 = ms(lambda: res.top(20))
        native.append(t_native)
        export.append(t_export)
        top.append(t_top)
        whole.append(t_native + t_export + t_top)
    rows.append(("result() + Result.top(20)", fmt(whole), nbytes_down))
    rows.append(("- native result() (finalize, D2H, strings)", fmt(native), nbytes_down))
    rows.append(("- export into Python", fmt(export), 0))
    rows.append(("- Result.top(20) host sort", fmt(top), 0))
    for label, k in ks:
        ts = []
        for _ in range(reps):
            job()
            t, got = ms(lambda: e.top_k(k))
            ts.append(t)
        rows.append((label, fmt(ts), e.stats()["download_bytes"]))
        if k == 20:
            assert got.words == want20.words and got.counts.tolist() == want20.counts.tolist(), "top_k(20) != host"
            assert got.total == want20.total
    return n, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("vocab", nargs="*", type=int, default=[100_000, 1_000_000])
    a = ap.parse_args()
    assert ops.device_count() > 0, "no GPU visible"
    print(f"# Output stage: result() + host selection vs top_k ({a.bytes} bytes, Zipf 1.0, {a.reps} repetitions)\n")
    for vocab in a.vocab:
        with ops.Engine(device=0) as e:
            e.synth_device(a.bytes, seed=1, vocab=vocab)
            n, rows = measure(e, a.bytes, a.reps)
        print(f"## vocab {vocab}: {n} keys\n")
        print("| call | median ms | min-max ms | bytes to the host |")
        print("|---|---:|---:|---:|")
        for label, t, b in rows:
            print(f"| {label} | {t} | {b if b else '-'} |")
        print(flush=True)


if __name__ == "__main__":
    main()
