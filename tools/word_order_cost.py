"""Cost of the alphabetical output: Engine.result(order="word") against
result() + a host sort.

A resident 1 GiB Zipf(1.0) job per vocabulary (100k and 1M words by default),
after a warm-up job that runs every call once.  Each repetition counts the
text again, drains the device, then times ONE output call with a host clock;
every call ends in a stream synchronise inside the engine and runs the same
finalize first (its time alone is the first row).

  result(order="word")        order on the GPU (wordorder.hip), gather of the six
                              columns, the whole table to the host in word order
  result() + Result.by_word() the route without it: the table in first-occurrence
                              order, its export into Python, sorted() on bytes
  result() + host std::sort   the CLI's host paths: wc::sort_by_word on the native
                              table (wc_result_sort_by_word)

The device order alone is then run through the kernel hook on the same words
(ops.debug_word_order): per level the rows it sorted, the host wall time (the
level's wait included) and the device time between stream events.

usage: python tools/word_order_cost.py [--reps 5] [--bytes 1073741824] [vocab ...]   (markdown on stdout)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mapreduce_amd import ops  # noqa: E402
from cuda_mapreduce_amd.ops._lib import check, check_ptr, lib  # noqa: E402


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
    first = e.result()  # warm-up: every call once
    e.result(order="word")
    n = len(first)
    rows = []
    ts = []
    for _ in range(reps):
        job()
        ts.append(ms(e.finalize_device)[0])
    rows.append(("finalize_device() alone", fmt(ts), 0))

    native, export, order_ms = [], [], []
    for _ in range(reps):
        job()
        t_native, p = ms(lambda: check_ptr(lib.wc_engine_result_by_word(e._p, None, 0)))
        st = e.stats()
        t_export, got = ms(lambda: ops.Result._from_native(p))
        native.append(t_native)
        export.append(t_export)
        order_ms.append(st["host_ms"]["word_order"])
    down = st["download_bytes"]
    rows.append(('result(order="word"), native (finalize, order, gather, D2H, strings)', fmt(native), down))
    rows.append(("- of it: order + gather + D2H + strings (host_ms.word_order)", fmt(order_ms), down))
    rows.append(("- export into Python (not in the line above)", fmt(export), 0))
    levels, unresolved = st["word_order"]["levels"], st["word_order"]["unresolved"]

    native, export, sort, whole = [], [], [], []
    for _ in range(reps):
        job()
        t_native, p = ms(lambda: check_ptr(lib.wc_engine_result(e._p, None, 0)))
        down_first = e.stats()["download_bytes"]
        t_export, res = ms(lambda: ops.Result._from_native(p))
        t_sort, want = ms(res.by_word)
        native.append(t_native)
        export.append(t_export)
        sort.append(t_sort)
        whole.append(t_native + t_export + t_sort)
    assert got.words == want.words and got.counts.tolist() == want.counts.tolist(), "device order != host order"
    assert got.first_off.tolist() == want.first_off.tolist() and got.total == want.total
    rows.append(("result() + Result.by_word()", fmt(whole), down_first))
    rows.append(("- native result() (finalize, D2H, strings)", fmt(native), down_first))
    rows.append(("- export into Python", fmt(export), 0))
    rows.append(("- Result.by_word() host sort (sorted on bytes)", fmt(sort), 0))

    native, sort = [], []
    for _ in range(reps):
        job()
        t_native, p = ms(lambda: check_ptr(lib.wc_engine_result(e._p, None, 0)))
        t_sort, _ = ms(lambda: check(lib.wc_result_sort_by_word(p)))
        sorted_words = ops.Result._from_native(p).words
        native.append(t_native + t_sort)
        sort.append(t_sort)
    assert sorted_words == want.words, "host std::sort != sorted()"
    rows.append(("native result() + host std::sort (the CLI's host paths)", fmt(native), down_first))
    rows.append(("- the std::sort alone (wc::sort_by_word)", fmt(sort), 0))

    per_level = []
    for _ in range(reps):
        perm, lv, d = ops.debug_word_order(first.words, details=True)
        per_level.append(d)
        assert lv == levels and d["unresolved"] == unresolved
    assert [first.words[i] for i in perm] == want.words
    return n, rows, levels, unresolved, per_level


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("vocab", nargs="*", type=int, default=[100_000, 1_000_000])
    a = ap.parse_args()
    assert ops.device_count() > 0, "no GPU visible"
    print(f"# Output in word order: result(order=\"word\") vs result() + host sort ({a.bytes} bytes, Zipf 1.0, "
          f"{a.reps} repetitions)\n")
    for vocab in a.vocab:
        with ops.Engine(device=0) as e:
            e.synth_device(a.bytes, seed=1, vocab=vocab)
            n, rows, levels, unresolved, per_level = measure(e, a.bytes, a.reps)
        print(f"## vocab {vocab}: {n} keys, word_order.levels {levels}, word_order.unresolved {unresolved}\n")
        print("| call | median ms | min-max ms | bytes to the host |")
        print("|---|---:|---:|---:|")
        for label, t, b in rows:
            print(f"| {label} | {t} | {b if b else '-'} |")
        print("\nThe device order alone (kernel hook, the same words):\n")
        print("| level | rows sorted | host median ms | host min-max ms | device median ms | device min-max ms |")
        print("|---:|---:|---:|---:|---:|---:|")
        for l in range(len(per_level[0]["rows"])):
            print(f"| {l} | {per_level[0]['rows'][l]} | {fmt([d['host_ms'][l] for d in per_level])} | "
                  f"{fmt([d['device_ms'][l] for d in per_level])} |")
        print(flush=True)


if __name__ == "__main__":
    main()
