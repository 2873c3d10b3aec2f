"""Cost of the byte map (Engine(byte_map=...), src/kernels/translate.hip) on the
flagship job.

The bench.py job — 1 GiB of resident Zipf(1.0) text, 100k-word vocabulary,
reset + count + device finalize per job — on three engines that differ only
in their map: none, fold_case, fold_case + split_punct.  The synthetic text is
letters of both cases and delimiters, no punctuation: the fold rewrites its
capitals (the key count per map is printed: a fold that merged words would
shrink the table the later stages see), split_punct adds nothing on this
text.  The translate kernel itself reads and writes every byte whatever the
map does to it, and the resident text is translated again by every job.

Per engine: `warmup` jobs, then `rounds` timed loops of `jobs` jobs each with
the stage marks off (as bench.py times its steps), the engines taking turns
so that clock drift hits all three alike; then one job with the marks on for
the stage split.  Per map: ms per job (median and min-max over the rounds),
Stats translate_ms, and the kernel's GB/s — bytes read plus bytes written
over translate_ms.

usage: python tools/translate_cost.py [--bytes 1073741824] [--jobs 200] [--warmup 20] [--rounds 3]
(markdown on stdout)
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cuda_mapreduce_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--jobs", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--vocab", type=int, default=100_000)
    a = ap.parse_args()
    assert ops.device_count() > 0, "no GPU visible"
    n = a.bytes // 1024 * 1024
    maps = [("none", None), ("fold_case", ops.byte_map(fold_case=True)),
            ("fold_case + split_punct", ops.byte_map(fold_case=True, split_punct=True))]
    engines, keys = [], []
    for name, m in maps:
        e = ops.Engine(device=0, chunk_bytes=n) if m is None else ops.Engine(device=0, chunk_bytes=n, byte_map=m)
        e.synth_device(n, seed=1, vocab=a.vocab)
        for _ in range(a.warmup):
            k = e.job_resident(n)
        keys.append(k)
        e.set_stage_events(False)
        e.sync()
        engines.append(e)
    times = [[] for _ in maps]
    for _ in range(a.rounds):
        for i, e in enumerate(engines):
            e.sync()
            t0 = time.perf_counter()
            for _ in range(a.jobs):
                e.job_resident(n)
            e.sync()
            times[i].append((time.perf_counter() - t0) / a.jobs * 1e3)
    print(f"# Byte map cost: {n} resident bytes, Zipf 1.0, {a.vocab}-word vocabulary; "
          f"{a.warmup} warm-up jobs, {a.rounds} rounds of {a.jobs} timed jobs\n")
    print("| map | keys | ms/job median | ms/job min-max | translate_ms | device_ms total | kernel GB/s (read + write) |")
    print("|---|---:|---:|---:|---:|---:|---:|")
    for (name, m), e, ts, k in zip(maps, engines, times, keys):
        e.set_stage_events(True)
        e.job_resident(n)
        e.sync()
        d = e.stats()["device_ms"]
        tr = d["translate"]
        assert (tr == 0) == (m is None), (name, d)
        rate = f"{2 * n / (tr * 1e-3) / 1e9:.0f}" if tr else "-"
        print(f"| {name} | {k} | {statistics.median(ts):.4f} | {min(ts):.4f}-{max(ts):.4f} | {tr:.4f} | {d['total']:.4f} | "
              f"{rate} |")
        e.close()
    print(flush=True)


if __name__ == "__main__":
    main()
