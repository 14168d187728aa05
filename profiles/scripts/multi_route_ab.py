"""Host-side A/B of the multi-adapter path: this library against another build of it (--other-lib, e.g. the parent commit's),
and the other build against itself for the spread of the box.

    python profiles/scripts/multi_route_ab.py --other-lib PATH [--rounds 3] [--out profiles/multi_route/ab.json]

One driver process starts worker processes in turn -- other, this, other again -- `--rounds` times (a process loads one
library; CAH_LIB_PATH selects it).  Every worker times the same workloads with host clocks around calls that end in a
device synchronise: C4 (96 adapters, uniform reads), C4's reads as a ragged packed batch (frames), 384 33-mers (groups of
tables) and the small batches of a length bucket, down to 10 000 reads, where the host's work per call shows, and the per-read calls
(cah_match_one_host / cah_locate_one_host on one read of 150 characters: all host work and launch latency).  A workload's
figure is the median call of a worker; `this_over_other` compares the medians over the rounds, `other_again_over_other` is
the same figure for two sets of runs of ONE library, and `band` the range of the other library's single workers around
their median: this library is no slower where its ratio lies inside what the other library does against itself."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def worker():
    import torch
    from cutadapt_amd import _lib, workloads
    from cutadapt_amd import adapters as A
    from cutadapt_amd.batch import ReadBatch, match_batch
    assert torch.cuda.is_available(), "this measurement needs the GPU"

    def plan_of(seqs):
        return _lib.Plan([A.BackAdapter(s, max_errors=0.1, min_overlap=3).matcher_spec() for s in seqs])

    def calls_ms(plan, batch, calls, path):
        res = match_batch(plan, batch)
        torch.cuda.synchronize()
        assert _lib.last_multi_path() == path, (path, _lib.last_multi_path())
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            match_batch(plan, batch, out=res)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms)

    out = {}
    c4 = workloads.SPECS["C4"]["adapters"]
    plan = plan_of(c4)
    batch = ReadBatch.synthetic(20_000_000, 150, c4, seed=4)
    out["C4 uniform 20M"] = calls_ms(plan, batch, 7, "stream")
    # the same kind of reads cut to 0 .. 150 characters and packed back to back: an offsets array, streamed in frames
    n = 5_000_000
    idx = torch.arange(n, dtype=torch.int64, device=batch.device)
    lens = ((idx * 2654435761 + 977) >> 5) % 151
    off = torch.zeros(n + 1, dtype=torch.int64, device=batch.device)
    torch.cumsum(lens, 0, out=off[1:])
    cols = torch.arange(150, device=batch.device)
    packed = batch.seqs[: n * 150].view(n, 150)[cols[None, :] < lens[:, None]].contiguous()
    ragged = ReadBatch(packed, off, validated=True)
    ragged.max_len = 150
    out["C4 ragged packed 5M"] = calls_ms(plan, ragged, 7, "stream")
    del ragged, packed
    for reads, length, calls in ((826_000, 150, 30), (826_000, 90, 30), (826_000, 40, 30), (100_000, 90, 100), (10_000, 150, 300)):
        small = ReadBatch.synthetic(reads, length, c4, seed=4)
        out[f"C4 small {reads} x {length}"] = calls_ms(plan, small, calls, "stream")
    del batch
    torch.cuda.empty_cache()
    prng = random.Random(2024)
    seqs = ["".join(prng.choice("ACGT") for _ in range(33)) for _ in range(384)]
    plan = plan_of(seqs)
    batch = ReadBatch.synthetic(5_000_000, 150, seqs, seed=5, p_adapter=0.4, p_edit=0.04, p_n=0.01)
    out["384 x 33 grouped 5M"] = calls_ms(plan, batch, 5, "stream")
    del batch
    # the per-read calls: one adapter, one read (a 3' adapter inside it: prefilter, scan and the tuple)
    L = _lib.lib()
    plan = plan_of([c4[0]])
    read = "".join(prng.choice("ACGT") for _ in range(110)) + c4[0][:40]
    for name, fn in (("match_one_host 150", L.cah_match_one_host), ("locate_one_host 150", L.cah_locate_one_host)):
        ms = []
        for i in range(3200):
            t0 = time.perf_counter()
            _lib.one_read(fn, plan.handle, read)
            ms.append(1e3 * (time.perf_counter() - t0))
        out[name] = statistics.median(ms[200:])
    print(json.dumps({"build_id": _lib.build_id(), "ms": out}), flush=True)


def run_worker(lib_path):
    env = dict(os.environ)
    env.pop("CAH_LIB_PATH", None)
    if lib_path:
        env["CAH_LIB_PATH"] = lib_path
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"worker failed ({r.returncode}): {(r.stdout + r.stderr)[-2000:]}")
    return json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--other-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_route", "ab.json"))
    a = ap.parse_args()
    if a.worker:
        return worker()
    assert a.other_lib and os.path.exists(a.other_lib), "--other-lib: the library to compare with"
    runs = {"other": [], "this": [], "other_again": []}
    for _ in range(a.rounds):
        for label, lib in (("other", a.other_lib), ("this", None), ("other_again", a.other_lib)):
            runs[label].append(run_worker(lib))
            print(label, json.dumps(runs[label][-1]["ms"]), flush=True)
    med = lambda label, w: statistics.median(r["ms"][w] for r in runs[label])
    rows = {}
    for w in runs["this"][0]["ms"]:
        base = med("other", w)
        singles = [r["ms"][w] / base for label in ("other", "other_again") for r in runs[label]]
        row = {"this_ms": [round(r["ms"][w], 4) for r in runs["this"]], "other_ms": [round(r["ms"][w], 4) for r in runs["other"]],
               "other_again_ms": [round(r["ms"][w], 4) for r in runs["other_again"]],
               "this_over_other": round(med("this", w) / base, 4), "other_again_over_other": round(med("other_again", w) / base, 4),
               "band": [round(min(singles), 4), round(max(singles), 4)]}
        row["inside_band"] = row["this_over_other"] <= row["band"][1]
        rows[w] = row
    doc = {"this_build_id": runs["this"][0]["build_id"], "other_build_id": runs["other"][0]["build_id"], "rounds": a.rounds,
           "unit": "ms per call, median of a worker's calls (host clock, the call ends in a device synchronise or the one-read calls' wait)", "workloads": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
