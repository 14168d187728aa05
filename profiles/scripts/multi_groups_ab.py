"""A/B of the grouped streaming multi-adapter form (multi2.h: m2_build_groups) against the per-adapter loop of the same
library, in ONE process and one call sequence (the loop via CAH_NO_MULTI_GROUPS=1, asked at every call), alternating.

    python profiles/scripts/multi_groups_ab.py [--reads 10000000] [--reps 3] [--out profiles/multi_groups/ab.json]

Plans: 129, 256 and 384 adapters of 20..40 characters, 384 33-mers, and 96 adapters of 20..40 at rate 0.2 (the plan one
table refuses for capacity), on synthetic reads of 150 characters.  Times are host clocks around calls that end in a
device synchronise; the results of both forms are compared read for read.  With CAH_LIB_PATH pointing at another build of
the library (--one-group only), the one-group workloads (96 33-mers, 96 mixed) are timed for a same-call comparison."""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def rs(prng, n):
    return "".join(prng.choice("ACGT") for _ in range(n))


def plans(prng):
    mixed = lambda count: [rs(prng, 20 + prng.randrange(21)) for _ in range(count)]
    return [("129x20-40", mixed(129), 0.1), ("256x20-40", mixed(256), 0.1), ("384x20-40", mixed(384), 0.1),
            ("384x33", [rs(prng, 33) for _ in range(384)], 0.1), ("96x20-40@0.2", mixed(96), 0.2)]


def one_group_plans(prng):
    return [("C4-like 96x33", [rs(prng, 33) for _ in range(96)], 0.1),
            ("96x20-40", [rs(prng, 20 + (7 * i) % 21) for i in range(96)], 0.1)]


def timed(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one-group", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "multi_groups", "ab.json"))
    a = ap.parse_args()
    import torch
    from cutadapt_amd import _lib
    from cutadapt_amd import adapters as A
    from cutadapt_amd.batch import ReadBatch, match_batch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    prng = random.Random(2024)
    rows = []
    for name, seqs, rate in (one_group_plans(prng) if a.one_group else plans(prng)):
        plan = _lib.Plan([A.BackAdapter(s, max_errors=rate, min_overlap=3).matcher_spec() for s in seqs])
        groups = plan.multi_groups() if hasattr(_lib.lib(), "cah_plan_multi_groups") else None
        batch = ReadBatch.synthetic(a.reads, 150, seqs, seed=5, p_adapter=0.4, p_edit=0.04, p_n=0.01)
        row = {"plan": name, "adapters": len(seqs), "rate": rate, "reads": a.reads, "groups": groups, "kind": plan.multi_kind(150)}
        forms = [("stream", None)] if a.one_group else [("stream", None), ("loop", "1")]
        times = {f: [] for f, _ in forms}
        keep = {}
        for rep in range(a.reps + 1):                                   # (the first repetition warms up)
            for form, flag in forms:
                if flag is None:
                    os.environ.pop("CAH_NO_MULTI_GROUPS", None)
                else:
                    os.environ["CAH_NO_MULTI_GROUPS"] = flag
                t, res = timed(lambda: match_batch(plan, batch), torch)
                path = _lib.last_multi_path()
                assert path == ("stream" if flag is None else "sequential"), (name, form, path)
                if rep:
                    times[form].append(t)
                keep[form] = (res.status.clone(), res.out6.clone())
        os.environ.pop("CAH_NO_MULTI_GROUPS", None)
        for form in times:
            row[form + "_ms"] = [round(1e3 * t, 2) for t in times[form]]
            row[form + "_greads_s"] = round(a.reads / min(times[form]) / 1e9, 3)
        if "loop" in times:
            row["equal"] = bool(torch.equal(keep["stream"][0], keep["loop"][0]) and torch.equal(keep["stream"][1], keep["loop"][1]))
            row["speedup"] = round(min(times["loop"]) / min(times["stream"]), 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"build_id": _lib.build_id() if hasattr(_lib, "build_id") else "", "lib": _lib.LIB_PATH, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
