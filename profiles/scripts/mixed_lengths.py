"""Mixed adapter lengths: the streaming multi-adapter form against the per-adapter loop, and C4 with this library against
another build of it.

    python profiles/scripts/mixed_lengths.py [--reads N] [--steps K] [--warmup W] [--other-lib PATH] [--out FILE]

96 random adapters of 20..40 characters (rate 0.1, min_overlap 3) on N x 150 bp device-resident synthetic reads, timed with
HIP events: the mixed form, then -- same process, same plan, same batch -- the per-adapter loop (CAH_NO_MULTI_MIXED=1: what
such a plan took before the mixed form existed).  Then `bench.py --config C4` in child processes, alternating between this
library and --other-lib (CAH_LIB_PATH; skipped without it), three times each.  Writes one JSON document."""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def time_steps(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def c4_rate(lib_path, steps, warmup):
    env = dict(os.environ)
    if lib_path:
        env["CAH_LIB_PATH"] = lib_path
        env["CAH_LIB_ANY_ABI"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C4", "--gpus", "1", "--steps", str(steps),
                          "--warmup", str(warmup)], env=env, capture_output=True, text=True, timeout=400)
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{"):
            d = json.loads(line)
            return {"Mreads_per_s": d["value"], "ms_per_step": d["ms_per_step"]}
    return {"error": (out.stdout + out.stderr)[-500:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_lengths.json"))
    args = ap.parse_args()
    import torch
    from cutadapt_amd import _lib
    from cutadapt_amd import adapters as A
    from cutadapt_amd.batch import ReadBatch, match_batch
    rng = random.Random(2026)
    seqs = ["".join(rng.choice("ACGT") for _ in range(20 + (7 * i) % 21)) for i in range(96)]
    plan = _lib.Plan([A.BackAdapter(s, max_errors=0.1, min_overlap=3).matcher_spec() for s in seqs])
    doc = {"build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "reads": args.reads, "read_len": 150,
           "adapters": "96 x 20..40 characters, rate 0.1, min_overlap 3", "steps": args.steps, "warmup": args.warmup,
           "multi_kind": plan.multi_kind(150)}
    batch = ReadBatch.synthetic(args.reads, 150, seqs, seed=3, p_adapter=0.25, p_edit=0.02, p_n=0.005)
    res = match_batch(plan, batch)
    torch.cuda.synchronize()
    doc["path_mixed"] = _lib.last_multi_path()
    doc["matched_fraction"] = float((res.status == 1).float().mean().item())
    ms = time_steps(torch, lambda: match_batch(plan, batch, out=res), args.steps, args.warmup)
    doc["mixed_ms"] = ms
    # the kernel families of the mixed form (cah profile scopes: HIP events around prefilter, scan, cell DP, merge)
    import ctypes as C
    L = _lib.lib()
    L.cah_profile_reset()
    L.cah_profile_enable(1)
    for _ in range(args.steps):
        match_batch(plan, batch, out=res)
    torch.cuda.synchronize()
    L.cah_profile_enable(0)
    pms, pl, pu = (C.c_double * 8)(), (C.c_int64 * 8)(), (C.c_int64 * 8)()
    _lib.check(L.cah_profile_read(pms, pl, pu))
    L.cah_profile_reset()
    doc["mixed_scope_ms_per_step"] = {"k_multi_stream": pms[_lib.PROF_FILTER] / args.steps, "k_multi_scan": pms[_lib.PROF_SCAN] / args.steps,
                                      "k_dp_packed": pms[_lib.PROF_DP] / args.steps}
    os.environ["CAH_NO_MULTI_MIXED"] = "1"
    match_batch(plan, batch, out=res)
    torch.cuda.synchronize()
    doc["path_loop"] = _lib.last_multi_path()
    ms2 = time_steps(torch, lambda: match_batch(plan, batch, out=res), args.steps, max(1, args.warmup - 1))
    del os.environ["CAH_NO_MULTI_MIXED"]
    doc["loop_ms"] = ms2
    med = lambda v: sorted(v)[len(v) // 2]
    doc["mixed_Greads_per_s"] = args.reads / med(ms) / 1e6
    doc["loop_Greads_per_s"] = args.reads / med(ms2) / 1e6
    doc["mixed_over_loop"] = med(ms2) / med(ms)
    del batch, res
    torch.cuda.empty_cache()
    doc["c4"] = {"this": [], "other": []}
    for _ in range(3):
        doc["c4"]["this"].append(c4_rate(None, args.steps, args.warmup))
        if args.other_lib:
            doc["c4"]["other"].append(c4_rate(args.other_lib, args.steps, args.warmup))
    ok = [r["Mreads_per_s"] for r in doc["c4"]["this"] if "Mreads_per_s" in r]
    if ok:
        doc["c4_Greads_per_s"] = med(ok) / 1e3
        doc["mixed_over_c4"] = doc["mixed_Greads_per_s"] / doc["c4_Greads_per_s"]
    other = [r["Mreads_per_s"] for r in doc["c4"]["other"] if "Mreads_per_s" in r]
    if ok and other:
        doc["c4_this_over_other"] = med(ok) / med(other)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
