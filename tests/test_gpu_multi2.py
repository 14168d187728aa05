"""The streaming form of the fused multi-adapter path (k_multi_stream + k_multi_scan, cutadapt_amd/csrc/multi2.hip)
on the GPU against the oracle applying MultipleAdapters' rule (reference adapters.py:1265-1286: kmers_present +
locate of every adapter on the whole read, best by score, errors, first adapter).  Equally long reads; the CPU twin of
these checks (the rules without the kernel) is tests/test_multi2_model.py."""
import os
import random

import numpy as np
import pytest

from test_gpu_multi import env, oracle_multiple, plan_for, rs
from test_multi2_model import tail_reads

pytestmark = pytest.mark.gpu


def run_uniform(orc, seqs, rate, min_overlap, reads, what, expect="stream", pair_cap=None):
    from cutadapt_amd.batch import ReadBatch, match_batch
    n = len(reads[0])
    assert all(len(r) == n for r in reads)
    plan, ads = plan_for(seqs, rate, min_overlap)
    if expect is not None:
        assert plan.multi_kind(n) == expect, (what, plan.multi_kind(n))
    sq, offs = orc.pack_reads(reads)
    batch = ReadBatch.from_host(sq, offs)
    assert batch.uniform_len == n
    with env(CAH_MULTI_PAIR_CAP=pair_cap):
        res = match_batch(plan, batch)
        got6, got_st, got_best = res.cpu()
        if expect is not None:
            from cutadapt_amd import _lib
            assert _lib.last_multi_path() == expect, (what, _lib.last_multi_path())      # what ran, not what could have
    want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
    bad = np.nonzero((got_st != want_st) | (got6 != want6).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got_st[bad[:3]], got6[bad[:3]], want_st[bad[:3]], want6[bad[:3]],
                           reads[int(bad[0])])
    f = want_st == 1
    assert np.array_equal(got_best[f], want_best[f]), what
    return int(f.sum())


def test_c4_reads_vs_oracle(hip, orc):
    """the benchmark's adapters and reads; batch sizes around the piece (64), tile (8192) and page borders"""
    from cutadapt_amd import workloads
    ads = workloads.SPECS["C4"]["adapters"]
    for n_reads, seed in ((1, 1), (63, 2), (64, 3), (65, 4), (8191, 5), (8193, 6), (40_000, 7)):
        sq, offs = orc.synth_reads(seed, 0, n_reads, 150, ads)
        reads = [bytes(sq[offs[i]:offs[i + 1]]).decode() for i in range(n_reads)]
        found = run_uniform(orc, ads, 0.1, 3, reads, f"C4 x {n_reads}")
        if n_reads >= 8191:
            assert found > 0.2 * n_reads
    # several chunks (a small pair capacity), adapters everywhere, many errors
    sq, offs = orc.synth_reads(8, 0, 30_000, 150, ads, p_adapter=0.9, p_edit=0.08, p_n=0.02)
    reads = [bytes(sq[offs[i]:offs[i + 1]]).decode() for i in range(30_000)]
    run_uniform(orc, ads, 0.1, 3, reads, "C4 dense, chunked", pair_cap=96 * 6000)


def test_uniform_fuzz_vs_oracle(hip, orc):
    """random adapter sets of one shape x reads that end with (edited) adapter prefixes, every eligible read length"""
    rng = np.random.default_rng(2024)
    prng = random.Random(7)
    streamed = 0
    for it in range(36):
        m = int(rng.choice([12, 20, 25, 30, 33, 34, 40, 50, 64]))
        count = int(rng.choice([2, 8, 24, 96, 128]))
        seqs = [rs(prng, m) for _ in range(count)]
        if it % 4 == 0:
            seqs[1] = seqs[0][:-1] + prng.choice("ACGT")
            seqs[-1] = seqs[0]
        rate = float(rng.choice([0.1, 0.12, 0.2]))
        O = int(rng.choice([1, 3, 5]))
        n = int(rng.choice([16, 31, 64, 80, 100, 117, 150, 160]))
        reads = tail_reads(rng, seqs, 3000, n, p_n=float(rng.choice([0.0, 0.01])))
        reads = [r if len(r) == n else (r + "A" * n)[:n] for r in reads]
        if it % 5 == 0:
            reads = [r.lower() if i % 7 == 0 else r for i, r in enumerate(reads)]
        plan, _ = plan_for(seqs, rate, O)
        kind = plan.multi_kind(n)
        streamed += kind == "stream"
        run_uniform(orc, seqs, rate, O, reads, f"it {it} m {m} x {count} rate {rate} O {O} n {n} ({kind})", expect=None,
                    pair_cap=count * 700 if it % 3 == 0 else None)
    assert streamed >= (10 if not os.environ.get("CAH_TEST_SEED_OFFSET") else 4), streamed      # (drawn cases: looser under shifted seeds)


def test_stream_equals_older_fused_path_at_scale(hip):
    """2 M reads: the streaming form and k_multi_filter + k_back_scan<true> of the same library agree read for read"""
    import torch
    from cutadapt_amd.batch import ReadBatch, match_batch
    rng = random.Random(97)
    for n_adapters, m, n_reads in ((96, 33, 2_000_000), (24, 20, 1_000_000)):
        seqs = [rs(rng, m) for _ in range(n_adapters)]
        batch = ReadBatch.synthetic(n_reads, 150, seqs, seed=50 + n_adapters, p_adapter=0.4, p_edit=0.04, p_n=0.01)
        plan, _ = plan_for(seqs, 0.1, 3)
        assert plan.multi_kind(150) == "stream"
        a = match_batch(plan, batch)
        torch.cuda.synchronize()
        a6, ast, ab = a.out6.clone(), a.status.clone(), a.best_adapter.clone()
        with env(CAH_NO_MULTI2="1"):
            b = match_batch(plan, batch)
            torch.cuda.synchronize()
        assert torch.equal(ast, b.status), (n_adapters, m)
        assert torch.equal(a6, b.out6), (n_adapters, m)
        found = ast == 1
        assert torch.equal(ab[found], b.best_adapter[found]), (n_adapters, m)
        assert int(found.sum()) > 0.3 * n_reads


def test_invalid_bytes_are_flagged(hip, orc):
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(5)
    seqs = [rs(prng, 33) for _ in range(16)]
    plan, ads = plan_for(seqs, 0.1, 3)
    reads = [rs(prng, 150) for _ in range(300)]
    sq, offs = orc.pack_reads(reads)
    sq = sq.copy()
    for r in (0, 17, 63, 64, 299):
        sq[offs[r] + (r % 150)] = 0xC3
    batch = ReadBatch.from_host(sq, offs)
    got6, got_st, _ = match_batch(plan, batch).cpu()
    assert set(np.nonzero(got_st == 2)[0].tolist()) == {0, 17, 63, 64, 299}


def test_occurrence_window_regressions(hip, orc):
    """the kernels on what a soak found in round 4 (CPU twin: tests/test_multi2_model.py, same name): a whole-adapter chunk
    that is a tail chunk too (20-character adapters at rate 0.15), reads shorter than the adapter, adapters inside the
    read with many edits, rates 0.08-0.25"""
    ads = ["TTTATATAGTCCCCCACACT", "GGTCAATGCCGATTGACTTA"]
    reads = ["CTCCTCAGAAGGCCCCGGAAACCGAGCGCCCATATGAGTTAAATACTCTAGGGTCATCTGTATATAGTCCGCCACAC",
             "CTCCTCAGAAGGCCCCGGAAACCGAGCGCCCATATGAGTTAAATACTCTAGGGTCATCTGTATATAGTCCCCCACAC",
             "CTCCTCAGAAGGCCCCGGAATTTATATAGTCCGCCACACTGAGTTAAATACTCTAGGGTCATCTGAAAAAAAAAAAA"]
    run_uniform(orc, ads, 0.15, 8, reads * 40, "chunk that is a tail chunk too", expect=None)
    rng = np.random.default_rng(31337)
    prng = random.Random(31338)
    streamed = 0
    for it in range(10):
        m = int(rng.choice([20, 24, 28, 30, 33, 35, 40, 64]))
        count = int(rng.choice([2, 3, 8, 24]))
        seqs = [rs(prng, m) for _ in range(count)]
        if it % 5 == 3:
            seqs[0] = (rs(prng, int(rng.choice([2, 3, 5]))) * m)[:m]
        rate = float(rng.choice([0.08, 0.1, 0.12, 0.15, 0.2, 0.25]))
        O = int(rng.choice([1, 3, 5]))
        n = int(rng.integers(40, 161))
        reads = tail_reads(rng, seqs, 1000, n, p_n=float(rng.choice([0.0, 0.01])))
        reads = [r if len(r) == n else (r + "A" * n)[:n] for r in reads]
        sq2, of2 = orc.synth_reads(int(rng.integers(1, 10 ** 6)), 0, 1000, n, seqs, p_adapter=float(rng.choice([0.3, 0.8])),
                                   p_edit=float(rng.choice([0.03, 0.08, 0.12])), p_n=0.005)
        reads += [bytes(sq2[of2[i]:of2[i + 1]]).decode() for i in range(1000)]
        plan, _ = plan_for(seqs, rate, O)
        streamed += plan.multi_kind(n) == "stream"
        run_uniform(orc, seqs, rate, O, reads, f"mixed it {it} m {m} x {count} rate {rate} O {O} n {n}", expect=None)
    # (5 with these seeds: the other plans take the older kernels; a count of drawn cases: looser under shifted seeds)
    assert streamed >= (4 if not os.environ.get("CAH_TEST_SEED_OFFSET") else 1), streamed


def _near_duplicates(prng, base, count):
    """adapters that share most of their chunks with `base`: every read that holds `base` pairs with every adapter"""
    out = [base]
    for i in range(1, count):
        s = list(base)
        p = (7 * i) % len(base)
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + i % 3) % 4]
        out.append("".join(s))
    return out


def test_every_adapter_on_every_read_with_a_minimal_pool(hip, orc):
    """Round-4 review: the page pool's gate is host arithmetic, and a pair beyond the pool used to be dropped without a word.
    The worst case the arithmetic is made for -- every adapter pairs with every read -- with the smallest pool the library
    accepts (CAH_MULTI_PAIR_CAP=1: the floor of one block's reserve): several rounds, every tuple against the oracle."""
    prng = random.Random(41)
    # (near-duplicates share their k-mers: homes of the streaming form's directory with more than CAH_M2_MAX_GROUP entries)
    for count, m, n_reads in ((8, 33, 40_000), (16, 33, 30_000), (24, 33, 20_000), (16, 20, 30_000)):
        # (whether 16 adapters may share a k-mer depends on the base adapter's chunks: draw until the plan streams)
        for _try in range(40):
            seqs = _near_duplicates(prng, rs(prng, m), count)
            if plan_for(seqs, 0.1, 3)[0].multi_kind(150) == "stream":
                break
        reads = []
        for i in range(n_reads):
            pos = prng.randrange(0, 150 - m + 12)
            r = rs(prng, pos) + seqs[i % count] + rs(prng, 150)
            reads.append(r[:150])
        found = run_uniform(orc, seqs, 0.1, 3, reads, f"{count} near-duplicates, minimal pool", pair_cap=1)
        assert found > 0.9 * n_reads


_OVERFLOW_SCRIPT = r"""
import os, random, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import pytest, torch
from cutadapt_amd import _lib
from cutadapt_amd.batch import ReadBatch, match_batch
from test_gpu_multi2 import _near_duplicates, plan_for, rs, env
prng = random.Random(43)
seqs = _near_duplicates(prng, rs(prng, 33), 8)
batch = ReadBatch.synthetic(300_000, 150, seqs, seed=77, p_adapter=0.95, p_edit=0.01, p_n=0.0)
plan, _ = plan_for(seqs, 0.1, 3)
assert plan.multi_kind(150) == "stream"
with env(CAH_MULTI_PAIR_CAP="1"):
    ok = match_batch(plan, batch)
    torch.cuda.synchronize()
    st_ok = ok.status.clone()
    with env(CAH_TEST_M2_UNGATED="1"):
        try:
            match_batch(plan, batch)
            torch.cuda.synchronize()
        except _lib.HipInternalError as exc:
            assert "page pool ran out" in str(exc), exc
            print("RAISED", "dev" if {dev} else "product")
        else:
            print("SERVED", "dev" if {dev} else "product")
            assert torch.equal(ok.status, st_ok)
        # ... and with the deferred error check the same overflow is no exception but CAH_STATUS_INTERNAL in EVERY status byte
        was = _lib.lib().cah_set_deferred_errors(1)
        try:
            bad = match_batch(plan, batch)
            torch.cuda.synchronize()
            if {dev}:
                assert bool((bad.status == _lib.STATUS_INTERNAL).all()), int((bad.status == _lib.STATUS_INTERNAL).sum())
                assert int(bad.out6.abs().sum()) == 0
                print("MARKED dev")
            else:
                assert torch.equal(bad.status, st_ok)
        finally:
            _lib.lib().cah_set_deferred_errors(was)
    # the library is not left in a bad state: the next call is served and agrees
    again = match_batch(plan, batch)
    torch.cuda.synchronize()
    assert torch.equal(again.status, st_ok) and torch.equal(again.out6, ok.out6)
    # the deferred error check (cah_set_deferred_errors: the call does not wait for its kernels): a gated pool still
    # synchronises (the host decides on further rounds) and serves the batch ...
    was = _lib.lib().cah_set_deferred_errors(1)
    try:
        d1 = match_batch(plan, batch)
        torch.cuda.synchronize()
        assert torch.equal(d1.status, st_ok) and torch.equal(d1.out6, ok.out6)
    finally:
        _lib.lib().cah_set_deferred_errors(was)
# ... and a pool that holds the batch's worst case returns without waiting: same rows; with the gate taken away (dev
# library only) no pool "holds the worst case" by the host's arithmetic, so the deferred form is not taken there
was = _lib.lib().cah_set_deferred_errors(1)
try:
    d2 = match_batch(plan, batch)
    torch.cuda.synchronize()
    assert torch.equal(d2.status, st_ok) and torch.equal(d2.out6, ok.out6)
    assert not bool((d2.status == _lib.STATUS_INTERNAL).any())
finally:
    assert _lib.lib().cah_set_deferred_errors(was) == 1
assert int((st_ok == 1).sum()) > 0.8 * 300_000
print("DONE")
"""


def test_pool_overflow_fails_loudly(hip):
    """... and when the gate IS taken away (CAH_TEST_M2_UNGATED=1, a switch only libcutadapt_hip_dev.so holds -- the same
    sources under -DCAH_DEV_KNOBS, cutadapt_amd/build.py: build_dev_library -- that lets the blocks draw tiles whatever the
    pool holds) the call does not return wrong tuples: the kernels flag the page they could not get, match_batch_multi
    answers CAH_EINTERNAL, the binding raises HipInternalError; the next call is served.  The PRODUCT library ignores the
    variable (round-5 review: a stray environment variable must not change what the shipped library does)."""
    import subprocess
    import sys
    from cutadapt_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(build.DEV_LIB_PATH), "python -m cutadapt_amd.build --dev"
    assert build.library_build_id(build.DEV_LIB_PATH) == build.source_hash(), "stale dev library"
    for dev in (True, False):
        e = dict(os.environ)
        e.pop("CAH_LIB_PATH", None)
        if dev:
            e["CAH_LIB_PATH"] = build.DEV_LIB_PATH
        r = subprocess.run([sys.executable, "-c", _OVERFLOW_SCRIPT.format(root=root, tests=os.path.join(root, "tests"), dev=dev)],
                           env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
        assert ("RAISED dev" if dev else "SERVED product") in r.stdout, r.stdout
        assert ("MARKED dev" in r.stdout) == dev, r.stdout


def test_first_occurrence_race_at_scale(hip, orc):
    """Round 4's second hole was a lane race (which lane emits a pair need not hold the pair's earliest occurrence) that no
    CPU model sees.  Adapters made of repeated chunks, reads with two and three copies: 3 x 4 M reads, the streaming form
    against the older kernels in full and against the oracle on a sample, three seeds."""
    import torch
    from cutadapt_amd.batch import ReadBatch, match_batch
    for seed in (11, 12, 13):
        prng = random.Random(1000 + seed)
        unit = rs(prng, 8)
        seqs = []
        for i in range(12):
            u2 = rs(prng, 8)
            seqs.append((unit + u2 + unit + rs(prng, 9))[:33] if i % 2 == 0 else (u2 + unit + rs(prng, 8) + unit + "A")[:33])
        plan, ads = plan_for(seqs, 0.1, 3)
        assert plan.multi_kind(150) == "stream"
        n_reads = 4_000_000
        batch = ReadBatch.synthetic(n_reads, 150, seqs, seed=seed, p_adapter=0.7, p_edit=0.03, p_n=0.002)
        # a second (and sometimes third) copy of the shared chunk in front of the adapter copy, in every fourth read
        view = batch.seqs.view(n_reads, 150)
        u = torch.tensor(list(unit.encode()), dtype=torch.uint8, device=batch.seqs.device)
        idx = torch.arange(0, n_reads, 4, device=batch.seqs.device)
        at = (idx * 2654435761 >> 7) % 120
        for t in range(8):
            view[idx, at + t] = u[t]
        idx3 = idx[::3]
        at3 = ((idx3 * 40503 >> 3) % 100) + 30
        for t in range(8):
            view[idx3, at3 + t] = u[t]
        a = match_batch(plan, batch)
        torch.cuda.synchronize()
        a6, ast, ab = a.out6.clone(), a.status.clone(), a.best_adapter.clone()
        with env(CAH_NO_MULTI2="1"):
            b = match_batch(plan, batch)
            torch.cuda.synchronize()
        assert torch.equal(ast, b.status) and torch.equal(a6, b.out6), seed
        f = ast == 1
        assert torch.equal(ab[f], b.best_adapter[f]), seed
        m = 20_000
        sq = batch.seqs[: m * 150].cpu().numpy()
        offs = np.arange(m + 1, dtype=np.int64) * 150
        want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
        assert np.array_equal(ast[:m].cpu().numpy(), want_st) and np.array_equal(a6[:m].cpu().numpy(), want6), seed
        fw = want_st == 1
        assert np.array_equal(ab[:m].cpu().numpy()[fw], want_best[fw]), seed
        assert int(f.sum()) > 0.4 * n_reads


def _lib_last_path():
    from cutadapt_amd import _lib
    return _lib.last_multi_path()


def test_views_of_a_uniform_batch_stream(hip, orc):
    """Round 6: views inside the reads of a uniform batch (reads cut by a modifier in front of the adapter search, reference
    cli.py:938-954) through the streaming multi-adapter form itself: k_multi_stream's RV form copies them END-ALIGNED into
    a frame of the parent's length, k_multi_scan works on the frame and reports in the view's coordinates, a shortcut whose
    alignment would begin in the pad goes to the cell DP on the view (host model: test_views_in_a_padded_frame).  Views
    cut at either end -- a 5' cut inside an adapter copy leaves its tail at the view's first characters --, every length
    0 .. n, parents of 100 / 150 / 151 / 160 and 64 characters, against the oracle on the views."""
    import torch
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(92)
    checked = 0
    for it, (count, m, n, rate) in enumerate(((24, 33, 150, 0.1), (8, 33, 151, 0.1), (24, 30, 100, 0.1), (3, 20, 64, 0.15),
                                              (48, 33, 160, 0.1), (8, 24, 150, 0.2))):
        seqs = [rs(prng, m) for _ in range(count)]
        plan, ads = plan_for(seqs, rate, 3)
        if plan.multi_kind(n) != "stream":
            continue
        n_reads = 60_000
        parent = ReadBatch.synthetic(n_reads, n, seqs, seed=40 + it, p_adapter=0.8, p_edit=0.04, p_n=0.004)
        idx = torch.arange(n_reads, dtype=torch.int64, device=parent.device)
        mode = idx % 4
        a = torch.where((mode == 1) | (mode == 3), ((idx * 2654435761) >> 9) % (n + 1), torch.zeros_like(idx))
        b = torch.where((mode == 2) | (mode == 3), a + ((idx * 40503 + 77) >> 4) % (n + 1 - a), torch.full_like(idx, n))
        lens = b - a
        lens[::997] = 0
        view = parent.view(a, lens)
        got = match_batch(plan, view)
        torch.cuda.synchronize()
        assert _lib_last_path() == "stream", _lib_last_path()
        h_seqs = parent.seqs.cpu().numpy()
        h_off = (parent.offsets[:n_reads] + a).cpu().numpy()
        h_len = lens.cpu().numpy()
        m_chk = 25_000
        reads = [bytes(h_seqs[int(o):int(o) + int(l)]).decode("latin-1") for o, l in zip(h_off[:m_chk], h_len[:m_chk])]
        sq, offs = orc.pack_reads(reads)
        want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
        g6, gst = got.out6[:m_chk].cpu().numpy(), got.status[:m_chk].cpu().numpy()
        bad = np.nonzero((gst != want_st) | (g6 != want6).any(axis=1))[0]
        assert len(bad) == 0, (it, len(bad), int(bad[0]), reads[int(bad[0])], g6[bad[0]].tolist(), want6[bad[0]].tolist(),
                               int(h_len[bad[0]]))
        fw = want_st == 1
        assert np.array_equal(got.best_adapter[:m_chk].cpu().numpy()[fw], want_best[fw]), it
        # ... and the whole batch against the per-lane kernels
        with env(CAH_NO_MULTI2_VIEWS="1", CAH_NO_FRAMES="1"):
            want = match_batch(plan, view)
            torch.cuda.synchronize()
        assert torch.equal(got.status, want.status) and torch.equal(got.out6, want.out6), it
        checked += 1
    assert checked >= 4, checked


def test_ragged_batches_stream_in_frames(hip, orc):
    """Ragged batches of a plan with several adapters that are no views of a uniform batch -- a packed batch with an offsets
    array, views anywhere in a buffer (what the reads of a raw FASTQ chunk are) -- through cah_match_batch_frames: every read
    end-aligned in a frame of the longest one's length, the copy gathered from the views' ends (multi2.hip: view_general).
    Lengths 0 .. 150 (empty reads, reads shorter than 16), the first and the last bytes of the buffer used, against the
    per-lane kernels in full and the oracle on a sample."""
    import torch
    from cutadapt_amd import batch as B
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(91)
    seqs = [rs(prng, 33) for _ in range(24)]
    plan, ads = plan_for(seqs, 0.1, 3)
    assert plan.multi_kind(150) == "stream"
    n = 300_000
    parent = ReadBatch.synthetic(n, 150, seqs, seed=31, p_adapter=0.6, p_edit=0.03, p_n=0.003)
    idx = torch.arange(n, dtype=torch.int64, device=parent.device)
    lens = ((idx * 2654435761 + 977) >> 5) % 151                      # 0 .. 150
    lens[::1000] = 0
    lens[0] = 150
    lens[n - 1] = 150
    starts = ((idx * 40503) >> 3) % (151 - lens)                      # anywhere inside the read
    # the packed layout (an offsets array): the reads copied back to back -- the buffer begins with read 0 and ends with the last
    packed_off = torch.zeros(n + 1, dtype=torch.int64, device=parent.device)
    torch.cumsum(lens, 0, out=packed_off[1:])
    cols = torch.arange(150, device=parent.device)
    keep = cols[None, :] < lens[:, None]
    gather = (parent.offsets[:n] + starts)[:, None] + cols[None, :]
    packed = parent.seqs[gather[keep]].contiguous()
    assert packed.numel() == int(packed_off[-1].item())
    pb = ReadBatch(packed, packed_off, validated=True)
    assert B._frame_len(plan, pb) == 150
    got = match_batch(plan, pb)
    torch.cuda.synchronize()
    assert _lib_last_path() == "stream", _lib_last_path()
    with env(CAH_NO_FRAMES="1"):
        pb2 = ReadBatch(packed, packed_off, validated=True)
        want = match_batch(plan, pb2)
        torch.cuda.synchronize()
        assert _lib_last_path() != "stream"
    assert torch.equal(got.status, want.status) and torch.equal(got.out6, want.out6)
    f = want.status == 1
    assert torch.equal(got.best_adapter[f], want.best_adapter[f])
    assert int(f.sum()) > 0.5 * n
    m = 30_000
    sq, offs = packed[: int(packed_off[m].item())].cpu().numpy(), packed_off[: m + 1].cpu().numpy()
    want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
    assert np.array_equal(got.status[:m].cpu().numpy(), want_st) and np.array_equal(got.out6[:m].cpu().numpy(), want6)
    # views scattered over a buffer with other bytes between them (starts + lengths, no offsets array order): the same reads
    # as views into the parent batch, handed over WITHOUT the uniform-batch tag
    vb = ReadBatch(parent.seqs, parent.offsets[:n] + starts, lens.to(torch.int32), n_reads=n, validated=True)
    vb.max_len = 150
    got2 = match_batch(plan, vb)
    torch.cuda.synchronize()
    assert _lib_last_path() == "stream"
    assert torch.equal(got2.status, want.status) and torch.equal(got2.out6, want.out6)
    # views in NO order over a buffer of 1.35 GB (neighbouring views more than 2^30 bytes apart: the gathering copy then has
    # no extent of the piece's own views to load freely in, every unit takes the careful way), against the per-lane kernels
    big = ReadBatch.synthetic(9_000_000, 150, seqs, seed=32, p_adapter=0.6, p_edit=0.03, p_n=0.003)
    pick = (((idx * 2654435761) >> 3) % 9_000_000)
    pick[1::2] = 8_999_999 - pick[1::2] % 1000                           # every other view at the buffer's far end
    far = ReadBatch(big.seqs, pick * 150 + starts, lens.to(torch.int32), n_reads=n, validated=True)
    far.max_len = 150
    got3 = match_batch(plan, far)
    torch.cuda.synchronize()
    assert _lib_last_path() == "stream"
    with env(CAH_NO_FRAMES="1"):
        far2 = ReadBatch(big.seqs, pick * 150 + starts, lens.to(torch.int32), n_reads=n, validated=True)
        want3 = match_batch(plan, far2)
        torch.cuda.synchronize()
    assert torch.equal(got3.status, want3.status) and torch.equal(got3.out6, want3.out6)
    assert int((want3.status == 1).sum()) > 0.4 * n


def test_frames_of_short_and_odd_batches(hip, orc):
    """cah_match_batch_frames at the edges: reads of 0 .. 20 characters (frames of 16 .. 20), a batch of empty reads, one
    long read among short ones, a batch whose longest read is longer than the streaming forms take (falls back by itself),
    for one adapter and for several -- against the oracle in full"""
    import torch
    from cutadapt_amd import adapters as A
    from cutadapt_amd import batch as B
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(93)
    seqs = [rs(prng, 20) for _ in range(8)]
    plan8, ads8 = plan_for(seqs, 0.1, 3)
    one = A.BackAdapter(seqs[0], max_errors=0.1, min_overlap=3)
    n = 70_000
    old_min = B.FRAME_MIN_READS
    B.FRAME_MIN_READS = 1000
    try:
        for what, lo, hi, long_one in (("short", 0, 20, None), ("empty", 0, 0, None), ("one long", 0, 40, 150), ("too long", 10, 60, 400)):
            reads = []
            for i in range(n):
                ln = prng.randint(lo, hi)
                r = rs(prng, ln)
                if ln >= 6 and i % 3 == 0:
                    cut = seqs[i % 8][: prng.randint(3, min(20, ln))]
                    r = r[: ln - len(cut)] + cut
                reads.append(r)
            if long_one:
                reads[n // 2] = rs(prng, long_one - 20) + seqs[3]
            sq, offs = orc.pack_reads(reads)
            for plan, ads in ((plan8, ads8), (one._fused_plan, [one])):
                batch = ReadBatch.from_host(sq, offs)
                frame = B._frame_len(plan, batch)
                if what == "too long":
                    assert frame == 0
                elif len(ads) == 8:
                    assert frame == max(16, int(np.diff(offs).max())), (what, frame)
                got = match_batch(plan, batch)
                torch.cuda.synchronize()
                want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
                g6, gst = got.out6.cpu().numpy(), got.status.cpu().numpy()
                bad = np.nonzero((gst != want_st) | (g6 != want6).any(axis=1))[0]
                assert len(bad) == 0, (what, len(ads), len(bad), reads[int(bad[0])], g6[bad[0]].tolist(), want6[bad[0]].tolist())
    finally:
        B.FRAME_MIN_READS = old_min


def test_frames_that_do_not_stream_are_plain_views(hip, orc):
    """cah_match_batch_frames with a frame the streaming multi-adapter form does not take -- 200 characters, longer than any
    table set allows, and 160 under CAH_NO_MULTI2_VIEWS=1: the call is served (CAH_OK) with the views as the plain views
    they are, by the older fused kernels for a plan of one shape, by the per-adapter loop for a mixed plan, which has no
    fused kernels behind it.  Rows against the oracle in full."""
    import torch
    from cutadapt_amd import _lib
    from cutadapt_amd.batch import ReadBatch, _stream_ptr
    prng = random.Random(94)
    one_shape = [rs(prng, 20) for _ in range(8)]
    mixed = [rs(prng, m) for m in (12, 16, 20, 24, 28, 33, 36, 40)]
    reads = []
    for i in range(2000):
        ln = prng.randint(30, 200)
        r = rs(prng, ln)
        if i % 3 != 2:
            ad = (one_shape + mixed)[i % 16]
            cut = ad[: prng.randint(3, len(ad))]
            r = r[: ln - len(cut)] + cut if i % 2 else (r[: ln - len(ad) - 5] + ad + r)[:ln]
        reads.append(r)
    # (the caller guarantees that no view is longer than its frame)
    for frame, views_off, batch_reads in ((200, None, reads), (160, "1", [r for r in reads if len(r) <= 160])):
        sq, offs = orc.pack_reads(batch_reads)
        n = len(batch_reads)
        for seqs, path in ((one_shape, "fused"), (mixed, "sequential")):
            plan, ads = plan_for(seqs, 0.1, 3)
            assert plan.multi_kind(160) == "stream" and plan.multi_kind(200) == path, (path, plan.multi_kind(160), plan.multi_kind(200))
            batch = ReadBatch.from_host(sq, offs)
            lens = (batch.offsets[1:] - batch.offsets[:-1]).to(torch.int32)
            out6 = torch.empty((n, 6), dtype=torch.int32, device=batch.device)
            status = torch.empty(n, dtype=torch.uint8, device=batch.device)
            best = torch.empty(n, dtype=torch.int32, device=batch.device)
            ws = batch.workspace(plan)
            with env(CAH_NO_MULTI2_VIEWS=views_off):
                rc = _lib.lib().cah_match_batch_frames(plan.handle, batch.seqs.data_ptr(), batch.offsets.data_ptr(), lens.data_ptr(),
                                                       frame, n, out6.data_ptr(), best.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                                       ws.numel(), _stream_ptr())
                torch.cuda.synchronize()
                assert rc == 0, (frame, path, rc)
                assert _lib.last_multi_path() == path, (frame, path, _lib.last_multi_path())
            want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
            g6, gst = out6.cpu().numpy(), status.cpu().numpy()
            bad = np.nonzero((gst != want_st) | (g6 != want6).any(axis=1))[0]
            assert len(bad) == 0, (frame, path, len(bad), batch_reads[int(bad[0])], g6[bad[0]].tolist(), want6[bad[0]].tolist())
            fw = want_st == 1
            assert np.array_equal(best.cpu().numpy()[fw], want_best[fw]), (frame, path)
            assert int(fw.sum()) > 0.3 * n


def test_characters_that_read_as_A_in_the_lookup_words(hip, orc):
    """The tables are looked up with two bits per character: anything but A / C / G / T -- an N, the NULs in front of a view in
    its frame -- reads as 'A' there (multi2.h: m2_roll2).  Adapters rich in A then meet k-mers everywhere in such reads: pairs
    that the scan must find nothing for.  N runs, poly-A, adapters behind and in front of N, uniform batches and ragged ones in
    frames (pads of up to 140 NULs), against the oracle in full"""
    import torch
    from cutadapt_amd import batch as B
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(4242)
    seqs = ["A" * 33, "A" * 16 + rs(prng, 17), rs(prng, 17) + "A" * 16, "ACGT" * 8 + "A"] + [rs(prng, 33) for _ in range(8)]
    n = 150

    def read_of(i, ln):
        kind = i % 8
        if kind == 0:
            r = "N" * ln
        elif kind == 1:
            r = "".join(prng.choice("AN") for _ in range(ln))
        elif kind == 2:
            r = "A" * ln
        elif kind == 3:                                               # an adapter prefix behind a run of N (and one inside it)
            ad = seqs[prng.randrange(len(seqs))]
            cut = ad[: prng.randint(3, 33)]
            r = (rs(prng, ln) + "N" * 12 + cut)[-ln:] if ln else ""
            if ln > 20 and prng.random() < 0.5:
                k = prng.randrange(ln - len(cut), ln) if len(cut) < ln else 0
                r = r[:k] + "N" + r[k + 1:]
        elif kind == 4:                                               # a whole adapter with an N next to it / in it
            ad = seqs[prng.randrange(len(seqs))]
            at = prng.randint(0, max(0, ln - 40))
            r = (rs(prng, at) + "N" + ad + "N" + rs(prng, ln))[:ln]
            if prng.random() < 0.4 and ln > at + 20:
                r = r[: at + 10] + "N" + r[at + 11:]
        else:
            r = "".join(prng.choice("ACGTN") if prng.random() < 0.1 else prng.choice("ACGT") for _ in range(ln))
        return (r + "A" * ln)[:ln]

    reads = [read_of(i, n) for i in range(6000)]
    found = run_uniform(orc, seqs, 0.1, 3, reads, "A-rich adapters, N-rich reads")
    assert found > 500
    # ... ragged, in frames: the pads are NULs
    plan, ads = plan_for(seqs, 0.1, 3)
    old_min = B.FRAME_MIN_READS
    B.FRAME_MIN_READS = 1000
    try:
        ragged = [read_of(i, prng.choice((16, 20, 33, 40, 77, 150, 160))) for i in range(20_000)]
        sq, offs = orc.pack_reads(ragged)
        batch = ReadBatch.from_host(sq, offs)
        assert B._frame_len(plan, batch) == 160
        got = match_batch(plan, batch)
        torch.cuda.synchronize()
        from cutadapt_amd import _lib
        assert _lib.last_multi_path() == "stream"
        want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
        g6, gst = got.out6.cpu().numpy(), got.status.cpu().numpy()
        bad = np.nonzero((gst != want_st) | (g6 != want6).any(axis=1))[0]
        assert len(bad) == 0, (len(bad), ragged[int(bad[0])], g6[bad[0]].tolist(), want6[bad[0]].tolist())
        assert int((want_st == 1).sum()) > 2000
    finally:
        B.FRAME_MIN_READS = old_min
