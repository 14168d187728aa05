"""The MIXED form of the streaming multi-adapter path on the GPU: one plan of 8..128 3' adapters of DIFFERENT lengths
(cutadapt_amd/csrc/api.cpp: build_multi_mixed; multi2.h: m2_build_mixed; k_multi_scan<KIND, true>, k_dp_packed<ROWS, true,
true>) against the oracle applying MultipleAdapters' rule (reference adapters.py:1265-1286) and against the per-adapter
loop of the same library (CAH_NO_MULTI_MIXED=1: what such a plan took before).  The CPU twin of the rules is
tests/test_multi2_mixed_model.py."""
import io
import random

import numpy as np
import pytest

from test_gpu_multi import env, oracle_multiple, plan_for, rs
from test_multi2_model import tail_reads

pytestmark = pytest.mark.gpu

TRUSEQ_LIKE = (19, 20, 21, 33, 34)


def mixed_adapters(prng, lens):
    return [rs(prng, m) for m in lens]


def reads_for(rng, prng, ads, count, n, p_n=0.005):
    """reads of n characters: (edited) adapter prefixes at the end, (edited) whole adapters inside, N, lower case"""
    reads = tail_reads(rng, ads, count // 2, n, p_n=p_n)
    reads = [r if len(r) == n else (r + "A" * n)[:n] for r in reads]
    for _ in range(count - len(reads)):
        body = list(rs(prng, n))
        if prng.random() < 0.8:
            ad = list(prng.choice(ads))
            for _e in range(prng.randrange(0, 1 + max(1, len(ad) // 8))):
                u, pos = prng.random(), prng.randrange(len(ad))
                if u < 0.5:
                    ad[pos] = prng.choice("ACGT")
                elif u < 0.75:
                    ad.insert(pos, prng.choice("ACGT"))
                elif len(ad) > 1:
                    del ad[pos]
            at = prng.randrange(n)
            body[at:at + len(ad)] = ad
        reads.append("".join(body[:n]))
    return [r.lower() if i % 9 == 0 else r for i, r in enumerate(reads)]


def check_uniform(orc, ads_seq, rate, O, reads, what, expect="stream", pair_cap=None):
    from cutadapt_amd import _lib
    from cutadapt_amd.batch import ReadBatch, match_batch
    n = len(reads[0])
    plan, ads = plan_for(ads_seq, rate, O)
    assert plan.multi_kind(n) == expect, (what, plan.multi_kind(n))
    sq, offs = orc.pack_reads(reads)
    batch = ReadBatch.from_host(sq, offs)
    assert batch.uniform_len == n
    with env(CAH_MULTI_PAIR_CAP=pair_cap):
        got6, got_st, got_best = match_batch(plan, batch).cpu()
        assert _lib.last_multi_path() == expect, (what, _lib.last_multi_path())
    want6, want_st, want_best = oracle_multiple(orc, ads, sq, offs)
    bad = np.nonzero((got_st != want_st) | (got6 != want6).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got_st[bad[:3]], got6[bad[:3]], want_st[bad[:3]], want6[bad[:3]], reads[int(bad[0])])
    f = want_st == 1
    assert np.array_equal(got_best[f], want_best[f]), what
    return int(f.sum())


PLANS = [
    # (lengths, rate, min_overlap, read length)
    ([12, 64, 20, 33, 40, 25, 31, 50], 0.1, 3, 48),
    ([12, 64, 20, 33, 40, 25, 31, 50], 0.1, 3, 150),         # the 64-mer's tail windows take all five chunks of the last half-row
    ([12, 64, 19, 20, 21, 33, 34, 48], 0.1, 1, 151),
    ([12, 52, 20, 33, 40, 25, 31, 50], 0.1, 3, 150),
    ([32, 33] * 4 + [20], 0.1, 3, 150),                      # 9 adapters across the 32-row border
    ([TRUSEQ_LIKE[i % 5] for i in range(24)], 0.1, 3, 100),
    ([12, 16, 20, 24, 28, 30, 32, 32], 0.2, 5, 64),          # every adapter in one 32-bit word
    ([20 + (7 * i) % 21 for i in range(96)], 0.1, 3, 150),
    ([16 + (5 * i) % 9 for i in range(128)], 0.1, 3, 151),
    ([12, 64, 19, 21, 33, 34, 45, 60, 13], 0.25, 8, 40),     # reads shorter than the longest adapter
    ([14, 22, 30, 38, 46, 50, 52, 52], 0.15, 1, 160),
]


@pytest.mark.parametrize("case", range(len(PLANS)))
def test_mixed_plans_vs_oracle(hip, orc, case):
    """batch sizes around the piece (64 reads) and the tile (8192), and a small pool: several rounds"""
    lens, rate, O, n = PLANS[case]
    rng = np.random.default_rng(500 + case)
    prng = random.Random(600 + case)
    ads = mixed_adapters(prng, lens)
    if case % 3 == 0:
        ads[1] = ads[0][:len(ads[1])] if len(ads[1]) < len(ads[0]) else ads[1]       # a prefix of another adapter
        ads[3] = (rs(prng, 3) * 30)[:len(ads[3])]                                     # a repetitive one
    big = 3000 if len(ads) >= 96 else 8193
    reads = reads_for(rng, prng, ads, big, n)
    found = check_uniform(orc, ads, rate, O, reads, f"case {case} x {big}")
    assert found > 0.2 * big
    for count in (63, 64, 65) + ((8191,) if big > 8191 else ()):
        check_uniform(orc, ads, rate, O, reads[:count], f"case {case} x {count}")
    check_uniform(orc, ads, rate, O, reads[:3000], f"case {case}, rounds", pair_cap=len(ads) * 600)


@pytest.mark.parametrize("lens", [[20 + (7 * i) % 21 for i in range(96)], [12, 64, 20, 33, 34, 19, 21, 48]], ids=["96x20-40", "8x12-64"])
def test_mixed_equals_the_per_adapter_loop_at_scale(hip, lens):
    """500 k synthetic reads: the mixed form and the per-adapter loop of the same library agree read for read.
    The 64-mer of 8x12-64 reaches 70 characters back from the read's end: its tail classes are probed in all five chunks of
    the read's last half-row (multi2_read_len_ok, mixed plans)."""
    import torch
    from cutadapt_amd import _lib
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(11 + len(lens))
    ads = mixed_adapters(prng, lens)
    n_reads = 500_000
    batch = ReadBatch.synthetic(n_reads, 150, ads, seed=70 + len(lens), p_adapter=0.4, p_edit=0.04, p_n=0.01)
    plan, _ = plan_for(ads, 0.1, 3)
    assert plan.multi_kind(150) == "stream"
    a = match_batch(plan, batch)
    torch.cuda.synchronize()
    assert _lib.last_multi_path() == "stream"
    a6, ast, ab = a.out6.clone(), a.status.clone(), a.best_adapter.clone()
    with env(CAH_NO_MULTI_MIXED="1"):
        assert plan.multi_kind(150) == "sequential"
        b = match_batch(plan, batch)
        torch.cuda.synchronize()
        assert _lib.last_multi_path() == "sequential"
    assert torch.equal(ast, b.status)
    assert torch.equal(a6, b.out6)
    found = ast == 1
    assert torch.equal(ab[found], b.best_adapter[found])
    assert int(found.sum()) > 0.2 * n_reads


def test_views_and_frames(hip, orc):
    """a mixed plan on views inside a uniform batch (the RV form) and on a ragged packed batch in frames
    (cah_match_batch_frames), reads cut to 30..150 characters, against the oracle"""
    import torch
    from cutadapt_amd import _lib
    from cutadapt_amd import batch as B
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(21)
    ads = mixed_adapters(prng, [TRUSEQ_LIKE[i % 5] for i in range(10)] + [12, 52])
    plan, aobj = plan_for(ads, 0.1, 3)
    assert plan.multi_kind(150) == "stream"
    n = 70_000
    parent = ReadBatch.synthetic(n, 150, ads, seed=33, p_adapter=0.7, p_edit=0.04, p_n=0.004)
    idx = torch.arange(n, dtype=torch.int64, device=parent.device)
    lens = 30 + ((idx * 2654435761 + 977) >> 5) % 121                  # 30 .. 150
    lens[0] = 150
    starts = ((idx * 40503) >> 3) % (151 - lens)
    m_chk = 6000

    def against_oracle(got, seqs_t, off_t, len_t, what):
        h = seqs_t.cpu().numpy()
        ho, hl = off_t[:m_chk].cpu().numpy(), len_t[:m_chk].cpu().numpy()
        reads = [bytes(h[int(o):int(o) + int(l)]).decode("latin-1") for o, l in zip(ho, hl)]
        sq, offs = orc.pack_reads(reads)
        want6, want_st, want_best = oracle_multiple(orc, aobj, sq, offs)
        g6, gst = got.out6[:m_chk].cpu().numpy(), got.status[:m_chk].cpu().numpy()
        bad = np.nonzero((gst != want_st) | (g6 != want6).any(axis=1))[0]
        assert len(bad) == 0, (what, len(bad), int(bad[0]), reads[int(bad[0])], g6[bad[0]].tolist(), want6[bad[0]].tolist())
        fw = want_st == 1
        assert np.array_equal(got.best_adapter[:m_chk].cpu().numpy()[fw], want_best[fw]), what
        assert fw.mean() > 0.2

    view = parent.view(starts, lens)
    got = match_batch(plan, view)
    torch.cuda.synchronize()
    assert _lib.last_multi_path() == "stream"
    against_oracle(got, parent.seqs, parent.offsets[:n] + starts, lens, "views")
    # the same reads packed back to back, with an offsets array: frames of the longest read
    packed_off = torch.zeros(n + 1, dtype=torch.int64, device=parent.device)
    torch.cumsum(lens, 0, out=packed_off[1:])
    cols = torch.arange(150, device=parent.device)
    keep = cols[None, :] < lens[:, None]
    gather = (parent.offsets[:n] + starts)[:, None] + cols[None, :]
    packed = parent.seqs[gather[keep]].contiguous()
    pb = ReadBatch(packed, packed_off, validated=True)
    assert B._frame_len(plan, pb) == 150
    got2 = match_batch(plan, pb)
    torch.cuda.synchronize()
    assert _lib.last_multi_path() == "stream"
    against_oracle(got2, packed, packed_off[:n], lens, "frames")
    assert torch.equal(got.status, got2.status) and torch.equal(got.out6, got2.out6)
    # ... and without frames the packed ragged batch takes the per-adapter loop, with the same results
    with env(CAH_NO_FRAMES="1"):
        got3 = match_batch(plan, ReadBatch(packed, packed_off, validated=True))
        torch.cuda.synchronize()
        assert _lib.last_multi_path() == "sequential"
    assert torch.equal(got.status, got3.status) and torch.equal(got.out6, got3.out6)


def test_invalid_bytes_are_flagged(hip, orc):
    from cutadapt_amd import _lib
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(5)
    ads = mixed_adapters(prng, [12, 19, 20, 21, 33, 34, 40, 52, 25, 30])
    plan, _ = plan_for(ads, 0.1, 3)
    reads = [rs(prng, 150) for _ in range(300)]
    sq, offs = orc.pack_reads(reads)
    sq = sq.copy()
    for r in (0, 17, 63, 64, 299):
        sq[offs[r] + (r % 150)] = 0xC3
    flagged = []
    for off in (None, "1"):
        with env(CAH_NO_MULTI_MIXED=off):
            _g6, got_st, _ = match_batch(plan, ReadBatch.from_host(sq, offs)).cpu()
            assert _lib.last_multi_path() == ("stream" if off is None else "sequential")
        flagged.append(set(np.nonzero(got_st == 2)[0].tolist()))
    assert flagged[0] == flagged[1] == {0, 17, 63, 64, 299}


def test_what_stays_on_the_per_adapter_loop(hip, orc):
    """reads of 200 characters, seven adapters, and a plan from absolute max_errors: "sequential", and still the oracle's results"""
    from cutadapt_amd import _lib
    from cutadapt_amd import adapters as A
    rng = np.random.default_rng(8)
    prng = random.Random(9)
    ads = mixed_adapters(prng, [12, 52, 20, 33, 34, 19, 21, 40])
    check_uniform(orc, ads, 0.1, 3, reads_for(rng, prng, ads, 1500, 200), "reads of 200", expect="sequential")
    check_uniform(orc, ads[:7], 0.1, 3, reads_for(rng, prng, ads[:7], 1500, 150), "seven adapters", expect="sequential")
    with env(CAH_MULTI_MIXED_MIN="4"):
        check_uniform(orc, ads[:7], 0.1, 3, reads_for(rng, prng, ads[:7], 1500, 150), "seven adapters, lowered limit")
    objs = [A.BackAdapter(s, max_errors=2, min_overlap=3) for s in ads]         # another rate per length
    plan = _lib.Plan([a.matcher_spec() for a in objs])
    assert plan.multi_kind(150) == "sequential"


def test_pipeline_streams_and_gives_the_same_bytes(hip):
    """trim_fastq_gpu with the adapters of a file of TruSeq / Nextera / small-RNA-like lengths (10 adapters) on ragged reads
    of 40..150 characters: every chunk's matching call takes the streaming form (the pipeline hands a mixed plan its views in
    frames), none does with CAH_NO_MULTI_MIXED=1, and the output bytes are the same -- also with --revcomp and for reversed
    (rightmost) matching, whose second buffers go through the same call"""
    from cutadapt_amd import adapters as A
    from cutadapt_amd.gpu_pipeline import trim_fastq_gpu
    prng = random.Random(31)
    seqs = mixed_adapters(prng, [TRUSEQ_LIKE[i % 5] for i in range(10)])
    rng = np.random.default_rng(32)
    records = []
    for i in range(4000):
        n = prng.randrange(40, 151)
        read = reads_for(rng, prng, seqs, 2, n, p_n=0.0)[i % 2].upper()
        qual = "".join(chr(33 + prng.randrange(2, 41)) for _ in range(n))
        records.append(f"@r{i} x\n{read}\n+\n{qual}\n")
    data = np.frombuffer("".join(records).encode(), dtype=np.uint8)
    for opts in ({}, {"revcomp": True}, {"quality_cutoff": (0, 20)}):
        outs = []
        for off in (None, "1"):
            with env(CAH_NO_MULTI_MIXED=off):
                ads = [A.BackAdapter(s, max_errors=0.1, min_overlap=3) for s in seqs]
                buf = io.BytesIO()
                stats = trim_fastq_gpu(data, buf, ads, chunk_bytes=1 << 18, threads=2, **opts)
                calls = sum(d["stream_calls"] for d in stats["per_device"].values())
                chunks = sum(d["chunks"] for d in stats["per_device"].values())
                outs.append((buf.getvalue(), calls, chunks))
        assert outs[0][2] >= 2, outs[0][2]
        assert outs[0][1] == outs[0][2] * (2 if opts.get("revcomp") else 1), (opts, outs[0][1:], "the mixed form did not run")
        assert outs[1][1] == 0, (opts, outs[1][1:])
        assert outs[0][0] == outs[1][0] and len(outs[0][0]) > 0, opts
        assert outs[0][0] != data.tobytes()                               # (something was trimmed)
