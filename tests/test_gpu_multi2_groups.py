"""GROUPS of tables in the streaming multi-adapter path on the GPU: a plan of more adapters (129..1024) or more k-mers than
one table set holds (cutadapt_amd/csrc/api.cpp: build_multi_groups; multi2.h: m2_build_groups; the kernels' adapter_base)
against the oracle applying MultipleAdapters' rule (reference adapters.py:1265-1286) and against the per-adapter loop of
the same library (CAH_NO_MULTI_GROUPS=1: what such a plan took before).  The CPU twin of the splitter and the merge is
tests/test_multi2_groups_model.py."""
import io
import random

import numpy as np
import pytest

from test_gpu_multi import env, oracle_multiple, plan_for, rs
from test_gpu_multi2_mixed import reads_for

pytestmark = pytest.mark.gpu


def distinct(prng, lens):
    out, seen = [], set()
    for m in lens:
        s = rs(prng, m)
        while s in seen:
            s = rs(prng, m)
        seen.add(s)
        out.append(s)
    return out


def lens_20_40(count):
    return [20 + (7 * i) % 21 for i in range(count)]


class Case:
    """a plan, reads of one length and the oracle's answer for them -- computed once, shared by the checks of a test"""

    def __init__(self, orc, seqs, rate, O, reads, expect="stream", groups=None):
        self.orc, self.seqs, self.reads, self.expect = orc, seqs, reads, expect
        self.plan, self.ads = plan_for(seqs, rate, O)
        self.n = len(reads[0])
        self.sq, self.offs = orc.pack_reads(reads)
        self.want = oracle_multiple(orc, self.ads, self.sq, self.offs)
        G = self.plan.multi_groups()
        assert self.plan.multi_kind(self.n) == expect, (self.plan.multi_kind(self.n), G)
        if expect == "stream":
            assert G > 1 and (groups is None or G == groups), G
        self.G = G

    def check(self, what, count=None, pair_cap=None, expect=None):
        from cutadapt_amd import _lib
        from cutadapt_amd.batch import ReadBatch, match_batch
        count = len(self.reads) if count is None else count
        expect = expect or self.expect
        offs = self.offs[:count + 1]
        sq = self.sq[:offs[-1]]
        with env(CAH_MULTI_PAIR_CAP=pair_cap):
            got6, got_st, got_best = match_batch(self.plan, ReadBatch.from_host(sq, offs)).cpu()
            assert _lib.last_multi_path() == expect, (what, _lib.last_multi_path())
        want6, want_st, want_best = (w[:count] for w in self.want)
        bad = np.nonzero((got_st != want_st) | (got6 != want6).any(axis=1))[0]
        assert len(bad) == 0, (what, len(bad), bad[:5], got_st[bad[:3]], got6[bad[:3]], want_st[bad[:3]], want6[bad[:3]],
                               self.reads[int(bad[0])])
        f = want_st == 1
        assert np.array_equal(got_best[f], want_best[f]), (what, np.nonzero(got_best[f] != want_best[f])[0][:5])
        return got_best[f]


@pytest.mark.parametrize("count,rate", [(129, 0.1), (130, 0.2), (256, 0.1), (257, 0.2), (300, 0.1)])
def test_counts_at_the_group_border(hip, orc, count, rate):
    rng = np.random.default_rng(800 + count)
    prng = random.Random(900 + count)
    seqs = distinct(prng, lens_20_40(count))
    c = Case(orc, seqs, rate, 3, reads_for(rng, prng, seqs, 3000, 150))
    assert c.G >= (count + 127) // 128
    best = c.check(f"{count} adapters x 3000")
    # the winners come from the first and from the last group, under their indices in the plan
    assert (best < 64).any() and (best >= count - 40).any()
    for n in (63, 64, 65):
        c.check(f"{count} adapters x {n}", count=n)


def test_1024_short_adapters(hip, orc):
    rng = np.random.default_rng(1024)
    prng = random.Random(1024)
    seqs = distinct(prng, [16 + (5 * i) % 9 for i in range(1024)])
    c = Case(orc, seqs, 0.1, 3, reads_for(rng, prng, seqs, 1500, 150))
    assert c.G >= 8
    best = c.check("1024 adapters x 1500")
    assert (best >= 896).any()


def test_a_plan_split_for_capacity(hip, orc):
    """96 adapters of 20..40 characters at rate 0.2: more k-mer entries than one table holds (the model's pick:
    tests/test_multi2_groups_model.py) -- two or more groups although the count would fit one"""
    rng = np.random.default_rng(96)
    prng = random.Random(3)
    seqs = distinct(prng, [20 + prng.randrange(21) for _ in range(96)])
    c = Case(orc, seqs, 0.2, 3, reads_for(rng, prng, seqs, 3000, 150))
    c.check("96 adapters at 0.2")
    with env(CAH_NO_MULTI_GROUPS="1"):
        assert c.plan.multi_kind(150) == "sequential"
        c.check("96 adapters at 0.2, the loop", expect="sequential")


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_ties_across_groups(hip, orc, reverse):
    """the same sequence in the first and in the last group answers the first; two adapters of different groups that share
    their first twelve characters tie on a read that ends with those (the lower index wins); a prefix of an adapter of the
    other group -- and all of it once more with the adapter list reversed"""
    rng = np.random.default_rng(77)
    prng = random.Random(77)
    seqs = distinct(prng, lens_20_40(200))
    seqs[190] = seqs[3]
    seqs[150] = seqs[20][:12] + rs(prng, len(seqs[150]) - 12)
    seqs[170] = seqs[7][:18]
    special = [seqs[3], seqs[150], seqs[20], seqs[170], seqs[7]]
    shared = seqs[20][:12]
    if reverse:
        seqs = seqs[::-1]
    reads = reads_for(rng, prng, special, 1200, 150) + [rs(prng, 138) + shared for _ in range(50)]
    c = Case(orc, seqs, 0.1, 3, reads, groups=2)
    best = c.check("ties")
    dup_first, dup_last = (3, 190) if not reverse else (9, 196)
    assert (best == dup_first).any() and not (best == dup_last).any()
    assert (c.want[1][-50:] == 1).all()


def test_small_pool_rounds_per_group(hip, orc):
    rng = np.random.default_rng(31)
    prng = random.Random(31)
    seqs = distinct(prng, lens_20_40(200))
    c = Case(orc, seqs, 0.1, 3, reads_for(rng, prng, seqs, 3000, 150), groups=2)
    c.check("rounds", pair_cap=600 * 100)


def test_views_and_frames(hip, orc):
    """200 adapters on views inside a uniform batch (the RV form) and on a ragged packed batch in frames"""
    import torch
    from cutadapt_amd import _lib
    from cutadapt_amd import batch as B
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(41)
    seqs = distinct(prng, lens_20_40(200))
    plan, aobj = plan_for(seqs, 0.1, 3)
    assert plan.multi_kind(150) == "stream" and plan.multi_groups() == 2
    n = 70_000                                                        # (batch.py frames a ragged batch from 65 536 reads on)
    parent = ReadBatch.synthetic(n, 150, seqs, seed=43, p_adapter=0.7, p_edit=0.04, p_n=0.004)
    idx = torch.arange(n, dtype=torch.int64, device=parent.device)
    lens = 30 + ((idx * 2654435761 + 977) >> 5) % 121                  # 30 .. 150
    lens[0] = 150
    starts = ((idx * 40503) >> 3) % (151 - lens)
    m_chk = 2000

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

    got = match_batch(plan, parent.view(starts, lens))
    torch.cuda.synchronize()
    assert _lib.last_multi_path() == "stream"
    against_oracle(got, parent.seqs, parent.offsets[:n] + starts, lens, "views")
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
    assert torch.equal(got.status, got2.status) and torch.equal(got.out6, got2.out6)
    assert torch.equal(got.best_adapter, got2.best_adapter)
    # ... and without frames the packed ragged batch takes the per-adapter loop, with the same results
    with env(CAH_NO_FRAMES="1"):
        got3 = match_batch(plan, ReadBatch(packed, packed_off, validated=True))
        torch.cuda.synchronize()
        assert _lib.last_multi_path() == "sequential"
    assert torch.equal(got.status, got3.status) and torch.equal(got.out6, got3.out6)


def test_invalid_bytes_and_deferred_errors(hip, orc):
    """a byte >= 0x80 flags its read (status 2) whatever the later groups find; the deferred error check gives the same rows"""
    from cutadapt_amd import _lib
    from cutadapt_amd.batch import ReadBatch, match_batch
    rng = np.random.default_rng(51)
    prng = random.Random(51)
    seqs = distinct(prng, lens_20_40(300))
    plan, _ = plan_for(seqs, 0.1, 3)
    assert plan.multi_kind(150) == "stream" and plan.multi_groups() == 3
    reads = reads_for(rng, prng, seqs, 600, 150)
    # (reads that END with an adapter of the last group: its kernels find something in the flagged reads too)
    for r in (0, 17, 63, 64, 599):
        reads[r] = reads[r][:110] + seqs[290 + r % 10][:40].ljust(40, "A")[:40]
    sq, offs = orc.pack_reads(reads)
    sq = sq.copy()
    for r in (0, 17, 63, 64, 599):
        sq[offs[r] + (r % 100)] = 0xC3
    out = []
    for mode in ("plain", "deferred", "loop"):
        was = _lib.lib().cah_set_deferred_errors(1 if mode == "deferred" else 0)
        try:
            with env(CAH_NO_MULTI_GROUPS="1" if mode == "loop" else None):
                g6, gst, gbest = match_batch(plan, ReadBatch.from_host(sq, offs)).cpu()
                assert _lib.last_multi_path() == ("sequential" if mode == "loop" else "stream"), mode
        finally:
            _lib.lib().cah_set_deferred_errors(was)
        assert set(np.nonzero(gst == 2)[0].tolist()) == {0, 17, 63, 64, 599}, mode
        out.append((g6, gst, gbest))
    for g6, gst, gbest in out[1:]:
        assert np.array_equal(gst, out[0][1]) and np.array_equal(g6, out[0][0])
        f = gst == 1
        assert np.array_equal(gbest[f], out[0][2][f])
    assert (out[0][1] == 1).mean() > 0.2


def test_groups_equal_the_per_adapter_loop_at_scale(hip):
    """200 k synthetic reads x 300 adapters: the grouped form and the per-adapter loop of the same library agree read for read"""
    import torch
    from cutadapt_amd import _lib
    from cutadapt_amd.batch import ReadBatch, match_batch
    prng = random.Random(311)
    seqs = distinct(prng, lens_20_40(300))
    batch = ReadBatch.synthetic(200_000, 150, seqs, seed=71, p_adapter=0.4, p_edit=0.04, p_n=0.01)
    plan, _ = plan_for(seqs, 0.1, 3)
    assert plan.multi_kind(150) == "stream" and plan.multi_groups() == 3
    a = match_batch(plan, batch)
    torch.cuda.synchronize()
    assert _lib.last_multi_path() == "stream"
    a6, ast, ab = a.out6.clone(), a.status.clone(), a.best_adapter.clone()
    with env(CAH_NO_MULTI_GROUPS="1"):
        assert plan.multi_kind(150) == "sequential"
        b = match_batch(plan, batch)
        torch.cuda.synchronize()
        assert _lib.last_multi_path() == "sequential"
    assert torch.equal(ast, b.status)
    assert torch.equal(a6, b.out6)
    found = ast == 1
    assert torch.equal(ab[found], b.best_adapter[found])
    assert int(found.sum()) > 0.2 * 200_000


def test_unchanged_ground(hip, orc):
    """a 96-adapter plan that fits one table is one group; 1 025 adapters, reads of 200 and a plan from absolute max_errors
    stay on the per-adapter loop, with the oracle's results"""
    from cutadapt_amd import _lib
    from cutadapt_amd import adapters as A
    rng = np.random.default_rng(61)
    prng = random.Random(61)
    fits = distinct(prng, lens_20_40(96))
    plan, _ = plan_for(fits, 0.1, 3)
    assert plan.multi_kind(150) == "stream" and plan.multi_groups() == 1
    one = distinct(prng, [33] * 96)
    plan, _ = plan_for(one, 0.1, 3)
    assert plan.multi_kind(150) == "stream" and plan.multi_groups() == 1
    many = distinct(prng, [16 + (5 * i) % 9 for i in range(1025)])
    c = Case(orc, many, 0.1, 3, reads_for(rng, prng, many, 300, 150), expect="sequential")
    assert c.G == 0
    c.check("1025 adapters")
    seqs = distinct(prng, lens_20_40(200))
    c = Case(orc, seqs, 0.1, 3, reads_for(rng, prng, seqs, 600, 200), expect="sequential")
    assert c.G == 2                                                   # (the tables exist: reads of 150 would stream)
    c.check("reads of 200")
    objs = [A.BackAdapter(s, max_errors=2, min_overlap=3) for s in seqs]          # another rate per length
    plan = _lib.Plan([a.matcher_spec() for a in objs])
    assert plan.multi_kind(150) == "sequential" and plan.multi_groups() == 0


def test_pipeline_streams_and_gives_the_same_bytes(hip):
    """trim_fastq_gpu with 150 adapters on ragged reads of 40..150 characters: every chunk's matching call streams, none
    does with CAH_NO_MULTI_GROUPS=1, and the output bytes are the same"""
    from cutadapt_amd import adapters as A
    from cutadapt_amd.gpu_pipeline import trim_fastq_gpu
    prng = random.Random(131)
    seqs = distinct(prng, lens_20_40(150))
    rng = np.random.default_rng(132)
    records = []
    for i in range(3000):
        n = prng.randrange(40, 151)
        read = reads_for(rng, prng, seqs, 2, n, p_n=0.0)[i % 2].upper()
        qual = "".join(chr(33 + prng.randrange(2, 41)) for _ in range(n))
        records.append(f"@r{i} x\n{read}\n+\n{qual}\n")
    data = np.frombuffer("".join(records).encode(), dtype=np.uint8)
    outs = []
    for off in (None, "1"):
        with env(CAH_NO_MULTI_GROUPS=off):
            ads = [A.BackAdapter(s, max_errors=0.1, min_overlap=3) for s in seqs]
            buf = io.BytesIO()
            stats = trim_fastq_gpu(data, buf, ads, chunk_bytes=1 << 18, threads=2)
            calls = sum(d["stream_calls"] for d in stats["per_device"].values())
            chunks = sum(d["chunks"] for d in stats["per_device"].values())
            outs.append((buf.getvalue(), calls, chunks))
    assert outs[0][2] >= 2, outs[0][2]
    assert outs[0][1] == outs[0][2], (outs[0][1:], "the grouped form did not run")
    assert outs[1][1] == 0, outs[1][1:]
    assert outs[0][0] == outs[1][0] and len(outs[0][0]) > 0
    assert outs[0][0] != data.tobytes()                               # (something was trimmed)
