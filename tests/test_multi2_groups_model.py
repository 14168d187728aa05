"""Host model of GROUPS of tables in the streaming multi-adapter path (cutadapt_amd/csrc/multi2.h: m2_build_groups): a plan
of more adapters (129..1024) or more k-mers than one table set holds goes through the streaming kernels as contiguous
groups of at most 128 adapters, merged under the adapters' indices in the plan.

No GPU: tests/host_model/multi2_groups_model.cpp compiles the product's splitter and table builders with g++, replays
every group with the existing model code and merges the groups' results in the product's key order (kernels.h: pack_best)
with the adapter's GLOBAL index.  The merged result must equal MultipleAdapters.match_to of the reference
(adapters.py:1265-1286) = the oracle's kmers_present + locate of every adapter on the whole read, best match by (score,
errors, first adapter) -- whatever the order the groups are replayed in.

What the splitter must keep: every adapter in exactly one group, contiguous ranges, at least 8 adapters per group, at
most 128; a plan that fits one table gives ONE group with tables equal byte for byte to the single builder's; a plan the
single builder refuses for a RULE (rate 0.08: error-free rows of 12 characters) stays refused, unsplit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_multi2_mixed_model import draw_reads, rand_seq
from test_multi2_model import matcher_blobs, oracle_multiple, ref_sets

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_model", "multi2_groups_model.cpp")
SO = os.path.join(HERE, "host_model", "libmulti2_groups_model.so")
CSRC = os.path.join(HERE, "..", "cutadapt_amd", "csrc")

REFUSED_NOT, REFUSED_CAPACITY, REFUSED_RULE = 0, 1, 2           # multi2.h: M2_REFUSED_*


@pytest.fixture(scope="module")
def groups_model():
    deps = [SRC] + [os.path.join(HERE, "host_model", f) for f in ("back_model.cpp", "multi2_model.cpp", "multi2_mixed_model.cpp")] + \
           [os.path.join(CSRC, h) for h in ("back_scan.h", "cah_device.h", "multi2.h", "multi_route.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    L.m2g_groups.argtypes = [C.c_char_p, i32, vp, i32, vp, vp, C.c_char_p, vp, vp]
    L.m2g_match_batch.argtypes = [C.c_char_p, i32, vp, i32, vp, vp, C.c_char_p, vp, vp, i64, vp, vp, vp, i32, i32]
    return L


class PlanData:
    def __init__(self, adapters, rate, min_overlap):
        self.adapters, self.rate, self.min_overlap = adapters, rate, min_overlap
        self.names = b"".join(a.encode() + b"\0" for a in adapters)
        self.blobs = matcher_blobs(adapters, rate, min_overlap)
        self.ra, self.rw, self.rk, self.per_adapter = ref_sets(adapters, rate, min_overlap)


def split(model, pd):
    """(G, [(base, count)], info) -- G 0: refused, info as m2g_groups documents it"""
    ranges = np.zeros(2 * 1024, dtype=np.int32)
    info = np.zeros(8, dtype=np.int32)
    G = model.m2g_groups(pd.names, len(pd.adapters), pd.blobs, len(pd.ra), pd.ra.ctypes.data, pd.rw.ctypes.data, pd.rk,
                         ranges.ctypes.data, info.ctypes.data)
    return G, [(int(ranges[2 * g]), int(ranges[2 * g + 1])) for g in range(max(G, 0))], info


def check_partition(n, G, ranges):
    """every adapter in exactly one group; contiguous ranges in order; 8..128 adapters per group"""
    assert G == len(ranges) >= 1
    at = 0
    for base, count in ranges:
        assert base == at, (ranges, "not contiguous")
        assert 8 <= count <= 128 or (G == 1 and count == n), ranges
        at += count
    assert at == n, ranges


def compare(model, pd, reads, label):
    seqs, offsets = orc.pack_reads(reads)
    n = len(offsets) - 1
    want6, want_st, want_best = oracle_multiple(pd.adapters, pd.rate, pd.min_overlap, pd.per_adapter, seqs, offsets)
    for subs, order in ((0, 0), (1, 1)):
        out6 = np.zeros((n, 6), dtype=np.int32)
        status = np.zeros(n, dtype=np.uint8)
        best = np.zeros(n, dtype=np.int32)
        G = model.m2g_match_batch(pd.names, len(pd.adapters), pd.blobs, len(pd.ra), pd.ra.ctypes.data, pd.rw.ctypes.data, pd.rk,
                                  seqs.ctypes.data, offsets.ctypes.data, n, out6.ctypes.data, status.ctypes.data,
                                  best.ctypes.data, subs, order)
        assert G >= 1, f"{label}: refused"
        bad = np.nonzero((status != want_st) | (out6 != want6).any(axis=1) | ((status == 1) & (best != want_best)))[0]
        if len(bad):
            r = int(bad[0])
            read = bytes(seqs[offsets[r]:offsets[r + 1]]).decode("latin-1")
            raise AssertionError(f"{label} (subs {subs}, order {order}): {len(bad)} of {n} reads differ; first: read {r} {read!r} "
                                 f"model {status[r]} {out6[r].tolist()} adapter {best[r]} oracle {want_st[r]} {want6[r].tolist()} "
                                 f"adapter {want_best[r]}")
    assert (want_st == 1).mean() > 0.2, label
    return want_best


def mixed_adapters(rng, count, lo, hi):
    ads = []
    seen = set()
    while len(ads) < count:
        s = rand_seq(rng, int(rng.integers(lo, hi + 1)))
        if s not in seen:
            seen.add(s)
            ads.append(s)
    return ads


# (count, rate, read length): the counts around the borders of two and three groups, either rate, every read length
BORDER_PLANS = [(129, 0.1, 150), (130, 0.2, 48), (256, 0.2, 151), (257, 0.1, 150), (300, 0.2, 150)]


@pytest.mark.parametrize("count,rate,read_len", BORDER_PLANS)
def test_counts_at_the_group_border(groups_model, count, rate, read_len):
    rng = np.random.default_rng(7000 + count)
    ads = mixed_adapters(rng, count, 20, 40)
    pd = PlanData(ads, rate, 3)
    G, ranges, info = split(groups_model, pd)
    assert G >= (count + 127) // 128 and info[0] == REFUSED_NOT and info[3] == 1, (G, info.tolist())
    check_partition(count, G, ranges)
    if rate == 0.1:
        # (about 24 entries per adapter at this rate: the cut by count is all there is -- near-equal groups, never 128 + 1)
        assert G == (count + 127) // 128, ranges
        assert max(c for _, c in ranges) - min(c for _, c in ranges) <= 1, ranges
    best = compare(groups_model, pd, draw_reads(rng, ads, read_len, 600), f"{count} adapters, rate {rate}, reads of {read_len}")
    # the winners come from every group
    for base, cnt in ranges:
        assert ((best >= base) & (best < base + cnt)).any(), (base, cnt)


def test_384_adapters_of_one_length(groups_model):
    rng = np.random.default_rng(7384)
    ads = mixed_adapters(rng, 384, 33, 33)
    pd = PlanData(ads, 0.1, 3)
    G, ranges, info = split(groups_model, pd)
    # (128 33-mers have about 3 000 k-mer entries, a table holds 2 304 -- 96 such adapters: the three groups by count are halved)
    assert G == 6 and ranges == [(64 * g, 64) for g in range(6)] and info[3] == 1, (G, ranges, info.tolist())
    compare(groups_model, pd, draw_reads(rng, ads, 150, 600), "384 33-mers")


def test_1024_short_adapters(groups_model):
    rng = np.random.default_rng(71024)
    ads = mixed_adapters(rng, 1024, 16, 24)
    pd = PlanData(ads, 0.1, 3)
    G, ranges, info = split(groups_model, pd)
    assert G >= 8 and info[3] == 1, (G, info.tolist())
    check_partition(1024, G, ranges)
    compare(groups_model, pd, draw_reads(rng, ads, 150, 500), "1024 adapters of 16..24")


def test_more_than_1024_adapters_are_refused(groups_model):
    rng = np.random.default_rng(71025)
    ads = mixed_adapters(rng, 1025, 16, 18)
    pd = PlanData(ads, 0.1, 3)
    G, _ranges, _info = split(groups_model, pd)
    assert G == 0


def capacity_plan(rng):
    """96 adapters of 20..40 characters at rate 0.2: more k-mer entries than one table holds"""
    return mixed_adapters(rng, 96, 20, 40), 0.2


def test_a_plan_refused_for_entries_is_split(groups_model):
    rng = np.random.default_rng(7096)
    ads, rate = capacity_plan(rng)
    pd = PlanData(ads, rate, 3)
    G, ranges, info = split(groups_model, pd)
    # the single builder refuses the whole plan, for CAPACITY alone
    assert info[1] == 0 and info[2] == REFUSED_CAPACITY, info.tolist()
    assert G >= 2 and info[0] == REFUSED_NOT and info[3] == 1, (G, info.tolist())
    check_partition(96, G, ranges)
    assert info[4] <= 2304
    compare(groups_model, pd, draw_reads(rng, ads, 150, 600), "96 adapters, rate 0.2")


@pytest.mark.parametrize("count", [40, 200])
def test_a_plan_refused_for_a_rule_stays_refused(groups_model, count):
    rng = np.random.default_rng(7008 + count)
    ads = mixed_adapters(rng, count, 20, 40)
    pd = PlanData(ads, 0.08, 3)
    G, _ranges, info = split(groups_model, pd)
    assert G == 0 and info[0] == REFUSED_RULE, (G, info.tolist())
    if count <= 128:
        assert info[1] == 0 and info[2] == REFUSED_RULE, info.tolist()


@pytest.mark.parametrize("lo,hi,count,rate", [(20, 40, 24, 0.1), (33, 33, 96, 0.1), (19, 34, 128, 0.1), (12, 64, 9, 0.25)])
def test_a_plan_that_fits_one_table_is_one_group(groups_model, lo, hi, count, rate):
    rng = np.random.default_rng(7100 + count)
    ads = mixed_adapters(rng, count, lo, hi)
    pd = PlanData(ads, rate, 3)
    G, ranges, info = split(groups_model, pd)
    assert info[1] == 1, "the single builder must take this plan"
    # one group over the whole plan, its tables byte for byte the single builder's
    assert G == 1 and ranges == [(0, count)] and info[3] == 1, (G, ranges, info.tolist())


def test_ties_across_groups(groups_model):
    """the same sequence in the first and in the last group answers the first; a prefix of an adapter of another group"""
    rng = np.random.default_rng(7200)
    ads = mixed_adapters(rng, 200, 24, 36)
    ads[150] = ads[3][:20]                                    # a prefix, in the other group
    ads.append(ads[5])                                        # the same sequence again, at the plan's end
    pd = PlanData(ads, 0.1, 3)
    G, ranges, _info = split(groups_model, pd)
    assert G == 2
    reads = draw_reads(rng, [ads[3], ads[5], ads[150]], 150, 600)
    best = compare(groups_model, pd, reads, "ties")
    assert (best == 5).any() and not (best == 200).any()
