"""Host-model fuzz of the MIXED form of the streaming multi-adapter path: adapters of different lengths in one plan
(cutadapt_amd/csrc/multi2.h: m2_build_mixed; multi2.hip: k_multi_scan<KIND, true>; kernels.hip: k_dp_packed<.., true, true>).

No GPU: tests/host_model/multi2_mixed_model.cpp compiles the product's table builder and rules with g++ and replays what
the kernels do read by read -- the prefilter of the one-shape plans unchanged, every pair's scan and cell DP with its own
adapter's length.  The merged result must equal MultipleAdapters.match_to of the reference (adapters.py:1265-1286) = the
oracle's kmers_present + locate of every adapter on the WHOLE read, best match by (score, errors, first adapter).

Which plans the builder refuses, and why (multi2.h): rate 0.08 always -- its error-free rows reach 12 characters, the
suffix compare holds ten; 96 and 128 adapters at the higher rates -- more than CAH_M2_MAX_ENTRIES k-mers, as for
adapters of one length.  The generator draws every rate and count of the issue's lists, those less often; the share of
its plans that must be accepted is two thirds, asserted chunk by chunk (measured: 234 of 300)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from test_multi2_model import matcher_blobs, oracle_multiple, ref_sets, tail_reads
from test_multi2_model import model as one_shape_model  # noqa: F401  (the fixture of the one-shape model)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_model", "multi2_mixed_model.cpp")
SO = os.path.join(HERE, "host_model", "libmulti2_mixed_model.so")
CSRC = os.path.join(HERE, "..", "cutadapt_amd", "csrc")

N_CHUNKS = 10
PLANS_PER_CHUNK = 30                    # 300 plans
READS_PER_PLAN = 700


@pytest.fixture(scope="module")
def mixed_model():
    deps = [SRC] + [os.path.join(HERE, "host_model", f) for f in ("back_model.cpp", "multi2_model.cpp")] + \
           [os.path.join(CSRC, h) for h in ("back_scan.h", "cah_device.h", "multi2.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    L.m2x_match_batch.argtypes = [C.c_char_p, i32, vp, i32, vp, vp, C.c_char_p, vp, vp, i64, vp, vp, vp, i32, vp, vp]
    L.m2m_match_batch.argtypes = [C.c_char_p, i32, i32, vp, i32, vp, vp, C.c_char_p, vp, vp, i64, vp, vp, vp, i32, vp, vp]
    return L


def call_mixed(model, adapters, blobs, refs, seqs, offsets, subs, pads=None):
    ra, rw, rk = refs
    n = len(offsets) - 1
    out6 = np.zeros((n, 6), dtype=np.int32)
    status = np.zeros(n, dtype=np.uint8)
    best = np.zeros(n, dtype=np.int32)
    stats = np.zeros(16, dtype=np.int64)
    rc = model.m2x_match_batch(b"".join(a.encode() + b"\0" for a in adapters), len(adapters), blobs, len(ra), ra.ctypes.data,
                               rw.ctypes.data, rk, seqs.ctypes.data, offsets.ctypes.data, n, out6.ctypes.data,
                               status.ctypes.data, best.ctypes.data, subs, stats.ctypes.data,
                               None if pads is None else pads.ctypes.data)
    return rc, out6, status, best, stats


def run_mixed(model, adapters, rate, min_overlap, seqs, offsets, label, pads=None):
    """None when the builder refuses the plan; else the statistics of the untracked replay"""
    blobs = matcher_blobs(adapters, rate, min_overlap)
    ra, rw, rk, per_adapter = ref_sets(adapters, rate, min_overlap)
    want = None
    totals = None
    for subs in (0, 1):
        rc, out6, status, best, stats = call_mixed(model, adapters, blobs, (ra, rw, rk), seqs, offsets, subs, pads)
        if rc == 1:
            return None
        if want is None:
            want = oracle_multiple(adapters, rate, min_overlap, per_adapter, seqs, offsets)
        want6, want_st, want_best = want
        bad = np.nonzero((status != want_st) | (out6 != want6).any(axis=1) | ((status == 1) & (best != want_best)))[0]
        if len(bad):
            r = int(bad[0])
            read = bytes(seqs[offsets[r]:offsets[r + 1]]).decode("latin-1")
            raise AssertionError(f"{label} (subs {subs}): {len(bad)} of {len(offsets) - 1} reads differ; first: read {r} {read!r} "
                                 f"model {status[r]} {out6[r].tolist()} adapter {best[r]} "
                                 f"({adapters[best[r]] if best[r] >= 0 else None}) oracle {want_st[r]} {want6[r].tolist()} "
                                 f"adapter {want_best[r]} ({adapters[want_best[r]] if want_best[r] >= 0 else None})")
        if subs == 0:
            totals = stats
    return totals


def rand_seq(rng, m):
    return "".join(rng.choice(list("ACGT"), size=m))


def draw_plan(rng, it):
    """(adapters, rate, min_overlap, read length) from the lists of the issue.  The table holds CAH_M2_MAX_ENTRIES k-mers
    (multi2.h) whichever builder fills it -- about 24 per adapter: the large counts are drawn less often and with the bulk
    of their lengths from 20..40, the adapter files the form is for"""
    count = int(rng.choice([8, 9, 24, 96, 128], p=[0.3, 0.25, 0.25, 0.1, 0.1]))
    lo, hi = (12, 65) if count < 96 else (20, 41)
    # (rate 0.08 is always refused -- the module's head: drawn, but less often than the rates that test the kernels' rules)
    rate = float(rng.choice([0.08, 0.1, 0.15, 0.2, 0.25], p=[0.08, 0.23, 0.23, 0.23, 0.23]))
    O = int(rng.choice([1, 3, 5, 8]))
    mode = it % 4
    if mode == 0:
        lens = [12, 64] + [int(x) for x in rng.integers(lo, hi, size=count - 2)]
    elif mode == 1:
        lens = [32, 33] + [int(x) for x in rng.integers(lo, hi, size=count - 2)]
    elif mode == 2:
        lens = [(19, 20, 21, 33, 34)[i % 5] for i in range(count)]
    else:
        lens = [int(x) for x in rng.integers(lo, hi, size=count)]
        if len(set(lens)) == 1:
            lens[0] = 12 if lens[0] != 12 else 13
    ads = [rand_seq(rng, m) for m in lens]
    if it % 5 == 1:
        # near-duplicates: a prefix of another adapter, two that differ in their last character only, a repetitive one
        ads[1] = ads[0][:max(12, len(ads[0]) - int(rng.integers(1, 8)))] if len(ads[0]) > 12 else ads[0] + "ACGT"
        ads[3] = ads[2][:-1] + ("A" if ads[2][-1] != "A" else "C")
        unit = rand_seq(rng, int(rng.integers(1, 4)))
        ads[4] = (unit * 64)[:len(ads[4])]
    ads = list(dict.fromkeys(ads))
    n = int(rng.integers(16, 161))                                       # (reads shorter than the longest adapter included)
    return ads, rate, O, n


def draw_reads(rng, ads, n, count):
    """reads of n characters: adapter prefixes at the end with edits, whole adapters inside (edited), N and lower case"""
    half = count // 2
    reads = tail_reads(rng, ads, half, n, p_n=float(rng.choice([0.0, 0.01])))
    bases = list("ACGT")
    for _ in range(count - half):
        body = list(rng.choice(bases, size=n))
        if rng.random() < 0.8:
            ad = list(ads[int(rng.integers(0, len(ads)))])
            for _e in range(int(rng.integers(0, 1 + max(1, len(ad) // 6)))):
                u, pos = rng.random(), int(rng.integers(0, len(ad)))
                if u < 0.5:
                    ad[pos] = str(rng.choice(bases))
                elif u < 0.75:
                    ad.insert(pos, str(rng.choice(bases)))
                elif len(ad) > 1:
                    del ad[pos]
            at = int(rng.integers(0, n))
            body[at:at + len(ad)] = ad
        if rng.random() < 0.02:
            body[int(rng.integers(0, n))] = "N"
        reads.append("".join(body[:n]))
    reads = [r if len(r) == n else (r + "A" * n)[:n] for r in reads]
    return [r.lower() if i % 5 == 0 else r for i, r in enumerate(reads)]


_accepted = {}


@pytest.mark.parametrize("chunk", range(N_CHUNKS))
def test_mixed_plans_against_the_oracle(mixed_model, chunk):
    rng = np.random.default_rng(9000 + chunk)
    built = 0
    for it in range(chunk * PLANS_PER_CHUNK, (chunk + 1) * PLANS_PER_CHUNK):
        ads, rate, O, n = draw_plan(rng, it)
        reads = draw_reads(rng, ads, n, READS_PER_PLAN)
        seqs, offsets = orc.pack_reads(reads)
        lens = sorted(set(len(a) for a in ads))
        st = run_mixed(mixed_model, ads, rate, O, seqs, offsets,
                       f"plan {it}: {len(ads)} adapters of {lens[0]}..{lens[-1]}, rate {rate}, O {O}, n {n}")
        built += st is not None
    _accepted[chunk] = built


def test_the_builder_accepts_two_thirds_of_the_plans(mixed_model):
    """the cap that keeps the fuzz from passing by refusing everything, over all the plans it draws (a chunk that has not
    run in this process is drawn again and asked with one read)"""
    for chunk in range(N_CHUNKS):
        if chunk in _accepted:
            continue
        rng = np.random.default_rng(9000 + chunk)
        built = 0
        for it in range(chunk * PLANS_PER_CHUNK, (chunk + 1) * PLANS_PER_CHUNK):
            ads, rate, O, n = draw_plan(rng, it)
            reads = draw_reads(rng, ads, n, READS_PER_PLAN)
            seqs, offsets = orc.pack_reads(reads[:1])
            ra, rw, rk, _ = ref_sets(ads, rate, O)
            built += call_mixed(mixed_model, ads, matcher_blobs(ads, rate, O), (ra, rw, rk), seqs, offsets, 0)[0] == 0
        _accepted[chunk] = built
    total = sum(_accepted[c] for c in range(N_CHUNKS))
    assert 3 * total >= 2 * N_CHUNKS * PLANS_PER_CHUNK, f"the mixed builder accepted {total} of {N_CHUNKS * PLANS_PER_CHUNK} plans"


def test_views_in_a_padded_frame(mixed_model):
    """views of a frame (k_multi_stream's RV form): prefilter and scan on the end-aligned frame, the cell DP and every
    coordinate on the view"""
    rng = np.random.default_rng(9100)
    built = 0
    for it in range(8):
        ads, rate, O, _n = draw_plan(rng, 2 + 4 * it)
        rate = max(rate, 0.1)
        N = int(rng.choice([100, 150, 151, 160]))
        reads = draw_reads(rng, ads, N, 400)
        views = []
        for i, r in enumerate(reads):
            mode = i % 4
            a = int(rng.integers(0, N + 1)) if mode in (1, 3) else 0
            b = int(rng.integers(a, N + 1)) if mode in (2, 3) else N
            views.append(r[a:b])
        seqs, offsets = orc.pack_reads(views)
        pads = (N - np.diff(offsets)).astype(np.int32)
        built += run_mixed(mixed_model, ads, rate, O, seqs, offsets, f"views {it} rate {rate} O {O} N {N}", pads=pads) is not None
    assert built >= 5, built


def test_equal_lengths_give_what_the_one_shape_builder_gives(mixed_model):
    """a plan of equally long adapters put through the mixed builder: the merged results of m2_build's tables"""
    rng = np.random.default_rng(9200)
    for m, rate, O, count in ((33, 0.1, 3, 24), (20, 0.15, 5, 8), (64, 0.1, 1, 9), (30, 0.2, 3, 12)):
        ads = [rand_seq(rng, m) for _ in range(count)]
        reads = draw_reads(rng, ads, 150, 1500)
        seqs, offsets = orc.pack_reads(reads)
        blobs = matcher_blobs(ads, rate, O)
        ra, rw, rk, _per = ref_sets(ads, rate, O)
        n = len(offsets) - 1
        for subs in (0, 1):
            rc, out6, status, best, _ = call_mixed(mixed_model, ads, blobs, (ra, rw, rk), seqs, offsets, subs)
            assert rc == 0, (m, rate)
            o6 = np.zeros((n, 6), dtype=np.int32)
            st = np.zeros(n, dtype=np.uint8)
            bs = np.zeros(n, dtype=np.int32)
            rc = mixed_model.m2m_match_batch("".join(ads).encode(), count, m, blobs, len(ra), ra.ctypes.data, rw.ctypes.data, rk,
                                             seqs.ctypes.data, offsets.ctypes.data, n, o6.ctypes.data, st.ctypes.data,
                                             bs.ctypes.data, subs, None, None)
            assert rc == 0, (m, rate)
            assert (status == st).all() and (out6 == o6).all() and (best[st == 1] == bs[st == 1]).all(), (m, rate, subs)
            assert (st == 1).mean() > 0.2


def test_what_the_builder_refuses(mixed_model):
    """a plan whose thresholds do not agree row by row (absolute max_errors: another rate per length) and a 0.08 plan"""
    rng = np.random.default_rng(9300)
    ads = [rand_seq(rng, m) for m in (20, 20, 24, 30, 33, 33, 34, 40)]
    seqs, offsets = orc.pack_reads(draw_reads(rng, ads, 100, 50))
    blobs = b"".join(matcher_blobs([a], 2.0 / len(a) + 1e-9, 3) for a in ads)          # max_errors = 2 for every length
    ra, rw, rk, _ = ref_sets(ads, 0.1, 3)
    assert call_mixed(mixed_model, ads, blobs, (ra, rw, rk), seqs, offsets, 0)[0] == 1
    assert run_mixed(mixed_model, ads, 0.08, 3, seqs, offsets, "rate 0.08") is None
    assert run_mixed(mixed_model, ads, 0.1, 3, seqs, offsets, "rate 0.1") is not None
