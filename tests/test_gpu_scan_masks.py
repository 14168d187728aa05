"""k_back_scan's column loop without predicates carried from column to column (GPU): the first EXACT_FULL column is noted
inside the step's rare booking branch, the guarded copy of the sixteen-column body compares a constant with the lane's
remaining columns.  Through the public match_batch only, bit for bit against the oracle, on batches BUILT to hold every
class the scan decides and the places where the new forms could go wrong -- and checked on the CPU to hold them."""
import functools
import os
import random

import numpy as np
import pytest

N_READS = 8192                       # above the 4 096 work-list entries at which the straggler launch switches on
ADAPTER_LENGTHS = (20, 32, 33, 34, 40)   # scan forms: one 32-bit word (20, 32), + 1 / 2 explicit rows (33 / 34), 64-bit (40)
RATE, MIN_OVERLAP = 0.1, 3


def _adapter(m):
    rng = random.Random(1000 + m)
    while True:
        a = "".join(rng.choice("ACGT") for _ in range(m))
        if all(a[i:i + 4] != a[i + 1:i + 5] for i in range(m - 4)):        # no long homopolymer: indels stay indels
            return a


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _subst(rng, s, positions):
    s = list(s)
    for i in positions:
        s[i] = rng.choice([c for c in "ACGT" if c != s[i]])
    return "".join(s)


def _embed(rng, n, piece, end):
    """a random read of n characters with `piece` ending at column `end` (cut at the read's borders)"""
    s = list(_rand(rng, n))
    lo = end - len(piece)
    for i, c in enumerate(piece):
        if 0 <= lo + i < n:
            s[lo + i] = c
    return "".join(s)


def _reads(m):
    """the batch of one adapter length: (reads, index of the read that gets a byte >= 0x80)"""
    rng = random.Random(m)
    ad = _adapter(m)
    k = int(RATE * m)
    reads = []
    n_of = lambda: rng.randint(max(34, m + 4), 150)
    # EXACT_FULL with the copy ending in the first, a middle and the LAST column of a sixteen-column chunk -- for windows
    # that end at the read end (chunks counted back from it) and for windows that start at column 0
    for back in (15, 7, 0, 16, 31, 32, 1):
        for _ in range(24):
            n = n_of()
            end = n - back - 16 * rng.randint(0, 5)
            reads.append(_embed(rng, n, ad, max(end, m)))
    for col in (1, 8, 16):
        for _ in range(24):
            n = n_of()
            reads.append(_embed(rng, n, ad, min(n, m + 16 * rng.randint(0, 1) + ((col - m) % 16))))
    # ... twice in one read: only the first copy counts
    for _ in range(64):
        n = rng.randint(2 * m + 10, 150) if 2 * m + 10 <= 150 else 150
        r = _embed(rng, n, ad, rng.randint(m, n // 2))
        reads.append(r[:n - m] + ad if rng.random() < 0.5 else _embed(rng, n, ad, n - 2)[:n // 2] + r[n // 2:])
    # EXACT_TAIL: the read ends with adapter[0:i], also with substitutions in a long tail
    for _ in range(600):
        n, i = n_of(), rng.randint(MIN_OVERLAP, m - 1)
        tail = ad[:i]
        if i >= 12 and rng.random() < 0.3:
            tail = _subst(rng, tail, [rng.randint(1, i - 2)])
        reads.append(_rand(rng, n - i) + tail)
    # SUBS_FULL: 1 .. k substitutions
    for _ in range(700):
        n = n_of()
        piece = _subst(rng, ad, rng.sample(range(1, m - 1), rng.randint(1, k)))
        reads.append(_embed(rng, n, piece, rng.randint(m, n)))
    # INDEL1_FULL: one deletion or one insertion (and, where the threshold allows, a substitution)
    for _ in range(700):
        n, i = n_of(), rng.randint(4, m - 5)
        piece = ad[:i] + ad[i + 1:] if rng.random() < 0.5 else ad[:i] + rng.choice("ACGT") + ad[i:]
        if k >= 2 and rng.random() < 0.3:
            piece = _subst(rng, piece, [rng.randint(1, 3) if i > m // 2 else len(piece) - 3])
        reads.append(_embed(rng, n, piece, rng.randint(len(piece), n)))
    # DP: two indels (k >= 2 for every length here), copies cut by the read end with an indel inside
    for _ in range(700):
        n = n_of()
        i, i2 = sorted(rng.sample(range(4, m - 4), 2))
        piece = ad[:i] + ad[i + 1:i2] + ad[i2 + 1:] if rng.random() < 0.5 else ad[:i] + "T" + ad[i:i2] + "G" + ad[i2:]
        end = rng.randint(len(piece), n) if rng.random() < 0.7 else n + rng.randint(1, m // 3)
        reads.append(_embed(rng, n, piece, end))
    # reads that end mid-chunk behind a window that starts at column 0: the copy near the read's start
    for _ in range(300):
        n = rng.randint(max(34, m + 2), min(150, m + 30))
        reads.append(_embed(rng, n, ad if rng.random() < 0.5 else _subst(rng, ad, [m // 2]), rng.randint(m, min(n, m + 6))))
    # reads shorter than one chunk (edge case outside the 34 .. 150 of the rest): guarded copy only
    for _ in range(200):
        n = rng.randint(MIN_OVERLAP, 15)
        reads.append(_rand(rng, n - min(n, 6)) + ad[:min(n, 6)] if rng.random() < 0.7 else ad[:n])
    # NONE behind the prefilter: a piece of the adapter's middle (k-mers hit, nothing aligns), far from the read end
    # (these are the stragglers of their waves) and near it
    while len(reads) < N_READS - 1500:
        n = n_of()
        lo = rng.randint(1, m // 3)
        piece = ad[lo:lo + rng.randint(m // 3, m // 2)]
        reads.append(_embed(rng, n, piece, rng.randint(len(piece), n - 1)))
    # plain random reads (most never reach the scan) and lightly mutated copies anywhere
    while len(reads) < N_READS:
        n = n_of()
        if rng.random() < 0.5:
            reads.append(_rand(rng, n))
        else:
            piece = "".join(c if rng.random() > 0.06 else rng.choice(["", c + "A", "C"]) for c in ad)
            reads.append(_embed(rng, n, piece, rng.randint(5, n + m // 2)))
    assert len(reads) == N_READS
    order = list(range(N_READS))
    rng.shuffle(order)
    reads = [reads[i] for i in order]
    # the read that gets the byte >= 0x80: one the scan follows to its end (an unedited tail, no whole copy) -- bytes behind
    # the column at which a read is finished are not promised to be looked at
    high = next(i for i, r in enumerate(reads) if r.endswith(ad[:14]) and ad not in r and len(r) >= 34)
    return reads, high


@functools.lru_cache(maxsize=None)
def _case(m):
    """reads, the oracle's answer and the CPU-side proof that the batch holds what it was built for -- once per length"""
    from oracle import oracle as orc
    from cutadapt_amd.kmer_heuristic import create_positions_and_kmers
    ad = _adapter(m)
    reads, high = _reads(m)
    seqs, offsets = orc.pack_reads(reads)
    seqs = seqs.copy()
    seqs[int(offsets[high]) + len(reads[high]) - 16] = 0xC1          # a byte >= 0x80 in the scan's last chunk, before the tail
    oa = orc.Aligner(ad, RATE, 14, False, False, 1, MIN_OVERLAP)
    of = orc.KmerFinder(create_positions_and_kmers(ad, MIN_OVERLAP, RATE, back_adapter=True, front_adapter=False))
    want6, want_st = orc.match_batch(oa, of, seqs, offsets)
    survivor = np.asarray(of.kmers_present_batch(seqs, offsets)).astype(bool)
    n = np.diff(offsets).astype(np.int64)
    found = want_st == 1
    rs, re_, qs, qe, sc, err = (want6[:, i].astype(np.int64) for i in range(6))
    full = found & (rs == 0) & (re_ == m)
    exact_full = full & (err == 0)
    present = {
        "survivors above the straggler switch": int(survivor.sum()) > 4096,
        "NONE": int((survivor & (want_st == 0)).sum()) >= 64,
        "EXACT_FULL": int(exact_full.sum()) >= 64,
        "EXACT_TAIL": int((found & (re_ < m) & (qe == n) & (err == 0)).sum()) >= 64,
        "EXACT_TAIL with substitutions": bool((found & (re_ < m) & (qe == n) & (err > 0) & (qe - qs == re_)).any()),
        "SUBS_FULL": int((full & (err > 0) & (qe - qs == m) & (sc == m - 2 * err)).sum()) >= 64,
        "INDEL1_FULL (deletion)": int((full & (err > 0) & (qe - qs == m - 1)).sum()) >= 32,
        "INDEL1_FULL (insertion)": int((full & (err > 0) & (qe - qs == m + 1)).sum()) >= 32,
        "DP (two indels)": int((found & (np.abs((qe - qs) - (re_ - rs)) >= 2)).sum()) >= 32,
        "shorter than one chunk": bool((survivor & (n < 16)).any()) and bool((found & (n < 16)).any()),
        "ends mid-chunk behind a window from column 0": bool((found & (n % 16 != 0) & (qs < 8)).any()),
        "byte >= 0x80": bool(survivor[high]) and want_st[high] == 2,
    }
    for back, name in ((15, "first"), (7, "a middle"), (0, "the last")):
        present[f"exact copy ends in {name} column of a chunk counted from the read end"] = \
            bool((exact_full & (qe < n) & ((n - qe) % 16 == back)).any())
    for col, name in ((1, "first"), (8, "a middle"), (0, "the last")):
        present[f"exact copy ends in {name} column of a chunk counted from column 0"] = \
            bool((exact_full & (qs < 16) & (qe % 16 == col)).any())
    return ad, seqs, offsets, want6, want_st, present


@pytest.mark.parametrize("m", ADAPTER_LENGTHS)
def test_batch_holds_every_class_and_edge_case(orc, m):
    """a test that silently misses a class passes for nothing: what the oracle says of the generated batch"""
    present = _case(m)[5]
    missing = [what for what, ok in present.items() if not ok]
    assert not missing, f"adapter of {m}: the batch lacks {missing}"


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{}, {"CAH_SCAN_RETRY": "0"}, {"CAH_SCAN_RETRY_CAP": "64"}],
                         ids=["default", "no straggler launch", "straggler list of 64"])
@pytest.mark.parametrize("m", ADAPTER_LENGTHS)
def test_scan_masks_vs_oracle(hip, m, knobs):
    import torch
    from cutadapt_amd import adapters as A
    from cutadapt_amd.batch import ReadBatch, match_batch
    ad, seqs, offsets, want6, want_st, _ = _case(m)
    plan = A.BackAdapter(ad, max_errors=RATE, min_overlap=MIN_OVERLAP)._fused_plan
    old = {key: os.environ.get(key) for key in knobs}
    os.environ.update(knobs)
    try:
        batch = ReadBatch.from_host(seqs, offsets)
        batch.workspace().fill_(0x7F)                    # list slots never written must not be read
        got6, got_st, _ = match_batch(plan, batch).cpu()
        torch.cuda.synchronize()
    finally:
        for key, value in old.items():
            if value is None:
                os.environ.pop(key, None)
            else:
                os.environ[key] = value
    bad = np.nonzero(got_st != want_st)[0]
    assert len(bad) == 0, f"adapter of {m}: status differs at reads {bad[:10]}: {got_st[bad[:10]]} vs {want_st[bad[:10]]}"
    bad = np.nonzero((got6 != want6).any(axis=1))[0]
    assert len(bad) == 0, f"adapter of {m}: tuples differ at reads {bad[:10]}: {got6[bad[:3]]} vs {want6[bad[:3]]}"
