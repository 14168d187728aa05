"""The model and the families the GPU tests of the k-mer prefilter kernels rest on (tests/kmer_model.py,
tests/kmer_families.py).  CPU only.

  * the model against the reference's recorded answers (tests/golden/kmers.json, all four wildcard modes), against the
    oracle on every read of every family, and -- where it is built -- against the compiled reference on the reads on
    which every window is defined (no positive stop beyond the read end);
  * the families: each reaches the kernel it is tagged with (the plan builder runs on the host), the tags name every
    prefilter kernel, and the reads do what they are made for.  For a plan without wildcards a read holds one occurrence
    of one k-mer, so window arithmetic alone (kmer_families.planted_answer) predicts the model; the reads must touch and
    cross every window edge that a read length leaves room for."""
import numpy as np
import pytest

import kmer_families as F
import kmer_model as M

FAMILIES = F.families()
# (family, probe): the windows that are shorter than their k-mer on purpose -- no read may pass through them
NEVER = {("tail_1", 1), ("tail_5", 1), ("head_0_5", 1), ("tails_share_a_word", 4), ("tails_and_head", 4)}


def _packed(reads):
    raw = [r.encode("latin-1") for r in reads]
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in raw], out=off[1:])
    buf = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy()
    return buf, off


def test_model_equals_the_recorded_reference_answers(golden):
    n = 0
    shapes = set()
    for c in golden("kmers.json"):
        sets = [(a, b, k) for a, b, k in c["sets"]]
        for read, want in c["reads"]:
            assert M.present(sets, read, c["wr"], c["wq"]) == want, (sets, c["wr"], c["wq"], read)
            n += 1
        shapes.add((c["wr"], c["wq"]))
    assert n == 1528 and len(shapes) == 4


def test_block_model_equals_the_plain_model():
    """the numpy form over blocks of equally long reads is the same function (every family, a spread of its reads)"""
    n = 0
    for fam in FAMILIES:
        for length in fam["lengths"][::5] + fam["lengths"][-1:]:
            rows = F.reads_of(fam, length)
            got = F.answers(fam, length)
            for k in list(range(0, len(rows), 17)) + [len(rows) - 1]:
                want = M.first_hit_end(fam["sets"], rows[k][0], fam["ref_wc"], fam["query_wc"])
                assert got[k] == (-1 if want is None else want), (fam["name"], length, rows[k])
                n += 1
    assert n > 5000


def test_model_equals_the_oracle_on_every_family(orc):
    total = 0
    for fam in FAMILIES:
        reads = [r[0] for r in F.all_reads(fam)]
        buf, off = _packed(reads)
        want = orc.KmerFinder(fam["sets"], fam["ref_wc"], fam["query_wc"]).kmers_present_batch(buf, off)
        got = (F.all_answers(fam) >= 0).astype(np.uint8)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (fam["name"], reads[bad[0]], int(got[bad[0]]), int(want[bad[0]]), bad.size)
        total += len(reads)
    assert 150_000 < total < 300_000, total
    assert max(len(F.all_reads(fam)) for fam in FAMILIES) < 20_000 and max(max(fam["lengths"]) for fam in FAMILIES) == 257


def test_model_equals_the_compiled_reference(ref):
    if ref is None:
        pytest.skip("oracle/_ref not built here")
    total = 0
    for fam in FAMILIES:
        if len(fam["sets"][0][2]) > 100:
            continue                                          # (1 024 words: the oracle has them; a per-read loop here would take minutes)
        finder = ref.KmerFinder(fam["sets"], fam["ref_wc"], fam["query_wc"])
        stops = [b for _, b, _ in fam["sets"] if b is not None and b > 0]
        for n in fam["lengths"]:
            if any(b > n for b in stops):
                continue                                      # the reference reads out of bounds there
            got = F.answers(fam, n) >= 0
            for (read, _, _), g in zip(F.reads_of(fam, n), got):
                assert finder.kmers_present(read) == bool(g), (fam["name"], read)
                total += 1
    assert total > 100_000


def test_families_reach_the_kernels_they_are_tagged_with():
    named = set()
    for fam in FAMILIES:
        for aligner in (False, True):
            assert F.routing_of(F.plan_of(fam, aligner)) == fam["tag"], (fam["name"], aligner)
        for mode in (0, 1):
            named.add(F.kernels(fam, mode))
        if fam["tag"]["kind"] == "lean":
            for env in ((), ("CAH_NO_STREAM2",), ("CAH_NO_STREAM",)):
                for n in fam["lengths"]:
                    named.add(F.kernels(fam, 1, "uniform", n, 70, env))
    named |= {k.split("<")[0] for k in named if k.startswith("k_filter_stream")}
    assert F.required_kernels() <= named, sorted(F.required_kernels() - named)


def test_heuristic_like_family_may_skip_columns():
    """the plan whose keys the queue-mode test holds to `key * 4 <= first_hit_end`: its matcher reports skip_ok"""
    from cutadapt_amd.kmer_heuristic import create_positions_and_kmers
    fam = F.by_name("heuristic_like")
    want = create_positions_and_kmers(F.ADAPTER, 3, 0.1, back_adapter=True, front_adapter=False)
    assert {(a, b, tuple(sorted(k))) for a, b, k in want} >= {(a, b, tuple(sorted(k))) for a, b, k in fam["sets"][:1]}, want
    assert F.skip_ok(F.plan_of(fam, True)) == 1
    assert F.skip_ok(F.plan_of(F.by_name("tail_7"), True)) == 0


def test_reads_touch_and_cross_every_window_edge():
    """For every (family, read length): an absent read; a present one whenever a probe fits its window at that length;
    for every window edge that the length leaves room for, the read whose only occurrence lies inside the window and
    touches the edge (present) and the read whose occurrence crosses it by exactly one character (absent).  Per family the
    edges must have been met at some length: both edges of every probed window, inside and crossed."""
    cases = 0
    for fam in FAMILIES:
        met = set()
        for n in fam["lengths"]:
            rows, got = F.reads_of(fam, n), F.answers(fam, n) >= 0
            assert len(rows) == len(got) and not got[0], (fam["name"], n)           # the background / empty read
            where = {(p, s): k for k, (_, p, s) in enumerate(rows)}
            for pi, (j, t, text) in enumerate(fam["probes"]):
                q = len(text)
                if not F.planted(fam, pi, n):
                    assert not any(p == pi for p, s in where)
                    continue
                ws, we = M.window(fam["sets"][j][0], fam["sets"][j][1], n)
                fits = we - ws >= q
                if not fam["arith"]:
                    # wildcards or k-mers that overlap: the model decides, the reads must still split
                    if fits:
                        assert got[where[(pi, ws)]] and got[where[(pi, we - q)]], (fam["name"], n, pi)
                        met |= {(pi, "start in"), (pi, "stop in")}
                    continue
                for s in range(n - q + 1):
                    assert got[where[(pi, s)]] == F.planted_answer(fam, n, pi, s), (fam["name"], n, pi, s)
                if not fits:
                    assert not any(got[where[(pi, s)]] for s in range(n - q + 1))
                    continue
                assert got[where[(pi, ws)]] and got[where[(pi, we - q)]]
                met |= {(pi, "start in"), (pi, "stop in")}
                if ws >= 1:
                    assert not got[where[(pi, ws - 1)]]
                    met.add((pi, "start crossed"))
                if we + 1 <= n:
                    assert not got[where[(pi, we - q + 1)]]
                    met.add((pi, "stop crossed"))
                cases += 1
        # every k-mer of every set is a probe (table and limit families: the last word's, which is what they are about) ...
        probed = {(j, t) for j, t, _ in fam["probes"]}
        every = {(j, t) for j, (_, _, kmers) in enumerate(fam["sets"]) for t in range(len(kmers))}
        assert probed == (every if fam["group"] not in ("tables", "limit") else {(0, len(fam["sets"][0][2]) - 1)}), fam["name"]
        # ... and, unless its window can never hold it, has a read in which it is present at either edge of its window
        for pi, (j, t, text) in enumerate(fam["probes"]):
            a, b, _ = fam["sets"][j]
            widest = b - a if 0 <= a < (b or 0) else -a if (a < 0 and not b) else 1 << 30
            never = widest < len(text)                                                # a window shorter than its k-mer
            assert never == ((fam["name"], pi) in NEVER), (fam["name"], pi)
            want = set() if never else {"start in", "stop in"}
            if fam["arith"] and not never:
                if a != 0:
                    want.add("start crossed")
                if b:
                    want.add("stop crossed")
            assert want <= {e for p, e in met if p == pi}, (fam["name"], pi, want, met)
    assert cases > 2000
