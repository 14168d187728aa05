"""The adapter sets and reads of tests/index_families.py on the CPU: that they reach what they are made for, with the reference's
own AdapterIndex as the judge (oracle/_ref), and that the dictionary cah_index_create builds for them -- queried through
cah_index_get, i.e. pack_key and the host loop past 32 characters -- holds exactly the reference's entries and nothing else.
The GPU side of the same families is tests/test_gpu_index_kernels.py."""
import os
import random
from collections import Counter

import pytest

import index_families as F

SETS = F.all_sets()
CONTENT = [ix for no in (1, 2, 4, 5) for ix in SETS[no]]

# len(reference index) of sets 1 and 2 as measured (the Hamming ones are C(L,3) 27 + C(L,2) 9 + 3 L + 1 of the k = 3 adapter plus
# 3 L + 1 of the k = 1 adapter; the edit environments are counts of the seeds as they stand)
N_STRINGS = {
    "bp29k1": 396, "bp30k1": 414, "bp31k1": 425, "bp32k1": 431, "bp33k1": 454, "bp34k1": 462, "bp35k1": 476,
    "bp31k2": 42209, "bp32k2": 46289, "bp33k2": 48590, "bp31h3": 125738, "bp32h3": 138578, "bp33h3": 152264,
    "bpmix": 5764, "bpnest": 868,
    "bs29k1": 402, "bs30k1": 413, "bs31k1": 424, "bs32k1": 447, "bs33k1": 449, "bs34k1": 460, "bs35k1": 479,
    "bs31k2": 42861, "bs32k2": 44562, "bs33k2": 49556, "bs31h3": 125738, "bs32h3": 138578, "bs33h3": 152264,
    "bsmix": 5770, "bsnest": 876,
    "lp48k2": 50577, "lp59k1": 804, "lp60k2": 81601, "lp40h3": 274022,
    "ls48k2": 52158, "ls59k1": 792, "ls60k2": 81651, "ls40h3": 274022,
}
HAMMING = {L: (L * (L - 1) * (L - 2) // 6) * 27 + (L * (L - 1) // 2) * 9 + 3 * L + 1 + 3 * L + 1 for L in (31, 32, 33, 40)}


def _need(ref):
    assert ref is not None, "oracle/_ref is not built: python oracle/build_ref.py"
    return ref


def _judged(ref, sets):
    """(index, read, kind, adapter, detail, answer) of every read of the sets"""
    for no in sets:
        for ix in SETS[no]:
            reads, answers = F.reads_and_answers(ref, ix)
            for (r, kind, a, d), w in zip(reads, answers):
                yield ix, r, kind, a, d, w


# ---- family properties --------------------------------------------------------------------------------------------------------

def test_rates_give_k_exactly():
    for no, sets in SETS.items():
        for ix in sets:
            for s, r, _ in ix["adapters"]:
                k = int(r * len(s))
                assert r == 0.0 or r == (k + 0.5) / len(s), ix["name"]
    assert [len(SETS[no]) for no in (1, 2, 3, 4, 5)] == [30, 8, 38, 22, 4]
    assert all(ix["wide"] == (any(len(s) > 60 or not set(s) <= set("ACGT") for s, _, _ in ix["adapters"])) for no in SETS for ix in SETS[no])


def test_edits_on_both_sides_of_the_word_boundary(ref):
    """matched and unmatched reads with the edit at distance 31 and at distance 32 from the anchored end, prefix and suffix,
    packed and wide"""
    _need(ref)
    seen = Counter()
    for ix, r, kind, a, d, w in _judged(ref, (1, 2, 3)):
        if kind in ("sub", "del", "ins", "n", "n_sub", "n_del", "junk") and d in (31, 32):
            seen[(ix["prefix"], ix["wide"], d, w is not None)] += 1
    for key in [(p, wd, d, m) for p in (True, False) for wd in (True, False) for d in (31, 32) for m in (True, False)]:
        assert seen[key] >= 20, (key, seen[key])


def test_reads_around_the_16_byte_load(ref):
    """matched and unmatched reads of exactly 15, 16 and 17 characters (the kernel's 16-byte load switches on at 16), in
    sets 1 to 4 and in the family made for it"""
    _need(ref)
    seen = Counter()
    for ix, r, kind, a, d, w in _judged(ref, (1, 2, 3, 4)):
        if len(r) in (15, 16, 17):
            seen[("sets", ix["prefix"], len(r), w is not None)] += 1
    for ix in F.sixteen():
        reads, answers = F.reads_and_answers(ref, ix, F.sixteen_reads(ix), tag="sixteen")
        for (r, kind, a, n), w in zip(reads, answers):
            assert len(r) == n
            if n in (15, 16, 17):
                seen[("sixteen", ix["prefix"], n, w is not None)] += 1
    for fam, least in (("sets", 3), ("sixteen", 20)):
        for key in [(fam, p, n, m) for p in (True, False) for n in (15, 16, 17) for m in (True, False)]:
            assert seen[key] >= least, (key, seen[key])


def test_n_reads_reach_every_outcome_of_the_realignment(ref):
    """an 'N' inside a looked-up affix sends the reference to adapter.match_to(affix): it accepts, it rejects (too many errors,
    or the k-mer heuristic of an indel adapter says no although an alignment exists), and where it accepts (errors, score)
    differ from the looked-up (errors, matches).  Counted per (prefix, wide) over sets 1 to 4; the stated minima are about
    a third of what the reference gave when the families were written (accept 6195 .. 6405, every one of them changed;
    reject 2347 .. 4516, of which the heuristic alone 609 .. 642)."""
    _need(ref)
    seen = Counter()
    for ix, r, kind, a, d, w in _judged(ref, (1, 2, 3, 4)):
        if not kind.startswith("n"):
            continue
        ri = F.ref_index(ref, ix)
        steps, _ = F.walk(ri, r)
        for length, looked, final, had_n in steps:
            if not had_n or looked is None:
                continue
            key = (ix["prefix"], ix["wide"])
            if final is None:
                seen[key + ("reject",)] += 1
                affix = ri._make_affix(r.upper(), length)
                adapter = ri._index[affix.replace("N", "A")][0]
                # the heuristic alone: the aligner itself would have matched
                seen[key + ("heuristic",)] += adapter.indels and adapter.aligner.locate(affix) is not None
            else:
                seen[key + ("accept",)] += 1
                seen[key + ("changed",)] += final != looked
    print(sorted(seen.items()))
    for p in (True, False):
        for wd in (True, False):
            assert seen[(p, wd, "accept")] >= 2000 and seen[(p, wd, "reject")] >= 750, seen
            assert seen[(p, wd, "changed")] >= 2000 and seen[(p, wd, "heuristic")] >= 200, seen


def test_nested_lengths_tie_exit_early_and_let_the_shorter_win(ref):
    """set 4 (and the nested index of set 1): reads for which two indexed lengths give equal matches and equal errors --
    the longer one is reported --, reads at which the reference's early exit fires, reads where a shorter length wins.
    The minima are about a third of the reference's counts (ties 167 .. 196, early exits 1039 .. 2109, shorter 348 .. 351
    per (prefix, wide))."""
    _need(ref)
    seen = Counter()
    for ix, r, kind, a, d, w in _judged(ref, (4,)):
        ri = F.ref_index(ref, ix)
        steps, exit_at = F.walk(ri, r)
        hits = [(length, final) for length, _, final, _ in steps if final is not None]
        key = (ix["prefix"], ix["wide"])
        assert (w is None) == (not hits)
        if not hits:
            continue
        best = max(m for _, (e, m) in hits)
        best_e = min(e for _, (e, m) in hits if m == best)
        winners = [length for length, (e, m) in hits if (e, m) == (best_e, best)]
        reported = w[4] if ix["prefix"] else len(r) - w[3]
        assert reported == max(winners) and (w[5], w[6]) == (best, best_e), (ix["name"], r, w, hits)
        seen[key + ("tie",)] += len(winners) > 1 and len({min(l, len(r)) for l in winners}) > 1
        seen[key + ("exit",)] += exit_at is not None
        seen[key + ("shorter",)] += reported < max(length for length, _ in hits)
    print(sorted(seen.items()))
    for p in (True, False):
        for wd in (True, False):
            for what, least in (("tie", 50), ("exit", 300), ("shorter", 100)):
                assert seen[(p, wd, what)] >= least, (p, wd, what, seen)


# ---- dictionary contents ------------------------------------------------------------------------------------------------------

def _edits(rng, s):
    """one further edit of s, the position drawn from both ends and from around character 32"""
    L = len(s)
    spots = [p for p in (0, 1, 15, 16, 30, 31, 32, 33, 34, L - 2, L - 1) if 0 <= p < L]
    p = rng.choice(spots) if rng.random() < 0.7 else rng.randrange(L)
    op = rng.choice("ssid")
    c = rng.choice("ACGT")
    if op == "s":
        return s[:p] + c + s[p + 1:]
    if op == "i":
        return s[:p] + c + s[p:]
    return s[:p] + s[p + 1:]


@pytest.mark.parametrize("ix", CONTENT, ids=[ix["name"] for ix in CONTENT])
def test_dictionary_holds_the_reference_entries_and_nothing_else(ref, ix):
    _need(ref)
    ri = F.ref_index(ref, ix)
    h = F.own_index(ix)._h
    assert h.n_strings == len(ri._index) and h.lengths == ri._lengths and h.n_ambiguous == ri._ambiguous, ix["name"]
    if ix["name"] in N_STRINGS and not int(os.environ.get("CAH_TEST_SEED_OFFSET", "0") or 0):
        assert h.n_strings == N_STRINGS[ix["name"]]
    if ix["name"][2:] in ("31h3", "32h3", "33h3", "40h3"):      # (derived, whatever the seed)
        assert h.n_strings == HAMMING[int(ix["name"][2:4])]
    number = {id(a): k for k, a in enumerate(ri._adapters)}
    get = h.get
    for s, (ad, e, m) in ri._index.items():
        if get(s) != (number[id(ad)], e, m):
            raise AssertionError((ix["name"], s, get(s), (number[id(ad)], e, m)))
    # negatives: strings one further edit away from dictionary strings are found exactly when the reference has them
    rng = random.Random(400 + len(ix["name"]))
    keys = list(ri._index) or [s for s, _, _ in ix["adapters"]]
    sample = set()
    for _ in range(40000):
        s = _edits(rng, rng.choice(keys))
        if len(keys) < 50 and rng.random() < 0.7:           # (a handful of strings has fewer than 2 000 neighbours: go on to theirs)
            s = _edits(rng, s)
        sample.add(s)
        if len(sample) == 2000:
            break
    assert len(sample) == 2000, (ix["name"], len(sample))
    present = 0
    for s in sample:
        inside = s in ri._index
        got = get(s)
        assert (got is not None) == inside, (ix["name"], s, got)
        present += inside
    # (with k = 0 every single edit leaves the dictionary; everywhere else both kinds are in the sample)
    if len(ri._index) > 100:
        assert 50 <= present <= len(sample) - 50, (ix["name"], present)


# ---- limits ----------------------------------------------------------------------------------------------------------------

def test_limits_of_the_index(ref):
    from cutadapt_amd import _lib
    for prefix in (True, False):
        ix = next(x for x in SETS[4] if x["name"] == ("np64" if prefix else "ns64"))
        h = F.own_index(ix)._h
        assert len(h.lengths) == 64 and h.lengths == list(range(73, 9, -1)) and h.n_strings == 64
        with pytest.raises(_lib.UnsupportedByHipPath, match="64 different string lengths"):
            _lib.Index(F.sixty_five_lengths(prefix)["adapters"], prefix)
        rng = random.Random(401)
        long = "".join(rng.choice("ACGT") for _ in range(1001))
        h = _lib.Index([(long[:1000], 0.0, False)], prefix)
        assert h.n_strings == 1 and h.lengths == [1000] and h.get(long[:1000]) == (0, 0, 1000)
        assert h.get(long[:999]) is None and h.get(long[1:1001]) is None
        with pytest.raises(_lib.UnsupportedByHipPath, match="1000-character limit"):
            _lib.Index([(long, 0.0, False)], prefix)
    if ref is not None:                                     # the reference builds the 65 lengths: the limit is this build's
        assert len(F.ref_index(ref, F.sixty_five_lengths())._lengths) == 65
