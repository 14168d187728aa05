"""Adapter sets and reads for the adapter-index tests (cutadapt_amd/csrc/index.hip), shared by tests/test_index_families.py
(CPU: the dictionary) and tests/test_gpu_index_kernels.py (GPU: k_index_lookup, k_index_lookup_wide).

An index is a dict {"name", "set", "prefix", "adapters": [(sequence, rate, indels)], "wide"}.  Every rate is (k + 0.5) / L,
so int(rate * L) == k holds exactly.  All adapters are built with adapter_wildcards=False (only set 5 needs it).

A packed key is 2 x 64 bits at two bits per character: the code branches at 32 characters, the kernel's first load at
16, so the sets put adapters at 29 .. 35, 40, 48, 59 and 60 characters and the reads put their edits at every position.
Reads are made per adapter, not drawn: the unedited adapter, one substitution / deletion / insertion at every position, pairs
of substitutions around the word boundary, k + 1 substitutions, 'N' at every position (with and without one further edit),
every truncation, and junk characters around 16 and 32.  Only the pads on the free side and the replacement characters
are random (random.Random(seed): CAH_TEST_SEED_OFFSET shifts them)."""
import random

EXTRA61 = "GATTACAGATTACACCGGTTAACCGGTTTGCATGCAAGCTTGGCCAATCGATCGTTAGCTAGC"[:61]
JUNK = " U\nRX"
PAIR_POS = (0, 15, 16, 30, 31, 32, 33)


def rate(L, k):
    r = (k + 0.5) / L
    assert int(r * L) == k
    return r


def _seq(rng, L):
    return "".join(rng.choice("ACGT") for _ in range(L))


def _pair(rng, L):
    """two adapters of L characters of which, at every position, exactly one has an 'A' (so an 'N' of a read meets an 'A'
    of one and another character of the other at every position) -- they differ everywhere"""
    a, b = [], []
    for _ in range(L):
        x = rng.choice("CGT")
        if rng.random() < 0.5:
            a.append("A"); b.append(x)
        else:
            a.append(x); b.append("A")
    return "".join(a), "".join(b)


def _index(name, set_no, prefix, adapters, wide=False, reads_from=None):
    """reads_from: the adapters that reads_for() makes reads of (default: all of them)"""
    return {"name": name, "set": set_no, "prefix": prefix, "adapters": list(adapters), "wide": wide, "reads_from": reads_from}


def _widened(ix):
    """the same index with one unrelated 61-mer (rate 0, no indels): the table switches to the wide layout"""
    return _index(ix["name"] + "+61", 3, ix["prefix"], ix["adapters"] + [(EXTRA61, 0.0, False)], wide=True)


def boundary(seed=201):
    """set 1: adapters around the 32-character word"""
    rng = random.Random(seed)
    out = []
    for prefix in (True, False):
        side = "p" if prefix else "s"
        for L in (29, 30, 31, 32, 33, 34, 35):
            a, b = _pair(rng, L)
            out.append(_index(f"b{side}{L}k1", 1, prefix, [(a, rate(L, 1), True), (b, rate(L, 1), True)]))
        for L in (31, 32, 33):
            a, b = _pair(rng, L)
            out.append(_index(f"b{side}{L}k2", 1, prefix, [(a, rate(L, 2), True), (b, rate(L, 2), True)]))
        for L in (31, 32, 33):                              # Hamming: C(L,3) 27 + C(L,2) 9 + 3 L + 1 strings (L = 33: 152 164)
            a, b = _pair(rng, L)
            out.append(_index(f"b{side}{L}h3", 1, prefix, [(a, rate(L, 3), False), (b, rate(L, 1), False)]))
        # indexed lengths 28 .. 36 in one table (each indel adapter brings L - 1, L, L + 1), Hamming adapters among them
        mix = [(_seq(rng, L), rate(L, 1), True) for L in (29, 31, 32, 33, 35)]
        mix += [(_seq(rng, 32), rate(32, 2), False), (_seq(rng, 33), rate(33, 1), False)]
        out.append(_index(f"b{side}mix", 1, prefix, mix))
        # ... and the same adapter at several lengths: nested across the word boundary
        x = _seq(rng, 35)
        nest = [(x[:L] if prefix else x[35 - L:], rate(L, 1), True) for L in (30, 32, 33, 35)]
        out.append(_index(f"b{side}nest", 1, prefix, nest))
    return out


def long_packed(seed=202):
    """set 2: the longest adapters the packed table holds; keys of up to 62 characters"""
    rng = random.Random(seed)
    out = []
    for prefix in (True, False):
        side = "p" if prefix else "s"
        for L, k in ((48, 2), (59, 1), (60, 2)):
            a, b = _pair(rng, L)
            out.append(_index(f"l{side}{L}k{k}", 2, prefix, [(a, rate(L, k), True), (b, rate(L, 1), True)]))
        a, b = _pair(rng, 40)                               # Hamming, k = 3: 274 121 strings
        out.append(_index(f"l{side}40h3", 2, prefix, [(a, rate(40, 3), False), (b, rate(40, 1), False)]))
    return out


def packed_against_wide(seed=None):
    """set 3: every index of sets 1 and 2 with the extra 61-mer"""
    return [_widened(ix) for ix in boundary() + long_packed()]


def nested(seed=204):
    """set 4: X[:10], X[:14] and X of one random X of 20 characters (suffixes of X for a suffix index), k from 0 to 2, indels
    mixed, packed and wide; and a wide index of exactly 64 lengths"""
    rng = random.Random(seed)
    out = []
    for prefix in (True, False):
        side = "p" if prefix else "s"
        x = _seq(rng, 20)
        cut = (lambda L: x[:L]) if prefix else (lambda L: x[20 - L:])
        combos = {
            "k000h": [(10, 0, False), (14, 0, False), (20, 0, False)],
            "k111i": [(10, 1, True), (14, 1, True), (20, 1, True)],
            "k012i": [(10, 0, True), (14, 1, True), (20, 2, True)],
            "k212m": [(10, 2, True), (14, 1, False), (20, 2, True)],
            "k122m": [(10, 1, False), (14, 2, True), (20, 2, False)],
        }
        for tag, c in combos.items():
            ix = _index(f"n{side}{tag}", 4, prefix, [(cut(L), rate(L, k), ind) for L, k, ind in c])
            out.append(ix)
            w = _widened(ix)
            w["set"] = 4
            out.append(w)
        y = _seq(rng, 73)
        out.append(_index(f"n{side}64", 4, prefix, [((y[:L] if prefix else y[73 - L:]), 0.0, False) for L in range(10, 74)], wide=True,
                          reads_from=(0, 6, 22, 23, 54, 63)))          # 10, 16, 32, 33, 64 and 73 characters
    return out


def sixty_five_lengths(prefix=True, seed=205):
    y = _seq(random.Random(seed), 74)
    return _index("n65", 4, prefix, [((y[:L] if prefix else y[74 - L:]), 0.0, False) for L in range(10, 75)], wide=True)


def empty(seed=206):
    """set 5: an adapter with a literal non-ACGT character, indels and k = 0 contributes no string at all"""
    rng = random.Random(seed)
    out = []
    for prefix in (True, False):
        side = "p" if prefix else "s"
        odd = _seq(rng, 6) + "R" + _seq(rng, 7)
        out.append(_index(f"e{side}alone", 5, prefix, [(odd, rate(14, 0), True)], wide=True))
        out.append(_index(f"e{side}next", 5, prefix, [(odd, rate(14, 0), True), (_seq(rng, 14), rate(14, 1), True)], wide=True))
    return out


def literal(seed=207):
    """wide indexes whose adapters hold literal 'R' and 'X' (kept by the Hamming sphere): junk in a read matches only itself"""
    rng = random.Random(seed)
    out = []
    for prefix in (True, False):
        t = list(_seq(rng, 36))
        t[_at(36, 15, prefix)], t[_at(36, 32, prefix)] = "R", "X"               # (distances from the anchored end)
        s = "".join(t)
        out.append(_index(f"x{'p' if prefix else 's'}lit", 6, prefix, [(s, rate(36, 1), False), (_seq(rng, 36), rate(36, 1), False)], wide=True))
    return out


def all_sets():
    return {1: boundary(), 2: long_packed(), 3: packed_against_wide(), 4: nested(), 5: empty()}


# ---- reads ------------------------------------------------------------------------------------------------------------------

def _other(rng, c):
    return rng.choice([x for x in "ACGT" if x != c.upper()])


def _place(affix, pad, prefix):
    return affix + pad if prefix else pad + affix


def _at(L, p, prefix):
    """string position of the character at distance p from the anchored end of an affix of L characters"""
    return p if prefix else L - 1 - p


def reads_for(ix, seed=300):
    """-> list of (read, kind, adapter number, detail); detail is the distance of the edit from the anchored end or the length"""
    rng = random.Random(seed + sum(ord(c) for c in ix["name"].split("+")[0]))      # (a widened index gets its base's reads)
    prefix = ix["prefix"]
    out = []
    count = [0]

    def add(affix, kind, a, detail, pad=None):
        if pad is None:
            pad = _seq(rng, count[0] % 21)
        r = _place(affix, pad, prefix)
        if count[0] % 7 == 3:
            r = r.lower()
        count[0] += 1
        out.append((r, kind, a, detail))

    for a, (seq, rt, indels) in enumerate(ix["adapters"]):
        if seq == EXTRA61 or (ix["reads_from"] is not None and a not in ix["reads_from"]):
            continue
        L, k = len(seq), int(rt * len(seq))
        s = list(seq)
        add(seq, "exact", a, 0)
        for p in range(L):                                  # p: distance from the anchored end
            i = _at(L, p, prefix)
            t = s[:]; t[i] = _other(rng, s[i]); add("".join(t), "sub", a, p)
            t = s[:]; del t[i]; add("".join(t), "del", a, p)
            t = s[:]; t.insert(i if prefix else i + 1, _other(rng, s[i])); add("".join(t), "ins", a, p)
        if k >= 2:
            pos = sorted({p for p in PAIR_POS + (L - 1,) if 0 <= p < L})
            for x in range(len(pos)):
                for y in range(x + 1, len(pos)):
                    t = s[:]
                    for p in (pos[x], pos[y]):
                        t[_at(L, p, prefix)] = _other(rng, s[_at(L, p, prefix)])
                    add("".join(t), "sub2", a, pos[y])
        if k >= 2 and indels:                               # two insertions: the key is L + 2 characters long
            for x in range(len(pos)):
                for y in range(x + 1, len(pos)):
                    t = s[:]
                    for p in (pos[y], pos[x]) if prefix else (pos[x], pos[y]):
                        i = _at(L, p, prefix)
                        t.insert(i if prefix else i + 1, _other(rng, s[i]))
                    add("".join(t), "ins2", a, pos[y])
        t = s[:]
        for p in range(k + 1):
            i = _at(L, (p * 7) % L, prefix)
            t[i] = _other(rng, s[i])
        add("".join(t), "sub_k1", a, k + 1)
        for p in range(L):                                  # 'N' -- meets an 'A' of this adapter or another character
            i = _at(L, p, prefix)
            t = s[:]; t[i] = "N"; add("".join(t), "n", a, p)
            j = _at(L, (p + L // 2) % L, prefix)
            t = s[:]; t[i] = "N"; t[j] = _other(rng, s[j]); add("".join(t), "n_sub", a, p)
            if indels and p % 3 == 0:
                t = s[:]; t[i] = "N"; del t[j]; add("".join(t), "n_del", a, p)
            if indels:                                      # an inserted 'N': the adapter's k-mer heuristic may say no
                t = s[:]; t.insert(i if prefix else i + 1, "N"); add("".join(t), "n_ins", a, p)
        full = _place(seq, _seq(rng, 3), prefix)
        for n in range(L + 4):                              # truncations: the read is the whole affix, 0 .. L + 3 characters
            add(full[:n] if prefix else full[len(full) - n:], "short", a, n, pad="")
        for c in JUNK:
            for p in (0, 15, 16, 31, 32):
                if p < L:
                    t = s[:]; t[_at(L, p, prefix)] = c; add("".join(t), "junk", a, p)
            add(seq, "junk_behind", a, L, pad=c + _seq(rng, 5) if prefix else _seq(rng, 5) + c)
    return out


def sixteen(seed=208):
    """the kernel's first 16 characters arrive in one 16-byte load when the read has at least 16: indexes of adapters of
    12 .. 20 characters (k = 1, indels: indexed lengths 11 .. 21) for reads of 0 .. 40 characters"""
    rng = random.Random(seed)
    out = []
    for prefix in (True, False):
        for L in range(12, 21):
            a, b = _pair(rng, L)
            out.append(_index(f"s{'p' if prefix else 's'}{L}", 7, prefix, [(a, rate(L, 1), True), (b, rate(L, 1), True)]))
    return out


def sixteen_reads(ix, seed=301):
    """for every n in 0 .. 40: the adapter unedited, with one substitution, with two (no match), with 'N' and with one deletion,
    cut or padded to exactly n characters -> (read, kind, adapter, n)"""
    rng = random.Random(seed + sum(ord(c) for c in ix["name"]))
    prefix = ix["prefix"]
    out = []
    for a, (seq, _, _) in enumerate(ix["adapters"]):
        L = len(seq)
        for n in range(41):
            for kind in ("exact", "sub", "sub2", "n", "del"):
                t = list(seq)
                p = _at(L, n % L, prefix)
                q = _at(L, (n + 5) % L, prefix)
                if kind in ("sub", "sub2"):
                    t[p] = _other(rng, t[p])
                if kind == "sub2":
                    t[q] = _other(rng, t[q])
                if kind == "n":
                    t[p] = "N"
                if kind == "del":
                    del t[p]
                full = _place("".join(t), _seq(rng, 41), prefix)
                r = full[:n] if prefix else full[len(full) - n:]
                out.append((r.lower() if (n + a) % 5 == 2 else r, kind, a, n))
    return out


# ---- the reference as judge ----------------------------------------------------------------------------------------------------

_cache = {}


def once(key, make):
    """computed once per session and shared, never changed"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def ref_adapters(ref, ix):
    cls = ref.adapters.PrefixAdapter if ix["prefix"] else ref.adapters.SuffixAdapter
    return [cls(s, max_errors=r, indels=i, adapter_wildcards=False) for s, r, i in ix["adapters"]]


def ref_index(ref, ix):
    """the reference's AdapterIndex of this index"""
    import logging
    logging.getLogger("cutadapt.adapters").setLevel(logging.ERROR)      # (its warning about similar adapters: set 'nest' has some)
    return once(("ri", ix["name"]), lambda: ref.adapters.AdapterIndex(ref_adapters(ref, ix), prefix=ix["prefix"]))


def own_index(ix):
    """this project's AdapterIndex: the k-mer sets of indel adapters go to cah_index_create as AdapterIndex.__init__ passes them"""
    from cutadapt_amd import adapters as A
    cls = A.PrefixAdapter if ix["prefix"] else A.SuffixAdapter
    return once(("mi", ix["name"]), lambda: A.AdapterIndex(
        [cls(s, max_errors=r, indels=i, adapter_wildcards=False) for s, r, i in ix["adapters"]], prefix=ix["prefix"]))


def answer(ri, read):
    """the reference's match_to(read) as (adapter number, astart, astop, rstart, rstop, score, errors) or None"""
    m = ri.match_to(read)
    if m is None:
        return None
    number = next(k for k, a in enumerate(ri._adapters) if a is m.adapter)
    return (number, m.astart, m.astop, m.rstart, m.rstop, m.score, m.errors)


def reads_and_answers(ref, ix, reads=None, tag="reads"):
    def make():
        rs = reads_for(ix) if reads is None else reads
        ri = ref_index(ref, ix)
        return rs, [answer(ri, r[0]) for r in rs]
    return once((tag, ix["name"]), make)


def walk(ri, read):
    """what the reference's dictionary says at every indexed length, longest first (its _match_to_multiple_lengths, step by
    step, on its own _index and _lookup_with_n): -> [(length, looked up entry or None, entry after the 'N' re-alignment or
    None, had_n)], and the length at which its early exit fires (or None)"""
    s = read.upper()
    steps, best_m, best_e, exit_at = [], -1, 1000, None
    single = len(ri._lengths) == 1
    for length in ri._lengths:
        if not single and length < best_m:
            exit_at = length
            break
        affix = ri._make_affix(s, length)
        had_n = "N" in affix
        looked = ri._index.get(affix.replace("N", "A"))
        final = ri._lookup_with_n(affix) if had_n else looked
        steps.append((length, None if looked is None else looked[1:], None if final is None else final[1:], had_n))
        if final is not None and (final[2] > best_m or (final[2] == best_m and final[1] < best_e)):
            best_m, best_e = final[2], final[1]
    return steps, exit_at


LONG = 520


def long_wide(seed=209):
    """the wide kernel's re-alignment columns (m + 1 entries each, in LDS, one set per wave): one indel adapter of 520
    characters (k = 1) next to a 40-mer -> (indexes, {prefix: (reads with 'N' in the affix, reads without)}).  One in four
    'N' reads is of the long adapter (its re-alignment is some 10^5 cells in one lane), the others of the short one."""
    rng = random.Random(seed)
    out, reads = [], {}
    for prefix in (True, False):
        big, small = _seq(rng, LONG), _seq(rng, 40)
        out.append(_index(f"w{'p' if prefix else 's'}{LONG}", 8, prefix, [(big, rate(LONG, 1), True), (small, rate(40, 1), True)], wide=True))
        spots = (0, 1, LONG - 2, LONG - 1, 500, 501, 503, 506, 509, 512, 515)
        big_n, small_n, plain = [], [], []
        for k in range(52):
            p = spots[k] if k < len(spots) else (k * 37) % LONG
            i = _at(LONG, p, prefix)
            t = list(big); t[i] = "N"
            if k % 3 == 1 and k > 12:                       # one further substitution: too many errors
                j = _at(LONG, (p + 300) % LONG, prefix); t[j] = _other(rng, t[j])
            if k % 3 == 2 and k > 12:                       # an 'N' inserted
                t.insert(i, "N")
            big_n.append(_place("".join(t), _seq(rng, k % 9), prefix))
        for k in range(160):
            i = _at(40, k % 40, prefix)
            t = list(small); t[i] = "N"
            j = _at(40, (k + 20) % 40, prefix)
            if k // 40 == 1:
                t[j] = _other(rng, t[j])
            if k // 40 == 2:
                t.insert(i, "N")
            if k // 40 == 3:
                del t[j]
            small_n.append(_place("".join(t), _seq(rng, k % 5), prefix))
        with_n = []
        for k in range(52):
            with_n += [big_n[k]] + small_n[3 * k:3 * k + 3]
        for k in range(150):
            long = k % 3 == 0
            seq, L = (big, LONG) if long else (small, 40)
            t = list(seq)
            i = _at(L, (k * 37) % L, prefix)
            if k % 2:
                t[i] = _other(rng, t[i])
            if k % 4 == 3:
                del t[_at(L, (k * 37 + L // 2) % L, prefix)]
            plain.append(_place("".join(t), _seq(rng, k % 9), prefix))
        reads[prefix] = (with_n, plain)
    return out, reads


def padded_reads(ix, at_least=64, seed=302):
    """the reads of reads_for() with the free side padded to at_least characters, the truncations left as they are: an index
    with the extra 61-mer looks a read of fewer than 61 characters up whole and reports the length 61, so only for longer reads
    do a packed index and its widened twin have the same answers"""
    rng = random.Random(seed + sum(ord(c) for c in ix["name"].split("+")[0]))
    out = []
    for r, kind, a, d in reads_for(ix):
        if kind != "short" and len(r) < at_least:
            r = _place(r, _seq(rng, at_least - len(r)), ix["prefix"])
        out.append((r, kind, a, d))
    return out
