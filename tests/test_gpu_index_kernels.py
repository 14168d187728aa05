"""The adapter index on the GPU (cutadapt_amd/csrc/index.hip: k_index_lookup, k_index_lookup_wide) through the C ABI,
cah_index_lookup_batch on tensors in HBM, on the adapter sets and reads of tests/index_families.py (whose reach the CPU
test tests/test_index_families.py pins).  Every row -- status, the six coordinates, best_adapter -- is compared exactly with
the reference's IndexedPrefixAdapters / IndexedSuffixAdapters.match_to (oracle/_ref) on the same read, for a window on the
slice as a string.  Every output row is pre-filled with a canary, so an unwritten row is seen, and 64 guard rows behind
out6, best_adapter and status must survive every call.  GPU only."""
import random

import numpy as np
import pytest

import index_families as F

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, 1
NONE, MATCH, INVALID = 0, 1, 2
MAX_READ_LEN = 1000000
GUARD = 64
CANARY_I32, CANARY_U8 = -1515870811, 0xA5
SETS = F.all_sets()


# ---- helpers ----------------------------------------------------------------------------------------------------------------

def _up(a, dtype=None):
    """numpy array -> tensor in HBM (never empty)"""
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).to("cuda:0") if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device="cuda:0")


def _p(t):
    return None if t is None else t if isinstance(t, int) else t.data_ptr()


def _bytes(r):
    return r if isinstance(r, bytes) else r.encode("latin-1")


def _packed(reads):
    """reads back to back -> (bytes as uint8 array, offsets int64[n + 1])"""
    reads = [_bytes(r) for r in reads]
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in reads], out=off[1:])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), off


def _guarded(n, cols, dtype, canary):
    import torch
    return torch.full((n + GUARD, cols) if cols else (n + GUARD,), canary, dtype=dtype, device="cuda:0")


def _lookup(hip, index, seqs, offsets, lens, n, best=True, stream=None, check=True):
    """one call on canary-filled outputs -> (rc, out6[n, 6], best_adapter[n] or None, status[n]); the guard rows are checked"""
    import torch
    from cutadapt_amd import _lib
    out6 = _guarded(n, 6, torch.int32, CANARY_I32)
    st = _guarded(n, 0, torch.uint8, CANARY_U8)
    ba = _guarded(n, 0, torch.int32, CANARY_I32) if best else None
    handle = index if index is None or isinstance(index, int) else index._h.handle
    rc = hip.cah_index_lookup_batch(handle, _p(seqs), _p(offsets), _p(lens), n, _p(out6), _p(ba), _p(st), stream)
    if check:
        _lib.check(rc)
    torch.cuda.synchronize()
    o, s = out6.cpu().numpy(), st.cpu().numpy()
    b = ba.cpu().numpy() if best else None
    m = max(n, 0)
    assert (o[m:] == CANARY_I32).all() and (s[m:] == CANARY_U8).all() and (b is None or (b[m:] == CANARY_I32).all()), \
        "rows >= n_reads were written"
    return rc, o[:m], (None if b is None else b[:m]), s[:m]


def _want(answers):
    """the reference's answers as the rows the kernel has to write: a read without a match gets six zeros and -1"""
    n = len(answers)
    o, b, s = np.zeros((n, 6), np.int32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    for k, w in enumerate(answers):
        if w is not None:
            o[k], b[k], s[k] = w[1:], w[0], MATCH
    return o, b, s


def _same(got, want, reads, label):
    go, gb, gs = got
    wo, wb, ws = want
    bad = (gs != ws) | (go != wo).any(axis=1)
    if gb is not None:
        bad |= gb != wb
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError((label, "first difference at read", k, reads[k], "got", int(gs[k]), go[k].tolist(), None if gb is None else int(gb[k]),
                              "reference", int(ws[k]), wo[k].tolist(), int(wb[k]), int(bad.sum()), "rows differ"))


def _run(hip, ref, ix, reads=None, tag="reads", label=None):
    """all reads of the index in one call, compared with the reference -> (reads, answers)"""
    reads, answers = F.reads_and_answers(ref, ix, reads, tag)
    buf, off = _packed([r[0] for r in reads])
    _, o, b, s = _lookup(hip, F.own_index(ix), _up(buf), _up(off), None, len(reads))
    _same((o, b, s), _want(answers), reads, label or ix["name"])
    return reads, answers


def _length(ix, read, w):
    """the indexed length a match reports: rstop of a prefix match, len(read) - rstart of a suffix match"""
    return w[4] if ix["prefix"] else len(read) - w[3]


# ---- a. the 32-character word --------------------------------------------------------------------------------------------------

def test_word_boundary_packed(hip, ref):
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    lengths = {True: set(), False: set()}
    both_sides = 0
    total = 0
    for ix in SETS[1] + SETS[2]:
        assert not ix["wide"]
        reads, answers = _run(hip, ref, ix)
        total += len(reads)
        mine = {_length(ix, r[0], w) for r, w in zip(reads, answers) if w is not None and len(r[0]) >= _length(ix, r[0], w)}
        lengths[ix["prefix"]] |= mine
        both_sides += ix["name"].endswith(("mix", "nest")) and min(mine) < 32 < max(mine)
    # from the expected values: keys of exactly 31, 32 and 33 characters, of more than 32 in a suffix index, of 62 characters,
    # and indexes of several lengths whose matches lie on both sides of 32
    for p in (True, False):
        assert {31, 32, 33, 62} <= lengths[p] and set(range(28, 37)) <= lengths[p], (p, sorted(lengths[p]))
    assert both_sides == 4 and total > 20000


# ---- b. the same reads through the other kernel ------------------------------------------------------------------------------

def test_wide_kernel_agrees_with_the_packed_one(hip, ref):
    """set 3: every index of sets 1 and 2 again with one unrelated 61-mer, which switches the table to the wide layout.  The
    reads are padded to 64 characters on the free side (an index that holds the length 61 looks a shorter read up whole and
    reports 61 -- the truncations, left as they are, are compared with the reference only): the rows of the two kernels are
    equal, and equal to the reference's"""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    base = {ix["name"]: ix for ix in SETS[1] + SETS[2]}
    compared = 0
    for wide in SETS[3]:
        ix = base[wide["name"].split("+")[0]]
        assert wide["wide"] and wide["adapters"][:-1] == ix["adapters"]
        reads, answers = F.reads_and_answers(ref, ix, F.padded_reads(ix), tag="padded")
        _, wanswers = F.reads_and_answers(ref, wide, reads, tag="padded")
        long = np.array([len(r[0]) >= 61 for r in reads])
        assert all(w == a for w, a, l in zip(wanswers, answers, long) if l) and long.sum() >= 350
        buf, off = _packed([r[0] for r in reads])
        tb, to = _up(buf), _up(off)
        _, o, b, s = _lookup(hip, F.own_index(ix), tb, to, None, len(reads))
        _, o2, b2, s2 = _lookup(hip, F.own_index(wide), tb, to, None, len(reads))
        _same((o, b, s), _want(answers), reads, ix["name"])
        _same((o2, b2, s2), _want(wanswers), reads, wide["name"])
        assert np.array_equal(o[long], o2[long]) and np.array_equal(b[long], b2[long]) and np.array_equal(s[long], s2[long]), wide["name"]
        compared += int(long.sum())
    assert compared > 20000


# ---- c. the 16-byte load -------------------------------------------------------------------------------------------------------

def test_sixteen_byte_load(hip, ref):
    """reads of 0 .. 40 characters against indexes of lengths 11 .. 21, back to back: they start at every address modulo 16
    and the last one ends at the tensor's last byte"""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    phases = {True: set(), False: set()}
    for ix in F.sixteen():
        reads = F.sixteen_reads(ix)
        reads.sort(key=lambda r: (r[3] * 7) % 41)           # (not by length: every length at many phases; the last one is long)
        reads, answers = F.reads_and_answers(ref, ix, reads, tag="sixteen sorted")
        buf, off = _packed([r[0] for r in reads])
        t = _up(buf)
        assert t.numel() == off[-1] and len(reads[-1][0]) >= 16 and t.data_ptr() % 16 == 0
        _, o, b, s = _lookup(hip, F.own_index(ix), t, _up(off), None, len(reads))
        _same((o, b, s), _want(answers), reads, ix["name"])
        phases[ix["prefix"]] |= {(int(off[k]) % 16, n >= 16) for k, (_, _, _, n) in enumerate(reads)}
        assert {n for _, _, _, n in reads} == set(range(41))
        assert any(w is not None for w in answers) and any(w is None for w in answers)
    for p in (True, False):
        assert phases[p] == {(ph, big) for ph in range(16) for big in (True, False)}


# ---- d. the 'N' re-alignment -----------------------------------------------------------------------------------------------------

def test_n_realignment_in_arranged_waves(hip, ref):
    """the wide kernel runs the re-alignment in LDS columns that the lanes of a wave take in turns: a wave in which all 64
    lanes need their turn, one with lane 0 only, one with lane 63 only, two waves of a block at once, a last partial block
    whose last read is an 'N' read, a batch of one -- with an indel adapter of 520 characters, so that the columns are used
    far beyond their first entries.  (The 'N' reads as they come are part of a, b and e: packed and wide.)"""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    indexes, all_reads = F.long_wide()
    for ix in indexes:
        with_n, plain = all_reads[ix["prefix"]]
        ri = F.ref_index(ref, ix)
        assert len(with_n) >= 129 and len(plain) >= 128 and max(ri._lengths) == F.LONG + 1
        answer = F.once(("long answers", ix["name"]), lambda: {r: F.answer(ri, r) for r in with_n + plain})
        assert sum(answer[r] is not None for r in with_n) > 60 and sum(answer[r] is None for r in with_n) > 40, [sum(answer[r] is not None for r in with_n)]
        far = [r for r in with_n if answer[r] is not None and "N" in (r[500:F.LONG] if ix["prefix"] else r[-F.LONG:-500])]
        assert len(far) >= 5                                  # accepted with the 'N' beyond column 500

        def block(n_lanes, n=256):
            """a batch of n reads, the rows in n_lanes hold reads with 'N'"""
            it_n, it_p = iter(with_n * 2), iter(plain * 3)
            return [next(it_n) if k in n_lanes else next(it_p) for k in range(n)]

        arrangements = {
            "all 64 lanes of wave 0": block(set(range(64))),
            "lane 0 only": block({0}),
            "lane 63 only": block({63}),
            "lane 0 of every wave": block({0, 64, 128, 192}),
            "waves 1 and 3 at once": block(set(range(64, 128)) | set(range(192, 256))),
            "256 + 1, the last one": block({256}, 257),
            "batch of 1": block({0}, 1),
            "batch of 1, far": [far[0]],
        }
        for label, reads in arrangements.items():
            buf, off = _packed(reads)
            _, o, b, s = _lookup(hip, F.own_index(ix), _up(buf), _up(off), None, len(reads))
            _same((o, b, s), _want([answer[r] for r in reads]), reads, (ix["name"], label))


# ---- e. several lengths --------------------------------------------------------------------------------------------------------

def test_lengths_rule(hip, ref):
    """set 4, packed and wide, and the index of 64 lengths: ties go to the longest indexed length, and the reported rstop
    (prefix) / rstart (suffix) carry the INDEXED length, not the adapter's and not the read's"""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    seen = {(p, wd): [0, 0, 0] for p in (True, False) for wd in (True, False)}
    for ix in SETS[4]:
        reads, answers = _run(hip, ref, ix)
        ri = F.ref_index(ref, ix)
        for (r, kind, a, d), w in zip(reads, answers):
            if w is None:
                continue
            length = _length(ix, r, w)
            c = seen[(ix["prefix"], ix["wide"])]
            c[0] += length != w[2]                               # not the adapter's length (astop)
            c[1] += length > len(r)                              # a shorter read: rstop behind its end / rstart negative
            steps, _ = F.walk(ri, r)
            hits = [l for l, _, final, _ in steps if final is not None and (final[1], final[0]) == (w[5], w[6])]
            c[2] += len({min(l, len(r)) for l in hits}) > 1 and length == max(hits)       # a tie, the longest reported
        if ix["name"].endswith("64"):
            assert len(ri._lengths) == 64 and len({_length(ix, r[0], w) for r, w in zip(reads, answers) if w is not None}) >= 60
    for key, c in seen.items():
        assert c[0] >= 100 and c[1] >= 20 and c[2] >= 20, (key, c)


# ---- f. windows ------------------------------------------------------------------------------------------------------------------

def test_windows_into_a_parent_buffer(hip, ref):
    """d_lens with d_offsets as starts: windows cut from both sides of longer reads, overlapping windows, empty ones.  What
    lies just outside is the rest of the adapter: for a suffix index its last characters right behind the window, for a
    prefix index its first characters right in front of it.  Row r holds the reference's answer on the slice as a string."""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    cuts = ((0, 0), (3, 0), (0, 3), (1, 1), (2, 5), (0, 1), (1, 0), (7, 0), (0, 7), (None, 0), (0, None), (16, 16))
    names = ("bp33k1", "bs33k1", "bp32k2", "bs32k2", "bp33k1+61", "bs33k1+61", "npk111i", "nsk111i", "npk212m+61", "nsk212m+61")
    by_name = {ix["name"]: ix for no in SETS for ix in SETS[no]}
    for name in names:
        ix = by_name[name]
        ri = F.ref_index(ref, ix)
        parents = [r[0] for r in F.reads_for(ix) if r[1] in ("exact", "sub", "del", "ins", "n", "short")]
        buf, off = _packed(parents)
        data = buf.tobytes().decode("latin-1")
        starts, lens = [], []
        for k, r in enumerate(parents):
            for c in range(3):                                # three windows into every parent: they overlap
                cl, cr = cuts[(k + 5 * c) % len(cuts)]
                cl = len(r) if cl is None else min(cl, len(r))
                cr = len(r) - cl if cr is None else min(cr, len(r) - cl)
                starts.append(int(off[k]) + cl)
                lens.append(len(r) - cl - cr)
        n = len(starts)
        slices = [data[a:a + w] for a, w in zip(starts, lens)]
        answers = F.once(("windows", name), lambda: [F.answer(ri, s) for s in slices])
        # the same windows with three more characters on the anchored side
        whole = F.once(("windows whole", name), lambda: [F.answer(ri, data[max(a - 3, 0):a + w] if ix["prefix"] else data[a:a + w + 3])
                                                         for a, w in zip(starts, lens)])
        assert lens.count(0) >= 50 and min(lens) == 0 and sum(w is not None for w in answers) >= 100
        # (the bytes outside matter: with three more characters on the anchored side many answers would be different)
        assert sum(x != y for x, y in zip(answers, whole)) >= 100, name
        _, o, b, s = _lookup(hip, F.own_index(ix), _up(buf), _up(starts, np.int64), _up(lens, np.int32), n)
        _same((o, b, s), _want(answers), slices, ("windows", name))


# ---- g. statuses, rows and arguments -----------------------------------------------------------------------------------------

def test_invalid_reads(hip, ref):
    """a byte >= 0x80 inside the longest indexed affix gives CAH_INVALID, best_adapter -1 and six zeros; behind it the byte
    is not read at all; a length above CAH_MAX_READ_LEN gives CAH_INVALID without a look at the (small) parent buffer"""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    by_name = {ix["name"]: ix for no in SETS for ix in SETS[no]}
    for name in ("bp33k1", "bs33k1", "bp33k1+61", "bs33k1+61", "bpmix", "bsmix+61"):
        ix = by_name[name]
        ri = F.ref_index(ref, ix)
        lmax = max(ri._lengths)
        seq = ix["adapters"][0][0]
        rng = random.Random(500)
        reads, answers = [], []
        for p in range(lmax + 6):                           # p: distance from the anchored end
            pad = "".join(rng.choice("ACGT") for _ in range(lmax + 6 - len(seq)))
            r = seq + pad if ix["prefix"] else pad + seq
            i = p if ix["prefix"] else len(r) - 1 - p
            for byte in (0x80, 0xC3, 0xFF):
                reads.append(r[:i].encode() + bytes([byte]) + r[i + 1:].encode())
                answers.append("invalid" if p < lmax else F.answer(ri, r[:i] + "A" + r[i + 1:]))
            reads.append(r.encode())                          # its neighbour is valid
            answers.append(F.answer(ri, r))
        wo, wb, ws = _want([None if w == "invalid" else w for w in answers])
        ws[[k for k, w in enumerate(answers) if w == "invalid"]] = INVALID
        assert (ws == INVALID).sum() == 3 * lmax and (ws == MATCH).sum() >= lmax
        buf, off = _packed(reads)
        _, o, b, s = _lookup(hip, F.own_index(ix), _up(buf), _up(off), None, len(reads))
        _same((o, b, s), (wo, wb, ws), reads, ("non-ASCII", name))
        # lengths above the limit: the parent holds 64 bytes
        small = _up(np.frombuffer((seq + "ACGT" * 16)[:64].encode(), dtype=np.uint8))
        lens = [MAX_READ_LEN + 1, len(seq) if ix["prefix"] else 64, 2 ** 31 - 1, MAX_READ_LEN + 1, 0]
        r1 = (seq + "ACGT" * 16)[:lens[1]]
        want = _want([None, F.answer(ri, r1), None, None, F.answer(ri, "")])
        want[2][[0, 2, 3]] = INVALID
        _, o, b, s = _lookup(hip, F.own_index(ix), small, _up([0, 0, 0, 63, 64], np.int64), _up(lens, np.int32), 5)
        _same((o, b, s), want, lens, ("too long", name))


def test_junk_characters(hip, ref):
    """space, U, newline, R, X: not in the packed dictionary (CAH_NONE, compared in a and b too); in a wide index whose adapters
    hold a literal 'R' and 'X' each matches only itself"""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    for ix in F.literal():
        reads, answers = _run(hip, ref, ix)
        junk = {(r.upper()[d if ix["prefix"] else len(r) - 1 - d], d): w
                for (r, kind, a, d), w in zip(reads, answers) if kind == "junk" and a == 0}
        assert len(junk) == 25
        assert {k for k, w in junk.items() if w is not None} == {("R", 15), ("X", 32)}, junk
        assert junk[("R", 15)][6] == 0 and junk[("X", 32)][6] == 0
    by_name = {ix["name"]: ix for no in SETS for ix in SETS[no]}
    for name in ("bp33k1", "bs33k1"):
        reads, answers = F.reads_and_answers(ref, by_name[name])
        # (junk in the adapter's last character still matches, one character shorter, as a deletion)
        inner = [w for r, w in zip(reads, answers) if r[1] == "junk" and r[3] <= 16]
        assert len(inner) == 30 and all(w is None for w in inner)
        assert all(w is not None for r, w in zip(reads, answers) if r[1] == "junk_behind")


def test_null_best_adapter_other_stream_and_empty_indexes(hip, ref):
    import torch
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    by_name = {ix["name"]: ix for no in SETS for ix in SETS[no]}
    for name in ("bp32k2", "bs32k2+61"):
        ix = by_name[name]
        reads, answers = F.reads_and_answers(ref, ix)
        buf, off = _packed([r[0] for r in reads])
        tb, to = _up(buf), _up(off)
        want = _want(answers)
        _, o, b, s = _lookup(hip, F.own_index(ix), tb, to, None, len(reads), best=False)
        assert b is None
        _same((o, None, s), want, reads, ("best_adapter NULL", name))
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        _, o, b, s = _lookup(hip, F.own_index(ix), tb, to, None, len(reads), stream=stream.cuda_stream)
        _same((o, b, s), want, reads, ("stream", name))
    # set 5: an index without a string answers CAH_NONE, -1 and six zeros for every read (no kernel: three memsets); next
    # to a normal adapter the empty one changes nothing
    for ix in SETS[5]:
        reads, answers = _run(hip, ref, ix)
        if ix["name"].endswith("alone"):
            assert F.own_index(ix)._h.lengths == [] and all(w is None for w in answers) and len(reads) > 100
            buf, off = _packed([r[0] for r in reads])
            _, o, b, s = _lookup(hip, F.own_index(ix), _up(buf), _up(off), None, len(reads), best=False)
            assert not o.any() and not s.any()
        else:
            assert sum(w is not None for w in answers) > 50 and all(w[0] == 1 for w in answers if w is not None)


def test_argument_errors_name_the_entry_and_launch_nothing(hip, ref):
    from cutadapt_amd import _lib
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    by_name = {ix["name"]: ix for no in SETS for ix in SETS[no]}
    for name in ("bp32k2", "bs32k2+61", "epalone"):
        ix = by_name[name]
        reads, answers = F.reads_and_answers(ref, ix)
        buf, off = _packed([r[0] for r in reads])
        tb, to = _up(buf), _up(off)
        n = len(reads)
        mi = F.own_index(ix)
        # n_reads == 0: CAH_OK, nothing written (not even with every pointer NULL)
        rc, o, b, s = _lookup(hip, mi, tb, to, None, 0)
        assert rc == OK
        assert hip.cah_index_lookup_batch(mi._h.handle, None, None, None, 0, None, None, None, None) == OK
        # _lookup allocates canary-filled outputs of n + 64 rows: after a refused call all of them still hold the canary
        import torch

        def refused(index, seqs, offsets, count, kill=None):
            out6 = _guarded(n, 6, torch.int32, CANARY_I32)
            st = _guarded(n, 0, torch.uint8, CANARY_U8)
            ba = _guarded(n, 0, torch.int32, CANARY_I32)
            args = [index, _p(seqs), _p(offsets), None, count, _p(out6), _p(ba), _p(st), None]
            if kill is not None:
                args[kill] = None
            assert hip.cah_index_lookup_batch(*args) == EINVAL, (name, count, kill)
            assert "cah_index_lookup_batch" in _lib.last_error(), _lib.last_error()
            torch.cuda.synchronize()
            assert (out6.cpu().numpy() == CANARY_I32).all() and (ba.cpu().numpy() == CANARY_I32).all() \
                and (st.cpu().numpy() == CANARY_U8).all(), (name, count, kill, "a refused call wrote")

        refused(mi._h.handle, tb, to, -1)
        refused(None, tb, to, n)
        refused(mi._h.handle, tb, to, n, kill=2)              # d_offsets
        refused(mi._h.handle, tb, to, n, kill=5)              # d_out6
        refused(mi._h.handle, tb, to, n, kill=7)              # d_status
        # ... and the same arguments put right do run
        _, o, b, s = _lookup(hip, mi, tb, to, None, n)
        _same((o, b, s), _want(answers), reads, ("after the errors", name))


# ---- h. rows without a match ---------------------------------------------------------------------------------------------------

def test_rows_without_a_match_are_zeroed(hip, ref):
    """cah_match_batch leaves six zeros in the row of a read without a match, and the header promises the same here: on
    outputs that hold the canary (a reused buffer) CAH_NONE and CAH_INVALID rows come back as zeros, packed and wide"""
    assert ref is not None, "oracle/_ref must travel to the GPU box"
    by_name = {ix["name"]: ix for no in SETS for ix in SETS[no]}
    for name in ("bp33k1", "bs33k1", "bp33k1+61", "bs33k1+61"):
        ix = by_name[name]
        reads, answers = F.reads_and_answers(ref, ix)
        raw = [_bytes(r[0]) for r in reads]
        raw += [b"\xff" + x[1:] if ix["prefix"] else x[:-1] + b"\xff" for x in raw[:300] if x]
        n_invalid = len(raw) - len(reads)
        buf, off = _packed(raw)
        _, o, b, s = _lookup(hip, F.own_index(ix), _up(buf), _up(off), None, len(raw))
        unmatched = [k for k, w in enumerate(answers) if w is None]
        assert len(unmatched) >= 100 and n_invalid >= 250
        assert (s[unmatched] == NONE).all() and (s[len(reads):] == INVALID).all()
        for rows in (unmatched, list(range(len(reads), len(raw)))):
            assert not o[rows].any(), (name, "rows without a match hold", o[rows][o[rows].any(axis=1)][:3].tolist())
            assert (b[rows] == -1).all()
        matched = [k for k, w in enumerate(answers) if w is not None]
        assert (s[matched] == MATCH).all() and (o[matched] != CANARY_I32).all()
