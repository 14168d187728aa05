"""The per-read trimming scans (cutadapt_amd/csrc/qualtrim.hip: k_quality_trim, k_nextseq_trim, k_poly_a_trim,
k_expected_errors, k_linked_views) and cah_validate_ascii_batch through the C ABI on tensors in HBM: every result is compared
-- integers exactly, doubles as .hex() -- with the plain restatement in tests/qualtrim_model.py (pinned on the CPU by
tests/test_qualtrim_model.py), on the reads of tests/qualtrim_families.py.  Each scan is one read per lane, 16 characters per
load with a byte-wise tail; the families put an exit in every lane of a first, a middle and a last chunk and in the tail,
and every claim of that kind is asserted on the model's own account of where it stopped.  Every output tensor has 64
guard rows behind it that must survive every call.  GPU only."""
import random

import numpy as np
import pytest

import qualtrim_families as F
import qualtrim_model as M

pytestmark = pytest.mark.gpu

EINVAL = 1
GUARD = 64
CANARY_I32, CANARY_I64, CANARY_F64, CANARY_U8 = -1515870811, -6510615555426900571, 12345.5, 0xA5
LANES = {(w, t) for w in ("first", "middle", "last") for t in range(16)}


# ---- helpers ----------------------------------------------------------------------------------------------------------------

def _up(a, dtype=None):
    """numpy array -> tensor in HBM (never empty)"""
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).to("cuda:0") if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device="cuda:0")


def _p(t):
    return None if t is None else t if isinstance(t, int) else t.data_ptr()


def _packed(reads):
    """reads back to back -> (bytes as uint8 array, offsets int64[n + 1])"""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in reads], out=off[1:])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), off


def _lens(reads):
    return np.array([len(x) for x in reads], dtype=np.int32)


def _guarded(n, cols, dtype, canary):
    import torch
    return torch.full((n + GUARD, cols) if cols else (n + GUARD,), canary, dtype=dtype, device="cuda:0")


def _rows(t, n, canary, what):
    """the first n rows of an output; everything behind them must still be the canary"""
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert (a[n:] == canary).all(), (what, "rows >= n_reads were written")
    return a[:n]


def _qt(L, quals, off, lens, n, cf, cb, base=33):
    import torch
    from cutadapt_amd import _lib
    out = _guarded(n, 2, torch.int32, CANARY_I32)
    _lib.check(L.cah_quality_trim_batch(_p(quals), _p(off), _p(lens), n, cf, cb, base, out.data_ptr(), None))
    return _rows(out, n, CANARY_I32, "quality_trim")


def _ns(L, seqs, quals, off, lens, n, cutoff=F.CUTOFF, base=33, qoff=None):
    import torch
    from cutadapt_amd import _lib
    out = _guarded(n, 0, torch.int32, CANARY_I32)
    if qoff is None:
        _lib.check(L.cah_nextseq_trim_batch(_p(seqs), _p(quals), _p(off), _p(lens), n, cutoff, base, out.data_ptr(), None))
    else:
        _lib.check(L.cah_nextseq_trim_batch_q(_p(seqs), _p(quals), _p(off), _p(qoff), _p(lens), n, cutoff, base, out.data_ptr(), None))
    return _rows(out, n, CANARY_I32, "nextseq")


def _pa(L, seqs, off, lens, n, rc):
    import torch
    from cutadapt_amd import _lib
    out = _guarded(n, 0, torch.int32, CANARY_I32)
    _lib.check(L.cah_poly_a_trim_batch(_p(seqs), _p(off), _p(lens), n, int(rc), out.data_ptr(), None))
    return _rows(out, n, CANARY_I32, "poly_a")


def _ee(L, quals, off, lens, n, base=33, status=True):
    """-> (values as .hex(), status bytes or None)"""
    import torch
    from cutadapt_amd import _lib
    out = _guarded(n, 0, torch.float64, CANARY_F64)
    st = _guarded(n, 0, torch.uint8, CANARY_U8) if status else None
    _lib.check(L.cah_expected_errors_batch(_p(quals), _p(off), _p(lens), n, base, out.data_ptr(), _p(st), None))
    values = [float(x).hex() for x in _rows(out, n, CANARY_F64, "expected_errors")]
    return values, (_rows(st, n, CANARY_U8, "expected_errors status").tolist() if status else None)


_cache = {}


def _once(key, make):
    """inputs and the model's answers are computed once and shared, never changed"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _table(golden):
    return _once("table", lambda: [float.fromhex(h) for h in golden("qualtrim.json")["error_table"]])


def _fam_a(base):
    return _once(("a", base), lambda: F.exit_sweep(base))


def _fam_b():
    return _once("b", lambda: F.zero_walks(102))


def _fam_c(base):
    return _once(("c", base), lambda: F.nextseq_sweep(base))


def _fam_d():
    return _once("d", lambda: F.poly_a_fixed()[0] + F.poly_a_random(103))


def _fam_e(base):
    return _once(("e", base), lambda: F.ee_valid(105, base) + F.ee_invalid(106, base)[0])


def _want_qt(tag, reads, cf, cb, base):
    return _once(("qt", tag, cf, cb, base), lambda: [M.quality_trim(q, cf, cb, base) for q in reads])


def _want_ns(tag, pairs, base):
    return _once(("ns", tag, base), lambda: [M.nextseq_trim(s, q, F.CUTOFF, base) for s, q in pairs])


def _want_pa(tag, reads, rc):
    return _once(("pa", tag, rc), lambda: [M.poly_a_trim(s, rc)[0] for s in reads])


def _want_ee(tag, reads, base, table):
    def make():
        res = [M.expected_errors(q, base, table)[0] for q in reads]
        return [v.hex() for v, _ in res], [M.MATCH if ok else M.INVALID for _, ok in res]
    return _once(("ee", tag, base), make)


def _same(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))[0])
        raise AssertionError((label, "first difference at read", at, got[at].tolist(), want[at].tolist()))


# ---- a. quality trimming: the exit position sweep -------------------------------------------------------------------------

def test_quality_trim_exit_sweep(hip):
    for base in F.BASES:
        reads = _fam_a(base)
        buf, off = _packed(reads)
        tb, to = _up(buf), _up(off)
        for cf, cb in F.QT_PARAMS:
            want = _want_qt("a", reads, cf, cb, base)
            _same(_qt(hip, tb, to, None, len(reads), cf, cb, base), [w[0] for w in want], ("a", cf, cb, base))
    # where the family leaves the two loops, by the model's own account (cutoffs 20 / 20)
    want = _want_qt("a", _fam_a(33), 20, 20, 33)
    front, back, neither = set(), set(), 0
    for q, (_, (seen_f, left_f), (seen_b, left_b)) in zip(_fam_a(33), want):
        if left_f:
            front.add(F.fwd_place(len(q), seen_f - 1))
        if left_b:
            back.add(F.bwd_place(len(q), len(q) - seen_b))
        neither += (not left_f and not left_b and len(q) >= 48)
    # an exit in every lane of a first, a middle and a last chunk, in the byte-wise tail, and in the last lane of the last
    # chunk of a read that is a multiple of 16 long (the tail loop is empty; backwards i ends at 0).
    # (What this holds is VALUES: a chunk loop that stops one chunk early -- `i > 16` for `i >= 16` -- leaves those 16
    # characters to the byte-wise tail, which computes the same; no comparison of results can tell the two apart.)
    assert LANES <= front and ("tail", None) in front, sorted(LANES - front)
    assert LANES <= back and ("tail", None) in back, sorted(LANES - back)
    assert neither >= 10
    mult16 = [(q, w) for q, w in zip(_fam_a(33), want) if len(q) in (32, 48, 64, 256)]
    assert any(lf and sf == len(q) for q, (_, (sf, lf), _) in mult16) and any(lb and sb == len(q) for q, (_, _, (sb, lb)) in mult16)
    assert any(not lf and not lb for _, (_, (_, lf), (_, lb)) in mult16)


# ---- b. quality trimming: walks around zero -------------------------------------------------------------------------------

def test_quality_trim_walks_around_zero(hip):
    reads = _fam_b()
    assert len(reads) >= 20000
    buf, off = _packed(reads)
    tb, to = _up(buf), _up(off)
    for cf, cb in ((20, 20), (23, 17), (17, 23)):
        want = _want_qt("b", reads, cf, cb, 33)
        _same(_qt(hip, tb, to, None, len(reads), cf, cb), [w[0] for w in want], ("b", cf, cb))
    res = [w[0] for w in _want_qt("b", reads, 20, 20, 33)]
    # (the fixed reads in front of the drawn ones) both outcomes: the collapse of start >= stop to (0, 0), and a segment
    # trimmed at both ends; bytes >= 0x80 count as negative qualities
    assert any(r == (0, 0) and len(q) >= 16 for q, r in zip(reads[:9], res)), res[:9]
    assert any(0 < r[0] < r[1] < len(q) for q, r in zip(reads[:9], res)), res[:9]
    assert reads[8][0] == 0x80 and res[8] == (1, 4), res[8]


# ---- c. NextSeq trimming -----------------------------------------------------------------------------------------------------

def test_nextseq_sweep(hip):
    for base in F.BASES:
        pairs = _fam_c(base)
        sbuf, off = _packed([s for s, _ in pairs])
        qbuf, _ = _packed([q for _, q in pairs])
        want = _want_ns("c", pairs, base)
        got = _ns(hip, _up(sbuf), _up(qbuf), _up(off), None, len(pairs), F.CUTOFF, base)
        _same(got, [w[0] for w in want], ("c", base))
    pairs, want = _fam_c(33), _want_ns("c", _fam_c(33), 33)
    places, past_g, at_g, never = set(), 0, 0, 0
    for (s, q), (stop, (seen, left)) in zip(pairs, want):
        if left:
            places.add(F.bwd_place(len(s), len(s) - seen))
            # a run of G (each adds 1 to the sum) that crosses at least one chunk boundary before the scan stops
            past_g += (s.endswith(b"G" * (seen - 1)) and seen - 1 > 16)
            at_g += (s[len(s) - seen] == ord("g"))
        never += (not left and len(s) >= 48)
    assert LANES <= places and ("tail", None) in places, sorted(LANES - places)
    assert past_g >= 10 and at_g >= 10 and never >= 10, (past_g, at_g, never)


def test_nextseq_in_a_fastq_chunk(hip):
    """cah_nextseq_trim_batch_q on @name / SEQ / + / QUAL records: the qualities at their own offsets, every pair of
    16-byte phases of the two"""
    pairs = _fam_c(33)
    parts, soff, qoff, pos = [], [], [], 0
    turn = [0] * 16
    for s, q in pairs:
        n = len(s)
        phase = turn[n % 16] % 16                                 # the sequence's phase; the qualities' is phase + n + 3
        turn[n % 16] += 1
        name = b"r" * (((phase - pos - 2) % 16) or 16)
        rec = b"@" + name + b"\n" + s + b"\n+\n" + q + b"\n"
        soff.append(pos + len(name) + 2)
        qoff.append(soff[-1] + n + 3)
        parts.append(rec)
        pos += len(rec)
    data = b"".join(parts)
    assert all(data[a:a + len(s)] == s and data[b:b + len(q)] == q for (s, q), a, b in zip(pairs[::97], soff[::97], qoff[::97]))
    phases = {(a % 16, b % 16) for (s, _), a, b in zip(pairs, soff, qoff) if len(s) >= 16}
    assert len(phases) == 256, len(phases)
    chunk = _up(np.frombuffer(data, dtype=np.uint8))
    assert chunk.data_ptr() % 16 == 0
    got = _ns(hip, chunk, chunk, _up(soff, np.int64), _up(_lens([s for s, _ in pairs])), len(pairs), qoff=_up(qoff, np.int64))
    _same(got, [w[0] for w in _want_ns("c", pairs, 33)], "c in a FASTQ chunk")


# ---- d. poly-A, both orientations ---------------------------------------------------------------------------------------------

def test_poly_a_both_orientations(hip):
    reads = _fam_d()
    fixed, deciding = _once("d fixed", F.poly_a_fixed)
    assert reads[:len(fixed)] == fixed and len(reads) >= len(fixed) + 20000
    buf, off = _packed(reads)
    tb, to = _up(buf), _up(off)
    for rc in (False, True):
        _same(_pa(hip, tb, to, None, len(reads), rc), _want_pa("d", reads, rc), ("d", rc))
    # the boundary tails: kept at exactly 0.2 and with one error fewer, not kept with one error more or one 'A' short;
    # the character that decides it in every lane of a chunk and in the byte-wise tail
    lanes = {False: set(), True: set()}
    for k, (index, kind, rc) in deciding.items():
        n = len(fixed[k])
        got = _want_pa("d", reads, rc)[k]
        tail = index + 1 if rc else n - index
        kept = (tail if rc else index)
        assert got == (kept if kind in (0, 2) and tail >= 3 else (0 if rc else n)), (fixed[k], rc, kind, got)
        if kind == 0:
            lanes[rc].add((F.fwd_place if rc else F.bwd_place)(n, index))
    for rc in (False, True):
        assert {t for w, t in lanes[rc] if w != "tail"} == set(range(16)) and ("tail", None) in lanes[rc], (rc, lanes[rc])


# ---- e. expected errors -------------------------------------------------------------------------------------------------------

def test_expected_errors(hip, golden):
    table = _table(golden)
    for base in F.BASES:
        reads = _fam_e(base)
        want_v, want_s = _want_ee("e", reads, base, table)
        buf, off = _packed(reads)
        tb, to = _up(buf), _up(off)
        got_v, got_s = _ee(hip, tb, to, None, len(reads), base)
        # (bit-identical doubles; -1.0 and CAH_INVALID for the read with the invalid byte ONLY: its neighbours are valid)
        assert got_s == want_s, (base, int(np.flatnonzero(np.array(got_s) != np.array(want_s))[0]))
        assert got_v == want_v, (base, [k for k in range(len(reads)) if got_v[k] != want_v[k]][:5])
        assert _ee(hip, tb, to, None, len(reads), base, status=False)[0] == want_v, base       # d_status = NULL
    # where the invalid byte sits: every lane of the 16-character loop, the groups of four, the single characters
    n_valid = len(F.ee_valid(105, 33))
    reads, bad = F.ee_invalid(106, 33)
    assert reads == _fam_e(33)[n_valid:]
    sixteen, four, single = set(), 0, 0
    for k in bad:
        n = len(reads[k])
        pos = [i for i in range(n) if reads[k][i] != reads[k - 1][i]]
        assert len(pos) == 1 and want_s is not None
        i = pos[0]
        if i < 16 * (n // 16):
            sixteen.add(i % 16)
        elif i < n - n % 4:
            four += 1
        else:
            single += 1
        assert _want_ee("e", _fam_e(33), 33, table)[1][n_valid + k - 1:n_valid + k + 2] == [M.MATCH, M.INVALID, M.MATCH]
    assert sixteen == set(range(16)) and four >= 16 and single >= 16, (sixteen, four, single)


# ---- f. windows -----------------------------------------------------------------------------------------------------------------

def test_windows_into_a_parent_batch(hip, golden):
    """every entry with (offsets, d_lens) windows cut 0 .. 17 characters short at both ends, empty ones included; what was
    cut away is poisoned with bytes that would change the result if they were read"""
    table = _table(golden)
    rng = random.Random(107)
    sizes = (0, 1, 15, 16, 17, 31, 32, 33, 34, 35, 36, 48, 49, 50, 64, 65, 81, 129)
    quals, seq_n, seq_p, offs, lens = [], [], [], [], []
    pos = 0
    for cl in range(18):
        for cr in range(18):
            for n in sizes:
                a, b = (cl, n - cr) if cl + cr <= n else (min(cl, n), min(cl, n))
                w = b - a
                q = bytes(rng.choice(b"\x00\xff\x7f ") for _ in range(a)) + bytes(33 + F.CUTOFF + rng.randint(-3, 3) for _ in range(w)) \
                    + bytes(rng.choice(b"\x00\xff\x7f ") for _ in range(n - b))
                sn = b"G" * a + bytes(rng.choice(b"GGGGGGAg") for _ in range(w)) + b"G" * (n - b)
                sp = b"T" * a + bytes(rng.choice(b"TTTTTTCA") for _ in range(w // 2)) + bytes(rng.choice(b"AAAAAACT") for _ in range(w - w // 2)) \
                    + b"A" * (n - b)
                quals.append(q); seq_n.append(sn); seq_p.append(sp)
                offs.append(pos + a); lens.append(w)
                pos += n
    n = len(offs)
    empty = sum(1 for w in lens if w == 0)
    assert n == 18 * 18 * len(sizes) and empty >= 324 and max(lens) == 129
    qb, sb, pb = b"".join(quals), b"".join(seq_n), b"".join(seq_p)
    win = lambda data: [data[o:o + w] for o, w in zip(offs, lens)]
    tq, tn, tp = (_up(np.frombuffer(x, dtype=np.uint8)) for x in (qb, sb, pb))
    to, tl = _up(offs, np.int64), _up(lens, np.int32)
    for cf, cb in ((20, 20), (23, 17)):
        _same(_qt(hip, tq, to, tl, n, cf, cb), [M.quality_trim(q, cf, cb)[0] for q in win(qb)], ("f quality", cf, cb))
    want_ns = [M.nextseq_trim(s, q, F.CUTOFF)[0] for s, q in zip(win(sb), win(qb))]
    _same(_ns(hip, tn, tq, to, tl, n), want_ns, "f nextseq")
    shifted = _up(np.frombuffer(b"#####" + qb, dtype=np.uint8))   # the same qualities five bytes further on, at their own offsets
    _same(_ns(hip, tn, shifted, to, tl, n, qoff=_up(np.array(offs) + 5, np.int64)), want_ns, "f nextseq_q")
    for rc in (False, True):
        _same(_pa(hip, tp, to, tl, n, rc), [M.poly_a_trim(s, rc)[0] for s in win(pb)], ("f poly_a", rc))
    res = [M.expected_errors(q, 33, table)[0] for q in win(qb)]
    got_v, got_s = _ee(hip, tq, to, tl, n)
    assert got_s == [M.MATCH] * n and got_v == [v.hex() for v, _ in res]


# ---- g. independence from the neighbours ---------------------------------------------------------------------------------------

def _layout(columns, k):
    """the reads of every column (same lengths) laid out with gaps of 0 .. 31 bytes in front of each, filled -- layout k --
    with 0x00, 0xFF, 'A' / 'T' / 'G', '#'; the gaps differ between the layouts, so every read lands at other 16-byte phases
    -> (one buffer per column, offsets, lens)"""
    parts = [[] for _ in columns]
    offs, pos = [], 0
    for r in range(len(columns[0])):
        gap = (r * (3 + 2 * k) + k) % 32
        fill = (b"\x00", b"\xff", b"ATG"[r % 3:r % 3 + 1], b"#")[k] * gap
        offs.append(pos + gap)
        for c, col in enumerate(columns):
            parts[c].append(fill)
            parts[c].append(col[r])
        pos += gap + len(columns[0][r])
    tail = (b"\x00", b"\xff", b"A", b"#")[k] * 48                 # (nothing of interest sits at the allocation's edge)
    return [np.frombuffer(b"".join(p) + tail, dtype=np.uint8) for p in parts], np.array(offs, dtype=np.int64), _lens(columns[0])


def test_results_do_not_depend_on_the_bytes_between_reads(hip, golden):
    table = _table(golden)
    qt_reads = _fam_a(33) + _fam_b()
    want_qt = [w[0] for w in _want_qt("a", _fam_a(33), 20, 20, 33)] + [w[0] for w in _want_qt("b", _fam_b(), 20, 20, 33)]
    pairs = _fam_c(33)
    want_ns = [w[0] for w in _want_ns("c", pairs, 33)]
    pa_reads = _fam_d()
    ee_reads = _fam_e(33)
    want_v, want_s = _want_ee("e", ee_reads, 33, table)
    phases = set()
    for k in range(4):
        (buf,), off, lens = _layout([qt_reads], k)
        _same(_qt(hip, _up(buf), _up(off), _up(lens), len(qt_reads), 20, 20), want_qt, ("g quality", k))
        phases.add(tuple(off[:64] % 16))
        (sbuf, qbuf), off, lens = _layout([[s for s, _ in pairs], [q for _, q in pairs]], k)
        _same(_ns(hip, _up(sbuf), _up(qbuf), _up(off), _up(lens), len(pairs)), want_ns, ("g nextseq", k))
        (buf,), off, lens = _layout([pa_reads], k)
        tb, to, tl = _up(buf), _up(off), _up(lens)
        for rc in (False, True):
            _same(_pa(hip, tb, to, tl, len(pa_reads), rc), _want_pa("d", pa_reads, rc), ("g poly_a", k, rc))
        (buf,), off, lens = _layout([ee_reads], k)
        got_v, got_s = _ee(hip, _up(buf), _up(off), _up(lens), len(ee_reads))
        assert got_s == want_s and got_v == want_v, ("g expected_errors", k)
    assert len(phases) == 4                                       # (four different layouts)


# ---- h. output bounds ---------------------------------------------------------------------------------------------------------

def test_only_rows_below_n_reads_are_written(hip, golden):
    """n_reads on either side of a wave and of a block of 256: the rows < n_reads hold the model's answers, the 64 guard
    rows behind them still hold the canary (_rows asserts it for every call of this file; here the counts are the point);
    n_reads = 0 touches nothing"""
    table = _table(golden)
    rng = random.Random(108)
    quals = F.zero_walks(108, 1025 - 9)
    assert len(quals) == 1025
    seqs = [bytes(rng.choice(b"AAAATTTTGGGGCg") for _ in range(len(q))) for q in quals]
    qbuf, off = _packed(quals)
    sbuf, _ = _packed(seqs)
    tq, ts, to = _up(qbuf), _up(sbuf), _up(off)
    tl, tqo = _up(_lens(quals)), _up(off[:-1] + 3)
    shifted = _up(np.frombuffer(b"###" + qbuf.tobytes(), dtype=np.uint8))
    want_qt = [M.quality_trim(q, 20, 20)[0] for q in quals]
    want_ns = [M.nextseq_trim(s, q, F.CUTOFF)[0] for s, q in zip(seqs, quals)]
    want_pa = {rc: [M.poly_a_trim(s, rc)[0] for s in seqs] for rc in (False, True)}
    res = [M.expected_errors(q, 33, table)[0] for q in quals]
    want_v, want_s = [v.hex() for v, _ in res], [M.MATCH if ok else M.INVALID for _, ok in res]
    assert M.INVALID in want_s and M.MATCH in want_s[:9]
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1025):
        _same(_qt(hip, tq, to, None, n, 20, 20), np.array(want_qt[:n]).reshape(n, 2), ("h quality", n))
        _same(_ns(hip, ts, tq, to, None, n), want_ns[:n], ("h nextseq", n))
        _same(_ns(hip, ts, shifted, to, tl, n, qoff=tqo), want_ns[:n], ("h nextseq_q", n))
        for rc in (False, True):
            _same(_pa(hip, ts, to, None, n, rc), want_pa[rc][:n], ("h poly_a", n, rc))
        got_v, got_s = _ee(hip, tq, to, None, n)
        assert got_v == want_v[:n] and got_s == want_s[:n], ("h expected_errors", n)


# ---- i. offsets beyond 2^31 and 2^32 ----------------------------------------------------------------------------------------

def test_offsets_beyond_2_31_and_2_32(hip, golden):
    """one allocation of 2^32 + 64 KiB bytes; reads in three clusters -- across 2^31, across 2^32, at the end --, the rest
    of the allocation as it came"""
    import torch
    table = _table(golden)
    total = (1 << 32) + (64 << 10)
    big = torch.empty(total, dtype=torch.uint8, device="cuda:0")
    base_ptr = big.data_ptr()
    rng = random.Random(109)
    a_all, c_all, d_all = _fam_a(33), _fam_c(33), _once("d fixed", F.poly_a_fixed)[0]
    quals = [a_all[i] for i in sorted(rng.sample(range(len(a_all)), 200))]
    pairs = [c_all[i] for i in sorted(rng.sample(range(len(c_all)), 200))]
    polys = [d_all[i] for i in sorted(rng.sample(range(len(d_all)), 200))]
    want_qt = [M.quality_trim(q, 20, 20)[0] for q in quals]
    res = [M.expected_errors(q, 33, table)[0] for q in quals]
    want_ns = [M.nextseq_trim(s, q, F.CUTOFF)[0] for s, q in pairs]
    want_pa = {rc: [M.poly_a_trim(s, rc)[0] for s in polys] for rc in (False, True)}

    def put(reads, start):
        """the reads back to back from byte `start` of the allocation -> (offsets, lens) on the device"""
        buf, off = _packed(reads)
        assert 0 <= start and start + len(buf) <= total
        big[start:start + len(buf)].copy_(torch.from_numpy(buf.copy()))
        return off[:-1] + start, _up(off[:-1] + start), _up(_lens(reads))

    def across(reads, edge):
        """a start that puts the middle read across `edge` (or the last read's end on it, at the allocation's end)"""
        _, off = _packed(reads)
        if edge == total:
            return total - int(off[-1])
        mid = next(i for i in range(len(reads) // 2, len(reads)) if len(reads[i]) >= 32)
        return edge - int(off[mid]) - len(reads[mid]) // 2

    for edge in (1 << 31, 1 << 32, total):
        at, to, tl = put(quals, across(quals, edge))
        n = len(quals)
        if edge != total:                                         # reads below, across and above the edge
            ends = at + _lens(quals)
            assert (ends < edge).any() and ((at < edge) & (ends > edge)).any() and (at > edge).any()
        else:
            assert int(at[-1]) + len(quals[-1]) == total and int(at[0]) > (1 << 32)
        _same(_qt(hip, base_ptr, to, tl, n, 20, 20), want_qt, ("i quality", edge))
        got_v, got_s = _ee(hip, base_ptr, to, tl, n)
        assert got_v == [v.hex() for v, _ in res] and got_s == [M.MATCH] * n, ("i expected_errors", edge)
        at, to, tl = put(polys, across(polys, edge))
        for rc in (False, True):
            _same(_pa(hip, base_ptr, to, tl, len(polys), rc), want_pa[rc], ("i poly_a", edge, rc))
        # NextSeq: the sequences across the edge, the qualities right behind them -- through a second base pointer (the
        # plain form: one offset for both) and at their own offsets (the _q form)
        seqs, quals_c = [s for s, _ in pairs], [q for _, q in pairs]
        nbytes = sum(len(s) for s in seqs)
        start = across(seqs, edge) - (nbytes + 7 if edge == total else 0)
        at, to, tl = put(seqs, start)
        qat, tqo, _ = put(quals_c, start + nbytes + 7)
        _same(_ns(hip, base_ptr, base_ptr + nbytes + 7, to, tl, len(pairs)), want_ns, ("i nextseq", edge))
        _same(_ns(hip, base_ptr, base_ptr, to, tl, len(pairs), qoff=tqo), want_ns, ("i nextseq_q", edge))
        if edge == 1 << 32:                                       # ... and all sequences below 2^32, all qualities above it
            at, to, tl = put(seqs, edge - nbytes - 5)
            qat, tqo, _ = put(quals_c, edge + 3)
            assert int(at[-1]) + len(seqs[-1]) < edge < int(qat[0])
            _same(_ns(hip, base_ptr, base_ptr, to, tl, len(pairs), qoff=tqo), want_ns, "i nextseq_q either side of 2^32")
    del big
    torch.cuda.empty_cache()


# ---- j. cah_linked_views ------------------------------------------------------------------------------------------------------

def test_linked_views(hip):
    import torch
    from cutadapt_amd import _lib
    rng = random.Random(110)
    n = 1025
    lens = [F.LENS[(7 * r) % len(F.LENS)] for r in range(n)]
    gaps = [r % 9 for r in range(n)]
    offs, pos = [], 0
    for k in range(n):
        offs.append(pos + gaps[k])
        pos += gaps[k] + lens[k]
    packed = [0]
    for k in range(n):
        packed.append(packed[-1] + lens[k])
    read_len = 37

    def case(r, length):
        """status 0 / 1 / 2 x query_stop 0, n, above n, negative, inside: all fifteen, in turn"""
        stop = (0, length, length + 1 + r % 5, -1 - r % 7, length // 2)[(r // 3) % 5]
        return r % 3, stop

    for form, (o, l, rl) in enumerate(((None, None, read_len), (packed, None, 0), (offs, lens, 0))):
        length = (lambda r: read_len) if rl else (lambda r: lens[r])
        cases = [case(r, length(r)) for r in range(n)]
        status = [s for s, _ in cases]
        out6 = [[rng.randrange(-5, 300), rng.randrange(-5, 300), rng.randrange(-5, 300), stop, 7, 8] for _, stop in cases]
        assert {(s, (q > 0) + (q >= length(r) > 0) + (q > length(r)) - (q < 0)) for r, (s, q) in enumerate(cases)} >= \
               {(s, k) for s in (0, 1, 2) for k in (-1, 0, 1, 2, 3)}
        want_starts, want_lens = M.linked_views(out6, status, o, l, rl)
        for count in (n, 257, 1, 0):
            starts = _guarded(count, 0, torch.int64, CANARY_I64)
            views = _guarded(count, 0, torch.int32, CANARY_I32)
            t6, ts = _up(out6, np.int32), _up(status, np.uint8)
            to = None if o is None else _up(o, np.int64)
            tl = None if l is None else _up(l, np.int32)
            _lib.check(hip.cah_linked_views(_p(t6), _p(ts), _p(to), _p(tl), rl, count, starts.data_ptr(), views.data_ptr(), None))
            _same(_rows(starts, count, CANARY_I64, "starts"), want_starts[:count], ("j starts", form, count))
            _same(_rows(views, count, CANARY_I32, "view_lens"), want_lens[:count], ("j view_lens", form, count))
        # every view lies inside its read
        assert all(0 <= v <= length(r) for r, v in enumerate(want_lens))


# ---- k. cah_validate_ascii_batch ------------------------------------------------------------------------------------------------

def test_validate_ascii_counts_reads(hip):
    import torch
    from cutadapt_amd import _lib
    rng = random.Random(111)
    reads, dirty = [], []
    for k in range(3000):
        q = bytearray(rng.choice(b"ACGTN\x7f\x00") for _ in range(F.LENS[k % len(F.LENS)]))
        if k % 7 == 3 and len(q) >= 3:                            # several bytes >= 0x80 in one read: still ONE read
            for i in {0, len(q) // 2, len(q) - 1} | ({rng.randrange(len(q))} if k % 2 else set()):
                q[i] = rng.randrange(0x80, 0x100)
            dirty.append(k)
        reads.append(bytes(q))
    assert len(dirty) >= 100 and M.ascii_bad_reads(reads) == len(dirty) < sum(b >= 0x80 for q in reads for b in q)
    buf, off = _packed(reads)
    tb, to = _up(buf), _up(off)
    bad = torch.full((1 + GUARD,), 77, dtype=torch.int32, device="cuda:0")

    def run(offsets, lens, n):
        bad.fill_(77)                                             # (the call has to reset it)
        _lib.check(hip.cah_validate_ascii_batch(_p(tb), _p(offsets), _p(lens), n, bad.data_ptr(), None))
        torch.cuda.synchronize()
        assert (bad[1:] == 77).all()
        return int(bad[0])

    assert run(to, None, len(reads)) == len(dirty)
    assert run(to, None, dirty[0]) == 0 and run(to, None, dirty[0] + 1) == 1
    assert run(to, None, 0) == 0 and run(None, None, 0) == 0
    # windows: the first and the last character cut away -- what is left of a dirty read still holds the byte in the middle --
    # and windows that exclude every offending byte
    lens = _lens(reads)
    inner = [M.ascii_bad_reads([q[1:len(q) - 1] for q in reads])]
    assert inner[0] == len(dirty)
    assert run(_up(off[:-1] + 1), _up(np.maximum(lens - 2, 0)), len(reads)) == inner[0]
    first_bad = [next((i for i, b in enumerate(q) if b >= 0x80), len(q)) for q in reads]
    assert run(to, _up(first_bad, np.int32), len(reads)) == 0
    one_more = np.minimum(np.array(first_bad) + 1, lens)
    assert run(to, _up(one_more, np.int32), len(reads)) == len(dirty)


# ---- l. argument errors ---------------------------------------------------------------------------------------------------------

def test_argument_errors_name_the_entry_and_launch_nothing(hip):
    import torch
    from cutadapt_amd import _lib
    L = hip
    reads = F.zero_walks(112, 91)
    n = len(reads)
    buf, off = _packed(reads)
    tb, to, tl = _up(buf), _up(off), _up(_lens(reads))
    b, o, l = tb.data_ptr(), to.data_ptr(), tl.data_ptr()
    i32 = _guarded(2 * n, 0, torch.int32, CANARY_I32)
    i64 = _guarded(n, 0, torch.int64, CANARY_I64)
    f64 = _guarded(n, 0, torch.float64, CANARY_F64)
    u8 = _guarded(n, 0, torch.uint8, CANARY_U8)
    o6 = _up(np.zeros((n, 6), np.int32))
    pi, pl, pf, pu, p6 = i32.data_ptr(), i64.data_ptr(), f64.data_ptr(), u8.data_ptr(), o6.data_ptr()
    calls = [
        ("cah_quality_trim_batch", lambda: L.cah_quality_trim_batch(b, o, None, -1, 0, 20, 33, pi, None)),
        ("cah_quality_trim_batch", lambda: L.cah_quality_trim_batch(b, None, l, n, 0, 20, 33, pi, None)),
        ("cah_quality_trim_batch", lambda: L.cah_quality_trim_batch(b, o, None, n, 0, 20, 33, None, None)),
        ("cah_nextseq_trim_batch", lambda: L.cah_nextseq_trim_batch(b, b, o, None, -1, 20, 33, pi, None)),
        ("cah_nextseq_trim_batch", lambda: L.cah_nextseq_trim_batch(b, b, None, l, n, 20, 33, pi, None)),
        ("cah_nextseq_trim_batch", lambda: L.cah_nextseq_trim_batch(b, b, o, None, n, 20, 33, None, None)),
        ("cah_nextseq_trim_batch_q", lambda: L.cah_nextseq_trim_batch_q(b, b, o, o, l, -1, 20, 33, pi, None)),
        ("cah_nextseq_trim_batch_q", lambda: L.cah_nextseq_trim_batch_q(b, b, None, o, l, n, 20, 33, pi, None)),
        ("cah_nextseq_trim_batch_q", lambda: L.cah_nextseq_trim_batch_q(b, b, o, None, l, n, 20, 33, pi, None)),
        ("cah_nextseq_trim_batch_q", lambda: L.cah_nextseq_trim_batch_q(b, b, o, o, None, n, 20, 33, pi, None)),
        ("cah_nextseq_trim_batch_q", lambda: L.cah_nextseq_trim_batch_q(b, b, o, o, l, n, 20, 33, None, None)),
        ("cah_poly_a_trim_batch", lambda: L.cah_poly_a_trim_batch(b, o, None, -1, 0, pi, None)),
        ("cah_poly_a_trim_batch", lambda: L.cah_poly_a_trim_batch(b, None, l, n, 0, pi, None)),
        ("cah_poly_a_trim_batch", lambda: L.cah_poly_a_trim_batch(b, o, None, n, 1, None, None)),
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, o, None, -1, 33, pf, pu, None)),
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, None, l, n, 33, pf, pu, None)),
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, o, None, n, 33, None, pu, None)),
        # the table has 94 entries, phred 0 .. 93: a base below 33 would let a valid byte index past it
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, o, None, n, 32, pf, pu, None)),
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, o, None, n, 0, pf, pu, None)),
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, o, None, n, -1, pf, pu, None)),
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, o, None, n, 127, pf, pu, None)),
        ("cah_expected_errors_batch", lambda: L.cah_expected_errors_batch(b, o, None, 0, 32, pf, pu, None)),
        ("cah_linked_views", lambda: L.cah_linked_views(p6, pu, o, l, 0, -1, pl, pi, None)),
        ("cah_linked_views", lambda: L.cah_linked_views(None, pu, o, l, 0, n, pl, pi, None)),
        ("cah_linked_views", lambda: L.cah_linked_views(p6, None, o, l, 0, n, pl, pi, None)),
        ("cah_linked_views", lambda: L.cah_linked_views(p6, pu, o, l, 0, n, None, pi, None)),
        ("cah_linked_views", lambda: L.cah_linked_views(p6, pu, o, l, 0, n, pl, None, None)),
        ("cah_linked_views", lambda: L.cah_linked_views(p6, pu, None, None, 0, n, pl, pi, None)),
        ("cah_linked_views", lambda: L.cah_linked_views(p6, pu, None, l, -4, n, pl, pi, None)),
        ("cah_validate_ascii_batch", lambda: L.cah_validate_ascii_batch(b, o, None, n, None, None)),
        ("cah_validate_ascii_batch", lambda: L.cah_validate_ascii_batch(b, None, None, n, pi, None)),
    ]
    for k, (name, call) in enumerate(calls):
        assert call() == EINVAL, (k, name)
        assert name in _lib.last_error(), (k, name, _lib.last_error())
    torch.cuda.synchronize()
    # nothing was launched: no output changed
    for t, canary in ((i32, CANARY_I32), (i64, CANARY_I64), (f64, CANARY_F64), (u8, CANARY_U8)):
        assert (t.cpu().numpy() == canary).all()
    # ... and the same arguments put right do run; base 33 and 126 are the ends of the range
    assert L.cah_expected_errors_batch(b, o, None, n, 33, pf, pu, None) == 0
    assert L.cah_expected_errors_batch(b, o, None, n, 126, pf, pu, None) == 0
    assert L.cah_quality_trim_batch(b, o, None, n, 0, 20, 33, pi, None) == 0
    torch.cuda.synchronize()
    assert (i32.cpu().numpy()[:2 * n] != CANARY_I32).all() and (i32.cpu().numpy()[2 * n:] == CANARY_I32).all()
