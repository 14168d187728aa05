"""A plain model of KmerFinder.kmers_present (reference _kmer_finder.pyx:170-257) for the prefilter tests.

A different algorithm from the kernels on purpose: no shift-and, no packing into words.  Per search set the window is
computed as _kmer_finder.pyx:186-204 does, a positive stop beyond the read end is clamped to the read end (what the
library, the oracle and tests/golden/make_golden.py implement -- the reference reads out of bounds there), and every
non-empty k-mer is tried at every start inside the window, character by character, under the relation of
_match_tables.matches_lookup.  The tables are restated here; nothing of the library is imported.

  window(start, stop, n)                     -> (ws, we), ws == we == 0 for "no search"
  chars_match(k, c, ref_wc, query_wc)        -> does k-mer character k accept read character c
  present(sets, read, ref_wc, query_wc)      -> bool
  first_hit_end(sets, read, ref_wc, query_wc)-> position of the last character of the earliest-ending occurrence
                                                that lies in its window, or None
  present_block / first_hit_end_block        the same over a block of equally long reads at once (numpy; one
                                             comparison per k-mer character over all starts of all reads)
Reads are str (latin-1: one character per byte) or bytes."""
import numpy as np

_A, _C, _G, _T = 1, 2, 4, 8
_IUPAC = dict(X=0, A=_A, C=_C, G=_G, T=_T, U=_T, R=_A | _G, Y=_C | _T, S=_G | _C, W=_A | _T, K=_G | _T, M=_A | _C,
              B=_C | _G | _T, D=_A | _G | _T, H=_A | _C | _T, V=_A | _C | _G, N=_A | _C | _G | _T | 0x80)
_ACGT = dict(A=_A, C=_C, G=_G, T=_T, U=_T)


def _up(ch):
    """ASCII upper case of one character (bytes.upper: nothing but a-z moves)"""
    return chr(ord(ch) - 32) if "a" <= ch <= "z" else ch


def _iupac(ch):
    return _IUPAC.get(_up(ch), 0)


def _acgt(ch):
    return _ACGT.get(_up(ch), 0x80)


def chars_match(k, c, ref_wc=False, query_wc=False):
    """k: a character of a k-mer, c: a character of the read.  NUL and bytes >= 0x80 of the read match nothing."""
    if not 0 < ord(c) < 128:
        return False
    if not ref_wc and not query_wc:
        return _up(k) == _up(c)
    if ref_wc and not query_wc:
        return (_iupac(k) & _acgt(c)) != 0
    if query_wc and not ref_wc:
        return (_acgt(k) & _iupac(c)) != 0
    return (_iupac(k) & _iupac(c)) != 0


def window(start, stop, n):
    """_kmer_finder.pyx:188-204 with the clamp of a positive stop; stop None or 0: to the end"""
    stop = 0 if stop is None else stop
    if start < 0:
        start = max(n + start, 0)
    elif start > n:
        return 0, 0
    if stop < 0:
        stop = n + stop
        if stop <= 0:
            return 0, 0
    elif stop == 0:
        stop = n
    stop = min(stop, n)
    if stop - start <= 0:
        return 0, 0
    return start, stop


def _text(read):
    return read.decode("latin-1") if isinstance(read, (bytes, bytearray)) else read


def occurrences(kmer, read, ws, we, ref_wc=False, query_wc=False):
    """starts s with ws <= s, s + len(kmer) <= we at which kmer matches"""
    q = len(kmer)
    return [s for s in range(ws, we - q + 1)
            if all(chars_match(kmer[i], read[s + i], ref_wc, query_wc) for i in range(q))]


def first_hit_end(sets, read, ref_wc=False, query_wc=False):
    read = _text(read)
    n = len(read)
    best = None
    for start, stop, kmers in sets:
        ws, we = window(start, stop, n)
        for kmer in kmers:
            if not kmer:
                continue
            occ = occurrences(kmer, read, ws, we, ref_wc, query_wc)
            if occ and (best is None or occ[0] + len(kmer) - 1 < best):
                best = occ[0] + len(kmer) - 1
    return best


def present(sets, read, ref_wc=False, query_wc=False):
    return first_hit_end(sets, read, ref_wc, query_wc) is not None


# ---- blocks of equally long reads -------------------------------------------------------------------------------------

_tables = {}


def _accepts(k, ref_wc, query_wc):
    """bool[256]: the byte values k-mer character k accepts"""
    key = (k, ref_wc, query_wc)
    if key not in _tables:
        _tables[key] = np.array([chars_match(k, chr(b), ref_wc, query_wc) for b in range(256)], dtype=bool)
    return _tables[key]


def as_block(reads):
    """equally long reads -> uint8[len(reads), n]"""
    raw = [r if isinstance(r, (bytes, bytearray)) else r.encode("latin-1") for r in reads]
    n = len(raw[0]) if raw else 0
    assert all(len(x) == n for x in raw)
    return np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(len(raw), n)


def first_hit_end_block(sets, block, ref_wc=False, query_wc=False):
    """int64[reads]: first_hit_end of every row of the block, -1 for None"""
    rows, n = block.shape
    none = np.iinfo(np.int64).max
    best = np.full(rows, none, dtype=np.int64)
    for start, stop, kmers in sets:
        ws, we = window(start, stop, n)
        for kmer in kmers:
            q = len(kmer)
            if q == 0 or we - ws < q:
                continue
            starts = we - ws - q + 1
            hit = np.ones((rows, starts), dtype=bool)
            for i, k in enumerate(kmer):                      # character i of the k-mer against every start at once
                hit &= _accepts(k, ref_wc, query_wc)[block[:, ws + i:ws + i + starts]]
            first = np.where(hit.any(axis=1), hit.argmax(axis=1) + ws + q - 1, none)
            best = np.minimum(best, first)
    best[best == none] = -1
    return best


def present_block(sets, block, ref_wc=False, query_wc=False):
    return first_hit_end_block(sets, block, ref_wc, query_wc) >= 0
