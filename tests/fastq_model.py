"""A plain restatement of the device FASTQ stage (include/cutadapt_hip.h, "the same formats ON THE DEVICE"): one short
function per C-ABI entry, written from the header's comments and the reference lines they cite (modifiers.py:170-198,
:280-297; steps.py:232-253; adapters.py:446-487, :931; cli.py:735-912).  Pure Python + numpy; nothing is imported from
cutadapt_amd or from the oracle, so that a GPU test compares a kernel with something that shares no code with it.
tests/test_fastq_model.py pins these functions to the host twins of fastq.cpp and to the reference's golden files."""
import numpy as np

_COMPLEMENT = bytes.maketrans(b"ACGTUMKRYVBHDacgtumkryvbhd", b"TGCAAKMYRBVDHtgcaakmyrbvdh")    # W, S, N and the rest stay


def _u8(buf):
    return np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8)


def index(buf):
    """cah_fastq_count_lines_device + cah_fastq_index_device -> (n_linefeeds, rec6 int64[n, 6], seq_off int64[n],
    seq_len int32[n], bad): four lines are one record, a last line without line feed counts, "\\r\\n" ends a line like
    "\\n"; bad = (first bad record, code) or None -- 1: no '@', 2: no '+', 3: sequence and quality lengths differ."""
    buf = _u8(buf)
    nl = np.flatnonzero(buf == 10).astype(np.int64)
    n_lines = len(nl) + (1 if len(buf) and buf[-1] != 10 else 0)
    n = n_lines // 4
    ls = np.concatenate((np.zeros(1, np.int64), nl + 1))[:4 * n]
    le = np.concatenate((nl, np.full(1, len(buf), np.int64)))[:4 * n]
    if n:
        le = le - ((le > ls) & (buf[np.maximum(le - 1, 0)] == 13))
    first = np.where(le > ls, buf[np.minimum(ls, len(buf) - 1)], 0) if n else np.zeros(0, np.uint8)
    ls, le, first = ls.reshape(n, 4), le.reshape(n, 4), first.reshape(n, 4)
    rec6 = np.stack((ls[:, 0] + 1, le[:, 0], ls[:, 1], le[:, 1], ls[:, 3], le[:, 3]), axis=1)
    code = np.where(first[:, 0] != ord("@"), 1, np.where(first[:, 2] != ord("+"), 2,
                    np.where(le[:, 1] - ls[:, 1] != le[:, 3] - ls[:, 3], 3, 0)))
    wrong = np.flatnonzero(code)
    bad = (int(wrong[0]), int(code[wrong[0]])) if len(wrong) else None
    return len(nl), rec6, ls[:, 1].copy(), (le[:, 1] - ls[:, 1]).astype(np.int32), bad


def bad_word(bad):
    """d_info[1] as cah_fastq_index_device leaves it: (first bad record + 1) << 8 | code, all bits set if there is none"""
    return -1 if bad is None else ((bad[0] + 1) << 8) | bad[1]


def _cut(beg, end, length):
    """[beg, end) cut to a read of `length` characters: beg < 0 -> 0, end > length -> length, end < beg -> empty"""
    a = np.maximum(np.asarray(beg, dtype=np.int64), 0)
    b = np.minimum(np.asarray(end, dtype=np.int64), length)
    return a, np.maximum(b, a)


def _gather(src, starts, lens):
    """the pieces src[starts[i] : starts[i] + lens[i]] back to back"""
    starts, lens = np.asarray(starts, np.int64).ravel(), np.asarray(lens, np.int64).ravel()
    off = np.cumsum(lens) - lens
    return src[np.repeat(starts - off, lens) + np.arange(int(lens.sum()), dtype=np.int64)]


def fmt(buf, rec6, beg, end, keep=None, flags=None, suffix=b""):
    """cah_fastq_format_device / cah_fastq_format_suffix_device: "@name[suffix]\\nSEQ[beg:end]\\n+\\nQUAL[beg:end]\\n" of every
    record with keep[r] != 0 (keep None: all) in record order; the suffix goes behind the names of records with flags[r] != 0"""
    buf, rec6 = _u8(buf), np.asarray(rec6, dtype=np.int64).reshape(-1, 6)
    n = len(rec6)
    sel = np.arange(n) if keep is None else np.flatnonzero(np.asarray(keep)[:n])
    r = rec6[sel]
    a, b = _cut(np.asarray(beg)[sel], np.asarray(end)[sel], r[:, 3] - r[:, 2])
    src = np.concatenate((buf, _u8(b"@\n+\n" + suffix)))
    c = len(buf)                                                              # where the constants start
    one = np.ones(len(sel), np.int64)
    sfx = len(suffix) * (np.asarray(flags)[sel] != 0) if (flags is not None and len(suffix)) else 0 * one
    starts = np.stack((c * one, r[:, 0], (c + 4) * one, (c + 1) * one, r[:, 2] + a, (c + 1) * one, r[:, 4] + a, (c + 1) * one), axis=1)
    lens = np.stack((one, r[:, 1] - r[:, 0], sfx, one, b - a, 3 * one, b - a, one), axis=1)
    return _gather(src, starts, lens).tobytes()


def info_rows(buf, rec6, out6, status, best, kinds, final_beg, final_end, names, is_rc=None, suffix=b""):
    """cah_info_format_device.  out6 int[rounds, n, 6], status / best [rounds, n]; kinds per adapter (None: all 3');
    names: the adapters' names as bytes.  Per read (steps.py:232-253): one row per round that matched, cut from the read
    as that round saw it -- each match trims it for the next (adapters.py:453-454, :486-487, :931) --, or the "-1" row."""
    data, rec6 = _u8(buf).tobytes(), np.asarray(rec6).reshape(-1, 6)
    n = len(rec6)
    out6, status, best = np.asarray(out6).reshape(-1, n, 6), np.asarray(status).reshape(-1, n), np.asarray(best).reshape(-1, n)
    lines = []
    for r in range(n):
        nb, ne, sb, se, qb, qe = (int(x) for x in rec6[r])
        name, seq, qual = data[nb:ne], data[sb:se], data[qb:qe]
        shown = name + (suffix if (is_rc is not None and is_rc[r]) else b"")
        rc = b"" if is_rc is None else (b"1" if is_rc[r] else b"0")
        matched = False
        for k in range(len(status)):
            if status[k, r] != 1:
                continue
            matched = True
            rstart, rstop, errors = int(out6[k, r, 2]), int(out6[k, r, 3]), int(out6[k, r, 5])
            re = min(max(rstop, 0), len(seq))
            rs = min(max(rstart, 0), re)
            ad = int(best[k, r]) if 0 <= int(best[k, r]) < len(names) else 0
            kind = 0 if kinds is None else int(kinds[ad])
            lines.append(b"\t".join([shown, b"%d" % errors, b"%d" % rs, b"%d" % re, seq[:rs], seq[rs:re], seq[re:],
                                     names[ad] if names else b"", qual[:rs], qual[rs:re], qual[re:], rc]) + b"\n")
            if kind == 1 or (kind == 2 and rstart == 0):
                seq, qual = seq[re:], qual[re:]                               # a 5' match keeps what follows it
            else:
                seq, qual = seq[:rs], qual[:rs]                               # a 3' match keeps what is in front
        if not matched:
            a, b = _cut(int(final_beg[r]), int(final_end[r]), len(seq))
            lines.append(b"\t".join([name, b"-1", seq[a:b], qual[a:b]]) + b"\n")
    return b"".join(lines)


def mark(buf, rec6, beg, end, mark_beg, mark_end, mode):
    """cah_mark_reads_device -> the changed chunk: of the characters [beg, end) of every read those outside [mark_beg,
    mark_end) become 'N' (mode 1) or lower case with the ones inside in upper case (mode 2) -- modifiers.py:170-198"""
    out = bytearray(_u8(buf).tobytes())
    for r, (nb, ne, sb, se, qb, qe) in enumerate(np.asarray(rec6).reshape(-1, 6).tolist()):
        a = max(int(beg[r]), 0)
        b = max(min(int(end[r]), se - sb), a)
        lo = min(max(int(mark_beg[r]), a), b)                                 # [lo, hi): the part of [a, b) inside the mark
        hi = min(max(int(mark_end[r]), lo), b)
        s = bytes(out[sb + a:sb + b])
        head, mid, tail = s[:lo - a], s[lo - a:hi - a], s[hi - a:]
        out[sb + a:sb + b] = (b"N" * len(head) + mid + b"N" * len(tail)) if mode == 1 else head.lower() + mid.upper() + tail.lower()
    return np.frombuffer(bytes(out), dtype=np.uint8)


def revcomp_in_place(buf, rec6, win_beg, win_len, flags):
    """cah_revcomp_in_place_device -> the changed chunk: inside its window every flagged read becomes its reverse
    complement (IUPAC codes, both cases; other bytes stay) and its qualities are reversed -- modifiers.py:280-297"""
    out = bytearray(_u8(buf).tobytes())
    for r, (nb, ne, sb, se, qb, qe) in enumerate(np.asarray(rec6).reshape(-1, 6).tolist()):
        if not flags[r]:
            continue
        a = min(max(0 if win_beg is None else int(win_beg[r]), 0), se - sb)
        n = max(min(int(win_len[r]), se - sb - a), 0)
        out[sb + a:sb + a + n] = bytes(out[sb + a:sb + a + n])[::-1].translate(_COMPLEMENT)
        out[qb + a:qb + a + n] = bytes(out[qb + a:qb + a + n])[::-1]
    return np.frombuffer(bytes(out), dtype=np.uint8)


def _filters(length, found, ee, min_len, max_len, max_ee, discard_trimmed, discard_untrimmed, counters):
    """the filters in the reference's order (cli.py:735-912), each counted on what the earlier ones left -> keep"""
    short = (length < min_len) if min_len >= 0 else np.zeros(len(length), bool)
    long_ = ~short & ((length > max_len) if max_len >= 0 else False)
    many = ~short & ~long_ & ((np.asarray(ee) > max_ee) if (ee is not None and max_ee >= 0) else False)
    keep = ~short & ~long_ & ~many
    if discard_trimmed:
        keep &= ~found
    elif discard_untrimmed:
        keep &= found
    counters[3] += int(length[keep].sum())
    counters[4] += int(short.sum())
    counters[5] += int(np.sum(long_))
    counters[7] += int(np.sum(many))
    return keep


def trim_decide(out6, status, best, win_beg, win_len, full_len, kinds, action=0, min_len=-1, max_len=-1,
                discard_trimmed=0, discard_untrimmed=0, intervals_only=0, counters=None):
    """cah_trim_decide_device (win_beg None, full_len None, win_len = the reads' lengths), _window_ (action 0) and
    _action_ -> (beg, end, keep, counters[8]); action 0 trim, 1 none, 2 retain, 3 crop (adapters.py:446-487).  counters:
    reads, with adapters, bp in, bp out, too short, too long, invalid reads, too many expected errors; accumulated."""
    out6, status = np.asarray(out6).reshape(-1, 6).astype(np.int64), np.asarray(status)
    wlen = np.asarray(win_len).astype(np.int64)
    counters = [0] * 8 if counters is None else list(counters)
    found = status == 1
    ad = np.zeros(len(status), np.int64) if best is None else np.maximum(np.asarray(best).astype(np.int64), 0)
    kind = np.asarray(kinds)[ad]
    rstart, rstop = out6[:, 2], out6[:, 3]
    before = (kind == 1) | ((kind == 2) & (rstart == 0))                      # 5': the read keeps what follows the match
    b, e = np.zeros(len(status), np.int64), wlen.copy()
    if action == 0:
        b, e = np.where(found & before, rstop, b), np.where(found & ~before, rstart, e)
    elif action == 2:
        b, e = np.where(found & before, rstart, b), np.where(found & ~before, rstop, e)
    elif action == 3:
        b, e = np.where(found, rstart, b), np.where(found, rstop, e)
    counters[0] += len(status)
    counters[1] += int(found.sum())
    counters[2] += int(np.asarray(wlen if full_len is None else full_len).astype(np.int64).sum())
    counters[6] += int((status == 2).sum())
    if intervals_only:
        keep = np.ones(len(status), bool)
    else:
        keep = _filters(e - b, found, None, min_len, max_len, -1.0, discard_trimmed, discard_untrimmed, counters)
    w0 = 0 if win_beg is None else np.asarray(win_beg).astype(np.int64)
    return (w0 + b).astype(np.int32), (w0 + e).astype(np.int32), keep.astype(np.uint8), counters


def trim_filter(beg, end, status, ee, min_len=-1, max_len=-1, max_ee=-1.0, discard_trimmed=0, discard_untrimmed=0,
                counters=None):
    """cah_trim_filter_device -> (keep, counters[8]): [3] bp out, [4] too short, [5] too long, [7] too many expected errors"""
    counters = [0] * 8 if counters is None else list(counters)
    length = np.asarray(end).astype(np.int64) - np.asarray(beg).astype(np.int64)
    keep = _filters(length, np.asarray(status) == 1, ee, min_len, max_len, max_ee, discard_trimmed, discard_untrimmed, counters)
    return keep.astype(np.uint8), counters
