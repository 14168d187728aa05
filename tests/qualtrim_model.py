"""The per-read trimming scans in plain Python, written from the reference's own lines (qualtrim.pyx:22-70, :73-113,
:116-165, expected_errors.h:103-140, adapters.py:1222-1224) and from nothing else: integers, `float`, one loop per scan, no
chunks.  tests/test_qualtrim_model.py pins it on the CPU; tests/test_gpu_qualtrim_kernels.py compares the kernels of
cutadapt_amd/csrc/qualtrim.hip with it exactly.

Every scan also says how many characters it examined from each end (the character it stopped on included) and whether
it stopped early, as a pair (examined, stopped).  The tests use that to show WHERE a case leaves a loop, never to compute
what they expect."""

MATCH, INVALID = 1, 2                                 # cutadapt_hip.h: CAH_MATCH, CAH_INVALID


def _char(b):
    """a byte as C's signed `char`"""
    return b - 256 if b >= 128 else b


def quality_trim(q, cutoff_front, cutoff_back, base=33):
    """quality_trim_index -> ((start, stop), (examined, stopped) of the 5' scan, (examined, stopped) of the 3' scan)"""
    n = len(q)
    start, stop = 0, n
    s = max_qual = 0
    seen_front, left_front = 0, False
    for i in range(n):
        seen_front += 1
        s += cutoff_front - (_char(q[i]) - base)
        if s < 0:
            left_front = True
            break
        if s > max_qual:
            max_qual = s
            start = i + 1
    s = max_qual = 0
    seen_back, left_back = 0, False
    for i in reversed(range(n)):
        seen_back += 1
        s += cutoff_back - (_char(q[i]) - base)
        if s < 0:
            left_back = True
            break
        if s > max_qual:
            max_qual = s
            stop = i
    if start >= stop:
        start, stop = 0, 0
    return (start, stop), (seen_front, left_front), (seen_back, left_back)


def nextseq_trim(seq, q, cutoff, base=33):
    """nextseq_trim_index -> (stop, (examined, stopped) of the scan from the 3' end)"""
    assert len(seq) == len(q)
    s = max_qual = 0
    max_i = len(q)
    seen, left = 0, False
    for i in reversed(range(len(q))):
        seen += 1
        v = _char(q[i]) - base
        if seq[i] == 0x47:                             # 'G', upper case only
            v = cutoff - 1
        s += cutoff - v
        if s < 0:
            left = True
            break
        if s > max_qual:
            max_qual = s
            max_i = i
    return max_i, (seen, left)


def poly_a_trim(seq, revcomp=False):
    """poly_a_trim_index -> (index, (examined, stopped)): there is no early exit, the whole read is looked at"""
    n = len(seq)
    best_score = score = errors = 0
    if revcomp:
        best_index = 0
        for i in range(n):
            if seq[i] == 0x54:                         # 'T'
                score += 1
            else:
                score -= 2
                errors += 1
            if score > best_score and errors * 5 <= i + 1:
                best_score = score
                best_index = i + 1
        if best_index < 3:
            best_index = 0
    else:
        best_index = n
        for i in reversed(range(n)):
            if seq[i] == 0x41:                         # 'A'
                score += 1
            else:
                score -= 2
                errors += 1
            if score > best_score and errors * 5 <= n - i:
                best_score = score
                best_index = i
        if best_index > n - 3:
            best_index = n
    return best_index, (n, False)


def expected_errors(q, base, table):
    """expected_errors_from_phreds -> ((value, ok), (examined, stopped)); base 33 .. 126, table: the 94 doubles.
    Four accumulators over the groups of four, the last 1 .. 3 characters into accumulator 0, e0 + e1 + e2 + e3 last."""
    assert 33 <= base <= 126 and len(table) == 94
    n = len(q)
    max_phred = 126 - base
    e = [0.0, 0.0, 0.0, 0.0]
    cursor = 0
    while cursor < n - 3:
        phreds = [(q[cursor + k] - base) & 0xFF for k in range(4)]
        if any(p > max_phred for p in phreds):
            return (-1.0, False), (cursor + 4, True)
        for k in range(4):
            e[k] += table[phreds[k]]
        cursor += 4
    while cursor < n:
        p = (q[cursor] - base) & 0xFF
        if p > max_phred:
            return (-1.0, False), (cursor + 1, True)
        e[0] += table[p]
        cursor += 1
    return (e[0] + e[1] + e[2] + e[3], True), (n, False)


def linked_views(out6, status, offs, lens, read_len):
    """where the 3' stage of a linked adapter looks: read[stop:], stop = query_stop (out6[r][3]) of a front MATCH, else 0,
    clamped into [0, n] -> (starts, view lengths).  read_len > 0: equally long reads back to back from byte 0; else
    offs[r], and lens[r] or -- lens None -- offs[r + 1] - offs[r]."""
    starts, view_lens = [], []
    for r in range(len(status)):
        if read_len > 0:
            off, n = r * read_len, read_len
        else:
            off = offs[r]
            n = lens[r] if lens is not None else offs[r + 1] - offs[r]
        stop = out6[r][3] if status[r] == MATCH else 0
        stop = min(max(stop, 0), n)
        starts.append(off + stop)
        view_lens.append(n - stop)
    return starts, view_lens


def ascii_bad_reads(reads):
    """cah_validate_ascii_batch: how many READS hold a byte >= 0x80"""
    return sum(1 for r in reads if any(b >= 0x80 for b in r))
