"""The device FASTQ stage (cutadapt_amd/csrc/fastq_gpu.hip) kernel by kernel, through the C ABI on tensors in HBM, at the
sizes the product runs at: every result is compared -- bytes and integers, exactly -- with the plain restatement in
tests/fastq_model.py (pinned on the CPU by tests/test_fastq_model.py), never with the library's own host code alone.
Every case that exists to reach a loop or a branch says so in a comment and asserts it on the input's own size.
The last three tests are end to end: rightmost adapters with every action and on read pairs, a non-ASCII adapter name
in the info file.  GPU only."""
import io
import random

import numpy as np
import pytest

import fastq_model as M

pytestmark = pytest.mark.gpu

NL_TILE_BYTES, SCAN_ELEMS = 16384, 2048              # fastq_gpu.hip
MAX_READ_LEN, MAX_NAME_SUFFIX = 1_000_000, 32         # cutadapt_hip.h
EINVAL = 1
CANARY = 0xA5


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _up(a, dtype=None):
    """numpy array (or None) -> tensor in HBM"""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).to("cuda:0") if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device="cuda:0")


def _p(t):
    return None if t is None else t.data_ptr()


def _host(t, n=None):
    a = t.cpu().numpy()
    return a if n is None else a[:n]


def _raw(data, offset=0):
    """the chunk in HBM, its first byte `offset` bytes behind a 16-byte boundary -> (tensor that owns it, pointer)"""
    import torch
    arr = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data
    hold = torch.empty(len(arr) + 32, dtype=torch.uint8, device="cuda:0")
    view = hold[offset:offset + len(arr)]
    view.copy_(torch.from_numpy(arr.copy()))
    assert view.data_ptr() % 16 == offset % 16
    return view, view.data_ptr()


def _scratch(L, nb, n):
    import torch
    need = int(L.cah_fastq_device_scratch_bytes(nb, n))
    return torch.empty(need, dtype=torch.uint8, device="cuda:0"), need


def _device_index(L, ptr, nb, n):
    """cah_fastq_count_lines_device + cah_fastq_index_device -> (line feeds, rec6, seq_off, seq_len, info[1])"""
    import torch
    from cutadapt_amd import _lib
    scratch, need = _scratch(L, nb, n)
    info = torch.full((8,), 7, dtype=torch.int64, device="cuda:0")
    _lib.check(L.cah_fastq_count_lines_device(ptr, nb, scratch.data_ptr(), need, info.data_ptr(), None))
    torch.cuda.synchronize()
    n_lf = int(info[0])
    rec6 = torch.full((max(n, 1), 6), -7, dtype=torch.int64, device="cuda:0")
    soff = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda:0")
    slen = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda:0")
    _lib.check(L.cah_fastq_index_device(ptr, nb, n_lf, n, scratch.data_ptr(), need, rec6.data_ptr(), soff.data_ptr(), slen.data_ptr(),
                                        info.data_ptr(), None))
    torch.cuda.synchronize()
    return n_lf, _host(rec6, n), _host(soff, n), _host(slen, n), int(info[1])


def _check_index(L, data, offsets=(0,), label=None):
    """the device's index of `data` equals the model's, from every base alignment in `offsets` -> the model's index"""
    want = M.index(data)
    n_lf, rec6, soff, slen, bad = want
    for off in offsets:
        hold, ptr = _raw(data, off)
        g_lf, g6, goff, glen, gbad = _device_index(L, ptr, len(data), len(rec6))
        assert g_lf == n_lf, (label, off, g_lf, n_lf)
        assert gbad == M.bad_word(bad), (label, off, gbad, bad)
        if bad is None:
            assert np.array_equal(g6, rec6), (label, off, np.flatnonzero((g6 != rec6).any(axis=1))[:5])
            assert np.array_equal(goff, soff) and np.array_equal(glen, slen), (label, off)
    return want


def _device_format(L, ptr, nb, rec6, beg, end, keep, flags=None, suffix=None, cap=0, chunk_bytes=None):
    """cah_fastq_format_device (suffix None) / cah_fastq_format_suffix_device into a buffer of `cap` bytes with 64 canary
    bytes behind it -> (info[3], the buffer with its canary)"""
    import torch
    from cutadapt_amd import _lib
    n = len(rec6)
    nb = nb if chunk_bytes is None else chunk_bytes
    scratch, need = _scratch(L, nb, n)
    info = torch.full((8,), 7, dtype=torch.int64, device="cuda:0")
    out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
    t6, tb, te, tk, tf = _up(rec6, np.int64), _up(beg, np.int32), _up(end, np.int32), _up(keep, np.uint8), _up(flags, np.uint8)
    if suffix is None:
        _lib.check(L.cah_fastq_format_device(ptr, _p(t6), n, _p(tb), _p(te), _p(tk), scratch.data_ptr(), need, nb, out.data_ptr(), cap,
                                             info.data_ptr(), None))
    else:
        _lib.check(L.cah_fastq_format_suffix_device(ptr, _p(t6), n, _p(tb), _p(te), _p(tk), _p(tf), suffix, len(suffix), scratch.data_ptr(),
                                                    need, nb, out.data_ptr(), cap, info.data_ptr(), None))
    torch.cuda.synchronize()
    return int(info[3]), _host(out)


def _check_format(L, data, rec6, beg, end, keep, flags=None, suffix=None, label=None, short=False):
    """formatted on the device with out_cap EXACTLY the total: the model's bytes, the canary untouched; short: again with
    out_cap one byte short -- the last kept record is left out, everything in front of it is there, the canary untouched"""
    want = np.frombuffer(M.fmt(data, rec6, beg, end, keep, flags, suffix or b""), dtype=np.uint8)
    hold, ptr = _raw(data)
    total, out = _device_format(L, ptr, len(data), rec6, beg, end, keep, flags, suffix, cap=len(want))
    assert total == len(want), (label, total, len(want))
    assert np.array_equal(out[:total], want), (label, int(np.flatnonzero(out[:total] != want)[0]))
    assert (out[total:] == CANARY).all(), label
    if short and total:
        kept = np.arange(len(rec6)) if keep is None else np.flatnonzero(keep)
        only = np.zeros(len(rec6), np.uint8)
        only[kept[-1]] = 1
        front = total - len(M.fmt(data, rec6, beg, end, only, flags, suffix or b""))
        total2, out = _device_format(L, ptr, len(data), rec6, beg, end, keep, flags, suffix, cap=total - 1)
        assert total2 == total, (label, total2)
        assert np.array_equal(out[:front], want[:front]) and (out[front:] == CANARY).all(), label
    return total


def _rec(name, seq, qual=None, plus=b"", eol=b"\n"):
    qual = b"I" * len(seq) if qual is None else qual
    return b"@" + name + eol + seq + eol + b"+" + plus + eol + qual + eol


def _letters(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


def _pool(rng, n, max_read=300, max_name=90, alphabet=b"ACGTNacgtn"):
    """pre-rendered records: reads of 0..max_read characters, names of 1..max_name bytes, qualities that may begin with
    '@' or '+', a tenth with a "+name" third line"""
    out = []
    for i in range(n):
        k = int(rng.integers(0, max_read + 1))
        name = (b"r%d " % i + _letters(rng, max_name, b"abcdefghij:/ 0123456789"))[:int(rng.integers(1, max_name + 1))]
        out.append(_rec(name, _letters(rng, k, alphabet), rng.integers(33, 75, k).astype(np.uint8).tobytes(),
                        plus=name if rng.random() < 0.1 else b""))
    return out


def _intervals(rng, lens, odd=0.1):
    """[beg, end) inside the reads and, for a share of them, outside: beg < 0, end > length, end < beg"""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    beg = (rng.random(n) * (lens + 1)).astype(np.int64)
    end = beg + (rng.random(n) * (lens - beg + 1)).astype(np.int64)
    out = rng.random(n) < odd
    beg = np.where(out, beg - rng.integers(0, 5, n), beg)
    end = np.where(out, end + rng.integers(-8, 8, n), end)
    return beg.astype(np.int32), end.astype(np.int32)


# ---- a. the indexer's small edges ---------------------------------------------------------------------------------------

def _edge_chunk(total, first_lf, tail):
    """A chunk of exactly `total` bytes: one record stretched (name and sequence) to fill it, its first line feed at byte
    `first_lf` (None: anywhere), then the odd records -- CRLF, an empty read, a bare '@', qualities that begin with '@' and
    with '+', a "+name" third line --; tail: the last line ends in "\\n", in nothing, or in "\\r" without a line feed.
    None if it does not fit."""
    if total < 6:
        return (b"@\n\n+\n\n")[:total]
    if total < 1000:
        odd = [_rec(b"", b"")]
        last = _rec(b"l", b"AC", b"+@")
    else:
        odd = [_rec(b"crlf rec", b"ACGT", b"IIII", eol=b"\r\n"), _rec(b"empty", b""), _rec(b"", b"AC", b"@+"),
               _rec(b"q", b"ACG", b"+@I"), _rec(b"plus", b"ACGTA", plus=b"plus"), _rec(b"both", b"AC", b"@!", plus=b"both", eol=b"\r\n")]
        last = _rec(b"last", b"GATTACA", b"@ABCDEF")
    last = {"lf": last, "none": last[:-1], "cr": last[:-1] + b"\r"}[tail]
    rest = b"".join(odd) + last
    room = total - len(rest) - 6                                  # what the stretched record's name, read and qualities share
    name_len = 3 if first_lf is None else first_lf - 1
    if room < name_len:
        return None
    seq_len, spare = divmod(room - name_len, 2)
    stretched = _rec(b"n" * name_len, b"ACGT" * (seq_len // 4) + b"ACGT"[:seq_len % 4], plus=b"x" * spare)
    data = stretched + rest
    assert len(data) == total and (first_lf is None or data.index(b"\n") == first_lf)
    return data


def test_indexer_small_edges(hip):
    """cah_fastq_count_lines_device + cah_fastq_index_device on chunks of 1 .. 32 769 bytes: the ends of a thread's 64-byte
    slice and of a 16 384-byte tile, every line ending, every odd record, from aligned and unaligned bases"""
    done = unaligned = 0
    for total in (1, 63, 64, 65, 16383, 16384, 16385, 32767, 32769):
        for first_lf in (None, 63, 64, 16383, 16384):             # (a line feed ON the last byte of a slice / tile and on the first of the next)
            for tail in ("lf", "none", "cr"):
                data = _edge_chunk(total, first_lf, tail)
                if data is None or (total < 6 and (first_lf is not None or tail != "lf")):
                    continue
                # load64's byte path from an unaligned base: the chunk again 1, 7 and 15 bytes behind a 16-byte boundary
                # (_raw asserts ptr % 16 == offset, i.e. (ptr % 16) != 0)
                offsets = (0, 1, 7, 15)
                n_lf, rec6, _, slen, bad = _check_index(hip, data, offsets, (total, first_lf, tail))
                assert bad is None and (total < 6 or len(rec6) >= 3)
                done += 1
                unaligned += len(offsets) - 1
    assert done >= 60 and unaligned >= 180, (done, unaligned)


# ---- b. long lines ------------------------------------------------------------------------------------------------------

def test_long_lines(hip):
    rng = np.random.default_rng(3)
    # a tile without a line feed: 40 000 characters between two reads of 10 -> whole tiles inside the read and inside
    # its qualities hold none
    recs = [_rec(b"short1", _letters(rng, 10)), _rec(b"long", _letters(rng, 40000), rng.integers(33, 75, 40000).astype(np.uint8).tobytes()),
            _rec(b"short2", _letters(rng, 10))]
    data = b"".join(recs)
    lf = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)
    assert np.diff(lf).max() >= 2 * NL_TILE_BYTES                 # (at least one whole tile between two line feeds)
    _, rec6, _, slen, _ = _check_index(hip, data, (0, 7))
    assert slen.tolist() == [10, 40000, 10]
    _check_format(hip, data, rec6, [0, 5, 3], [10, 39999, 7], None, short=True)
    # the longest read the library takes
    big = _rec(b"max", _letters(rng, MAX_READ_LEN), rng.integers(33, 75, MAX_READ_LEN).astype(np.uint8).tobytes())
    data = recs[0] + big + recs[2]
    _, rec6, _, slen, _ = _check_index(hip, data)
    assert slen.tolist() == [10, MAX_READ_LEN, 10]
    _check_format(hip, data, rec6, [0, 1, 0], [10, MAX_READ_LEN, 10], None)


# ---- c. the production shape ----------------------------------------------------------------------------------------------

def test_production_chunk(hip):
    """one chunk of max(8 x CUs, 1024) + 3 tiles of mixed records: indexed and formatted"""
    cus = _cus()
    rng = np.random.default_rng(4)
    pool = _pool(rng, 3000)
    lens = np.array([len(x) for x in pool])
    tiles = max(8 * cus, 1024) + 3
    pick = rng.integers(0, len(pool), tiles * NL_TILE_BYTES // int(lens.min() + 1) // 8)
    size = np.cumsum(lens[pick])
    pick = pick[:int(np.searchsorted(size, (tiles - 1) * NL_TILE_BYTES + 1)) + 1]
    data = b"".join([pool[i] for i in pick])
    n_tiles = -(-len(data) // NL_TILE_BYTES)
    # the second pass of k_tile_scan over tile counts (1024 per pass) and the grid-stride loops of k_nl_count / k_nl_write
    # (8 x CUs blocks)
    assert n_tiles > max(1024, 8 * cus), (n_tiles, cus)
    _, rec6, _, slen, bad = _check_index(hip, data)
    n = len(rec6)
    assert bad is None and n == len(pick)
    # the wave-stride loop of k_format (64 x CUs waves) and more than two scan blocks
    assert n > 64 * cus and n > 2 * SCAN_ELEMS, (n, cus)
    beg, end = _intervals(rng, slen)
    keep = (rng.random(n) < 0.8).astype(np.uint8)
    _check_format(hip, data, rec6, beg, end, keep)


# ---- d. the carry over block sums -------------------------------------------------------------------------------------------

def test_scan_block_sum_carry(hip):
    """1026 x 2048 records of the minimal form with real records spliced in: the only reachable shape that takes the
    one-block scan past 1024 block sums"""
    rng = np.random.default_rng(5)
    n_min = 1026 * SCAN_ELEMS
    real = _pool(rng, 300, max_read=120, max_name=70)
    at = np.sort(rng.integers(0, n_min, len(real)))
    parts, last = [], 0
    for k, pos in enumerate(at.tolist()):
        parts.append(b"@\n\n+\n\n" * (pos - last))
        parts.append(real[k])
        last = pos
    parts.append(b"@\n\n+\n\n" * (n_min - last))
    data = b"".join(parts)
    _, rec6, _, slen, bad = _check_index(hip, data)
    n = len(rec6)
    n_scan_blocks = -(-n // SCAN_ELEMS)
    # the second pass of k_tile_scan over the block sums of the output-length scan
    assert bad is None and n == n_min + len(real) and n_scan_blocks > 1024, (n, n_scan_blocks)
    beg, end = _intervals(rng, slen)
    keep = (rng.random(n) < 0.9).astype(np.uint8)
    keep[SCAN_ELEMS * 1024 - 3:SCAN_ELEMS * 1024 + 3] = 1       # (records either side of the 1024th block sum are written)
    _check_format(hip, data, rec6, beg, end, keep)


# ---- e. malformed input -------------------------------------------------------------------------------------------------------

def test_first_bad_record_and_its_code(hip):
    rng = np.random.default_rng(6)
    recs = _pool(rng, 3000, max_read=60, max_name=30)
    recs = [r if len(r.split(b"\n")[1]) else _rec(b"x", b"A") for r in recs]     # (every read has a character to lose)

    def broken(r, code):
        name, seq, plus, qual, _ = r.split(b"\n")
        if code == 1:
            return b"\n".join([b"X" + name[1:], seq, plus, qual, b""])
        if code == 2:
            return b"\n".join([name, seq, b"-" + plus[1:], qual, b""])
        return b"\n".join([name, seq, plus, qual[:-1], b""])

    good = b"".join(recs)
    assert _check_index(hip, good)[4] is None                     # a well-formed chunk leaves all bits of info[1] set
    for first in (1, 2, 3):
        # several bad records of different codes in different blocks of 256 records; the first one is of code `first`
        where = {700 + 10 * first: first, 1500: 1 + first % 3, 1800: 1 + (first + 1) % 3, 2900: first}
        data = b"".join(broken(r, where[i]) if i in where else r for i, r in enumerate(recs))
        bad = _check_index(hip, data, (0, 15))[4]
        assert bad == (700 + 10 * first, first), bad
    # the first record, the last record, and a bad record behind one with an empty name line
    for at, code in ((0, 3), (2999, 2), (2999, 1)):
        data = b"".join(broken(r, code) if i == at else r for i, r in enumerate(recs))
        assert _check_index(hip, data)[4] == (at, code)


# ---- f. the formatter's edges ---------------------------------------------------------------------------------------------------

def test_formatter_edges(hip):
    cus = _cus()
    rng = np.random.default_rng(7)
    names = (0, 1, 63, 64, 65, 200)                               # a name >= 64 bytes: the name loop's second stride
    bodies = (0, 1, 63, 64, 65, 129)
    pool = [_rec(_letters(rng, names[i % 6], b"abcdefgh:/ 0123456789"), _letters(rng, 140), rng.integers(33, 75, 140).astype(np.uint8).tobytes())
            for i in range(600)]
    counts = (1, SCAN_ELEMS - 1, SCAN_ELEMS, SCAN_ELEMS + 1, 64 * cus + 5)
    n_all = counts[-1]
    assert n_all > 64 * cus                                       # the wave-stride loop of k_format
    order = rng.integers(0, len(pool), n_all)
    data_all = [pool[i] for i in order]
    body = np.array(bodies)[rng.integers(0, 6, n_all)]
    beg = (rng.random(n_all) * (141 - body)).astype(np.int64)
    end = beg + body
    for k, (b, e) in enumerate(((-3, 50), (100, 500), (90, 20), (-7, 400), (140, 140), (0, 0))):     # beg < 0, end > len, end < beg
        beg[k::97], end[k::97] = b, e
    ran = 0
    for n in counts:
        data = b"".join(data_all[:n])
        rec6 = M.index(data)[1]
        assert len(rec6) == n and max(r[1] - r[0] for r in rec6[:6]) >= 64 or n == 1
        b, e = beg[:n].astype(np.int32), end[:n].astype(np.int32)
        first_out, last_out = np.ones(n, np.uint8), np.ones(n, np.uint8)
        first_out[0], last_out[-1] = 0, 0
        flags = (rng.random(n) < 0.5).astype(np.uint8)
        for keep, sfx in ((None, None), (np.zeros(n, np.uint8), b"/"), (first_out, b"s" * MAX_NAME_SUFFIX), (last_out, b""),
                          ((rng.random(n) < 0.7).astype(np.uint8), b" rc"), (None, b"y" * MAX_NAME_SUFFIX), (last_out, None)):
            _check_format(hip, data, rec6, b, e, keep, None if sfx is None else flags, sfx, label=(n, sfx), short=True)
            ran += 1
    assert ran == 35


# ---- g. info rows ----------------------------------------------------------------------------------------------------------------

def _device_info_rows(L, ptr, nb, rec6, out6, status, best, kinds, fbeg, fend, names, is_rc, suffix, cap):
    import torch
    from cutadapt_amd import _lib
    n, rounds = len(rec6), len(status)
    scratch, need = _scratch(L, nb, n)
    total = torch.full((1,), 7, dtype=torch.int64, device="cuda:0")
    out = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda:0")
    name_off = np.zeros(len(names) + 1, dtype=np.int32)
    np.cumsum([len(x) for x in names], out=name_off[1:])
    t = [_up(rec6, np.int64), _up(out6, np.int32), _up(status, np.uint8), _up(best, np.int32), _up(kinds, np.uint8), _up(fbeg, np.int32),
         _up(fend, np.int32), _up(np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)), _up(name_off), _up(is_rc, np.uint8)]
    _lib.check(L.cah_info_format_device(ptr, _p(t[0]), n, _p(t[1]), _p(t[2]), _p(t[3]), rounds, _p(t[4]), _p(t[5]), _p(t[6]),
                                        _p(t[7]) if names else None, _p(t[8]) if names else None, len(names), _p(t[9]), suffix or None,
                                        len(suffix or b""), scratch.data_ptr(), need, nb, out.data_ptr(), cap, total.data_ptr(), None))
    torch.cuda.synchronize()
    return int(total[0]), _host(out)


def test_info_rows(hip):
    cus = _cus()
    rng = np.random.default_rng(8)
    values = (0, 9, 10, 99, 100, 999, 1000, 9999, 10000)          # one .. five digits, either side of every power of ten
    big = [_rec(b"big%d " % j + b"n" * (60 + j), _letters(rng, 12000), rng.integers(33, 75, 12000).astype(np.uint8).tobytes())
           for j in range(18)]
    small = _pool(rng, 500, max_read=40, max_name=100)
    n = 64 * cus + 5
    # more records than one scan block and than the 64 x CUs waves of k_info_format (its wave-stride loop)
    assert n > SCAN_ELEMS and n > 64 * cus
    recs = big + [small[i] for i in rng.integers(0, len(small), n - len(big))]
    data = b"".join(recs)
    _, rec6, _, slen, bad = M.index(data)
    assert bad is None and len(rec6) == n
    assert (rec6[:, 1] - rec6[:, 0] >= 64).sum() > 100            # read names >= 64 bytes: the name loop's second stride
    lens = slen.astype(np.int64)
    names = [b"", b"a", b"x" * 70, "näme✓".encode("utf-8")]
    assert len(names[3]) > len(names[3].decode("utf-8"))          # (multi-byte UTF-8)
    kinds = np.array([0, 1, 2, 2], dtype=np.uint8)
    # small records: any round may be absent, coordinates inside the read and beyond what the earlier rounds left (the
    # clamps), adapter indices out of range
    status = (rng.random((3, n)) < 0.5).astype(np.uint8)
    status[:, ::11] = np.array([1, 0, 1], dtype=np.uint8)[:, None]            # three rounds, the middle one absent
    status[:, 5::13] = 2                                          # (an invalid read is not a match)
    out6 = np.zeros((3, n, 6), dtype=np.int32)
    out6[:, :, 2] = np.where(rng.random((3, n)) < 0.3, 0, rng.random((3, n)) * (lens + 3))          # kind 2 with rstart 0 and > 0
    out6[:, :, 3] = out6[:, :, 2] + rng.random((3, n)) * (lens + 1)
    out6[:, :, 5] = rng.integers(0, 4, (3, n))
    out6[:, :, 4] = rng.integers(0, 40, (3, n))
    best = rng.integers(-1, 6, (3, n)).astype(np.int32)
    for j in range(18):                                           # the long reads: five-digit coordinates
        status[:, j] = (1, 0, 1)
        v = values[j % 9]
        out6[0, j, 2], out6[0, j, 3], out6[0, j, 5] = (v, max(v, values[min(j % 9 + 1, 8)]), v) if j < 9 else (0, v, values[8 - j % 9])
        best[0, j] = j % 4 if j < 9 else 2
        out6[2, j, 2], out6[2, j, 3], out6[2, j, 5] = values[(j + 3) % 9], 11000, j
        best[2, j] = (j + 1) % 4
    assert out6[0, :18, 2:4].max() >= 10000                       # five-digit coordinates
    fbeg, fend = _intervals(rng, lens, odd=0.2)
    is_rc = (rng.random(n) < 0.5).astype(np.uint8)
    hold, ptr = _raw(data)
    ran = 0
    for kn, kk, rc, sfx in ((names, kinds, None, b""), (names, kinds, is_rc, b" rc"), (names, None, is_rc, b""),
                            ([], np.array([2], dtype=np.uint8), None, b""), (names[1:2], np.array([1], dtype=np.uint8), is_rc, b"s" * MAX_NAME_SUFFIX)):
        want = np.frombuffer(M.info_rows(data, rec6, out6, status, best, kk, fbeg, fend, kn, rc, sfx), dtype=np.uint8)
        total, out = _device_info_rows(hip, ptr, len(data), rec6, out6, status, best, kk, fbeg, fend, kn, rc, sfx, cap=len(want))
        assert total == len(want), (ran, total, len(want))
        assert np.array_equal(out[:total], want), (ran, int(np.flatnonzero(out[:total] != want)[0]))
        assert (out[total:] == CANARY).all(), ran
        # one byte short: the last row is left out, what is in front of it is there, the canary untouched
        front = int(np.flatnonzero(want[:-1] == 10)[-1]) + 1
        total2, out = _device_info_rows(hip, ptr, len(data), rec6, out6, status, best, kk, fbeg, fend, kn, rc, sfx, cap=len(want) - 1)
        assert total2 == total and np.array_equal(out[:front], want[:front]) and (out[front:] == CANARY).all(), ran
        ran += 1
    assert ran == 5


# ---- h. marking -----------------------------------------------------------------------------------------------------------------

def _seq_mask(nb, rec6):
    d = np.zeros(nb + 1, dtype=np.int64)
    np.add.at(d, rec6[:, 2], 1)
    np.add.at(d, rec6[:, 3], -1)
    return np.cumsum(d)[:nb] > 0


def test_marking(hip):
    import torch
    from cutadapt_amd import _lib
    cus = _cus()
    rng = np.random.default_rng(9)
    alphabet = b"@AZ[\\`az{0123456789ACGTNacgtn"                  # the edges of the case arithmetic
    n = 64 * cus + 5
    assert n > 64 * cus                                           # the wave-stride loop of k_mark_reads
    lens = np.where(np.arange(n) < 1200, np.array([0, 1, 63, 64, 65, 300])[np.arange(n) % 6], rng.integers(0, 13, n))
    recs = [_rec(b"r%d" % i, _letters(rng, int(k), alphabet), rng.integers(33, 75, int(k)).astype(np.uint8).tobytes()) for i, k in enumerate(lens)]
    data = b"".join(recs)
    _, rec6, _, slen, bad = M.index(data)
    assert bad is None and np.array_equal(slen, lens)
    beg, end = _intervals(rng, lens, odd=0.0)                     # windows inside the read
    # the mark before, inside, after, equal to and around the window, empty and turned round
    kind = np.arange(n) % 7
    inner_b = beg + (rng.random(n) * (end - beg + 1)).astype(np.int32)
    inner_e = inner_b + (rng.random(n) * (end - inner_b + 1)).astype(np.int32)
    mb = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [beg - 9, inner_b, end, beg, beg - 2, inner_b], inner_e)
    me = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [beg, inner_e, end + 9, end, end + 2, inner_b], inner_b)
    original = np.frombuffer(data, dtype=np.uint8)
    outside = ~_seq_mask(len(data), rec6)
    for mode in (1, 2):
        hold, ptr = _raw(data)
        t = [_up(rec6, np.int64), _up(beg, np.int32), _up(end, np.int32), _up(mb, np.int32), _up(me, np.int32)]
        _lib.check(hip.cah_mark_reads_device(ptr, _p(t[0]), n, _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), mode, None))
        torch.cuda.synchronize()
        got = _host(hold)
        want = M.mark(data, rec6, beg, end, mb, me, mode)
        assert np.array_equal(got, want), (mode, int(np.flatnonzero(got != want)[0]))
        assert np.array_equal(got[outside], original[outside])   # names and qualities of every record unchanged
        assert (got != original).sum() > 1000                     # (and something was marked)


# ---- i. reverse complement in place ---------------------------------------------------------------------------------------------

def test_revcomp_in_place(hip):
    import torch
    from cutadapt_amd import _lib
    cus = _cus()
    rng = np.random.default_rng(10)
    alphabet = b"ACGTUMKRYVBHDWSNacgtumkryvbhdwsn[{@0-*."          # every IUPAC letter in both cases, bytes without a complement
    n = 64 * cus + 5
    assert n > 64 * cus                                           # the wave-stride loop of k_revcomp_in_place
    windows = np.array([0, 1, 2, 63, 64, 65, 127, 128, 129, 1001])
    lens = np.where(np.arange(n) < 80, 1100, rng.integers(0, 20, n))
    recs = [_rec(b"r%d" % i, _letters(rng, int(k), alphabet), rng.integers(33, 75, int(k)).astype(np.uint8).tobytes()) for i, k in enumerate(lens)]
    data = b"".join(recs)
    _, rec6, _, slen, bad = M.index(data)
    assert bad is None and np.array_equal(slen, lens)
    win_len = np.where(np.arange(n) < 80, windows[np.arange(n) % 10], rng.integers(-2, 25, n)).astype(np.int32)
    # the window's start inside the read, negative and beyond it
    win_beg = np.where(np.arange(n) % 5 == 3, -4, np.where(np.arange(n) % 5 == 4, lens + 3, (rng.random(n) * (lens + 1)).astype(np.int64))).astype(np.int32)
    win_beg[:40] = rng.integers(0, 90, 40)                        # (the long reads: every window length whole, twice)
    flags = (rng.random(n) < 0.6).astype(np.uint8)
    flags[:40] = 1
    original = np.frombuffer(data, dtype=np.uint8)
    for wb in (None, win_beg):
        hold, ptr = _raw(data)
        t = [_up(rec6, np.int64), _up(wb, np.int32), _up(win_len, np.int32), _up(flags, np.uint8)]
        _lib.check(hip.cah_revcomp_in_place_device(ptr, _p(t[0]), n, _p(t[1]), _p(t[2]), _p(t[3]), None))
        torch.cuda.synchronize()
        got = _host(hold)
        want = M.revcomp_in_place(data, rec6, wb, win_len, flags)
        assert np.array_equal(got, want), (wb is None, int(np.flatnonzero(got != want)[0]))
        touched = np.zeros(len(data), dtype=bool)
        for r in np.flatnonzero(flags):
            touched[rec6[r, 2]:rec6[r, 3]] = True
            touched[rec6[r, 4]:rec6[r, 5]] = True
        assert np.array_equal(got[~touched], original[~touched])  # unflagged records, every name: untouched
        assert (got != original).sum() > 1000


# ---- j. decisions and filters ---------------------------------------------------------------------------------------------------

def test_decisions_and_filters(hip):
    import torch
    from cutadapt_amd import _lib
    cus = _cus()
    rng = np.random.default_rng(11)
    n = 1024 * cus + 77
    assert n > 1024 * cus                                         # the grid-stride loops of k_trim_decide / k_trim_filter (4 x CUs blocks of 256)
    lens = rng.integers(0, 200, n).astype(np.int32)
    status = rng.choice(np.array([0, 1, 2], dtype=np.uint8), n, p=[0.3, 0.6, 0.1])
    best = rng.integers(0, 3, n).astype(np.int32)
    best[status != 1] = -1
    kinds = np.array([0, 1, 2], dtype=np.uint8)                   # 3', 5', anywhere
    out6 = rng.integers(0, 50, (n, 6)).astype(np.int32)           # (rows of reads without a match: never looked at)
    out6[:, 2] = np.where(rng.random(n) < 0.3, 0, rng.random(n) * (lens + 1))                       # rstart = 0 and > 0
    out6[:, 3] = out6[:, 2] + rng.random(n) * (lens - out6[:, 2] + 1)
    win_beg = rng.integers(0, 10, n).astype(np.int32)
    full_len = (win_beg + lens + rng.integers(0, 10, n)).astype(np.int32)
    t6, tst, tbest, tlen, tkinds, twb, tfull = (_up(out6), _up(status), _up(best), _up(lens), _up(kinds), _up(win_beg), _up(full_len))
    d_beg = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_end = torch.empty(n, dtype=torch.int32, device="cuda:0")
    d_keep = torch.empty(n, dtype=torch.uint8, device="cuda:0")

    def compare(label, rc, want, counters):
        _lib.check(rc)
        torch.cuda.synchronize()
        wb, we, wk, wc = want
        if wb is not None:
            assert np.array_equal(_host(d_beg), wb) and np.array_equal(_host(d_end), we), label
        assert np.array_equal(_host(d_keep), wk), label
        assert _host(counters).tolist() == wc, (label, _host(counters).tolist(), wc)
        return wc

    # the three entries, every action x adapter kind, limits at the exact boundary and off, the discards, best NULL / given,
    # windows; every call goes TWICE into the same counters, which accumulate
    runs = 0
    for entry, action, bst, wbeg, full, lim, dt, du, only in (
            ("plain", 0, best, None, None, (40, 120), 0, 0, 0), ("plain", 0, None, None, None, (-1, -1), 1, 0, 0),
            ("plain", 0, best, None, None, (0, 0), 0, 1, 0),
            ("window", 0, best, win_beg, full_len, (40, -1), 0, 1, 0), ("window", 0, best, None, full_len, (-1, 120), 0, 0, 0),
            ("window", 0, best, win_beg, full_len, (40, 120), 1, 1, 1),
            ("action", 0, best, win_beg, full_len, (30, 100), 1, 1, 0), ("action", 1, best, None, full_len, (40, 120), 0, 1, 0),
            ("action", 2, best, win_beg, full_len, (40, 120), 0, 0, 0), ("action", 3, best, win_beg, full_len, (10, 30), 1, 0, 0),
            ("action", 2, None, win_beg, full_len, (-1, -1), 0, 0, 1), ("action", 3, best, None, full_len, (5, -1), 0, 0, 0)):
        counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        wc = None
        for _ in range(2):
            want = M.trim_decide(out6, status, bst, wbeg, lens, full, kinds, action, lim[0], lim[1], dt, du, only, wc)
            tb, tw = (tbest if bst is not None else None), (twb if wbeg is not None else None)
            if entry == "plain":
                rc = hip.cah_trim_decide_device(_p(t6), _p(tst), _p(tb), _p(tlen), n, _p(tkinds), lim[0], lim[1], dt, du, _p(d_beg), _p(d_end),
                                                _p(d_keep), _p(counters), None)
            elif entry == "window":
                rc = hip.cah_trim_decide_window_device(_p(t6), _p(tst), _p(tb), _p(tw), _p(tlen), _p(tfull), n, _p(tkinds), lim[0], lim[1], dt,
                                                       du, only, _p(d_beg), _p(d_end), _p(d_keep), _p(counters), None)
            else:
                rc = hip.cah_trim_decide_action_device(_p(t6), _p(tst), _p(tb), _p(tw), _p(tlen), _p(tfull), n, _p(tkinds), action, lim[0],
                                                       lim[1], dt, du, only, _p(d_beg), _p(d_end), _p(d_keep), _p(counters), None)
            wc = compare((entry, action, lim, dt, du, only), rc, want, counters)
        kept_len = (want[1] - want[0]).astype(np.int64)
        if not only:                                              # reads exactly at a limit (kept) and one beside it (counted)
            assert lim[0] < 0 or ((kept_len == lim[0]).any() and (kept_len == lim[0] - 1).any() or lim[0] == 0)
            assert lim[1] < 0 or ((kept_len == lim[1]).any() and (kept_len == lim[1] + 1).any())
        assert wc[0] == 2 * n and wc[6] == 2 * int((status == 2).sum())
        runs += 1
    assert runs == 12
    # the filters behind the modifiers: ee NULL, equal to max_ee (kept) and just above it (counted)
    fb, fe = want[0], want[1]
    tfb, tfe = _up(fb), _up(fe)
    ee = rng.random(n) * 4.0
    ee[::3] = 2.0
    ee[1::3] = np.nextafter(2.0, 3.0)
    tee = _up(ee)
    for e_arr, max_ee, lim, dt, du in ((None, 2.0, (20, 90), 0, 0), (ee, 2.0, (20, 90), 0, 0), (ee, 2.0, (-1, -1), 1, 0), (ee, -1.0, (20, -1), 0, 1),
                                       (ee, 2.0, (-1, 90), 1, 1)):
        counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
        wc = None
        for _ in range(2):
            wk, wc = M.trim_filter(fb, fe, status, e_arr, lim[0], lim[1], max_ee, dt, du, wc)
            rc = hip.cah_trim_filter_device(_p(tfb), _p(tfe), _p(tst), _p(tee) if e_arr is not None else None, n, lim[0], lim[1], max_ee, dt, du,
                                            _p(d_keep), _p(counters), None)
            compare(("filter", max_ee, lim, dt, du), rc, (None, None, wk, wc), counters)
        if e_arr is not None and max_ee >= 0:
            assert wc[7] > 0 and wc[7] < 2 * n
    kept_len = (fe - fb).astype(np.int64)
    assert (kept_len == 20).any() and (kept_len == 19).any() and (kept_len == 90).any() and (kept_len == 91).any()


# ---- k. argument errors ---------------------------------------------------------------------------------------------------------

def test_argument_errors_launch_nothing(hip):
    import torch
    L = hip
    data = b"".join(_pool(np.random.default_rng(12), 50))
    _, rec6, soff, slen, _ = M.index(data)
    n, nb = len(rec6), len(data)
    hold, ptr = _raw(data)
    scratch, need = _scratch(L, nb, n)
    info = torch.full((8,), 7, dtype=torch.int64, device="cuda:0")
    t6, tb, te = _up(rec6, np.int64), _up(np.zeros(n, np.int32)), _up(slen)
    g6 = torch.full((n, 6), -7, dtype=torch.int64, device="cuda:0")
    goff = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
    glen = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    out = torch.full((nb + 8 * n,), CANARY, dtype=torch.uint8, device="cuda:0")
    st, best, kinds = _up(np.ones(n, np.uint8)), _up(np.zeros(n, np.int32)), _up(np.zeros(1, np.uint8))
    o6 = _up(np.zeros((n, 6), np.int32))
    keep = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    counters = torch.zeros(8, dtype=torch.int64, device="cuda:0")
    nm, noff = _up(np.frombuffer(b"ab", dtype=np.uint8)), _up(np.array([0, 2], np.int32))
    sp, op, ip = scratch.data_ptr(), out.data_ptr(), info.data_ptr()
    need0 = int(L.cah_fastq_device_scratch_bytes(nb, 0))
    calls = [
        # scratch one byte too small
        L.cah_fastq_count_lines_device(ptr, nb, sp, need0 - 1, ip, None),
        L.cah_fastq_index_device(ptr, nb, 4 * n, n, sp, need - 1, _p(g6), _p(goff), _p(glen), ip, None),
        L.cah_fastq_format_device(ptr, _p(t6), n, _p(tb), _p(te), None, sp, need - 1, nb, op, out.numel(), ip, None),
        L.cah_fastq_format_suffix_device(ptr, _p(t6), n, _p(tb), _p(te), None, _p(st), b" rc", 3, sp, need - 1, nb, op, out.numel(), ip, None),
        L.cah_info_format_device(ptr, _p(t6), n, _p(o6), _p(st), _p(best), 1, None, _p(tb), _p(te), _p(nm), _p(noff), 1, None, None, 0, sp,
                                 need - 1, nb, op, out.numel(), ip, None),
        # negative counts
        L.cah_fastq_count_lines_device(ptr, -1, sp, need, ip, None),
        L.cah_fastq_index_device(ptr, nb, 4 * n, -1, sp, need, _p(g6), _p(goff), _p(glen), ip, None),
        L.cah_fastq_index_device(ptr, nb, -1, n, sp, need, _p(g6), _p(goff), _p(glen), ip, None),
        L.cah_fastq_format_device(ptr, _p(t6), -1, _p(tb), _p(te), None, sp, need, nb, op, out.numel(), ip, None),
        L.cah_info_format_device(ptr, _p(t6), -1, _p(o6), _p(st), _p(best), 1, None, _p(tb), _p(te), _p(nm), _p(noff), 1, None, None, 0, sp,
                                 need, nb, op, out.numel(), ip, None),
        L.cah_info_format_device(ptr, _p(t6), n, _p(o6), _p(st), _p(best), 1, None, _p(tb), _p(te), _p(nm), _p(noff), -1, None, None, 0, sp,
                                 need, nb, op, out.numel(), ip, None),
        L.cah_mark_reads_device(ptr, _p(t6), -1, _p(tb), _p(te), _p(tb), _p(te), 1, None),
        L.cah_mark_reads_device(ptr, _p(t6), n, _p(tb), _p(te), _p(tb), _p(te), 3, None),
        L.cah_revcomp_in_place_device(ptr, _p(t6), -1, None, _p(te), _p(st), None),
        L.cah_trim_decide_device(_p(o6), _p(st), None, _p(te), -1, _p(kinds), -1, -1, 0, 0, _p(tb), _p(te), _p(keep), _p(counters), None),
        L.cah_trim_decide_action_device(_p(o6), _p(st), None, None, _p(te), _p(te), n, _p(kinds), 4, -1, -1, 0, 0, 0, _p(tb), _p(te), _p(keep),
                                        _p(counters), None),
        L.cah_trim_filter_device(_p(tb), _p(te), _p(st), None, -1, -1, -1, -1.0, 0, 0, _p(keep), _p(counters), None),
        # NULL outputs (and inputs)
        L.cah_fastq_count_lines_device(ptr, nb, sp, need, None, None),
        L.cah_fastq_index_device(ptr, nb, 4 * n, n, sp, need, None, _p(goff), _p(glen), ip, None),
        L.cah_fastq_index_device(ptr, nb, 4 * n, n, sp, need, _p(g6), _p(goff), None, ip, None),
        L.cah_fastq_format_device(ptr, _p(t6), n, _p(tb), _p(te), None, sp, need, nb, None, out.numel(), ip, None),
        L.cah_fastq_format_device(ptr, _p(t6), n, _p(tb), _p(te), None, None, need, nb, op, out.numel(), ip, None),
        L.cah_info_format_device(ptr, _p(t6), n, _p(o6), _p(st), _p(best), 1, None, _p(tb), _p(te), _p(nm), _p(noff), 1, None, None, 0, sp,
                                 need, nb, None, out.numel(), ip, None),
        L.cah_info_format_device(ptr, _p(t6), n, _p(o6), _p(st), _p(best), 1, None, _p(tb), _p(te), _p(nm), _p(noff), 1, None, None, 0, sp,
                                 need, nb, op, out.numel(), None, None),
        L.cah_mark_reads_device(None, _p(t6), n, _p(tb), _p(te), _p(tb), _p(te), 1, None),
        L.cah_mark_reads_device(ptr, _p(t6), n, _p(tb), _p(te), None, _p(te), 2, None),
        L.cah_revcomp_in_place_device(None, _p(t6), n, None, _p(te), _p(st), None),
        L.cah_trim_decide_device(_p(o6), _p(st), None, _p(te), n, _p(kinds), -1, -1, 0, 0, None, _p(te), _p(keep), _p(counters), None),
        L.cah_trim_decide_window_device(_p(o6), _p(st), None, None, _p(te), _p(te), n, _p(kinds), -1, -1, 0, 0, 0, _p(tb), _p(te), None,
                                        _p(counters), None),
        L.cah_trim_decide_action_device(_p(o6), _p(st), None, None, _p(te), _p(te), n, _p(kinds), 0, -1, -1, 0, 0, 0, _p(tb), _p(te), _p(keep),
                                        None, None),
        L.cah_trim_filter_device(_p(tb), _p(te), _p(st), None, n, -1, -1, -1.0, 0, 0, None, _p(counters), None),
    ]
    torch.cuda.synchronize()
    assert calls == [EINVAL] * len(calls), calls
    # nothing was launched: no output changed, the chunk is as it was
    assert (_host(g6) == -7).all() and (_host(goff) == -7).all() and (_host(glen) == -7).all()
    assert (_host(out) == CANARY).all() and (_host(keep) == 9).all() and (_host(counters) == 0).all()
    assert np.array_equal(_host(tb), np.zeros(n, np.int32)) and np.array_equal(_host(te), slen)
    assert _host(hold).tobytes() == data
    # ... and the same arguments put right do run
    assert _check_index(L, data)[4] is None


# ---- end to end: rightmost adapters with every action and on read pairs, a non-ASCII adapter name ---------------------------------

AD = ["AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", "TGGAATTCTCGGGTGCCAAGG", "ACGTACGTTT"]


def test_rightmost_adapters_with_every_action_equal_the_host_pipeline(hip):
    from cutadapt_amd import adapters as A
    from cutadapt_amd import gpu_pipeline as G
    from cutadapt_amd.pipeline import trim_fastq
    from test_gpu_fastq_device import _fastq
    rng = random.Random(31)
    sets = [lambda: [A.RightmostBackAdapter(AD[0])], lambda: [A.RightmostFrontAdapter(AD[1])],
            lambda: [A.RightmostFrontAdapter(AD[2]), A.RightmostBackAdapter(AD[1])]]
    ran = 0
    for action in ("retain", "crop", "mask", "lowercase"):
        for k, make in enumerate(sets):
            data = _fastq(rng, 1000, AD, crlf=bool(k % 2), lower=action == "lowercase", twice=True)
            ads = make()
            want = io.BytesIO()
            ws = trim_fastq(io.BytesIO(data), want, ads, index=False, action=action, minimum_length=5)
            # (what gpu_pipeline's eligibility says today: rightmost adapters among themselves are served on the device)
            way = "all-device" if G._all_device_adapters(ads, 1, False) else "general"
            for chunk in (4096, 1 << 20):
                got = io.BytesIO()
                gs = G.trim_fastq_gpu(np.frombuffer(data, dtype=np.uint8), got, ads, chunk_bytes=chunk, threads=2, assemble="device",
                                      index=False, action=action, minimum_length=5)
                assert gs["way"] == way, (action, k, gs["way"])
                assert got.getvalue() == want.getvalue(), (action, k, chunk)
                assert (gs["reads"], gs["with_adapters"], gs["bp_in"], gs["bp_out"]) == \
                       (ws["reads"], ws["with_adapters"], ws["bp_in"], ws["bp_out"]), (action, k)
            assert ws["with_adapters"] > 100
            ran += 1
    assert ran == 12


def test_rightmost_adapters_on_both_mates_equal_the_host_paired_driver(hip):
    from cutadapt_amd import adapters as A
    from cutadapt_amd import gpu_pipeline as G
    from cutadapt_amd.pipeline import trim_fastq_paired
    from test_gpu_fastq_device import _fastq
    rng = random.Random(32)
    n = 1000
    f1 = _fastq(rng, n, AD[:1], twice=True)
    f2 = _fastq(rng, n, AD[1:2], twice=True).replace(b"@read", b"@mate")
    for ci, (r1, r2, top) in enumerate((
            (dict(adapters=[A.RightmostBackAdapter(AD[0])]), dict(adapters=[A.RightmostBackAdapter(AD[1])]), dict(minimum_length=20)),
            (dict(adapters=[A.RightmostFrontAdapter(AD[0][:15]), A.RightmostBackAdapter(AD[0])], times=2, quality_cutoff=(0, 20)),
             dict(adapters=[A.RightmostFrontAdapter(AD[1][:12])], cut=[2]), dict(minimum_length=(15, 10), pair_filter="both")))):
        w1, w2 = io.BytesIO(), io.BytesIO()
        ws = trim_fastq_paired(io.BytesIO(f1), io.BytesIO(f2), w1, w2, dict(r1), dict(r2), **top)
        way = "all-device" if (G._mate_all_device(dict(r1)) is not None and G._mate_all_device(dict(r2)) is not None) else "general"
        for chunk in (4096, 1 << 20):
            g1, g2 = io.BytesIO(), io.BytesIO()
            gs = G.trim_fastq_gpu_paired(io.BytesIO(f1), io.BytesIO(f2), g1, g2, dict(r1), dict(r2), chunk_bytes=chunk, threads=2, **top)
            assert gs["way"] == way, (ci, gs["way"], way)
            assert g1.getvalue() == w1.getvalue() and g2.getvalue() == w2.getvalue(), (ci, chunk)
            assert (gs["pairs"], gs["pairs_written"]) == (ws["pairs"], ws["pairs_written"]), ci
            assert gs["with_adapters"] == ws["with_adapters"], ci
        assert np.min(ws["with_adapters"]) > 100, ws["with_adapters"]


def test_info_file_with_a_non_ascii_adapter_name(hip):
    """-a näme=SEQ --info-file on the all-device way: the adapters' names go to the device as UTF-8, their offsets in bytes"""
    from cutadapt_amd import adapters as A
    from cutadapt_amd.gpu_pipeline import trim_fastq_gpu
    from cutadapt_amd.pipeline import trim_fastq
    from test_gpu_fastq_device import _fastq
    data = _fastq(random.Random(33), 1000, AD)
    ads = [A.BackAdapter(AD[0], name="näme"), A.FrontAdapter(AD[1], name="plain"), A.BackAdapter(AD[2], name="✓")]
    want, want_info = io.BytesIO(), io.BytesIO()
    trim_fastq(io.BytesIO(data), want, ads, index=False, info_file=want_info)
    assert want_info.getvalue().count("näme".encode("utf-8")) > 100 and want_info.getvalue().count("✓".encode("utf-8")) > 10
    for chunk in (4096, 1 << 20):
        got, got_info = io.BytesIO(), io.BytesIO()
        gs = trim_fastq_gpu(np.frombuffer(data, dtype=np.uint8), got, ads, chunk_bytes=chunk, threads=2, assemble="device", index=False,
                            info_file=got_info)
        assert gs["way"] == "all-device", gs["way"]
        assert got.getvalue() == want.getvalue(), chunk
        assert got_info.getvalue() == want_info.getvalue(), chunk
