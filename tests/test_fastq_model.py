"""tests/fastq_model.py -- the plain restatement the device FASTQ kernels are compared with
(tests/test_gpu_fastq_kernels.py) -- pinned on the CPU: to the host twins of fastq.cpp (cah_fastq_scan,
cah_fastq_write_trimmed, cah_records_write) on every FASTQ golden, CRLF copies of them and seeded random records, and
to the reference's committed outputs for the info-file, mask and lowercase cases of the manifest."""
import ctypes as C
import glob
import gzip
import os

import numpy as np
import pytest

import fastq_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FQ = os.path.join(HERE, "golden", "fastq")


def _random_fastq(seed, n, crlf=False, final_newline=True):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)
    recs = []
    for i in range(n):
        k = int(rng.integers(0, 200)) if rng.random() > 0.05 else 0
        s = alphabet[rng.integers(0, len(alphabet), k)].tobytes()
        q = rng.integers(33, 75, k).astype(np.uint8).tobytes()               # (may begin with '@' or '+')
        name = b"" if rng.random() < 0.02 else b"r%d" % i + (b" c:" + b"x" * int(rng.integers(0, 90)) if rng.random() < 0.3 else b"")
        recs.append(b"@" + name + b"\n" + s + b"\n+" + (name if rng.random() < 0.1 else b"") + b"\n" + q + b"\n")
    data = b"".join(recs)
    if crlf:
        data = data.replace(b"\n", b"\r\n")
    if not final_newline:
        data = data[:-2] if crlf else data[:-1]
    return data


def _inputs():
    out = []
    for path in sorted(glob.glob(os.path.join(FQ, "*.fastq"))):
        data = open(path, "rb").read()
        out.append((os.path.basename(path), data))
        if b"\r" not in data:
            out.append((os.path.basename(path) + "+crlf", data.replace(b"\n", b"\r\n")))
    out.append(("random", _random_fastq(11, 2000)))
    out.append(("random+crlf", _random_fastq(12, 2000, crlf=True)))
    out.append(("random-lf", _random_fastq(13, 2000, final_newline=False)))
    out.append(("random+crlf-lf", _random_fastq(14, 2000, crlf=True, final_newline=False)))
    assert len(out) >= 30
    return out


def _host_scan(data):
    from cutadapt_amd import _lib
    buf = np.frombuffer(data, dtype=np.uint8)
    rec = np.empty((data.count(b"\n") // 4 + 2, 6), dtype=np.int64)
    n, consumed = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.lib().cah_fastq_scan(buf.ctypes.data if len(data) else None, len(data), 1, len(rec), rec.ctypes.data,
                                         C.byref(n), C.byref(consumed)))
    assert consumed.value == len(data)
    return rec[:n.value].copy()


def _host_write(data, rec, beg, end, keep, mode=None):
    """cah_fastq_write_trimmed (mode None) or cah_records_write(mode) on a scanned chunk"""
    from cutadapt_amd import _lib
    L = _lib.lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    n = len(rec)
    rec = np.ascontiguousarray(rec)
    beg, end = np.ascontiguousarray(beg, dtype=np.int32), np.ascontiguousarray(end, dtype=np.int32)
    keep = None if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    out = np.empty(len(data) + 4 * n + 64, dtype=np.uint8)
    out_len = C.c_int64(0)
    kp = keep.ctypes.data if keep is not None else None
    if mode is None:
        _lib.check(L.cah_fastq_write_trimmed(buf.ctypes.data, rec.ctypes.data, n, beg.ctypes.data, end.ctypes.data, kp,
                                             out.ctypes.data, len(out), C.byref(out_len)))
    else:
        seqs, offsets = np.empty(len(data) + 1, dtype=np.uint8), np.empty(n + 1, dtype=np.int64)
        _lib.check(L.cah_pack_sequences(buf.ctypes.data, rec.ctypes.data, n, seqs.ctypes.data, offsets.ctypes.data))
        _lib.check(L.cah_records_write(buf.ctypes.data, rec.ctypes.data, n, seqs.ctypes.data, offsets.ctypes.data, beg.ctypes.data,
                                       end.ctypes.data, kp, mode, out.ctypes.data, len(out), C.byref(out_len)))
    return out[:out_len.value].tobytes()


def _intervals(rng, lens):
    """intervals inside the reads and, for a fifth of them, outside: beg < 0, end > length, end < beg"""
    n = len(lens)
    beg = (rng.random(n) * (lens + 1)).astype(np.int64)
    end = beg + (rng.random(n) * (lens - beg + 1)).astype(np.int64)
    odd = rng.random(n) < 0.2
    beg = np.where(odd, beg - rng.integers(0, 5, n), beg)
    end = np.where(odd, end + rng.integers(-8, 8, n), end)
    return beg.astype(np.int32), end.astype(np.int32)


def test_index_equals_the_host_scanner():
    for name, data in _inputs():
        n_lf, rec6, seq_off, seq_len, bad = M.index(data)
        rec = _host_scan(data)
        assert n_lf == data.count(b"\n") and bad is None, name
        assert rec6.shape == rec.shape and np.array_equal(rec6, rec), name
        assert np.array_equal(seq_off, rec[:, 2]) and np.array_equal(seq_len, rec[:, 3] - rec[:, 2]), name
    assert M.index(b"")[1].shape == (0, 6) and M.index(b"@")[1].shape == (0, 6)
    # the three format errors, the first bad record named with its own code
    good = b"@r\nACGT\n+\nIIII\n"
    for code, wrong in ((1, b"r\nACGT\n+\nIIII\n"), (1, b"\nACGT\n+\nIIII\n"), (2, b"@r\nACGT\n-\nIIII\n"), (2, b"@r\nACGT\n\nIIII\n"),
                        (3, b"@r\nACGT\n+\nIII\n")):
        assert M.index(good * 3 + wrong + good)[4] == (3, code)
        assert M.bad_word(M.index(good * 3 + wrong + good)[4]) == (4 << 8) | code
        with pytest.raises(ValueError):
            _host_scan(good * 3 + wrong + good)
    assert M.bad_word(None) == -1


def test_fmt_equals_the_host_writers():
    rng = np.random.default_rng(21)
    for name, data in _inputs():
        _, rec6, _, seq_len, _ = M.index(data)
        n = len(rec6)
        whole = M.fmt(data, rec6, np.zeros(n, np.int32), seq_len)
        assert whole == _host_write(data, rec6, np.zeros(n, np.int32), seq_len, None), name
        if b"\r" not in data and data.endswith(b"\n") and b"\n+\n" in data and data.count(b"\n+\n") == n:
            assert whole == data, name                                        # (already in the output's form)
        beg, end = _intervals(rng, seq_len.astype(np.int64))
        for keep in (None, np.zeros(n, np.uint8), (rng.random(n) < 0.6).astype(np.uint8)):
            got = M.fmt(data, rec6, beg, end, keep)
            assert got == _host_write(data, rec6, beg, end, keep), name
            assert got == _host_write(data, rec6, beg, end, keep, 0), name
    # the suffix: a plain per-record restatement (the host has no twin of it)
    data = _random_fastq(31, 300)
    _, rec6, _, seq_len, _ = M.index(data)
    beg, end = _intervals(rng, seq_len.astype(np.int64))
    flags, keep = (rng.random(300) < 0.5).astype(np.uint8), (rng.random(300) < 0.8).astype(np.uint8)
    want = b""
    for r in range(300):
        nb, ne, sb, se, qb, qe = rec6[r]
        a = min(max(int(beg[r]), 0), se - sb)
        b = max(min(int(end[r]), se - sb), a)
        if keep[r]:
            want += b"@" + data[nb:ne] + (b"/suffix" if flags[r] else b"") + b"\n" + data[sb + a:sb + b] + b"\n+\n" + data[qb + a:qb + b] + b"\n"
    assert M.fmt(data, rec6, beg, end, keep, flags, b"/suffix") == want


def test_mark_equals_the_host_writer():
    rng = np.random.default_rng(22)
    for name, data in _inputs():
        _, rec6, _, seq_len, _ = M.index(data)
        n = len(rec6)
        beg, end = _intervals(rng, seq_len.astype(np.int64))
        zero = np.zeros(n, np.int32)
        for mode in (1, 2):
            marked = M.mark(data, rec6, zero, seq_len, beg, end, mode)
            assert M.fmt(marked, rec6, zero, seq_len) == _host_write(data, rec6, beg, end, None, mode), (name, mode)


def test_mark_reproduces_the_mask_and_lowercase_goldens(orc):
    """-b CAAG --times 3 --action mask / lowercase (reference test_commandline.py:303, :308): the rounds from the CPU
    oracle's aligner, an "anywhere" match counting as 5' when it starts at position 0 (adapters.py:931)"""
    aligner = orc.Aligner("CAAG", 0.1, 15, False, False, 1, 3)

    def kept(seq):
        b, e = 0, len(seq)
        for _ in range(3):
            m = aligner.locate(seq[b:e].upper())
            if m is None:
                break
            b, e = (b + m[3], e) if m[2] == 0 else (b, b + m[2])
        return b, e

    data = open(os.path.join(FQ, "in_anywhere_repeat.fastq"), "rb").read()
    _, rec6, _, seq_len, _ = M.index(data)
    iv = np.array([kept(data[r[2]:r[3]].decode()) for r in rec6], dtype=np.int32)
    zero = np.zeros(len(rec6), np.int32)
    marked = M.mark(data, rec6, zero, seq_len, iv[:, 0], iv[:, 1], 1)
    assert M.fmt(marked, rec6, zero, seq_len) == open(os.path.join(FQ, "out_anywhere_repeat.fastq"), "rb").read()
    assert marked.tobytes().count(b"N") > 50                                  # (the case does mask something)
    # the FASTA case: records of two lines, the record table written by hand (the marker looks at the sequence columns only)
    lines = open(os.path.join(FQ, "in_action_lowercase.fasta"), "rb").read().split(b"\n")
    want = open(os.path.join(FQ, "out_action_lowercase.fasta"), "rb").read().split(b"\n")
    assert len(lines) == len(want) and all(x.startswith(b">") for x in lines[0:-1:2]) and lines[-1] == b""
    done = 0
    for name, seq, wname, wseq in zip(lines[0:-1:2], lines[1::2], want[0:-1:2], want[1::2]):
        rec = np.array([[0, 0, 0, len(seq), 0, 0]], dtype=np.int64)
        b, e = kept(seq.decode())
        got = M.mark(seq, rec, [0], [len(seq)], [b], [e], 2)
        assert (name, got.tobytes()) == (wname, wseq)
        done += 1
    assert done >= 5


def test_info_rows_reproduce_the_info_file_goldens():
    """the manifest's --info-file cases on FASTQ input (reference test_info_file.py:14, :35): errors, rstart, rstop and the
    adapter of every row are read from the committed reference output -- the matcher's results --, everything else (the
    cut sequences and qualities, the rows of the later round on what the earlier one left, the "-1" rows) is the model's"""
    for inp, golden, names in (("in_illumina.fastq.gz", "info_illumina.info.txt", [b"adapt"]),
                               ("in_illumina5.fastq", "info_illumina5.info.txt", [b"adapt", b"adapt2"])):
        path = os.path.join(FQ, inp)
        data = gzip.open(path, "rb").read() if inp.endswith(".gz") else open(path, "rb").read()
        want = open(os.path.join(FQ, golden), "rb").read()
        _, rec6, _, seq_len, _ = M.index(data)
        n = len(rec6)
        read_names = [data[r[0]:r[1]] for r in rec6]
        assert len(set(read_names)) == n
        where = {nm: i for i, nm in enumerate(read_names)}
        out6 = np.zeros((2, n, 6), dtype=np.int32)
        status, best = np.zeros((2, n), dtype=np.uint8), np.zeros((2, n), dtype=np.int32)
        rows = 0
        for line in want.split(b"\n")[:-1]:
            f = line.split(b"\t")
            if f[1] == b"-1":
                continue
            r = where[f[0]]
            k = int(status[0, r])                                             # (the read's second row is round 2)
            out6[k, r, 2], out6[k, r, 3], out6[k, r, 5] = int(f[2]), int(f[3]), int(f[1])
            status[k, r], best[k, r] = 1, names.index(f[7])
            rows += 1
        assert rows > 5
        got = M.info_rows(data, rec6, out6, status, best, None, np.zeros(n, np.int32), seq_len, names)
        # (the reference compares these files with `diff --ignore-trailing-space`: the committed copies lack the empty
        # reverse-complement column at the end of a match row; nothing else may differ)
        assert got.replace(b"\t\n", b"\n") == want, golden
        assert got.count(b"\t\n") == rows
