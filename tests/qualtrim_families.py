"""The inputs of tests/test_gpu_qualtrim_kernels.py (and of the reference part of tests/test_qualtrim_model.py): reads built
so that the scans of cutadapt_amd/csrc/qualtrim.hip leave their loops at every place a 16-character chunk loop with a
byte-wise tail can get wrong.  Plain bytes, no device.  What is deterministic is built by construction; what is random
comes from random.Random(seed), so a soak run's seed offset draws other reads."""
import random

LENS = list(range(51)) + [63, 64, 65, 79, 80, 81, 127, 128, 129, 150, 151, 255, 256, 257]
CUTOFF = 20                                            # the cutoff the reads are built around
QT_PARAMS = [(20, 0), (0, 20), (20, 20), (15, 25)]     # (cutoff_front, cutoff_back) of family a
BASES = (33, 64)


def exit_sweep(base):
    """a: for every n and every p in 0 .. n, p characters one below the cutoff then characters 40 above it (the 5' scan
    gains 1 per character and leaves at the first good one while p < 40), and the mirror image for the 3' scan"""
    lo, hi = base + CUTOFF - 1, base + CUTOFF + 40
    reads = []
    for n in LENS:
        for p in range(n + 1):
            reads.append(bytes([lo]) * p + bytes([hi]) * (n - p))
            reads.append(bytes([hi]) * (n - p) + bytes([lo]) * p)
    return reads


def zero_walks(seed, count=20000, base=33):
    """b: qualities uniform in cutoff +- 3 (the partial sums hover around 0), a share of bytes below `base` and of bytes
    >= 0x80 (negative as `char`).  In front of the drawn reads, fixed ones: both ends bad and the middle good (start < stop
    survives), and everything bad (start >= stop: the collapse to (0, 0))."""
    lo, hi = base + CUTOFF - 1, base + CUTOFF + 40
    reads = []
    for n in (5, 16, 33, 64):
        reads.append(bytes([lo, lo]) + bytes([hi]) * n + bytes([lo, lo, lo]))
        reads.append(bytes([lo]) * n)
    # a byte >= 0x80 in front: a large NEGATIVE quality, the 5' sum jumps up and survives what follows ((1, 4); read as
    # unsigned it would be a very good quality that ends the 5' scan at once: (0, 4))
    reads.append(bytes([0x80, hi, hi, hi, lo]))
    rng = random.Random(seed)
    for _ in range(count):
        n = rng.choice(LENS)
        q = bytearray(base + CUTOFF + rng.randint(-3, 3) for _ in range(n))
        if rng.random() < 0.3:
            for _ in range(rng.randint(1, 3)):
                if n:
                    q[rng.randrange(n)] = rng.randrange(0, base) if rng.random() < 0.5 else rng.randrange(0x80, 0x100)
        reads.append(bytes(q))
    return reads


def nextseq_sweep(base):
    """c: (sequence, qualities) for every n and p -- a run of p 'G' at the 3' end whose qualities would stop the scan at
    once were it not for the 'G' (the sum gains 1 per 'G'); the same with one lower-case 'g' inside the run (which stops
    it); family a's 3' image on a read without 'G'; an all-'G' read that never stops"""
    lo, hi = base + CUTOFF - 1, base + CUTOFF + 40
    out = []
    for n in LENS:
        other = (b"ACT" * (n // 3 + 1))[:n]
        for p in range(n + 1):
            out.append((b"A" * (n - p) + b"G" * p, bytes([hi]) * n))
            s = bytearray(b"A" * (n - p) + b"G" * p)
            if p:
                s[n - 1 - p // 2] = ord("g")
            out.append((bytes(s), bytes([hi]) * n))
            out.append((other, bytes([hi]) * (n - p) + bytes([lo]) * p))
            out.append((b"G" * n, bytes([lo]) * (n - p) + bytes([hi]) * p))
    return out


def poly_a_fixed():
    """d, by construction: all-A and all-T reads of every length; tails of 0 .. 6 (shorter than 3 does not count); tails
    whose error share is exactly 0.2, one error more, one fewer.  A boundary tail is e errors at the very end and 4e
    'A' in front of them: the scan from the 3' end has e errors on its books when it reaches the 'A's, and the first 'A'
    that satisfies errors * 5 <= length is the LAST one, 5e - 1 characters from the end -- at equality.  e = 1 .. 16
    puts that character in every lane of a 16-character chunk (5 and 16 are coprime).
    -> (reads, deciding: {read number: (index of the deciding character, kind 0 .. 3, for the poly-T orientation?)})"""
    reads, deciding = [], {}
    for n in LENS:
        reads += [b"A" * n, b"T" * n]
        for k in range(min(6, n) + 1):
            reads += [b"C" * (n - k) + b"A" * k, b"T" * k + b"G" * (n - k)]
    for e in range(1, 17):
        for m in (0, 1, 5, 16, 20, 37):
            # exactly 0.2 (kept), one error more (not kept), one fewer (kept), one 'A' short of 0.2 (not kept)
            for kind, (hits, errs) in enumerate(((4 * e, e), (4 * e, e + 1), (4 * e, e - 1), (4 * e - 1, e))):
                deciding[len(reads)] = (m, kind, False)
                reads.append(b"C" * m + b"A" * hits + b"C" * errs)
                deciding[len(reads)] = (errs + hits - 1, kind, True)
                reads.append(b"G" * errs + b"T" * hits + b"G" * m)
    return reads, deciding


def poly_a_random(seed, count=20000):
    """d, drawn: reads over {A, C} and over {T, G} with P(A) = P(T) = 0.85"""
    rng = random.Random(seed)
    reads = []
    for k in range(count):
        n = rng.choice(LENS)
        hit, miss = (0x41, 0x43) if k % 2 == 0 else (0x54, 0x47)
        reads.append(bytes(hit if rng.random() < 0.85 else miss for _ in range(n)))
    return reads


def ee_valid(seed, base, per_len=4):
    """e: every length, valid phred values"""
    rng = random.Random(seed)
    return [bytes(rng.randint(base, 126) for _ in range(n)) for n in LENS for _ in range(per_len)]


def ee_invalid(seed, base):
    """e: one invalid byte (base - 1, 127, 0x80, 0xFF) at every position of reads of 16 .. 35 characters -- every lane of
    the 16-character loop, the groups of four and the single characters behind them --, every such read between two
    valid ones.  -> (reads, the numbers of the invalid ones)"""
    rng = random.Random(seed)
    reads, bad = [], []
    for n in range(16, 36):
        for pos in range(n):
            for byte in (base - 1, 127, 0x80, 0xFF):
                q = bytearray(rng.randint(base, 126) for _ in range(n))
                reads.append(bytes(q))
                q[pos] = byte
                bad.append(len(reads))
                reads.append(bytes(q))
    reads.append(bytes(rng.randint(base, 126) for _ in range(20)))
    return reads, bad


def fwd_place(n, index):
    """where a scan from the 5' end in chunks of 16 with a byte-wise tail has character `index` of a read of n:
    ('first' | 'middle' | 'last' | 'only', lane) inside a chunk, ('tail', None) behind the chunks"""
    chunks = n // 16
    if index >= 16 * chunks:
        return "tail", None
    k = index // 16
    where = "only" if chunks == 1 else "first" if k == 0 else "last" if k == chunks - 1 else "middle"
    return where, index % 16


def bwd_place(n, index):
    """the same for a scan from the 3' end (its chunks end where the last one began, its tail is the read's first n % 16
    characters)"""
    chunks = n // 16
    dist = n - 1 - index
    if dist >= 16 * chunks:
        return "tail", None
    k = dist // 16
    where = "only" if chunks == 1 else "first" if k == 0 else "last" if k == chunks - 1 else "middle"
    return where, 15 - dist % 16
