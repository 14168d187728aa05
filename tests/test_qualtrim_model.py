"""tests/qualtrim_model.py pinned on the CPU: the golden vectors of tests/golden/qualtrim.json (made by the reference),
the reference's own known answers (the ones tests/test_qualtrim.py::test_reference_known_answers lists) and -- where
oracle/_ref is built -- the compiled reference itself on the very reads tests/test_gpu_qualtrim_kernels.py gives the
kernels.  No GPU."""
import types

import pytest

import qualtrim_families as F
import qualtrim_model as M


def _b(s):
    return s.encode("latin-1")


def _table(golden):
    return [float.fromhex(h) for h in golden("qualtrim.json")["error_table"]]


def test_golden_vectors(golden):
    g = golden("qualtrim.json")
    table = _table(golden)
    for qual, cf, cb, base, exp in g["quality_trim"]:
        assert list(M.quality_trim(_b(qual), cf, cb, base)[0]) == exp, (qual, cf, cb, base)
    for seq, qual, cutoff, base, exp in g["nextseq"]:
        assert M.nextseq_trim(_b(seq), _b(qual), cutoff, base)[0] == exp, (seq, qual, cutoff)
    for seq, rc, exp in g["poly_a"]:
        assert M.poly_a_trim(_b(seq), rc)[0] == exp, (seq, rc)
    for qual, base, exp in g["expected_errors"]:
        (value, ok), _ = M.expected_errors(_b(qual), base, table)
        assert ok and value.hex() == exp, (qual, base)
    assert len(g["quality_trim"]) == 400 and len(g["nextseq"]) > 0 and len(g["poly_a"]) == 400 and len(g["expected_errors"]) > 0


def test_reference_known_answers(golden):
    table = _table(golden)
    assert M.nextseq_trim(b"", b"", 22)[0] == 0
    assert M.nextseq_trim(b"TCTCGTATGCCGTCTTATGCTTGAAAAAAAAAAGGGGGGGGGGGGGGGGGNNNNNNNNNNNGGNGG",
                          b"AA//EAEE//A6///E//A//EA/EEEEEEAEA//EEEEEEEEEEEEEEE###########EE#EA", 22)[0] == 33
    for sequence, tail in [("", ""), ("GGGGGGGGAAAGAAGAAGAAGAAGAAGAAG", ""), ("TTTAGA", ""), ("TTTAGAA", ""), ("TTTAG", "AAA"),
                           ("TCAAGAAGTCCTTTACCAGCTTTC", "AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA"),
                           ("TCAAGAAGTCCTTTACCAGCTTTC", "AAATAAAAAAAAAAAAAAAAAAAAAAAAAAAAA"),
                           ("GCAGATCACCTT", "AAAAAAAAAAAAAAAAAAAAAAAAAAAATAAA"), ("GCAGATCACCTT", "AAAAAAAAAAAAAAAAAAAAAAAAAAAAT"),
                           ("GCAGATCACCTT", "AAAAAAAAAAAAAAAAAAAAAAAAAAAATCG"), ("GCAGATCACCTAT", "AAAACAAAAAAACAAAAAAAACAAAAAA"),
                           ("TTTT", "AAATAAAA"), ("GGGGGGGGAAAGAAGAAGAAGAAGAAGAAG", "AAA")]:
        assert M.poly_a_trim(_b(sequence + tail))[0] == len(sequence)
    for head, sequence in [("", ""), ("", "TGTCCC"), ("TTT", "GTCCC"), ("TTTTTTTTTTTTTTTTTTTTT", "CAAGAAGTCCCCAGCTTTC"),
                           ("TTTATTTTTTTTTTTTTTTTTTTTTTTTTTTTT", "CAAGAAGTCCTTTACCAGCTTTC"),
                           ("AGCTTTTTTTTTTTTTTTTTTTTTTTTTTTT", "GCAGATCACCTT"), ("TTTATTTT", "AAAA")]:
        assert M.poly_a_trim(_b(head + sequence), True)[0] == len(head)
    enc = lambda quals: bytes(q + 33 for q in quals)
    ee = lambda q: M.expected_errors(q, 33, table)[0]
    assert ee(b"") == (0.0, True)
    assert ee(enc([10]))[0] == pytest.approx(0.1)
    assert ee(enc([10, 20, 30]))[0] == pytest.approx(0.111)
    assert ee(enc([10, 10, 20, 30, 40]))[0] == pytest.approx(0.2111)
    assert ee(b" ") == (-1.0, False)                              # (the reference: "Not a valid phred value")
    assert M.quality_trim(b"IIII##", 10, 10)[0] == (0, 4)


def test_examined_counts_and_places():
    """what the GPU tests' coverage claims rest on"""
    assert M.quality_trim(b"", 20, 20) == ((0, 0), (0, False), (0, False))
    lo, hi = bytes([33 + 19]), bytes([33 + 60])
    assert M.quality_trim(lo * 3 + hi * 5, 20, 0) == ((3, 8), (4, True), (1, True))
    assert M.quality_trim(lo * 8, 20, 20) == ((0, 0), (8, False), (8, False))
    assert M.quality_trim(hi * 7 + lo, 0, 20)[2] == (2, True)
    assert M.nextseq_trim(b"AAGG", hi * 4, 20) == (2, (3, True))
    assert M.nextseq_trim(b"GGGG", hi * 4, 20) == (0, (4, False))
    assert M.nextseq_trim(b"AAgG", hi * 4, 20) == (3, (2, True))   # lower-case g is no G
    assert M.quality_trim(bytes([0x80]) * 4, 20, 20)[1] == (4, False)        # -128 as `char`: the sums only grow
    assert F.fwd_place(48, 0) == ("first", 0) and F.fwd_place(48, 31) == ("middle", 15) and F.fwd_place(48, 47) == ("last", 15)
    assert F.fwd_place(50, 48) == ("tail", None) and F.fwd_place(16, 3) == ("only", 3) and F.fwd_place(15, 3) == ("tail", None)
    assert F.bwd_place(48, 47) == ("first", 15) and F.bwd_place(48, 16) == ("middle", 0) and F.bwd_place(48, 0) == ("last", 0)
    assert F.bwd_place(50, 1) == ("tail", None) and F.bwd_place(50, 2) == ("last", 0) and F.bwd_place(50, 49) == ("first", 15)
    assert len(F.LENS) == 65 and all(n in F.LENS for n in (0, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 128, 256))


def test_linked_views_and_ascii_count():
    out6 = [[0, 0, 0, s, 0, 0] for s in (0, 4, 10, 11, -3, 7, 7)]
    status = [1, 1, 1, 1, 1, 0, 2]
    assert M.linked_views(out6, status, None, None, 10) == ([0, 14, 30, 40, 40, 50, 60], [10, 6, 0, 0, 10, 10, 10])
    offs = [5, 15, 15, 20, 40, 41, 50, 60]
    assert M.linked_views(out6, status, offs, None, 0) == ([5, 15, 20, 31, 40, 41, 50], [10, 0, 0, 9, 1, 9, 10])
    lens = [3, 9, 9, 9, 0, 2, 2]
    assert M.linked_views(out6, status, offs, lens, 0) == ([5, 19, 24, 29, 40, 41, 50], [3, 5, 0, 0, 0, 2, 2])
    assert M.ascii_bad_reads([b"abc", b"\x80\xff\x90", b"", b"a\x7f", b"z\x80"]) == 2


def test_model_equals_compiled_reference_on_the_kernel_test_families(ref, golden):
    if ref is None or ref.qualtrim is None:
        pytest.skip("oracle/_ref not built")
    R = ref.qualtrim
    table = _table(golden)
    s = lambda b: b.decode("latin-1")
    ran = 0
    for base in F.BASES:                                          # a, b
        reads = F.exit_sweep(base) + F.zero_walks(102, base=base)
        for cf, cb in F.QT_PARAMS:
            for q in reads:
                assert M.quality_trim(q, cf, cb, base)[0] == R.quality_trim_index(s(q), cf, cb, base), (q, cf, cb, base)
            ran += len(reads)
        for seq, q in F.nextseq_sweep(base):                      # c
            rec = types.SimpleNamespace(sequence=s(seq), qualities=s(q))
            assert M.nextseq_trim(seq, q, F.CUTOFF, base)[0] == R.nextseq_trim_index(rec, F.CUTOFF, base), (seq, q, base)
            ran += 1
    for seq in F.poly_a_fixed()[0] + F.poly_a_random(103):        # d
        for rc in (False, True):
            assert M.poly_a_trim(seq, rc)[0] == R.poly_a_trim_index(s(seq), rc), (seq, rc)
        ran += 1
    for base in F.BASES:                                          # e
        for q in F.ee_valid(105, base):
            (value, ok), _ = M.expected_errors(q, base, table)
            assert ok and value.hex() == R.expected_errors(s(q), base).hex(), (q, base)
        reads, bad = F.ee_invalid(106, base)
        bad = set(bad)
        for k, q in enumerate(reads):
            (value, ok), _ = M.expected_errors(q, base, table)
            assert ok == (k not in bad) and (ok or value == -1.0), (q, base)
            if ok:
                assert value.hex() == R.expected_errors(s(q), base).hex(), (q, base)
            else:                                                 # (non-ASCII or "Not a valid phred value")
                with pytest.raises(ValueError):
                    R.expected_errors(s(q), base)
            ran += 1
    assert ran > 100000
