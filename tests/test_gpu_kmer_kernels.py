"""The k-mer prefilter kernels (kernels.hip: k_filter, k_filter_lean, k_filter_stream; stream2.hip: k_filter_stream2)
through the C ABI, on the search sets and reads of tests/kmer_families.py against the plain model of tests/kmer_model.py
(both pinned on the CPU by tests/test_kmer_model.py: the model equals the reference's recorded answers and the oracle).

Every family runs in two modes.  PRESENT (MODE 0): cah_kmers_present_batch, byte for byte, packed, as d_offsets + d_lens
views with 0xFF between, in front of and behind the reads, and the same from a base address that is not 16-byte aligned;
64 guard rows behind d_present must survive.  QUEUE (MODE 1): the family's sets as the prefilter of a 3' aligner, the
survivor queue that cah_match_batch* leaves (test_gpu_stream._survivors) = exactly the model's present reads, the
survivors' tuples = the oracle's, and every route that serves a plan -- stream2, stream, the uniform and the ragged
per-lane kernel -- leaves the same keys.  Which kernel a call reaches is asserted from the plan (kmer_families.kernels
restates the launchers' rules on what the library reports about the plan).  GPU only."""
import os

import numpy as np
import pytest

import kmer_families as F
import kmer_model as M
from test_gpu_stream import _survivors

pytestmark = pytest.mark.gpu

OK, EUNSUPPORTED = 0, 5
ABSENT, PRESENT, INVALID = 0, 1, 2
GUARD, CANARY = 64, 0x5A
MAX_LAUNCH = 9000
GROUPS = F.groups()


# ---- helpers ------------------------------------------------------------------------------------------------------------

def _up(a, dtype=None):
    import torch
    a = np.ascontiguousarray(a, dtype=dtype)
    return torch.from_numpy(a.copy()).to("cuda:0") if a.size else torch.zeros(1, dtype=torch.from_numpy(a).dtype, device="cuda:0")


def _raw(reads):
    return [r if isinstance(r, bytes) else r.encode("latin-1") for r in reads]


def _packed(reads):
    raw = _raw(reads)
    off = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) or b"\xff", dtype=np.uint8), off


def _gapped(reads, first_gap=1):
    """reads with 1..37 bytes of 0xFF in front of each and behind the last -> (bytes, starts int64[n], lens int32[n])"""
    parts, starts, lens, at = [], [], [], 0
    for k, x in enumerate(_raw(reads)):
        gap = 1 + (first_gap - 1 + 5 * k) % 37
        parts.append(b"\xff" * gap)
        at += gap
        starts.append(at)
        lens.append(len(x))
        parts.append(x)
        at += len(x)
    parts.append(b"\xff" * 23)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.array(starts, np.int64), np.array(lens, np.int32)


def _present(hip, plan, seqs, offsets, lens, n, expect=OK):
    """one call on canary-filled rows -> present[n]; the 64 guard rows behind them are checked"""
    import torch
    out = torch.full((n + GUARD,), CANARY, dtype=torch.uint8, device="cuda:0")
    rc = hip.cah_kmers_present_batch(plan.handle, 0, seqs.data_ptr(), offsets.data_ptr(),
                                     None if lens is None else lens.data_ptr(), n, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    got = out.cpu().numpy()
    assert (got[n:] == CANARY).all(), "rows >= n_reads were written"
    return got[:n]


def _same(got, want, reads, label):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, "first difference at read", int(bad[0]), reads[bad[0]], "got", int(got[bad[0]]),
                           "model", int(want[bad[0]]), int(bad.size), "rows differ")


def _present_layouts(hip, fam, shift):
    """all reads of the family, in launches of at most MAX_LAUNCH reads, in the three layouts"""
    import torch
    plan = F.plan_of(fam)
    assert F.routing_of(plan) == fam["tag"], fam["name"]
    reads = [r[0] for r in F.all_reads(fam)]
    want = (F.all_answers(fam) >= 0).astype(np.uint8)
    assert want.any() and not want.all()
    for lo in range(0, len(reads), MAX_LAUNCH):
        part, w = reads[lo:lo + MAX_LAUNCH], want[lo:lo + MAX_LAUNCH]
        n = len(part)
        buf, off = _packed(part)
        _same(_present(hip, plan, _up(buf), _up(off), None, n), w, part, (fam["name"], F.kernels(fam, 0), "packed"))
        buf, starts, lens = _gapped(part, first_gap=1 + lo % 37)
        ts, tl = _up(starts), _up(lens)
        _same(_present(hip, plan, _up(buf), ts, tl, n), w, part, (fam["name"], F.kernels(fam, 0), "views"))
        room = torch.full((len(buf) + 16,), 0xFF, dtype=torch.uint8, device="cuda:0")
        assert room.data_ptr() % 16 == 0
        room[shift:shift + len(buf)] = _up(buf)
        _same(_present(hip, plan, room[shift:], ts, tl, n), w, part, (fam["name"], F.kernels(fam, 0), "views, base + %d" % shift))
    return len(reads)


class _env:
    def __init__(self, names):
        self.names = names

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.names}
        for k in self.names:
            os.environ[k] = "1"

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _oracle(orc, fam):
    return (orc.Aligner(F.ADAPTER, 0.1, 14, False, False, 1, 3),
            orc.KmerFinder(fam["sets"], fam["ref_wc"], fam["query_wc"]))


def _queue(fam, reads, views=False, env=()):
    """cah_match_batch* on the reads -> ({read: key}, out6, status)"""
    import torch
    from cutadapt_amd.batch import ReadBatch, match_batch
    plan = F.plan_of(fam, aligner=True)
    if views:
        buf, starts, lens = _gapped(reads)
        batch = ReadBatch(_up(buf), _up(starts), _up(lens), validated=True)
    else:
        batch = ReadBatch.from_strings(reads)
    with _env(env):
        out6, status, _ = match_batch(plan, batch).cpu()
    torch.cuda.synchronize()
    return _survivors(batch, len(reads)), out6, status


def _check_queue(fam, reads, want_keys, got, oracle_rows, label):
    """want_keys: kmer_families.keys of the reads (-1: not present)"""
    q, out6, status = got
    want = set(np.flatnonzero(want_keys >= 0).tolist())
    assert set(q) == want, (label, "queue and model differ at reads", sorted(set(q) ^ want)[:5])
    order = sorted(q)
    keys = np.array([q[i] for i in order], dtype=np.int64)
    bad = np.flatnonzero(keys != want_keys[order])
    assert bad.size == 0, (label, "keys: read", order[bad[0]] if bad.size else None, reads[order[bad[0]]] if bad.size else None,
                           "got", int(keys[bad[0]]) if bad.size else None, "from the code", int(want_keys[order][bad[0]]) if bad.size else None)
    w6, wst = oracle_rows
    assert np.array_equal(status, wst) and np.array_equal(out6, w6), (label, "tuples differ from the oracle's")


def _queue_general(orc, fam):
    reads = [r[0] for r in F.all_reads(fam)]
    fhe = F.all_keys(fam)
    aligner, finder = _oracle(orc, fam)
    assert F.routing_of(F.plan_of(fam, True)) == fam["tag"]
    name = F.kernels(fam, 1)
    for lo in range(0, len(reads), MAX_LAUNCH):
        part, f = reads[lo:lo + MAX_LAUNCH], fhe[lo:lo + MAX_LAUNCH]
        buf, off = _packed(part)
        rows = orc.match_batch(aligner, finder, buf.copy(), off)
        a = _queue(fam, part)
        _check_queue(fam, part, f, a, rows, (fam["name"], name, "packed"))
        b = _queue(fam, part, views=True)
        _check_queue(fam, part, f, b, rows, (fam["name"], name, "views"))
        assert a[0] == b[0], (fam["name"], "keys of the packed and the view layout differ")


def _queue_lean(orc, fam):
    """equally long packed reads by default, with CAH_NO_STREAM2=1 and with CAH_NO_STREAM=1; all reads as views and as one
    ragged packed batch: the same queue under the same keys"""
    aligner, finder = _oracle(orc, fam)
    assert F.routing_of(F.plan_of(fam, True)) == fam["tag"]
    kernels = set()
    uniform_keys = []
    for n in fam["lengths"]:
        rows = F.reads_of(fam, n)
        if n == 0:
            uniform_keys.append({})
            continue
        reads = [r[0] for r in rows]
        fhe = F.keys(fam, n)
        while len(reads) < 70:                                 # (more than a tiny batch, and at least 16 characters)
            reads, fhe = reads + reads, np.concatenate([fhe, fhe])
        buf, off = _packed(reads)
        want = orc.match_batch(aligner, finder, buf.copy(), off)
        first = None
        for env in ((), ("CAH_NO_STREAM2",), ("CAH_NO_STREAM",)):
            name = F.kernels(fam, 1, "uniform", n, len(reads), env)
            kernels.add(name.split("<")[0] if "stream" in name else name)
            got = _queue(fam, reads, env=env)
            _check_queue(fam, reads, fhe, got, want, (fam["name"], n, name))
            first = first if first is not None else got[0]
            assert got[0] == first, (fam["name"], n, name, "keys differ from the default route's")
        uniform_keys.append({i: k for i, k in first.items() if i < len(rows)})
    reads = [r[0] for r in F.all_reads(fam)]
    fhe = F.all_keys(fam)
    buf, off = _packed(reads)
    want = orc.match_batch(aligner, finder, buf.copy(), off)
    name = F.kernels(fam, 1, "ragged")
    kernels.add(name)
    ragged = _queue(fam, reads)
    _check_queue(fam, reads, fhe, ragged, want, (fam["name"], name, "ragged packed"))
    views = _queue(fam, reads, views=True)
    _check_queue(fam, reads, fhe, views, want, (fam["name"], name, "views"))
    assert views[0] == ragged[0]
    at, merged = 0, {}
    for n, keys in zip(fam["lengths"], uniform_keys):
        merged.update({at + i: k for i, k in keys.items()})
        at += len(F.reads_of(fam, n))
    assert merged == ragged[0], (fam["name"], "keys of the uniform routes and the ragged kernel differ")
    return kernels


# ---- routing ------------------------------------------------------------------------------------------------------------

def test_every_family_reaches_its_kernel(hip):
    named = set()
    for fam in F.families():
        for aligner in (False, True):
            assert F.routing_of(F.plan_of(fam, aligner)) == fam["tag"], (fam["name"], aligner)
        named |= {F.kernels(fam, 0), F.kernels(fam, 1)}
    by = F.by_name
    assert F.kernels(by("g_mix"), 0) == "k_filter<0,lds,narrow>" and F.kernels(by("tn_65"), 1) == "k_filter<1,hbm,narrow>"
    assert F.kernels(by("tw_32"), 0) == "k_filter<0,lds,wide>" and F.kernels(by("tw_33"), 1) == "k_filter<1,hbm,wide>"
    assert F.kernels(by("c12_d3"), 1, "uniform", 64, 70) == "k_filter_stream2"
    assert F.kernels(by("c12_d3"), 1, "uniform", 64, 70, ("CAH_NO_STREAM2",)) == "k_filter_stream<3,1,2>"
    assert F.kernels(by("c12_d3"), 1, "uniform", 64, 70, ("CAH_NO_STREAM",)) == "k_filter_lean<uniform,3,1,2>"
    assert F.kernels(by("c36_d0"), 1, "uniform", 161, 70) == "k_filter_lean<uniform,0,3,6>"
    assert F.kernels(by("c26_d0"), 1, "uniform", 160, 70) == "k_filter_stream<0,2,6>"
    assert F.kernels(by("c23_d3"), 0) == "k_filter_lean<ragged,3,2,3>"


# ---- present mode -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["general narrow", "general wide", "tables", "lean classes", "lean tails", "lean heads", "wildcards"])
def test_present_mode_equals_the_model(hip, group):
    total = 0
    for k, fam in enumerate(GROUPS[group]):
        total += _present_layouts(hip, fam, shift=1 + k % 15)
    assert total > 10000


def test_present_mode_at_every_base_shift(hip):
    """one general and one lean family from base addresses 1 .. 15 bytes past a 16-byte boundary"""
    for name in ("g_neg_pos", "tails_and_head"):
        for shift in range(1, 16):
            _present_layouts(hip, F.by_name(name), shift)


def test_word_limit(hip):
    """1 024 packed words work (one k-mer per word, the hit planted for the last); 1 025 are refused and nothing is launched"""
    fam = F.by_name("tn_1024")
    assert 90 <= _present_layouts(hip, fam, 7) <= 120
    fam = F.by_name("tn_1025")
    plan = F.plan_of(fam)
    assert plan.n_kmer_entries() == 1025
    reads = [r[0] for r in F.all_reads(fam)]
    buf, off = _packed(reads)
    got = _present(hip, plan, _up(buf), _up(off), None, len(reads), expect=EUNSUPPORTED)
    assert (got == CANARY).all()


def test_tile_edges_and_empty_batch(hip, orc):
    """n_reads around FILTER_TILE / LEAN_TILE (8 192) and the wave (64) on 20-character reads, both modes; n_reads = 0
    returns CAH_OK and writes nothing"""
    for name in ("g_mix", "tail_7"):
        fam = F.by_name(name)
        plan = F.plan_of(fam)
        rows, fhe = F.reads_of(fam, 20), F.keys(fam, 20)
        aligner, finder = _oracle(orc, fam)
        assert (fhe >= 0).any() and (fhe < 0).any()
        for count in (1, 63, 64, 65, 8191, 8192, 8193):
            pick = [(7 * k) % len(rows) for k in range(count)]
            reads, f = [rows[k][0] for k in pick], fhe[pick]
            buf, off = _packed(reads)
            tb, to = _up(buf), _up(off)
            _same(_present(hip, plan, tb, to, None, count), (f >= 0).astype(np.uint8), reads, (name, count))
            want = orc.match_batch(aligner, finder, buf.copy(), off)
            for env in ((), ("CAH_NO_STREAM",), ("CAH_NO_UNIFORM",)):
                _check_queue(fam, reads, f, _queue(fam, reads, env=env), want, (name, count, env))
        assert (_present(hip, plan, tb, to, None, 0) == CANARY).all()


# ---- invalid bytes ------------------------------------------------------------------------------------------------------

def test_invalid_bytes_inside_the_windows(hip):
    """What cah_kmers_present_batch guarantees (include/cutadapt_hip.h): a read without an occurrence in a window and with
    a byte >= 0x80 inside the union of its windows is CAH_INVALID -- from the general and the lean kernels alike.  Bytes
    outside every window or behind the first hit are not promised and not asserted.  (Bytes >= 0x80 outside every read:
    the 0xFF gaps of every view layout above.)"""
    seen = {"general": 0, "lean": 0}
    for name in ("g_mix", "g_neg_pos", "g_pos_pos", "w_neg_pos", "w_64", "tn_9", "c12_d3", "c36_d0", "head_only", "tail_only",
                 "tails_and_head", "lead_30"):
        fam = F.by_name(name)
        plan = F.plan_of(fam)
        for n in (1, 19, 30, 50, 100):
            inside = np.zeros(n, dtype=bool)
            for a, b, _ in fam["sets"]:
                ws, we = M.window(a, b, n)
                inside[ws:we] = True
            reads, promised = [], []
            for p in range(n):
                for byte in (0x80, 0xC3, 0xFF):
                    r = bytearray(F.BACKGROUND.encode() * n)
                    r[p] = byte
                    reads.append(bytes(r))
                    promised.append(bool(inside[p]))
            reads.append(F.BACKGROUND.encode() * n)
            promised.append(False)
            promised = np.array(promised)
            buf, off = _packed(reads)
            got = _present(hip, plan, _up(buf), _up(off), None, len(reads))
            assert (got[promised] == INVALID).all(), (name, n, np.flatnonzero(promised & (got != INVALID))[:5].tolist())
            assert got[-1] == ABSENT and not (got == PRESENT).any()
            buf, starts, lens = _gapped(reads)
            again = _present(hip, plan, _up(buf), _up(starts), _up(lens), len(reads))
            assert np.array_equal(again, got), (name, n, "views")
            seen[fam["tag"]["kind"]] += int(promised.sum())
    assert seen["general"] > 1000 and seen["lean"] > 1000


# ---- queue mode ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["general narrow", "general wide", "tables", "wildcards"])
def test_queue_mode_general(hip, orc, group):
    ran = 0
    for fam in GROUPS[group]:
        if fam["tag"]["kind"] == "general":
            _queue_general(orc, fam)
            ran += 1
    assert ran >= 3
    if group == "tables":
        _queue_general(orc, F.by_name("tn_1024"))


@pytest.mark.parametrize("group", ["lean classes", "lean tails", "lean heads", "wildcards"])
def test_queue_mode_lean(hip, orc, group):
    kernels = set()
    for fam in GROUPS[group]:
        if fam["tag"]["kind"] == "lean":
            kernels |= _queue_lean(orc, fam)
    assert {"k_filter_stream"} <= kernels and any(k.startswith("k_filter_lean<uniform") for k in kernels)
    if group != "wildcards":
        assert "k_filter_stream2" in kernels
    if group == "lean classes":
        want = {k for k in F.required_kernels() if k.startswith("k_filter_lean")}
        assert want <= kernels, sorted(want - kernels)


def test_keys_never_pass_the_first_whole_read_hit(hip, orc):
    """the property the cost scan's column skipping relies on, for plans whose matcher reports skip_ok -- a lean one and a
    general one, where it rests on the whole-read words going first (api.cpp) -- with every k-mer of the whole-read set
    planted: key * 4 is at or before the end of the earliest occurrence of a k-mer of the whole-read set"""
    for name in ("heuristic_like", "g_heuristic_like"):
        fam = F.by_name(name)
        assert F.skip_ok(F.plan_of(fam, True)) == 1 and F.routing_of(F.plan_of(fam, True)) == fam["tag"]
        whole = [s for s in fam["sets"] if s[0] == 0 and s[1] is None]
        assert len(whole) == 1 and {j for j, t, _ in fam["probes"]} == set(range(len(fam["sets"])))
        assert sum(j == 0 for j, t, _ in fam["probes"]) == 3
        checked = 0
        for n in fam["lengths"]:
            if n == 0:
                continue
            reads = [r[0] for r in F.reads_of(fam, n)]
            ends = M.first_hit_end_block(whole, M.as_block(reads), fam["ref_wc"], fam["query_wc"])
            for env, views in (((), False), (("CAH_NO_STREAM",), False), ((), True)):
                q, _, _ = _queue(fam, reads, views=views, env=env)
                for i, key in q.items():
                    assert key <= 255
                    if ends[i] >= 0:
                        assert key * 4 <= ends[i], (name, n, reads[i], key, int(ends[i]))
                        checked += 1
        assert checked > 1000, (name, checked)
