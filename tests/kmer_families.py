"""Search sets and reads for the direct tests of the k-mer prefilter kernels (k_filter, k_filter_lean, k_filter_stream,
k_filter_stream2).  Deterministic: no random numbers.

A FAMILY is one plan: search sets (start, stop, k-mers) in the ABI's / KmerFinder's form, the wildcard mode, the k-mers
that are planted in reads (PROBES) and a TAG: the kernel the plan must reach.  tests/test_gpu_kmer_kernels.py asserts the
tag against Plan.prefilter_kind(), cah_plan_n_kmer_entries and cah_plan_debug_lean; kernels() restates the launchers'
rules (kernels.hip: launch_filter, launch_filter_lean) on the tag, so that every test can say which kernel it ran.

READS of a family, for every read length n of LENGTHS and n in {p - 1, p, p + 1} for every window parameter p of the plan:
one probe at a time planted at every start 0 .. n - q in a background of 'T', the all-background read, and (n = 0) the
empty read.  Reads with an odd start are written in lower case.  No k-mer holds a T, and without reference wildcards
the background matches no character of any k-mer; with them the N that _ref_wild puts into a k-mer matches the
background too, and the k-mer's other characters still do not.  Every k-mer of every set is a probe (in the table and
limit families only the last word's, which is what they are about); the last k-mer of a set is planted at every length,
the others at THIN and the window parameters' lengths.

kernels() INFERS which kernel served a call: nothing observes a launch.  It is a restatement of launch_filter and
launch_filter_lean, right for the launchers as they are; if their rules change, the labels and required_kernels() have
to follow, and the comparisons would not notice on their own because every route gives equal answers.

The k-mers of a plan without wildcards are chosen so that none occurs inside another: a read then holds exactly one
occurrence of exactly one k-mer, and whether it is present follows from window arithmetic alone (planted_answer) -- the
self-check that keeps the GPU tests from passing vacuously."""
import numpy as np

import kmer_model as M

LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 159, 160, 161, 255, 256, 257)
THIN = (16, 17, 33, 64, 65, 81, 129, 160, 161, 257)
LEAN_SPAN = 64
ADAPTER = "ACGGACCAGCAAGGCACGAC"                     # 20 characters; the 3' aligner of the queue-mode tests
BACKGROUND = "T"

_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- k-mers ------------------------------------------------------------------------------------------------------------

def _candidate(i, q, alphabet):
    """the i-th string of q characters: the digits of i first (distinct i give distinct strings of one length as long as
    len(alphabet) ** q > i), then a fixed sequence that does not repeat with a short period"""
    out, v, x = [], i, 12345 + 7919 * i
    for p in range(q):
        if v or p == 0:
            out.append(alphabet[v % len(alphabet)])
            v //= len(alphabet)
        else:
            x = (x * 1103515245 + 12345) % (1 << 31)
            out.append(alphabet[(x >> 16) % len(alphabet)])
    return "".join(out)


class _Kmers:
    """hands out k-mers none of which occurs inside another"""

    def __init__(self, alphabet="ACG"):
        self.alphabet = alphabet
        self.used = []
        self.by_len = {}
        self.next = {}

    def new(self, q):
        i = self.next.get(q, 0)
        while True:
            k = _candidate(i, q, self.alphabet)
            i += 1
            if k in self.by_len.get(q, ()):
                continue
            if all((k not in u and u not in k) for u in self.used if len(u) != q):
                break
        self.next[q] = i
        self.used.append(k)
        self.by_len.setdefault(q, set()).add(k)
        return k


_REF_WILD = {"A": "R", "C": "M", "G": "S"}           # IUPAC codes that still hold the letter and never T


def _ref_wild(k):
    """an IUPAC form of an ACG k-mer: every third character widened, one N (matches every read character) in the middle"""
    out = [(_REF_WILD[c] if i % 3 == 1 else c) for i, c in enumerate(k)]
    if len(k) >= 5:
        out[2] = "N"
    return "".join(out)


def _query_wild(k):
    """an instance of a k-mer as a read with IUPAC characters writes it"""
    return "".join(("N" if i % 3 == 2 else "R" if (c == "A" and i % 3 == 0) else c) for i, c in enumerate(k))


# ---- families ----------------------------------------------------------------------------------------------------------

def general(narrow, n_words):
    entry = 4 if narrow else 8
    return dict(kind="general", narrow=narrow, lds=n_words * 128 * entry <= 32 * 1024, n_words=n_words)


def lean(n_lead, n_gated, n_tail, lead_delay, tw_ok, n_tw):
    cls = (1, 2) if n_lead <= 1 and n_gated <= 2 else (2, 3) if n_lead <= 2 and n_gated <= 3 else (2, 6) if n_lead <= 2 else (3, 6)
    return dict(kind="lean", cls=cls, n_lead=n_lead, n_gated=n_gated, n_tail=n_tail, lead_delay=lead_delay, tw_ok=tw_ok, n_tw=n_tw)


def _family(name, shape, tag, ref_wc=False, query_wc=False, lengths=None, group=None):
    """shape: (start, stop, lengths of the k-mers to make, or the k-mers themselves)"""
    made = _Kmers()
    sets, plants = [], []
    explicit = False
    for start, stop, what in shape:
        kmers = []
        for w in what:
            if isinstance(w, str):
                explicit = True
                kmers.append(w)
            else:
                kmers.append(made.new(w))
        sets.append((start, stop, kmers))
    for j, (start, stop, kmers) in enumerate(sets):
        for t in range(len(kmers)):
            if t == len(kmers) - 1 or group not in ("tables", "limit"):
                plants.append((j, t))
    plan_sets = [(a, b, [_ref_wild(k) if ref_wc else k for k in kmers]) for a, b, kmers in sets]
    params = sorted({abs(v) for a, b, _ in sets for v in (a, b or 0) if v})
    if lengths is None:
        lengths = sorted(set(LENGTHS) | {n for p in params for n in (p - 1, p, p + 1) if n >= 0})
    return dict(name=name, sets=plan_sets, base_sets=sets, ref_wc=ref_wc, query_wc=query_wc, tag=tag, group=group,
                probes=[(j, t, _query_wild(sets[j][2][t]) if query_wc else sets[j][2][t]) for j, t in plants],
                arith=not (ref_wc or query_wc or explicit), lengths=list(lengths), params=params,
                thin={pi for pi, (j, t) in enumerate(plants) if t != len(sets[j][2]) - 1},
                thin_lengths=set(THIN) | {n for p in params for n in (p - 1, p, p + 1)})


PARTIAL = (("pos_start", 3, None), ("neg_stop", 0, -3), ("neg_neg", -20, -3), ("neg_pos", -20, 40), ("pos_pos", 3, 70))
# ((3, 70): a window (a, b) with 0 <= a < b <= 64 is a head window of the lean kernels -- the head_* families)
WIDE_PARTIAL = (("pos_start", 3, None), ("neg_stop", 0, -3), ("neg_neg", -60, -3), ("neg_pos", -60, 70), ("pos_pos", 3, 70))
PAST_SPAN = (("tail65", -(LEAN_SPAN + 1), None), ("head65", 0, LEAN_SPAN + 1))
MIX = [(3, None, (6,)), (0, -3, (7,)), (-20, 40, (8,))]
LEAN_WILD = [(0, None, (10,)), (-9, None, (6,)), (4, 30, (7,))]


def _build():
    fams = []
    add = lambda *a, **k: fams.append(_family(*a, **k))
    # general, narrow words
    for label, a, b in PARTIAL + PAST_SPAN:
        add("g_" + label, [(a, b, (6,))], general(True, 1), group="general narrow")
    add("g_mix", MIX, general(True, 3), group="general narrow")
    add("g_overcap_lead", [(0, None, (30, 30, 30, 30))], general(True, 4), group="general narrow")
    add("g_overcap_gated", [(0, None, (10,)), (-40, None, (17,) * 7)], general(True, 8), group="general narrow")
    # general, wide words
    for q in (33, 40, 63, 64):
        add("w_%d" % q, [(0, None, (q,))], general(False, 1), group="general wide")
    add("w_mixed", [(0, None, (33, 5, 40, 6, 63, 64))], general(False, 4), group="general wide")
    for label, a, b in WIDE_PARTIAL + PAST_SPAN:                # (wide enough for a k-mer of 40 characters)
        add("w_" + label, [(a, b, (40,))], general(False, 1), group="general wide")
    # table placement and word groups: one k-mer per word, the hit planted for the last word only
    for n in (8, 9, 16, 17, 64, 65):
        add("tn_%d" % n, [(1, None, (17,) * n)], general(True, n), group="tables")
    for n in (6, 7, 12, 13, 32, 33):
        add("tw_%d" % n, [(1, None, (33,) * n)], general(False, n), group="tables")
    add("tn_1024", [(1, None, (17,) * 1024)], general(True, 1024), lengths=range(17, 30), group="limit")
    add("tn_1025", [(1, None, (17,) * 1025)], general(True, 1025), lengths=(20,), group="limit")
    # lean: slot classes x delay
    tail5, tails17 = (-10, None, (5,)), (-40, None, (17,) * 4)
    add("c12_d3", [(0, None, (28,)), tail5], lean(1, 1, 1, 3, 1, 1), group="lean classes")
    add("c12_d0", [(0, None, (30,)), tail5], lean(1, 1, 1, 0, 0, 0), group="lean classes")
    add("c23_d3", [(0, None, (20, 20)), tail5], lean(2, 1, 1, 3, 1, 1), group="lean classes")
    add("c23_d0", [(0, None, (16, 16, 16)), tail5], lean(2, 1, 1, 0, 0, 0), group="lean classes")
    add("c26_d3", [(0, None, (28,)), tails17], lean(1, 4, 4, 3, 1, 4), group="lean classes")
    add("c26_d0", [(0, None, (30,)), tails17], lean(1, 4, 4, 0, 0, 0), group="lean classes")
    add("c36_d3", [(0, None, (28, 28, 28)), tail5], lean(3, 1, 1, 3, 1, 1), group="lean classes")
    add("c36_d0", [(0, None, (30, 30, 30)), tail5], lean(3, 1, 1, 0, 0, 0), group="lean classes")
    # lean: lead k-mer lengths (29 / 30: the edge of lead_delay)
    for q in (1, 28, 29, 30, 32):
        d = 3 if q + 3 <= 32 else 0
        add("lead_%d" % q, [(0, None, (q,))], lean(1, 0, 0, d, 1 if d else 0, 0), group="lean tails")
    # lean: tail windows around the k-mer length q = 6, head windows
    for L in (1, 5, 6, 7, 63, 64):
        add("tail_%d" % L, [(0, None, (10,)), (-L, None, (6,))], lean(1, 1, 1, 3, 1, 1), group="lean tails")
    add("tail_only", [(-7, None, (6,))], lean(0, 1, 1, 3, 1, 1), group="lean tails")
    for a, b in ((0, 5), (0, 6), (0, 64), (5, 11), (5, 64)):
        add("head_%d_%d" % (a, b), [(0, None, (10,)), (a, b, (6,))], lean(1, 1, 0, 3, 0, 0), group="lean heads")
    add("head_only", [(5, 64, (6,))], lean(0, 1, 0, 3, 0, 0), group="lean heads")
    shared = [(0, None, (10,)), (-8, None, (5,)), (-20, None, (5,)), (-64, None, (5,)), (-3, None, (5,))]
    add("tails_share_a_word", shared, lean(1, 1, 1, 3, 1, 1), group="lean heads")
    add("tails_and_head", shared + [(2, 30, (5,))], lean(1, 2, 1, 3, 0, 0), group="lean heads")
    # what kmer_heuristic builds for ADAPTER at 10 % errors: the three chunks over the whole read (-> skip_ok) and tail sets
    a = ADAPTER
    add("heuristic_like", [(0, None, (a[0:7], a[7:14], a[14:20])), (-4, None, (a[:4],)), (-9, None, (a[:5], a[5:9]))],
        lean(1, 1, 1, 3, 1, 1), group="lean heads")
    # ... and the same whole-read set next to a tail window past the lean span: a general plan whose matcher reports skip_ok
    add("g_heuristic_like", [(0, None, (a[0:7], a[7:14], a[14:20])), (-(LEAN_SPAN + 1), None, (a[:5],))],
        general(True, 2), group="general narrow")
    # all four wildcard modes on a general and on a lean family
    for rw, qw in ((True, False), (False, True), (True, True)):
        label = "_r%dq%d" % (rw, qw)
        add("g_mix" + label, MIX, general(True, 3), ref_wc=rw, query_wc=qw, group="wildcards")
        add("lean_wild" + label, LEAN_WILD, lean(1, 2, 1, 3, 0, 0), ref_wc=rw, query_wc=qw, group="wildcards")
    add("lean_wild_r0q0", LEAN_WILD, lean(1, 2, 1, 3, 0, 0), group="wildcards")
    return fams


def families():
    return once("families", _build)


def by_name(name):
    return {f["name"]: f for f in families()}[name]


def groups():
    out = {}
    for f in families():
        out.setdefault(f["group"], []).append(f)
    return out


# ---- reads ---------------------------------------------------------------------------------------------------------------

def planted(fam, probe, n):
    """is the probe planted in reads of length n?"""
    return probe not in fam["thin"] or n in fam["thin_lengths"]


def reads_of(fam, n):
    """[(read, probe index or -1, start or -1)] of length n"""
    def make():
        if n == 0:
            return [("", -1, -1)]
        out = [(BACKGROUND * n, -1, -1)]
        for pi, (j, t, text) in enumerate(fam["probes"]):
            q = len(text)
            if not planted(fam, pi, n):
                continue
            for s in range(n - q + 1):
                r = BACKGROUND * s + text + BACKGROUND * (n - s - q)
                out.append((r.lower() if s % 2 else r, pi, s))
        return out
    return once(("reads", fam["name"], n), make)


def all_reads(fam):
    """every read of the family, shortest first: [(read, probe, start)]"""
    return once(("all reads", fam["name"]), lambda: [r for n in fam["lengths"] for r in reads_of(fam, n)])


def answers(fam, n):
    """the model's first_hit_end of every read of reads_of(fam, n): int64[reads], -1 = not present"""
    def make():
        rows = reads_of(fam, n)
        if n == 0:
            return np.array([-1], dtype=np.int64)
        return M.first_hit_end_block(fam["sets"], M.as_block([r[0] for r in rows]), fam["ref_wc"], fam["query_wc"])
    return once(("answers", fam["name"], n), make)


def all_answers(fam):
    return once(("all answers", fam["name"]), lambda: np.concatenate([answers(fam, n) for n in fam["lengths"]]))


def word_groups(fam):
    """the packed words of a general plan as k_filter walks them (api.cpp: the k-mers of a set go greedily into words of 32
    bits, or of 64 if any k-mer is longer than 32; whole-read words first; kernels.hip: groups of 8 narrow / 6 wide words):
    [[(start, stop, k-mers of the word)]]"""
    t = fam["tag"]
    bits, slots = (32, 8) if t["narrow"] else (64, 6)
    words = []
    for a, b, kmers in fam["sets"]:
        cur, used = [], 0
        for k in kmers:
            if cur and used + len(k) > bits:
                words.append((a, b, cur))
                cur, used = [], 0
            cur.append(k)
            used += len(k)
        words.append((a, b, cur))
    words = [w for w in words if w[0] == 0 and w[1] is None] + [w for w in words if not (w[0] == 0 and w[1] is None)]
    assert len(words) == t["n_words"], (fam["name"], len(words))
    return [words[g:g + slots] for g in range(0, len(words), slots)]


def keys(fam, n):
    """the survivor queue's key of every read of reads_of(fam, n), -1 for a read that is not present -- from the code:
    the lean and streaming kernels walk all words over 16-character chunks from position 0 and name the 4-character
    group in which the earliest k-mer that lies in its window ends: key = min(end >> 2, 255).  k_filter takes the words in
    groups, a read leaves at the first GROUP with a hit, and a group's chunks start at `lo`, the start of the union of the
    group's windows (kernels.hip: `int pos = lo`), so its 4-character groups are counted from there:
    key = min((lo + 4 * ((end - lo) // 4)) >> 2, 255) with the earliest end among that group's k-mers."""
    def make():
        ends = answers(fam, n)
        if fam["tag"]["kind"] == "lean" or n == 0:
            return np.where(ends >= 0, np.minimum(ends >> 2, 255), -1)
        block = M.as_block([r[0] for r in reads_of(fam, n)])
        out = np.full(len(ends), -1, dtype=np.int64)
        for group in word_groups(fam):
            spans = [M.window(a, b, n) for a, b, _ in group]
            spans = [(ws, we) for ws, we in spans if we > ws]
            if not spans:
                continue
            lo = min(ws for ws, _ in spans)
            e = M.first_hit_end_block(group, block, fam["ref_wc"], fam["query_wc"])
            take = (out < 0) & (e >= 0)
            out[take] = np.minimum((lo + 4 * ((e[take] - lo) // 4)) >> 2, 255)
        assert np.array_equal(out >= 0, ends >= 0)
        return out
    return once(("keys", fam["name"], n), make)


def all_keys(fam):
    return once(("all keys", fam["name"]), lambda: np.concatenate([keys(fam, n) for n in fam["lengths"]]))


def planted_answer(fam, n, probe, start):
    """window arithmetic alone (families with arith): is the read with probe `probe` at `start` present?"""
    if probe < 0:
        return False
    j, t, text = fam["probes"][probe]
    ws, we = M.window(fam["sets"][j][0], fam["sets"][j][1], n)
    return ws <= start and start + len(text) <= we


# ---- the library's view of a family ----------------------------------------------------------------------------------------

def specs_of(fam, aligner=False):
    """the family's search sets as a KmerFinder plan, or as the prefilter of a 3' aligner (flags 14) for ADAPTER at 10 %"""
    from cutadapt_amd import _lib
    kw = dict(kmer_sets=fam["sets"], kmer_ref_wildcards=fam["ref_wc"], kmer_query_wildcards=fam["query_wc"])
    if aligner:
        return _lib.MatcherSpec(ADAPTER, 0.1, flags=14, min_overlap=3, **kw)
    return _lib.MatcherSpec(kind=_lib.KIND_KMER_ONLY, **kw)


def plan_of(fam, aligner=False):
    from cutadapt_amd import _lib
    return once(("plan", fam["name"], aligner), lambda: _lib.Plan([specs_of(fam, aligner)]))


def _lean_struct():
    import ctypes as C
    chars, lead, gated, gate_len, tw, dist = 128, 3, 6, 96, 4, 100

    class Lean(C.Structure):                                 # struct CahLeanFilter (cah_device.h); the size is checked
        _fields_ = [(k, C.c_int32) for k in ("ok", "n_lead", "n_gated", "n_tail", "tail_span", "head_span", "lead_delay")] + [
            ("lead_init", C.c_uint32 * lead), ("lead_found", C.c_uint32 * lead), ("lead_pass", C.c_uint32 * lead),
            ("gated_found", C.c_uint32 * gated), ("gated_span", C.c_int32 * gated),
            ("lead_mask", C.c_uint32 * chars * lead), ("gated_mask", C.c_uint32 * chars * gated),
            ("gate_init", C.c_uint32 * gate_len * gated), ("tw_ok", C.c_int32), ("n_tw", C.c_int32),
            ("tw_span", C.c_int32 * tw), ("tw_init", C.c_uint32 * tw), ("tw_pass", C.c_uint32 * tw),
            ("tw_mask", C.c_uint32 * chars * tw), ("tw_found", C.c_uint32 * dist * tw)]
    return Lean


def _matcher_ints(plan):
    """(skip_ok, narrow_words) of struct CahMatcher (cah_device.h): behind twelve ints and two arrays of CAH_MAX_M + 1"""
    import ctypes as C
    import struct
    from cutadapt_amd import _lib
    L = _lib.lib()
    need = C.c_size_t(0)
    _lib.check(L.cah_plan_debug_matcher(plan.handle, 0, None, 0, C.byref(need)))
    buf = (C.c_uint8 * need.value)()
    _lib.check(L.cah_plan_debug_matcher(plan.handle, 0, buf, need.value, C.byref(need)))
    ints = struct.unpack_from("<12i", bytes(buf), 0)
    both = struct.unpack_from("<2i", bytes(buf), 4 * (12 + 2 * 65))
    # the layout is the one assumed: the fields around the two have the values the plan was made with
    sp = plan.specs[0]
    longest = max(len(k) for _, _, kmers in sp.kmer_sets for k in kmers)
    assert ints[11] == plan.n_kmer_entries() and ints[9] == 1 and ints[1] == len(sp.sequence), ints
    assert (ints[3], ints[5]) == (sp.flags, sp.min_overlap) or sp.kind == _lib.KIND_KMER_ONLY, ints
    assert both[0] in (0, 1) and both[1] == (1 if longest <= 32 else 0), both
    return both


def skip_ok(plan):
    return _matcher_ints(plan)[0]


def routing_of(plan):
    """what the library says about the plan's prefilter, in the form of a tag"""
    import ctypes as C
    from cutadapt_amd import _lib
    L = _lib.lib()
    kind = plan.prefilter_kind()
    if kind == "general":
        return general(_matcher_ints(plan)[1] == 1, plan.n_kmer_entries())
    assert kind == "lean", kind
    Lean = _lean_struct()
    need = C.c_size_t(0)
    _lib.check(L.cah_plan_debug_lean(plan.handle, 0, None, 0, C.byref(need)))
    assert need.value == C.sizeof(Lean), (need.value, C.sizeof(Lean))
    lf = Lean()
    _lib.check(L.cah_plan_debug_lean(plan.handle, 0, C.byref(lf), need.value, C.byref(need)))
    assert lf.ok == 1
    # the layout is the one assumed: the spans say what the plan's sets say
    sets = plan.specs[0].kmer_sets
    assert lf.tail_span == max([-a for a, b, _ in sets if a < 0] + [0]), lf.tail_span
    assert lf.head_span == max([b for a, b, _ in sets if b] + [0]), lf.head_span
    assert lf.n_tail <= lf.n_gated <= 6 and lf.n_lead <= 3 and lf.tw_ok in (0, 1) and 0 <= lf.n_tw <= 4
    return lean(lf.n_lead, lf.n_gated, lf.n_tail, lf.lead_delay, lf.tw_ok, lf.n_tw)


# ---- which kernel -------------------------------------------------------------------------------------------------------

STREAM_MAX_LEN, STREAM2_MAX_LEN = 160, 640


def kernels(fam, mode, layout="ragged", n=0, n_reads=0, env=()):
    """the kernel that serves a batch of the family (kernels.hip: launch_filter, launch_filter_lean; api.cpp: run_filter).
    mode 0: cah_kmers_present_batch (never told that a batch is uniform: always the ragged variant), mode 1: the prefilter
    of cah_match_batch*.  layout 'uniform': equally long packed reads of n characters (cah_match_batch_uniform, or a packed
    batch that the device-side check finds uniform); 'ragged': anything else, d_lens views included."""
    t = fam["tag"]
    if t["kind"] == "general":
        return "k_filter<%d,%s,%s>" % (mode, "lds" if t["lds"] else "hbm", "narrow" if t["narrow"] else "wide")
    inst = "%d,%d,%d" % (t["lead_delay"], t["cls"][0], t["cls"][1])
    if layout != "uniform" or mode == 0:
        return "k_filter_lean<ragged,%s>" % inst
    no_stream, no_stream2 = "CAH_NO_STREAM" in env, "CAH_NO_STREAM2" in env
    big = n_reads * n >= 16
    if t["tw_ok"] and t["n_lead"] <= 2 and t["n_tw"] <= 4 and not no_stream and not no_stream2:
        return "k_filter_stream2" if (1 <= n <= STREAM2_MAX_LEN and big) else "k_filter_lean<uniform,%s>" % inst
    if not no_stream and n <= STREAM_MAX_LEN and big:
        return "k_filter_stream<%s>" % inst
    return "k_filter_lean<uniform,%s>" % inst


def required_kernels():
    """what the suite has to name in at least one routing assertion"""
    need = {"k_filter<%d,%s,%s>" % (m, l, w) for m in (0, 1) for l in ("lds", "hbm") for w in ("narrow", "wide")}
    for c in ((1, 2), (2, 3), (2, 6), (3, 6)):
        for d in (3, 0):
            need |= {"k_filter_lean<%s,%d,%d,%d>" % (v, d, c[0], c[1]) for v in ("ragged", "uniform")}
    return need | {"k_filter_stream", "k_filter_stream2"}
