"""The host side of the multi-adapter path without a GPU (cutadapt_amd/csrc/multi_route.h): which path a batch of a plan
takes and with which layout, how the streaming form's page pool is cut into grid, gate and rounds, where the path's scratch
lies -- tests/host_model/multi_route_model.cpp compiles the product's header with g++.

The expectations of the first three tests are Python transcriptions of the expressions api.cpp held before the header
existed (cah_plan_multi_kind, multi_streams, the head of match_batch_impl and of match_batch_multi_once, the shape_of
lambda, cah_plan_workspace_bytes), not calls into the header.  The last test asks the real library, on this machine, for
what its plans say (multi_kind, multi_groups, workspace sizes, the switches at plan creation and afterwards): literals
recorded from the library as it was before the routes moved into the header."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_gpu_multi import env
from test_multi2_groups_model import capacity_plan, mixed_adapters

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_model", "multi_route_model.cpp")
SO = os.path.join(HERE, "host_model", "libmulti_route_model.so")
CSRC = os.path.join(HERE, "..", "cutadapt_amd", "csrc")

SEQUENTIAL, FUSED, STREAM = 0, 1, 2                             # include/cutadapt_hip.h: CAH_MULTI_*
PAGE, CLASSES, TILE = 1024, 6, 1024                             # multi2.h: CAH_M2_PAGE, CAH_M2_PAIR_CLASSES; multi2.hip: M2_TILE


@pytest.fixture(scope="module")
def model():
    deps = [SRC] + [os.path.join(CSRC, h) for h in ("multi_route.h", "cah_device.h", "multi2.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    i64, i32, vp = C.c_int64, C.c_int32, C.c_void_p
    L.mr_route.argtypes = [i32, i32, i32, i32, i32, i32, vp]
    L.mr_route.restype = None
    for name, n_args in (("mr_pages_per_tile", 1), ("mr_block_reserve", 1), ("mr_pages_worst", 2), ("mr_pool_pages", 1)):
        getattr(L, name).argtypes = [i64] * n_args
        getattr(L, name).restype = i64
    L.mr_pair_cap.argtypes = [i64, i64, i64, i32]
    L.mr_pair_cap.restype = i64
    L.mr_pool_shape.argtypes = [i64, i64, i64, i32, i32, vp]
    L.mr_pool_shape.restype = None
    L.mr_one_launch_for_all.argtypes = [vp, i32, i64, i64, i32, i32]
    L.mr_scratch.argtypes = [i64, i64, vp]
    return L


# ---- 1. the route table -------------------------------------------------------------------------------------------
FORMS = ("none", "one shape with tables", "one shape without tables", "mixed", "groups of one length", "groups of mixed lengths")
LAYOUTS = ("uniform", "ragged with lengths", "views", "frames", "suffix-only", "packed")
PLAIN = (0, False, False, False)                                # UniformLayout(): len, suffix, inner, general


def read_len_ok(table_ok, n):
    """the model's stand-in for multi2_read_len_ok"""
    return table_ok == 1 and 16 <= n <= 160


def route_before(form, refuse, layout, length, ws_multi, switches):
    """(path, layout the path gets) as api.cpp decided it, in five places, before multi_route.h"""
    NO_MULTI, NO_MULTI2, NO_VIEWS, NO_MIXED, NO_GROUPS = (bool(switches >> i & 1) for i in range(5))
    # the plan's flags
    hdr_ok = form in (1, 2)
    mixed = form >= 3                                           # (set on groups too: "no fused form behind the groups")
    groups = form >= 4
    groups_one_length = form == 4
    tables = [1, 1, 2 if refuse else 1] if groups else ([2 if refuse else 1] if form in (1, 3) else [])
    m2_ok = bool(tables) and not groups
    # the batch: (len, suffix, inner, general), d_lens, d_offsets
    ul_in = {0: (length, False, False, False), 1: PLAIN, 2: (length, True, True, False), 3: (length, True, True, True),
             4: (length, True, False, False), 5: PLAIN}[layout]
    d_lens = layout in (1, 2, 3, 4)
    d_offsets = layout != 0

    def multi_streams(ul):
        views = ul[2] and d_lens and d_offsets
        if not tables or ul[0] <= 0 or not (not d_lens or (views and not NO_VIEWS)) or NO_MULTI2:
            return False
        if groups and NO_GROUPS:
            return False
        return all(read_len_ok(t, ul[0]) for t in tables)

    # match_batch_impl
    multi_form = hdr_ok and ws_multi
    ul_multi = ul_in if (ul_in[2] and d_lens) else (PLAIN if ul_in[1] else ul_in)
    mixed_go = mixed and ws_multi and multi_streams(ul_multi) and not (NO_MIXED and not groups_one_length) and not NO_MULTI
    demoted = ul_in[3] and multi_form and not (m2_ok and read_len_ok(tables[0], ul_in[0]) and not NO_MULTI2 and not NO_VIEWS)
    ul = PLAIN if demoted else ul_in
    ul_rest = PLAIN if ul[1] else ul
    if not (multi_form or mixed_go):
        return SEQUENTIAL, ul                                   # (the loop's prefilter gets ul, its other kernels ul_rest)
    # match_batch_multi_once
    ul = ul if (ul[2] and d_lens) else ul_rest
    if multi_streams(ul):
        return STREAM, ul
    assert not mixed, "a mixed plan has no fused form for this batch"
    return FUSED, (PLAIN if ul[2] else ul)


def kind_before(form, refuse, read_len, switches):
    """cah_plan_multi_kind before multi_route.h"""
    NO_MULTI, NO_MULTI2, _NO_VIEWS, NO_MIXED, NO_GROUPS = (bool(switches >> i & 1) for i in range(5))
    groups = form >= 4
    tables = [1, 1, 2 if refuse else 1] if groups else ([2 if refuse else 1] if form in (1, 3) else [])
    if form >= 3:
        len_ok = bool(tables) and all(read_len_ok(t, read_len) for t in tables)
        off = NO_MULTI2 or NO_MULTI or (groups and NO_GROUPS) or (form != 4 and NO_MIXED)
        return STREAM if (len_ok and not off) else SEQUENTIAL
    if form == 0:
        return SEQUENTIAL
    return STREAM if (form == 1 and read_len_ok(tables[0], read_len) and not NO_MULTI2) else FUSED


def test_every_route(model):
    out = np.zeros(5, dtype=np.int32)
    seen = set()
    for form, refuse, layout, length, fits, sw in itertools.product(range(6), (0, 1), range(6), (150, 200), (0, 1), range(32)):
        model.mr_route(form, refuse, layout, length, fits, sw, out.ctypes.data)
        got = (int(out[0]), (int(out[1]), bool(out[2]), bool(out[3]), bool(out[4])))
        want = route_before(form, refuse, layout, length, bool(fits), sw)
        what = (FORMS[form], "one table set refuses" if refuse else "", LAYOUTS[layout], length, "fits" if fits else "small workspace", f"{sw:05b}")
        assert got == want, (what, got, want)
        if layout == 0 and fits:
            assert got[0] == kind_before(form, refuse, length, sw), what
        seen.add((form, got[0]))
    # every form reaches every path it has
    assert seen == {(0, SEQUENTIAL), (1, SEQUENTIAL), (1, FUSED), (1, STREAM), (2, SEQUENTIAL), (2, FUSED), (3, SEQUENTIAL), (3, STREAM),
                    (4, SEQUENTIAL), (4, STREAM), (5, SEQUENTIAL), (5, STREAM)}
    # the route nothing else pins: frames of a one-shape plan that do not stream are the plain views they are, on the fused kernels
    for length, sw in ((200, 0), (150, 4)):
        model.mr_route(1, 0, 3, length, 1, sw, out.ctypes.data)
        assert out.tolist() == [FUSED, 0, 0, 0, 0]
    # the two asymmetries: CAH_NO_MULTI at call time means mixed and grouped plans only; CAH_NO_MULTI_MIXED not groups of one length
    for form, sw, path in ((1, 1, STREAM), (3, 1, SEQUENTIAL), (4, 1, SEQUENTIAL), (3, 8, SEQUENTIAL), (5, 8, SEQUENTIAL), (4, 8, STREAM)):
        model.mr_route(form, 0, 0, 150, 1, sw, out.ctypes.data)
        assert out[0] == path, (FORMS[form], sw)


# ---- 2. the pool ---------------------------------------------------------------------------------------------------
def pages_per_tile(A):
    return (1024 * A + (PAGE - 64)) // (PAGE - 63)


def block_reserve(A):
    return 3 * pages_per_tile(A) + 16 * CLASSES


def pages_worst(A, n_reads):
    tiles = (n_reads + 1023) // 1024
    return tiles * pages_per_tile(A) + min(max(tiles, 1), 512) * 16 * CLASSES + 2


def pair_cap_before(limit, A, n_reads, has_tables):
    """multi_pair_cap below the environment and device lookup"""
    limit = min(limit, (1 << 31) - 4 * PAGE)
    limit = max(limit, A)
    fused = min(n_reads * A, limit)
    if not has_tables:
        return fused
    floor_pages = 2 * block_reserve(A) + 2 * pages_per_tile(A)
    pages = min(pages_worst(A, n_reads), max(limit // PAGE, floor_pages))
    return max(fused, pages * PAGE + pages // 2 + 2)


def pool_pages(cap):
    return (cap * 8) // (PAGE * 8 + 4)


def shape_before(Ag, cnt, max_pages, n_cus, ungated):
    """the shape_of lambda of match_batch_multi_once: (grid, gate, rounds, ungated)"""
    per_tile, open_pages = pages_per_tile(Ag), 16 * CLASSES
    n_tiles = (cnt + TILE - 1) // TILE
    grid, gate, rounds = min(n_tiles, n_cus), max_pages, 1
    if n_tiles * per_tile + grid * open_pages > max_pages:
        grid = max(1, min(grid, (max_pages // 2) // block_reserve(Ag)))
        gate = max_pages - grid * block_reserve(Ag)
        sure = max(1, int((gate - grid * open_pages) / per_tile))         # (C++ division: towards zero)
        rounds = (n_tiles + sure - 1) // sure
    if ungated:
        gate, rounds = 1 << 60, 1
    return grid, gate, rounds, bool(ungated)


POOL_GRID = list(itertools.product((1, 8, 96, 128), (1, 1023, 1024, 1025, 10 ** 6, 2 ** 30), (1, 256)))


def pool_sizes(Ag, cnt):
    """the floor multi_pair_cap guarantees, the batch's worst case, one value halfway"""
    lo = pool_pages(pair_cap_before(1, Ag, cnt, True))
    worst = pages_worst(Ag, cnt)
    return lo, (lo + worst) // 2, worst


def test_pool_shapes(model):
    out = np.zeros(4, dtype=np.int64)
    gated = ungated_seen = several_rounds = 0
    for Ag, cnt, n_cus in POOL_GRID:
        assert model.mr_pages_per_tile(Ag) == pages_per_tile(Ag) and model.mr_block_reserve(Ag) == block_reserve(Ag)
        assert model.mr_pages_worst(Ag, cnt) == pages_worst(Ag, cnt)
        for limit, has_tables in itertools.product((1, 50_000_000, 1 << 40), (0, 1)):
            cap = pair_cap_before(limit, Ag, cnt, has_tables)
            assert model.mr_pair_cap(limit, Ag, cnt, has_tables) == cap, (limit, Ag, cnt, has_tables)
            assert model.mr_pool_pages(cap) == pool_pages(cap)
            if has_tables:                                       # the pages and their header words fit the pair area
                assert pool_pages(cap) * (PAGE * 8 + 4) <= cap * 8
        for max_pages, ungated in itertools.product(pool_sizes(Ag, cnt), (0, 1)):
            what = (Ag, cnt, n_cus, max_pages, ungated)
            model.mr_pool_shape(Ag, cnt, max_pages, n_cus, ungated, out.ctypes.data)
            grid, gate, rounds, ung = (int(x) for x in out)
            assert (grid, gate, rounds, bool(ung)) == shape_before(Ag, cnt, max_pages, n_cus, ungated), what
            # what the kernels rely on
            n_tiles = (cnt + TILE - 1) // TILE
            assert 1 <= grid <= n_cus, what
            if ungated:
                assert rounds == 1, what
                ungated_seen += 1
            elif gate != max_pages:
                assert gate + grid * block_reserve(Ag) <= max_pages, what
                sure = max(1, int((gate - grid * 16 * CLASSES) / pages_per_tile(Ag)))
                assert rounds * sure >= n_tiles, what
                gated += 1
                several_rounds += rounds > 1
            else:
                assert rounds == 1 and n_tiles * pages_per_tile(Ag) + grid * 16 * CLASSES <= max_pages, what
    assert gated > 20 and several_rounds > 10 and ungated_seen > 100, (gated, several_rounds, ungated_seen)


def test_one_launch_for_all(model):
    yes = no = 0
    for (Ag, cnt, n_cus), ungated in itertools.product(POOL_GRID, (0, 1)):
        for counts in ([Ag], [Ag, 8, 128], [128, Ag]):
            for max_pages in pool_sizes(max(counts), cnt):
                shapes = [shape_before(c, cnt, max_pages, n_cus, ungated) for c in counts]
                want = all(rounds == 1 and (gate == max_pages or ung) for _grid, gate, rounds, ung in shapes)
                arr = np.array(counts, dtype=np.int32)
                got = model.mr_one_launch_for_all(arr.ctypes.data, len(counts), cnt, max_pages, n_cus, ungated)
                assert bool(got) == want, (counts, cnt, n_cus, max_pages, ungated)
                yes += want
                no += not want
    assert yes > 50 and no > 50, (yes, no)


# ---- 3. the scratch ------------------------------------------------------------------------------------------------
def test_scratch_layout(model):
    off = np.zeros(6, dtype=np.uint64)
    for cap, n_reads in itertools.product((1, 4095, 2 ** 31 - 4 * PAGE), (0, 1, 255, 256, 257, 10 ** 8)):
        rc = model.mr_scratch(cap, n_reads, off.ctypes.data)
        assert rc in (1, 2), (cap, n_reads)                      # (1: the constructor's pointers were compared too)
        assert rc == 1 or int(off[5]) > 64 << 20
        o = [int(x) for x in off]
        ws_key_bytes = (8 * n_reads + 255) & ~255
        ws_keys_bytes = (n_reads + 255) & ~255
        # cah_plan_workspace_bytes' formula
        assert o[5] == ws_key_bytes + cap * 20 + 2 * ws_keys_bytes + 256, (cap, n_reads)
        # best keys (8 per read), pairs (8 per pair), DP list (4), its windows (8), a 16-bit word per read: one behind the other
        sizes = (8 * n_reads, 8 * cap, 4 * cap, 8 * cap, 2 * n_reads)
        assert o[0] == 0
        for i in range(5):
            assert o[i] + sizes[i] <= o[i + 1], (cap, n_reads, i)
        assert o[1] % 256 == 0 and o[4] % 4 == 0


# ---- the real library, no device -----------------------------------------------------------------------------------
SWITCHES = ("CAH_NO_MULTI", "CAH_NO_MULTI2", "CAH_NO_MULTI2_VIEWS", "CAH_NO_MULTI_MIXED", "CAH_NO_MULTI_GROUPS")
KIND_LENGTHS = (15, 16, 80, 81, 150, 160, 161, 1000)
WS_READS = (0, 1, 1024, 1025, 10 ** 6, 10 ** 8)
PAIR_CAPS = ("1", "50000000")


def abi_plans():
    """name -> (adapters, rate)"""
    rng = np.random.default_rng(20261)
    return {
        "4 adapters": (mixed_adapters(rng, 4, 33, 33), 0.1),
        "96 x 33": (mixed_adapters(rng, 96, 33, 33), 0.1),
        "12 of 20..40": (mixed_adapters(rng, 12, 20, 40), 0.1),
        "160 x 20": (mixed_adapters(rng, 160, 20, 20), 0.1),
        "200 of 20..40": (mixed_adapters(rng, 200, 20, 40), 0.1),
        "capacity split": capacity_plan(np.random.default_rng(7096)),
    }


def _plan(adapters, rate):
    from cutadapt_amd import _lib
    from cutadapt_amd import adapters as A
    return _lib.Plan([A.BackAdapter(s, max_errors=rate, min_overlap=3).matcher_spec() for s in adapters])


def _kinds(plan):
    """one letter per length of KIND_LENGTHS"""
    return "".join({"sequential": "q", "fused": "f", "stream": "S"}[plan.multi_kind(n)] for n in KIND_LENGTHS)


def _workspaces(plan):
    from cutadapt_amd import _lib
    out = []
    for cap in PAIR_CAPS:
        with env(CAH_MULTI_PAIR_CAP=cap):
            out.append([int(_lib.lib().cah_plan_workspace_bytes(plan.handle, n)) for n in WS_READS])
    return out


def abi_observe():
    """what the library says about the plans: kinds, groups, workspace sizes; with every switch set before the plan is made
    (kinds, groups, the workspace for 1 025 reads) and set only afterwards (kinds)"""
    seen = {}
    clean = {k: None for k in SWITCHES + ("CAH_MULTI_MIN", "CAH_MULTI_MIXED_MIN", "CAH_MULTI_PAIR_CAP")}
    with env(**clean):
        for name, (adapters, rate) in abi_plans().items():
            plan = _plan(adapters, rate)
            rec = {"kinds": _kinds(plan), "groups": plan.multi_groups(), "workspace": _workspaces(plan), "before": {}, "after": {}}
            for sw in SWITCHES:
                with env(**{sw: "1"}):
                    rec["after"][sw] = _kinds(plan)
                    early = _plan(adapters, rate)
                    rec["before"][sw] = [_kinds(early), early.multi_groups(), _workspaces(early)[0][3]]
                # ... and a plan made under the switch, asked without it
                rec["before"][sw].append(_kinds(early))
            seen[name] = rec
    return seen


Q8 = "qqqqqqqq"
OFF = [Q8, 0, 25856, Q8]                                        # no multi-adapter form was built: the base workspace


def _abi(kinds, groups, ws_small, ws_large, ws_1025, before, after):
    """`before` / `after`: what differs from "the switch changes nothing" ([kinds, groups, ws_1025, kinds] / kinds)"""
    same = [kinds, groups, ws_1025, kinds]
    return {"kinds": kinds, "groups": groups,
            "workspace": [ws_small + [ws_1025] + ws_large[:2], ws_small + [ws_1025] + ws_large[2:]],
            "before": {sw: before.get(sw, same) for sw in SWITCHES}, "after": {sw: after.get(sw, kinds) for sw in SWITCHES}}


BIG = [1028118400, 3762992768]                                  # 10^6 and 10^8 reads under a cap of 50 M pairs
ABI_EXPECTED = {
    "4 adapters": {"kinds": Q8, "groups": 0, "workspace": [[6400, 7680, 24576, 25856, 17632000, 1762506752]] * 2,
                   "before": {sw: OFF for sw in SWITCHES}, "after": {sw: Q8 for sw in SWITCHES}},
    "96 x 33": _abi("fSSSSSff", 1, [2014716, 4127224, 4153592], [48450520, 2783324888] + BIG, 8233160,
                    {"CAH_NO_MULTI": OFF, "CAH_NO_MULTI2": ["ffffffff", 0, 39040, "ffffffff"]}, {"CAH_NO_MULTI2": "ffffffff"}),
    "12 of 20..40": _abi("qSSqSSqq", 1, [2014716, 2283124, 2309492], [33697720, 2768572088] + BIG, 4544960,
                         {"CAH_NO_MULTI": OFF, "CAH_NO_MULTI2": OFF, "CAH_NO_MULTI_MIXED": OFF},
                         {"CAH_NO_MULTI": Q8, "CAH_NO_MULTI2": Q8, "CAH_NO_MULTI_MIXED": Q8}),
    "160 x 20": _abi("qSSSSSqq", 2, [2014716, 3778904, 3805272], [45663880, 2780538248] + BIG, 7536500,
                     {"CAH_NO_MULTI": OFF, "CAH_NO_MULTI2": OFF, "CAH_NO_MULTI_GROUPS": [Q8, 2, 7536500, "qSSSSSqq"]},
                     {"CAH_NO_MULTI": Q8, "CAH_NO_MULTI2": Q8, "CAH_NO_MULTI_GROUPS": Q8}),
    "200 of 20..40": _abi("qSSqSSqq", 4, [2014716, 3123224, 3149592], [40418440, 2775292808] + BIG, 6225140,
                          {"CAH_NO_MULTI": OFF, "CAH_NO_MULTI2": OFF, "CAH_NO_MULTI_MIXED": OFF,
                           "CAH_NO_MULTI_GROUPS": [Q8, 4, 6225140, "qSSqSSqq"]},
                          {"CAH_NO_MULTI": Q8, "CAH_NO_MULTI2": Q8, "CAH_NO_MULTI_MIXED": Q8, "CAH_NO_MULTI_GROUPS": Q8}),
    "capacity split": _abi("qSSqSSqq", 2, [2014716, 3082244, 3108612], [40090600, 2774964968] + BIG, 6143180,
                           {"CAH_NO_MULTI": OFF, "CAH_NO_MULTI2": OFF, "CAH_NO_MULTI_MIXED": OFF,
                            "CAH_NO_MULTI_GROUPS": [Q8, 2, 6143180, "qSSqSSqq"]},
                           {"CAH_NO_MULTI": Q8, "CAH_NO_MULTI2": Q8, "CAH_NO_MULTI_MIXED": Q8, "CAH_NO_MULTI_GROUPS": Q8}),
}


def test_plans_through_the_library():
    seen = abi_observe()
    assert set(seen) == set(ABI_EXPECTED)
    for name, rec in seen.items():
        for key, want in ABI_EXPECTED[name].items():
            assert rec[key] == want, (name, key, rec[key], want)


if __name__ == "__main__":
    import pprint
    pprint.pprint(abi_observe(), width=150, sort_dicts=False)
