// multi_route_model.cpp -- the product's multi_route.h behind a C interface, compiled with g++: the route of a batch, the
// arithmetic of the streaming form's page pool and the layout of the path's scratch, asked without a device
// (tests/test_multi_route_model.py; multi_route_sanitize.cpp walks the same grids under the sanitizers).
// TEST INFRASTRUCTURE ONLY: the product never loads this file.
#include "../../cutadapt_amd/csrc/multi_route.h"

// stand-ins for multi2.hip's: a table set whose header says ok == 1 takes 16 .. 160 characters, ok == 2 marks one that refuses
bool multi2_read_len_ok(const CahMulti2Header& h, int n) { return h.ok == 1 && n >= 16 && n <= 160; }
int multi2_tile_reads() { return 1024; }

namespace {

// form_case: 0 none, 1 one shape with tables, 2 one shape without, 3 mixed, 4 groups of one length, 5 groups of mixed
// lengths (three groups); refuse: one table set (the last group's) does not take the batch's length
MultiPlan plan_of(int form_case, bool refuse) {
    MultiPlan mp;
    const int ok = refuse ? 2 : 1;
    if (form_case == 1 || form_case == 2) {
        mp.form = M_ONE_SHAPE; mp.one_length = true; mp.hdr.ok = 1;
        if (form_case == 1) mp.m2.hdr.ok = ok;
    } else if (form_case == 3) {
        mp.form = M_MIXED; mp.m2.hdr.ok = ok; mp.m2.hdr.mixed = 1;
    } else if (form_case >= 4) {
        mp.form = M_GROUPS; mp.one_length = form_case == 4;
        mp.groups.resize(3);
        for (int g = 0; g < 3; g++) { mp.groups[(size_t)g].base = 64 * g; mp.groups[(size_t)g].count = 64; mp.groups[(size_t)g].m2.hdr.ok = 1; }
        mp.groups[2].m2.hdr.ok = ok;
    }
    return mp;
}

// layout: 0 uniform, 1 ragged with a lengths array (no frame), 2 views of a uniform batch, 3 frames anywhere, 4 suffix-only,
// 5 a packed batch (offsets alone)
MultiBatch batch_of(int layout, int len, bool ws_fits) {
    MultiBatch b;
    b.ws_fits = ws_fits;
    b.has_lens = layout >= 1 && layout <= 4;
    if (layout == 0 || layout >= 2) b.ul.len = layout == 5 ? 0 : len;
    b.ul.suffix = layout >= 2 && layout <= 4;
    b.ul.inner = layout == 2 || layout == 3;
    b.ul.general = layout == 3;
    return b;
}

}  // namespace

extern "C" {

// switches: bit 0 CAH_NO_MULTI, 1 CAH_NO_MULTI2, 2 CAH_NO_MULTI2_VIEWS, 3 CAH_NO_MULTI_MIXED, 4 CAH_NO_MULTI_GROUPS.
// out: path, then the layout's len, suffix, inner, general
void mr_route(int form_case, int refuse, int layout, int len, int ws_fits, int switches, int32_t* out) {
    MultiSwitches sw;
    sw.no_multi = switches & 1; sw.no_multi2 = switches & 2; sw.no_multi2_views = switches & 4;
    sw.no_multi_mixed = switches & 8; sw.no_multi_groups = switches & 16;
    const MultiRoute r = multi_route(plan_of(form_case, refuse != 0), batch_of(layout, len, ws_fits != 0), sw);
    out[0] = r.path; out[1] = r.ul.len; out[2] = r.ul.suffix; out[3] = r.ul.inner; out[4] = r.ul.general;
}

int64_t mr_pages_per_tile(int64_t A) { return m2_pages_per_tile(A); }
int64_t mr_block_reserve(int64_t A) { return m2_block_reserve(A); }
int64_t mr_pages_worst(int64_t A, int64_t n_reads) { return m2_pages_worst(A, n_reads); }
int64_t mr_pair_cap(int64_t limit, int64_t A, int64_t n_reads, int has_tables) { return m2_pair_cap(limit, A, n_reads, has_tables != 0); }
int64_t mr_pool_pages(int64_t cap) { return m2_pool_pages(cap); }

// out: grid, gate, rounds, ungated
void mr_pool_shape(int64_t Ag, int64_t cnt, int64_t max_pages, int n_cus, int ungated, int64_t* out) {
    const M2PoolShape sh = m2_pool_shape(Ag, cnt, max_pages, n_cus, ungated != 0);
    out[0] = sh.grid; out[1] = sh.gate; out[2] = sh.rounds; out[3] = sh.ungated;
}

// a plan of G groups of counts[g] adapters (G == 1: a plan of one table set)
int mr_one_launch_for_all(const int32_t* counts, int G, int64_t n_reads, int64_t max_pages, int n_cus, int ungated) {
    MultiPlan mp;
    int n_plan = 0;
    for (int g = 0; g < G; g++) n_plan += counts[g];
    if (G == 1) { mp.form = M_ONE_SHAPE; mp.m2.hdr.ok = 1; }
    else {
        mp.form = M_GROUPS;
        mp.groups.resize((size_t)G);
        for (int g = 0, at = 0; g < G; at += counts[g], g++) { mp.groups[(size_t)g].base = at; mp.groups[(size_t)g].count = counts[g]; }
    }
    return m2_one_launch_for_all(mp, n_plan, n_reads, max_pages, n_cus, ungated != 0) ? 1 : 0;
}

// off: where the five regions begin, and the scratch's size.  Returns 1 when a MultiScratch over a real buffer of that size
// puts its pointers there (asked for sizes of up to 64 MB), 0 when it does not, 2 when the size was not tried
int mr_scratch(int64_t cap, int64_t n_reads, uint64_t* off) {
    size_t o[6];
    MultiScratch::offsets(cap, n_reads, o);
    for (int i = 0; i < 6; i++) off[i] = o[i];
    if (MultiScratch::bytes(cap, n_reads) != o[5]) return 0;
    if (o[5] > ((size_t)64 << 20)) return 2;
    std::vector<char> buf(o[5]);
    const MultiScratch sc(buf.data(), cap, n_reads);
    return (char*)sc.best_key == buf.data() + o[0] && (char*)sc.pairs == buf.data() + o[1] && (char*)sc.dpq == buf.data() + o[2] &&
           (char*)sc.win == buf.data() + o[3] && (char*)sc.wmeta == buf.data() + o[4];
}

}  // extern "C"
