// multi_route.h -- the HOST side of the multi-adapter path that needs no device: which form a plan has, which path a batch
// of it takes, how the page pool of the streaming form is cut and where the path's scratch lies.  No HIP in here: api.cpp
// includes it, and so does tests/host_model/multi_route_model.cpp under plain g++ (tests/test_multi_route_model.py).
//
// THE ROUTE of a batch (multi_route): one of the three paths of include/cutadapt_hip.h, decided once per call.
//
//   "streams" below: the plan has table sets (n_tables() > 0), the layout has a length (a uniform batch, or views / frames
//   of a uniform or frame length -- a lengths array WITHOUT such a length never streams), EVERY table set takes that length
//   (multi2_read_len_ok), and none of CAH_NO_MULTI2, CAH_NO_MULTI2_VIEWS (views and frames only) and CAH_NO_MULTI_GROUPS
//   (groups only) says no.
//
//   plan's form    workspace holds   switched off          streams   path         layout the path gets
//   -------------  ----------------  --------------------  --------  -----------  ---------------------------------------
//   M_NONE         any               --                    --        SEQUENTIAL   the caller's
//   any other      no                --                    --        SEQUENTIAL   the caller's
//   M_ONE_SHAPE    yes               (never, see i)        yes       STREAM       the caller's; suffix-only: plain views
//   M_ONE_SHAPE    yes               (never, see i)        no        FUSED        uniform: the caller's; else plain views
//   M_MIXED        yes               NO_MULTI, NO_MIXED    --        SEQUENTIAL   the caller's
//   M_GROUPS       yes               NO_MULTI, NO_MIXED*   --        SEQUENTIAL   the caller's      (* see ii)
//   M_MIXED/GROUPS yes               no                    yes       STREAM       the caller's; suffix-only: plain views
//   M_MIXED/GROUPS yes               no                    no        SEQUENTIAL   the caller's (no fused kernels behind them)
//
//   "plain views" is UniformLayout(): starts and lengths, nothing known about a parent.  Frames that do not stream (a frame
//   length no table set takes, CAH_NO_MULTI2_VIEWS=1) are thereby demoted to the plain views they are.  On the SEQUENTIAL
//   path the layout is the prefilter's; every other kernel of the loop sees a suffix-only layout as plain views.
//
//   Two asymmetries, kept as they are:
//   (i)  a one-shape plan honours CAH_NO_MULTI at plan creation only (build_multi then builds no form: M_NONE); a mixed or
//        grouped plan honours it there AND at every call.
//   (ii) CAH_NO_MULTI_MIXED does not apply to groups whose adapters are all equally long (one_length).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/cutadapt_hip.h"
#include "cah_device.h"
#include "multi2.h"

// multi2.hip's (kernels.h declares them for the library; a host model brings stand-ins of its own)
bool multi2_read_len_ok(const CahMulti2Header& h, int read_len);
int multi2_tile_reads();

// the form build_multi gave a plan's adapters
enum MultiForm {
    M_NONE,          // no multi-adapter form: the per-adapter loop
    M_ONE_SHAPE,     // adapters of one shape (hdr.ok): the fused kernels, and the streaming tables in m2 where m2.hdr.ok
    M_MIXED,         // adapters of different lengths in ONE table set (m2, m2_build_mixed); no fused kernels behind it
    M_GROUPS         // more adapters or k-mers than one table set holds: `groups`; no fused kernels behind them
};

// host tables of the multi-adapter path (see CahMultiHeader)
struct MultiPlan {
    MultiForm form = M_NONE;
    bool one_length = false;              // the plan's adapters are all equally long
    CahMultiHeader hdr;                   // M_ONE_SHAPE (hdr.ok stays 0 otherwise: the older fused kernels are one-shape)
    std::vector<CahMultiDir> dir;
    std::vector<CahMultiEntry> entries;
    std::vector<uint32_t> bitmap;
    std::vector<uint64_t> scan_tab, row_tab;   // every form but M_NONE; a grouped plan's are indexed from the group's base
    M2Tables m2;                          // M_ONE_SHAPE, M_MIXED: the streaming form's tables (m2.hdr.ok: there are some)
    int longest = 0;                      // M_MIXED, M_GROUPS: the (first) longest adapter: word form, ROWS and thr_last come from it
    // M_GROUPS (multi2.h: m2_build_groups): every group has tables of its own over the adapters [base, base + count)
    struct Group { int base = 0, count = 0, longest = 0; M2Tables m2; };   // longest: the group's, as an index INSIDE it
    std::vector<Group> groups;
    MultiPlan() { memset(&hdr, 0, sizeof(hdr)); memset(&m2.hdr, 0, sizeof(m2.hdr)); }
    // the table sets a batch goes through, in order: the groups', or the one of a plan that fits a table (none: no streaming form)
    int n_tables() const { return !groups.empty() ? (int)groups.size() : (m2.hdr.ok ? 1 : 0); }
    const M2Tables& tables(int g) const { return groups.empty() ? m2 : groups[(size_t)g].m2; }
    int group_base(int g) const { return groups.empty() ? 0 : groups[(size_t)g].base; }
    int group_count(int g, int n_plan) const { return groups.empty() ? n_plan : groups[(size_t)g].count; }
    int group_longest(int g) const { return groups.empty() ? (form == M_MIXED ? longest : 0) : groups[(size_t)g].longest; }
    int largest_group(int n_plan) const {
        int c = groups.empty() ? n_plan : 0;
        for (const Group& g : groups) c = std::max(c, g.count);
        return c;
    }
};

// equally long reads the host vouches for (cah_match_batch_uniform): read r = d_seqs[first + r * len ..); len == 0: the
// packed layout (offsets / lens)
// suffix: (first, len) describe a PARENT batch of equally long reads and d_offsets / d_lens views that end where
// its reads end (cah_match_batch_suffix_views): only the streaming prefilter makes use of that, every other kernel
// sees plain views.
// inner (with suffix): the views may end before the parent's reads do (cah_match_batch_views)
// general (with inner): views anywhere in the buffer, len is a frame length (cah_match_batch_frames)
struct UniformLayout { int64_t first = 0; int32_t len = 0; bool suffix = false; bool inner = false; bool general = false; };

// the switches asked at every call (A/B measurements, parity tests), read by api.cpp
struct MultiSwitches {
    bool no_multi = false;                // CAH_NO_MULTI
    bool no_multi2 = false;               // CAH_NO_MULTI2
    bool no_multi2_views = false;         // CAH_NO_MULTI2_VIEWS
    bool no_multi_mixed = false;          // CAH_NO_MULTI_MIXED
    bool no_multi_groups = false;         // CAH_NO_MULTI_GROUPS
};

struct MultiBatch {
    UniformLayout ul;                     // the caller's layout
    bool has_lens = false;                // there is a lengths array (views, frames, a ragged batch of starts + lengths)
    bool ws_fits = false;                 // the workspace holds the plan's scratch (cah_plan_workspace_bytes)
};

struct MultiRoute {
    int path = CAH_MULTI_SEQUENTIAL;
    UniformLayout ul;                     // the layout that path gets (the table above)
};

inline MultiRoute multi_route(const MultiPlan& mp, const MultiBatch& b, const MultiSwitches& sw) {
    MultiRoute r;
    r.ul = b.ul;
    if (mp.form == M_NONE || !b.ws_fits) return r;
    const bool fused_behind = mp.form == M_ONE_SHAPE;
    if (!fused_behind && (sw.no_multi || (sw.no_multi_mixed && !mp.one_length))) return r;
    // views keep their layout (the streaming form takes them end-aligned); a suffix-only layout is no uniform batch here
    const bool views = b.ul.inner && b.has_lens;
    const UniformLayout ul = (views || !b.ul.suffix) ? b.ul : UniformLayout();
    bool streams = mp.n_tables() > 0 && ul.len > 0 && (!b.has_lens || (views && !sw.no_multi2_views)) && !sw.no_multi2 &&
                   !(mp.form == M_GROUPS && sw.no_multi_groups);
    for (int g = 0; streams && g < mp.n_tables(); g++) streams = multi2_read_len_ok(mp.tables(g).hdr, ul.len);
    if (streams) { r.path = CAH_MULTI_STREAM; r.ul = ul; }
    // (the older kernels take views through their starts and lengths alone)
    else if (fused_behind) { r.path = CAH_MULTI_FUSED; r.ul = ul.inner ? UniformLayout() : ul; }
    return r;
}

// What the mixed form and the groups of tables ask of a WHOLE plan's matchers: all scan-eligible with kacc == k, one
// min_overlap, agreement on thr[] and, row by row, on thr_last[].  longest: the (first) longest adapter; k_of[a] = kacc of
// adapter a.  (api.cpp asks the adapters' descriptions for the rest: plain-ACGT 3' adapters, whole-read or tail sets.)
inline bool m2_matchers_eligible(const CahMatcher* mts, int n, int& longest, std::vector<int>& k_of) {
    longest = 0;
    for (int a = 1; a < n; a++) if (mts[a].m > mts[longest].m) longest = a;
    const CahMatcher& ml = mts[longest];
    k_of.assign((size_t)n, 0);
    for (int a = 0; a < n; a++) {
        const CahMatcher& mt = mts[a];
        if (!mt.scan_ok || mt.m < 1 || mt.m > CAH_MAX_M || mt.kacc != mt.k || mt.min_overlap != ml.min_overlap) return false;
        if (memcmp(mt.thr, ml.thr, sizeof(mt.thr)) != 0) return false;
        for (int i = 0; i <= mt.m; i++) if (mt.thr_last[i] != ml.thr_last[i]) return false;
        k_of[(size_t)a] = mt.kacc;
    }
    return true;
}

// ---- the streaming form's pool (multi2.h: pages of CAH_M2_PAGE pairs, one class each).  A closed page may lack up to 63
// pairs; every wave of a block holds one open page per class; a block has at most three tiles in flight (its waves may
// straddle two, the third is drawn ahead).
inline int64_t m2_pages_per_tile(int64_t A) { return (1024 * A + (CAH_M2_PAGE - 64)) / (CAH_M2_PAGE - 63); }   // (multi2.hip: M2_TILE)
inline int64_t m2_block_reserve(int64_t A) { return 3 * m2_pages_per_tile(A) + 16 * CAH_M2_PAIR_CLASSES; }
inline int64_t m2_pages_worst(int64_t A, int64_t n_reads) {
    const int64_t tiles = (n_reads + 1023) / 1024;
    return tiles * m2_pages_per_tile(A) + std::min<int64_t>(std::max<int64_t>(tiles, 1), 512) * 16 * CAH_M2_PAIR_CLASSES + 2;
}

// Pairs the scratch has room for: what the batch can produce in the worst case (every adapter on every read), bounded
// by `limit` (api.cpp: CAH_MULTI_PAIR_CAP, or what the device's free memory allows).  A: the LARGEST group's adapters --
// groups of tables share the pool one after the other.  The fused form handles larger batches in chunks of cap / n_adapters
// reads; the streaming form in ROUNDS that end when the pool runs low (a typical batch of 100 M reads x 96 adapters has
// 0.45 G pairs and takes one).
inline int64_t m2_pair_cap(int64_t limit, int64_t A, int64_t n_reads, bool has_tables) {
    // (the cell DP's work list holds pair indices as int32: the pool never has 2^31 pairs or more, whatever the knob says)
    limit = std::min<int64_t>(limit, ((int64_t)1 << 31) - 4 * CAH_M2_PAGE);
    if (limit < A) limit = A;
    const int64_t fused = std::min(n_reads * A, limit);
    if (!has_tables) return fused;                          // (no streaming form for this plan: no page pool, no floor)
    // (one block of the streaming prefilter must always be able to run)
    const int64_t floor_pages = 2 * m2_block_reserve(A) + 2 * m2_pages_per_tile(A);
    const int64_t pages = std::min(m2_pages_worst(A, n_reads), std::max(limit / CAH_M2_PAGE, floor_pages));
    // (a page header word per page lives behind the pages, inside the pair area)
    return std::max(fused, pages * CAH_M2_PAGE + pages / 2 + 2);
}
// the pages a pair area of cap pairs holds: CAH_M2_PAGE pairs + one header word each
inline int64_t m2_pool_pages(int64_t cap) { return (cap * 8) / (CAH_M2_PAGE * 8 + 4); }

// The launch grid, the gate and the rounds of a group of Ag adapters on a block of cnt reads.  ungated: the dev library's
// CAH_TEST_M2_UNGATED (api.cpp reads it) takes the gate away to provoke the pool's overflow.
struct M2PoolShape { int64_t grid, gate, rounds; bool ungated; };
inline M2PoolShape m2_pool_shape(int64_t Ag, int64_t cnt, int64_t max_pages, int n_cus, bool ungated) {
    const int64_t per_tile = m2_pages_per_tile(Ag), open_pages = 16 * CAH_M2_PAIR_CLASSES;
    const int64_t TILE = multi2_tile_reads(), n_tiles = (cnt + TILE - 1) / TILE;
    M2PoolShape sh{std::min<int64_t>(n_tiles, n_cus), max_pages, 1, false};
    if (n_tiles * per_tile + sh.grid * open_pages > max_pages) {
        // the batch might not fit the pool: blocks stop drawing tiles once what is in flight could fill it, and
        // the rounds go on until the tiles are done -- `rounds` is the count for the worst case (every adapter on
        // every read); a round that finds no tile left costs four empty launches
        sh.grid = std::max<int64_t>(1, std::min(sh.grid, (max_pages / 2) / m2_block_reserve(Ag)));
        sh.gate = max_pages - sh.grid * m2_block_reserve(Ag);
        const int64_t sure = std::max<int64_t>(1, (sh.gate - sh.grid * open_pages) / per_tile);
        sh.rounds = (n_tiles + sure - 1) / sure;
    }
    if (ungated) { sh.gate = (int64_t)1 << 60; sh.rounds = 1; sh.ungated = true; }
    return sh;
}
// Does the pool hold the worst case of the whole batch for EVERY group, so that one launch per group draws every tile and
// the host has nothing to decide?  (The deferred error check holds only then, which must be known before the first group runs.)
inline bool m2_one_launch_for_all(const MultiPlan& mp, int n_plan, int64_t n_reads, int64_t max_pages, int n_cus, bool ungated) {
    for (int g = 0; g < mp.n_tables(); g++) {
        const M2PoolShape sh = m2_pool_shape(mp.group_count(g, n_plan), n_reads, max_pages, n_cus, ungated);
        if (!(sh.rounds == 1 && (sh.gate == max_pages || sh.ungated))) return false;
    }
    return true;
}

// ---- the scratch of the multi-adapter path, behind the base workspace (cah_plan_workspace_bytes):
// [best key per read] [pairs] [DP list] [its column windows] [streaming form: a 16-bit word per read, multi2.h]
// cap: m2_pair_cap's pairs
inline size_t ws_align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct MultiScratch {
    unsigned long long* best_key;
    uint64_t* pairs;
    int32_t* dpq;
    int32_t* win;
    uint16_t* wmeta;
    // per pair: the pair, its entry in the DP list, the entry's column window (two int32)
    static constexpr size_t pairs_bytes = sizeof(uint64_t), dpq_bytes = sizeof(int32_t), win_bytes = 2 * sizeof(int32_t);
    static constexpr size_t pair_bytes = pairs_bytes + dpq_bytes + win_bytes;
    // where the five regions begin and, [5], where the scratch ends
    static void offsets(int64_t cap, int64_t n_reads, size_t off[6]) {
        size_t p = 0;
        off[0] = p; p += ws_align256(sizeof(unsigned long long) * (size_t)n_reads);
        off[1] = p; p += pairs_bytes * (size_t)cap;
        off[2] = p; p += dpq_bytes * (size_t)cap;
        off[3] = p; p += win_bytes * (size_t)cap;
        off[4] = p; p += 2 * ws_align256((size_t)n_reads);
        off[5] = p + 256;
    }
    static size_t bytes(int64_t cap, int64_t n_reads) { size_t off[6]; offsets(cap, n_reads, off); return off[5]; }
    MultiScratch(char* extra, int64_t cap, int64_t n_reads) {
        size_t off[6];
        offsets(cap, n_reads, off);
        best_key = (unsigned long long*)(extra + off[0]);
        pairs = (uint64_t*)(extra + off[1]);
        dpq = (int32_t*)(extra + off[2]);
        win = (int32_t*)(extra + off[3]);
        wmeta = (uint16_t*)(extra + off[4]);
    }
};
