// multi2_groups_model.cpp -- HOST MODEL of GROUPS of tables in the streaming multi-adapter path: a plan of more adapters
// (129..1024) or more k-mers than one table set holds, cut by multi2.h's m2_build_groups into contiguous groups with a
// table set each.  TEST INFRASTRUCTURE ONLY: the product never loads this file.
//
// Every group is replayed with the existing model code, unchanged -- m2m_match_batch (multi2_model.cpp) for a group of one
// length, m2x_match_batch (multi2_mixed_model.cpp) otherwise -- over the group's own adapters; the groups' results are
// merged the way the kernels merge them: one key per match in the product's order (pack_best) with the adapter's index in
// the PLAN, group base + index inside the group, and the largest key wins.  tests/test_multi2_groups_model.py compares
// the merged result with the oracle's kmers_present + locate of every adapter on the whole read.
#include "multi2_mixed_model.cpp"

#include "../../cutadapt_amd/csrc/multi_route.h"

namespace {

struct Plan {
    std::vector<std::string> ads;
    std::vector<CahMatcher> mts;
    std::vector<std::vector<M2RefKmer>> ref;
    std::vector<int> k_of;
    int longest = 0;
    bool eligible = true;
};

Plan read_plan(const char* adapters, int A, const void* blobs, int32_t n_ref, const int32_t* ref_adapter,
               const int32_t* ref_window, const char* ref_kmers) {
    Plan p;
    const char* ap = adapters;
    for (int a = 0; a < A; a++) { p.ads.push_back(std::string(ap)); ap += strlen(ap) + 1; }
    p.mts.resize((size_t)A);
    memcpy(p.mts.data(), blobs, sizeof(CahMatcher) * (size_t)A);
    p.ref.resize((size_t)A);
    const char* kp = ref_kmers;
    for (int i = 0; i < n_ref; i++) {
        p.ref[(size_t)ref_adapter[i]].push_back({std::string(kp), ref_window[i]});
        kp += strlen(kp) + 1;
    }
    // what api.cpp asks of the whole plan's matchers before it builds groups (multi_route.h, the product's own)
    p.eligible = m2_matchers_eligible(p.mts.data(), A, p.longest, p.k_of);
    return p;
}

bool one_length(const std::vector<std::string>& ads) {
    for (const std::string& ad : ads) if (ad.size() != ads[0].size()) return false;
    return true;
}

// the existing builder on these adapters alone
bool build_single(const Plan& p, int base, int count, M2Tables& t, int* why) {
    const std::vector<std::string> ads(p.ads.begin() + base, p.ads.begin() + base + count);
    const std::vector<std::vector<M2RefKmer>> rf(p.ref.begin() + base, p.ref.begin() + base + count);
    const CahMatcher& ml = p.mts[(size_t)p.longest];
    if (one_length(ads)) return m2_build(ads, ml.thr_last, p.k_of[(size_t)base], p.k_of[(size_t)base], ml.min_overlap, rf, t, why);
    return m2_build_mixed(ads, ml.thr_last, p.k_of.data() + base, ml.min_overlap, rf, t, why);
}

bool same_tables(const M2Tables& x, const M2Tables& y) {
    auto eq = [](const auto& u, const auto& v) {
        return u.size() == v.size() && (u.empty() || memcmp(u.data(), v.data(), u.size() * sizeof(u[0])) == 0);
    };
    return memcmp(&x.hdr, &y.hdr, sizeof(x.hdr)) == 0 && eq(x.dir, y.dir) && eq(x.entries, y.entries) && eq(x.bitmap, y.bitmap) &&
           eq(x.prefix, y.prefix) && eq(x.ref_begin, y.ref_begin) && eq(x.ref_list, y.ref_list);
}

}  // namespace

extern "C" {

// The plan's groups.  ranges: [2 * g] = base, [2 * g + 1] = count (room for 1024 groups).  info (8 x int32): [0] why
// m2_build_groups refused (M2_REFUSED_*), [1] did the single builder take the WHOLE plan (0 / 1; -1: more than 128
// adapters, not asked), [2] why it refused, [3] 1 when every group's tables equal, byte for byte, what the existing
// builder (m2_build / m2_build_mixed) makes of that group's adapters alone, [4] the largest group's entries.
// Returns G, 0 when the plan is refused, -1 when it is not eligible at all.
int m2g_groups(const char* adapters, int A, const void* blobs, int32_t n_ref, const int32_t* ref_adapter,
               const int32_t* ref_window, const char* ref_kmers, int32_t* ranges, int32_t* info) {
    const Plan p = read_plan(adapters, A, blobs, n_ref, ref_adapter, ref_window, ref_kmers);
    for (int i = 0; i < 8; i++) info[i] = 0;
    if (!p.eligible) return -1;
    const CahMatcher& ml = p.mts[(size_t)p.longest];
    info[1] = -1;
    if (A <= 128) {
        M2Tables t;
        int why = 0;
        info[1] = build_single(p, 0, A, t, &why) ? 1 : 0;
        info[2] = why;
    }
    std::vector<M2Group> gs;
    int why = 0;
    const bool ok = m2_build_groups(p.ads, ml.thr_last, p.k_of.data(), ml.min_overlap, p.ref, gs, &why);
    info[0] = why;
    if (!ok) return 0;
    info[3] = 1;
    for (size_t g = 0; g < gs.size(); g++) {
        ranges[2 * g] = gs[g].base; ranges[2 * g + 1] = gs[g].count;
        M2Tables t;
        if (!build_single(p, gs[g].base, gs[g].count, t, nullptr) || !same_tables(t, gs[g].t)) info[3] = 0;
        info[4] = std::max(info[4], (int32_t)gs[g].t.hdr.n_entries);
    }
    return (int)gs.size();
}

// The batch through every group and the merge.  Arguments as m2x_match_batch; order: 0 = the groups first to last, 1 =
// last to first (the merge must not care).  Returns G, 0 when the plan is refused.
int m2g_match_batch(const char* adapters, int A, const void* blobs, int32_t n_ref, const int32_t* ref_adapter,
                    const int32_t* ref_window, const char* ref_kmers, const uint8_t* seqs, const int64_t* offsets,
                    int64_t n_reads, int32_t* out6, uint8_t* status, int32_t* best, int subs, int order) {
    const Plan p = read_plan(adapters, A, blobs, n_ref, ref_adapter, ref_window, ref_kmers);
    if (!p.eligible) return 0;
    const CahMatcher& ml = p.mts[(size_t)p.longest];
    std::vector<M2Group> gs;
    if (!m2_build_groups(p.ads, ml.thr_last, p.k_of.data(), ml.min_overlap, p.ref, gs)) return 0;
    std::vector<unsigned long long> key((size_t)n_reads, 0ull);
    std::vector<uint8_t> invalid((size_t)n_reads, 0);
    std::vector<int32_t> g6((size_t)n_reads * 6), gbest((size_t)n_reads);
    std::vector<uint8_t> gst((size_t)n_reads);
    for (size_t gi = 0; gi < gs.size(); gi++) {
        const M2Group& gr = gs[order ? gs.size() - 1 - gi : gi];
        // the group's adapters as a plan of their own: strings, matchers, search sets with group-local adapter numbers
        std::string names, flat, kmers;
        std::vector<int32_t> ra, rw;
        bool same = true;
        for (int a = 0; a < gr.count; a++) {
            const std::string& ad = p.ads[(size_t)(gr.base + a)];
            same = same && ad.size() == p.ads[(size_t)gr.base].size();
            names += ad; names.push_back('\0');
            flat += ad;
            for (const M2RefKmer& rk : p.ref[(size_t)(gr.base + a)]) {
                ra.push_back(a); rw.push_back(rk.window);
                kmers += rk.kmer; kmers.push_back('\0');
            }
        }
        const void* gb = (const char*)blobs + sizeof(CahMatcher) * (size_t)gr.base;
        int rc;
        if (same)
            rc = m2m_match_batch(flat.c_str(), gr.count, (int)p.ads[(size_t)gr.base].size(), gb, (int32_t)ra.size(), ra.data(), rw.data(),
                                 kmers.c_str(), seqs, offsets, n_reads, g6.data(), gst.data(), gbest.data(), subs, nullptr, nullptr);
        else
            rc = m2x_match_batch(names.c_str(), gr.count, gb, (int32_t)ra.size(), ra.data(), rw.data(), kmers.c_str(), seqs, offsets,
                                 n_reads, g6.data(), gst.data(), gbest.data(), subs, nullptr, nullptr);
        if (rc != 0) return 0;
        for (int64_t r = 0; r < n_reads; r++) {
            if (gst[(size_t)r] == 2) invalid[(size_t)r] = 1;
            if (gst[(size_t)r] != 1) continue;
            const int32_t* o = &g6[(size_t)r * 6];
            key[(size_t)r] = std::max(key[(size_t)r], pack_best(o[4], o[5], gr.base + gbest[(size_t)r], o[1], o[2], o[3]));
        }
    }
    for (int64_t r = 0; r < n_reads; r++) {
        int32_t* o = out6 + r * 6;
        for (int i = 0; i < 6; i++) o[i] = 0;
        status[r] = 0; best[r] = -1;
        if (invalid[(size_t)r]) { status[r] = 2; continue; }
        const unsigned long long k = key[(size_t)r];
        if (!k) continue;
        const int rel = (int)(k & 0xFFu), qstart = (int)((k >> 8) & 0xFFFFFu), ref_stop = (int)((k >> 28) & 0x7Fu);
        o[0] = 0; o[1] = ref_stop; o[2] = qstart; o[3] = qstart + rel;
        o[4] = (int)((k >> 54) & 0xFFu) - 128; o[5] = 127 - (int)((k >> 47) & 0x7Fu);
        best[r] = 4095 - (int)((k >> 35) & 0xFFFu);
        status[r] = 1;
    }
    return (int)gs.size();
}

}  // extern "C"
