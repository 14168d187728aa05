// multi2_mixed_model.cpp -- HOST MODEL of the MIXED form of the streaming multi-adapter path: adapters of different
// lengths in one plan (multi2.h: m2_build_mixed; multi2.hip: k_multi_scan<KIND, true>; kernels.hip: k_dp_packed<ROWS,
// true, true>).  TEST INFRASTRUCTURE ONLY: the product never loads this file.
//
// k_multi_stream is the kernel of the one-shape plans, unchanged: the prefilter of multi2_model.cpp (filter_read) is
// replayed as it is over the mixed tables.  What differs is behind it: every pair is scanned with ITS adapter's m, k and
// chunking (window, reach, rows, precise window), in the word form of the plan's LONGEST adapter -- 32 bits when that has
// at most 32 characters, 64 bits otherwise --, against the longest adapter's thr_last, and the cell DP's corner check
// compares with min(lmax_row[row], the adapter's length).  tests/test_multi2_mixed_model.py compares the merged result
// with the oracle's kmers_present + locate of every adapter on the whole read.
#include "multi2_model.cpp"

extern "C" {

// adapters: A NUL-terminated strings back to back.  blobs: A CahMatcher structs.  The other arguments: m2m_match_batch.
// stats (may be NULL): [0] whole-read pairs, [1] hi, [2] lo, [3] suffix compares that matched, [6] pairs to the cell DP,
// [7] pairs scanned on the window of their one occurrence, [15] corner checks.
// Returns 0; 1 when the mixed builder refuses the plan (it would stay on the per-adapter loop).
int m2x_match_batch(const char* adapters, int A, const void* blobs, int32_t n_ref, const int32_t* ref_adapter,
                    const int32_t* ref_window, const char* ref_kmers, const uint8_t* seqs, const int64_t* offsets,
                    int64_t n_reads, int32_t* out6, uint8_t* status, int32_t* best, int subs, int64_t* stats,
                    const int32_t* pads) {
    std::vector<std::string> ads;
    const char* ap = adapters;
    for (int a = 0; a < A; a++) { ads.push_back(std::string(ap)); ap += strlen(ap) + 1; }
    std::vector<CahMatcher> mts((size_t)A);
    memcpy(mts.data(), blobs, sizeof(CahMatcher) * (size_t)A);
    std::vector<std::vector<M2RefKmer>> ref((size_t)A);
    const char* kp = ref_kmers;
    for (int i = 0; i < n_ref; i++) {
        ref[(size_t)ref_adapter[i]].push_back({std::string(kp), ref_window[i]});
        kp += strlen(kp) + 1;
    }
    // what build_multi (api.cpp) asks before it calls the mixed builder: kacc == k, one min_overlap, thr_last equal on the
    // rows two adapters share
    int longest = 0;
    for (int a = 0; a < A; a++) if (mts[(size_t)a].m > mts[(size_t)longest].m) longest = a;
    const CahMatcher& ml = mts[(size_t)longest];
    std::vector<int> k_of((size_t)A);
    for (int a = 0; a < A; a++) {
        const CahMatcher& mt = mts[(size_t)a];
        if (!mt.scan_ok || mt.kacc != mt.k || mt.min_overlap != ml.min_overlap) return 1;
        for (int i = 0; i <= mt.m; i++) if (mt.thr_last[i] != ml.thr_last[i]) return 1;
        k_of[(size_t)a] = mt.kacc;
    }
    M2Tables t;
    if (!m2_build_mixed(ads, ml.thr_last, k_of.data(), ml.min_overlap, ref, t)) return 1;
    const int kind = ml.m <= 32 ? 1 : 0;                               // (the explicit-row forms are one-shape: multi2.hip)
    auto thr = [&](int i) { return ml.thr_last[i]; };
    for (int64_t r = 0; r < n_reads; r++) {
        const uint8_t* const qv = seqs + offsets[r];
        const int nv = (int)(offsets[r + 1] - offsets[r]);
        const int pad = pads ? pads[r] : 0;
        std::vector<uint8_t> padded;
        const uint8_t* q = qv;
        int n = nv;
        if (pad > 0) {
            padded.assign((size_t)(pad + nv), 0);
            memcpy(padded.data() + pad, qv, (size_t)nv);
            q = padded.data(); n = pad + nv;
        }
        int32_t* o = out6 + r * 6;
        for (int i = 0; i < 6; i++) o[i] = 0;
        status[r] = 0; best[r] = -1;
        bool invalid = false;
        for (int i = 0; i < n; i++) invalid = invalid || q[i] >= 0x80;
        if (invalid) { status[r] = 2; continue; }
        ReadState st;
        filter_read(t, q, n, st, pad);
        unsigned long long bestkey = 0;
        for (auto& ex : st.exact) {
            bestkey = std::max(bestkey, pack_best(ex.second, 0, ex.first, ex.second, nv - ex.second, nv));
            if (stats) stats[3]++;
        }
        unsigned wm = CAH_M2_NO_FLAG;
        for (int a = 0; a < A; a++)
            if (st.seen[a] && st.wideonly[a]) wm = wm == CAH_M2_NO_FLAG ? (unsigned)a : CAH_M2_MANY_FLAGS;
        uint32_t rlast = 0x24924924u;
        for (int i = 0; i < n; i++) rlast = (rlast << 3) | m2_code(q[i]);
        for (const Pair& pr : st.pairs) {
            const CahMatcher& mt = mts[(size_t)pr.adapter];
            BackScanParams p;                                           // the PAIR's own
            p.m = mt.m; p.k = mt.k; p.kacc = mt.kacc; p.min_overlap = mt.min_overlap; p.half_m = mt.m / 2;
            const int reach = p.m + p.k + 1;
            const bool tail = (pr.flags & CAH_M2_PAIR_TAIL) != 0;
            int j0 = tail ? (pr.key << 2) : std::max(0, (pr.key << CAH_KEY_SHIFT) - p.m - p.k - 1);
            const bool precise = (pr.flags & CAH_M2_PAIR_PRECISE) != 0 && wm != (unsigned)pr.adapter && wm != CAH_M2_MANY_FLAGS;
            int jend = n, tail0 = 0;
            if (pr.flags & CAH_M2_PAIR_PRECISE) {
                int jw, jb;
                m2_precise_window(pr.key, (int)(pr.flags >> CAH_M2_PAIR_CHUNK_SHIFT) & 3, p.m, p.k, p.m / (p.k + 1), p.m % (p.k + 1), n, jw, jb);
                if (precise) {
                    j0 = jw; jend = jb;
                    tail0 = m2_exact_tail(rlast, t.prefix[(size_t)pr.adapter], p.min_overlap, t.hdr.lmax0, n);
                } else {
                    j0 = std::max(0, (pr.key & ~15) - p.m - p.k - 1);
                }
            }
            int max_row = std::min(p.m, n - std::min(j0, n) + p.kacc);
            const bool is_lo = tail && pr.cls == M2_LO;
            if (is_lo) max_row = std::min(max_row, t.hdr.rows_lo);
            j0 = bs_align_window(std::min(j0, n), n);
            if (precise) {
                jend = std::min(n, j0 + ((jend - j0 + 15) & ~15));
                if (stats) stats[7]++;
            }
            if (stats) stats[tail ? (is_lo ? 2 : 1) : 0]++;
            bool exact = false;
            int j = j0, o0 = 0, o1 = 0, cls = BS_NONE, jfa = -1;
            auto run = [&](auto& s, auto step, auto finish, auto finish_stopped) {
                while (j < jend) {
                    ++j;
                    if (step(s, q[j - 1] & 127)) { exact = true; break; }
                }
                jfa = s.jfa;
                if (exact) { cls = BS_EXACT_FULL; o0 = j; }
                else if (!precise) cls = finish(s);
                else if (jfa < 0) cls = BS_NONE;
                else {
                    cls = finish_stopped(s);
                    if (tail0 > 0) { cls = BS_DP; o0 = std::max(j0, jfa - reach); o1 = 2 * n + 1; }
                }
            };
            // the kernel's waves: a whole-read wave with a full window tracks (subs), every other wave does not; a tail
            // pair runs the bare recurrence.  subs = 1 replays "every whole-read pair tracked", subs = 0 "none"
            const bool track = subs && !tail;
            if (!track && is_lo && kind == 0 && t.hdr.rows_lo <= 32) {
                // k_multi_scan's "lo" pages in the 64-bit form: the adapter's first 32 rows in one plain 32-bit word
                BackScanParams p32 = p;
                p32.m = 32;
                BackScanState32<0> s;
                bs32_init(s, p32);
                run(s, [&](BackScanState32<0>& z, int c) { return bs32_step<false, 0, false>(z, (uint32_t)(mt.scanmask[c] >> (64 - p.m)), 0u, j, p32); },
                    [&](BackScanState32<0>& z) { return bs32_finish<0, false>(z, n, j0, p32, thr, o0, o1, false, max_row); },
                    [&](BackScanState32<0>& z) { return bs32_finish<0, false>(z, n, j0, p32, thr, o0, o1, true, max_row); });
            } else if (kind == 0) {
                BackScanState s;
                bs_init(s, p);
                if (track) run(s, [&](BackScanState& z, int c) { return bs_step<true>(z, mt.scanmask[c], j, p); },
                               [&](BackScanState& z) { return bs_finish<true>(z, n, j0, p, thr, o0, o1, false, max_row); },
                               [&](BackScanState& z) { return bs_finish<true>(z, n, j0, p, thr, o0, o1, true, max_row); });
                else if (tail) run(s, [&](BackScanState& z, int c) { return bs_step<false, false>(z, mt.scanmask[c], j, p); },
                                   [&](BackScanState& z) { return bs_finish<false>(z, n, j0, p, thr, o0, o1, false, max_row); },
                                   [&](BackScanState& z) { return bs_finish<false>(z, n, j0, p, thr, o0, o1, true, max_row); });
                else run(s, [&](BackScanState& z, int c) { return bs_step<false>(z, mt.scanmask[c], j, p); },
                         [&](BackScanState& z) { return bs_finish<false>(z, n, j0, p, thr, o0, o1, false, max_row); },
                         [&](BackScanState& z) { return bs_finish<false>(z, n, j0, p, thr, o0, o1, true, max_row); });
            } else {
                // (every adapter has at most 32 characters: its top-aligned 64-bit word's upper half, pad rows by its own m)
                BackScanState32<0> s;
                bs32_init(s, p);
                auto eq = [&](int c) { return (uint32_t)(mt.scanmask[c] >> 32); };
                if (track) run(s, [&](BackScanState32<0>& z, int c) { return bs32_step<true, 0>(z, eq(c), 0u, j, p); },
                               [&](BackScanState32<0>& z) { return bs32_finish<0, true>(z, n, j0, p, thr, o0, o1, false, max_row); },
                               [&](BackScanState32<0>& z) { return bs32_finish<0, true>(z, n, j0, p, thr, o0, o1, true, max_row); });
                else if (tail) run(s, [&](BackScanState32<0>& z, int c) { return bs32_step<false, 0, false>(z, eq(c), 0u, j, p); },
                                   [&](BackScanState32<0>& z) { return bs32_finish<0, false>(z, n, j0, p, thr, o0, o1, false, max_row); },
                                   [&](BackScanState32<0>& z) { return bs32_finish<0, false>(z, n, j0, p, thr, o0, o1, true, max_row); });
                else run(s, [&](BackScanState32<0>& z, int c) { return bs32_step<false, 0>(z, eq(c), 0u, j, p); },
                         [&](BackScanState32<0>& z) { return bs32_finish<0, false>(z, n, j0, p, thr, o0, o1, false, max_row); },
                         [&](BackScanState32<0>& z) { return bs32_finish<0, false>(z, n, j0, p, thr, o0, o1, true, max_row); });
            }
            unsigned long long key = 0;
            bool in_pad = false;
            auto shortcut = [&](int score, int errors, int ref_stop, int qs, int qe) {
                if (qs < pad) { in_pad = true; return; }
                key = pack_best(score, errors, pr.adapter, ref_stop, qs - pad, qe - pad);
            };
            if (cls == BS_EXACT_FULL) shortcut(p.m, 0, p.m, o0 - p.m, o0);
            else if (cls == BS_EXACT_TAIL) shortcut(o0 - 2 * o1, o1, o0, n - o0, n);
            else if (cls == BS_SUBS_FULL) shortcut(p.m - 2 * o1, o1, p.m, o0 - p.m, o0);
            else if (cls == BS_INDEL1_FULL)
                shortcut(p.m - 2 * (o1 >> 1) - (o1 & 1), o1 >> 1, p.m, o0 - p.m + ((o1 & 1) ? 1 : -1), o0);
            if (in_pad) { cls = BS_DP; o0 = 0; o1 = 2 * n + 1; }
            if (cls == BS_DP) {
                if (tail && !in_pad) o0 = std::max(0, (jfa >= 0 ? jfa : n) - reach);
                int t6[6];
                if (stats) stats[6]++;
                const int first = std::max(0, o0 - pad), last = std::max(0, std::min(n, o1 >> 1) - pad);
                if (dp_window(mt, qv, nv, std::min(first, nv), std::min(last, nv), (o1 & 1) != 0, t6)) {
                    // the corner of multi2.h's head, with the adapter's OWN last class clipped to its length
                    bool ref_ok = true;
                    if (tail && nv - t6[2] > std::min((int)t.hdr.lmax_row[t6[1]], p.m)) {
                        ref_ok = m2_ref_present(t.ref_list.data(), t.ref_begin[(size_t)pr.adapter], t.ref_begin[(size_t)pr.adapter + 1], qv, nv, t.hdr.ref_span);
                        if (stats) stats[15]++;
                    }
                    if (ref_ok) key = pack_best(t6[4], t6[5], pr.adapter, t6[1], t6[2], t6[3]);
                }
            }
            if (precise && cls == BS_NONE && tail0 > 0) key = pack_best(tail0, 0, pr.adapter, tail0, nv - tail0, nv);
            bestkey = std::max(bestkey, key);
        }
        if (bestkey) {
            const unsigned long long k = bestkey;
            const int rel = (int)(k & 0xFFu), qstart = (int)((k >> 8) & 0xFFFFFu), ref_stop = (int)((k >> 28) & 0x7Fu);
            o[0] = 0; o[1] = ref_stop; o[2] = qstart; o[3] = qstart + rel;
            o[4] = (int)((k >> 54) & 0xFFu) - 128; o[5] = 127 - (int)((k >> 47) & 0x7Fu);
            best[r] = 4095 - (int)((k >> 35) & 0xFFFu);
            status[r] = 1;
        }
    }
    return 0;
}

}  // extern "C"
