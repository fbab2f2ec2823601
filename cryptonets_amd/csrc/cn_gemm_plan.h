// HOT LOOP A on the host: how a scalar GEMM (DenseMatrixBySparseVectorMultiply) is planned, decided here and nowhere else - the arithmetic class of its weights and
// the kernel form, the pairing and grouping of gather lists, the weight tiles in the kernels' layouts (cn_k_gemm.hip.h), the digit-GEMM bound of cn_square_gemm and
// the image that reaches the device.  cn_scalar_gemm, cn_gemm_plan_create and the cached plans of deferred square + dense layers plan over 32-bit indices
// (gemm_plan_indices), a flush of the deferred queue over device addresses (gemm_plan_addresses).  Host-only and free of HIP: a plain C++ compiler builds it
// (tests/cpp/gemm_plan.cpp).
#pragma once
#include "cn_policy.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <unordered_map>
#include <vector>

// the switches of a context the planner reads: the options "f64", "gemm_mfma", "gemm_pair", "digit_mfma", "digit_i32" (gemm_switches, cn_eval.hip)
struct GemmSwitches { bool f64, gemm_mfma, gemm_pair, digit_mfma, digit_i32; };
// a refusal: CN_ERR_ARG of include/cnhip.h and the text cn_fail reports
static const int GEMM_ERR_ARG = -1;
struct GemmRefusal {
    int rc = 0; char msg[96] = {0};
    explicit operator bool() const { return rc != 0; }
};
inline GemmRefusal gemm_refuse(const char *text) { GemmRefusal r; r.rc = GEMM_ERR_ARG; snprintf(r.msg, sizeof r.msg, "%s", text); return r; }
inline size_t gemm_al(size_t b) { return (b + 255) & ~(size_t)255; }
static const uint32_t GEMM_NONE = 0xffffffffu;        // member table: no such output in this group

// ---------------------------------------------------------------- weight classification and kernel form
inline uint64_t gemm_abs_weight(const DevConsts &hc, uint64_t w) { return w >= hc.t_half ? hc.t.q - w : w; }       // |w| of a residue mod t, centred
inline uint64_t lift_scalar(const DevConsts &hc, uint64_t w, uint32_t j) { return w >= hc.t_half ? w + hc.lift_inc[j] : w; }
// small signed weights (|w| < 2^20 after centring mod t - every PoolLayer weight round(w*scale) is): exact-FP64 limb-split kernel
inline bool gemm_weights_small(const DevConsts &hc, const uint64_t *W, size_t count) {
    for (size_t x = 0; x < count; x++) if (gemm_abs_weight(hc, W[x]) >> 20) return false;
    return true;
}
struct GemmArith { bool small, two; uint32_t lazy; int bits; };
inline GemmArith gemm_arith(const DevConsts &hc, const GemmSwitches &sw, bool weights_small) {
    const CnModRange qr = cn_mod_range(hc, 0, hc.k);
    const int bits = qr.bits;
    GemmArith g;
    g.bits = bits;
    g.small = weights_small && sw.f64 && bits <= 49;             // the kernel folds its limb sums with exact-FP64 modular arithmetic (q < 2^49.4)
    g.two = qr.light;                                            // 2 limbs of 22 bits, else 3 limbs of 17 bits
    if (g.small) g.lazy = g.two ? 1024u : 32768u;                // terms whose limb products (< 2^42 / 2^37) still sum exactly below 2^52
    else g.lazy = (2 * bits >= 127) ? 1u : (uint32_t)std::min<uint64_t>(1u << 20, 1ull << (127 - 2 * bits));   // products of two values < q_max in 128 bits
    return g;
}
// ---- the matrix-core form of a scalar GEMM (k_scalar_gemm_mfma): eligibility, weight digit planes, A fragments
// 6 signed base-256 digits cover residues below 2^46 (x + 0x80..80 must stay below 2^48); i32 accumulators hold K * P * 2^14 < 2^31
inline bool gemm_mfma_ok(const DevConsts &hc, const GemmSwitches &sw, const GemmArith &ar, uint32_t M, uint32_t K) {
    return sw.gemm_mfma && ar.small && ar.bits <= 46 && M >= 16 && (uint64_t)K * 3 < (1u << 17) && !(hc.n & 31);
}
static const uint64_t GEMM_RES_CLIP = 127, GEMM_RES_MAX = 254;      // clipped + residual form (gemm_residual_form): |c| <= 127, |w| <= 254
inline uint32_t gemm_weight_planes(const DevConsts &hc, const uint64_t *W, size_t count) {
    uint64_t amax = 0;
    for (size_t x = 0; x < count; x++) amax = std::max(amax, gemm_abs_weight(hc, W[x]));
    return amax <= 127 ? 1u : (amax <= 32639 ? 2u : 3u);          // signed digits -128..127: |w| <= 127 / 32639 / 8355711
}

// the outputs of every distinct gather list, the lists in lexicographic order: the order of the groups in every table
template <class KEY> inline std::map<std::vector<KEY>, std::vector<uint32_t>> gemm_outputs_by_list(const KEY *keys, uint32_t O, uint32_t K) {
    std::map<std::vector<KEY>, std::vector<uint32_t>> groups;
    for (uint32_t o = 0; o < O; o++) groups[std::vector<KEY>(keys + (size_t)o * K, keys + (size_t)(o + 1) * K)].push_back(o);
    return groups;
}
// ---------------------------------------------------------------- pairing of gather lists
// Gather lists that overlap are merged in PAIRS (round 5).  A convolution window of 25 taps shares 15 of them with its neighbour; as two gather lists every shared
// input word travels from L2 to a CU twice - and that traffic, not HBM and not instruction issue, is what the layer waits for (profiles/HISTORY.md, round 5: the
// CryptoNets convolution 370-380 us with one list per window, 300-320 us with the windows in pairs; wider tiles lose again: their outputs no longer fit the
// 10-output register tile).  Two lists that share at least half of their inputs become ONE list (the union, 35 entries for two neighbouring 5 x 5 windows at stride
// 2) whose outputs carry the weight 0 for the entries of the other list: a zero weight is "no term" in DenseMatrixBySparseVectorMultiply, the outputs are the same
// words.  Only for small signed weights (the FP64 kernels), lists of at most 64 entries without repeated inputs and at most 5 outputs each (a pair then fills the
// 10-output tile).  gidx / W2 / K are rewritten in place; returns false when nothing was merged.
inline bool pair_gather_lists(uint32_t O, uint32_t &K, std::vector<int32_t> &gidx, const uint64_t *W, std::vector<uint64_t> &W2) {
    if (K > 64 || O < 2) return false;
    const auto groups = gemm_outputs_by_list(gidx.data(), O, K);
    const size_t G = groups.size();
    if (G < 2 || G > 65536) return false;
    struct L { std::vector<int32_t> in; const std::vector<uint32_t> *outs; const std::vector<int32_t> *list; int32_t mate = -1; };
    std::vector<L> ls; ls.reserve(G);
    for (auto &kv : groups) {
        if (kv.second.size() > 5) return false;
        L l; l.outs = &kv.second; l.list = &kv.first;
        for (int32_t id : kv.first) if (id >= 0) l.in.push_back(id);
        std::sort(l.in.begin(), l.in.end());
        if (std::adjacent_find(l.in.begin(), l.in.end()) != l.in.end()) return false;       // an input twice in one list: its two weights would have to be added
        ls.push_back(std::move(l));
    }
    std::unordered_map<int32_t, std::vector<uint32_t>> where;                               // input -> lists that gather it
    for (uint32_t i = 0; i < G; i++) for (int32_t id : ls[i].in) where[id].push_back(i);
    bool any = false;
    std::vector<uint32_t> cnt(G, 0), touched;
    for (uint32_t i = 0; i < G; i++) {
        if (ls[i].mate >= 0) continue;
        touched.clear();
        for (int32_t id : ls[i].in) for (uint32_t j : where[id]) if (j > i && ls[j].mate < 0) { if (!cnt[j]++) touched.push_back(j); }
        uint32_t best = 0; int32_t bj = -1;
        for (uint32_t j : touched) { if (cnt[j] > best || (cnt[j] == best && (int32_t)j < bj)) { best = cnt[j]; bj = (int32_t)j; } cnt[j] = 0; }
        if (bj >= 0 && 2 * best >= std::min(ls[i].in.size(), ls[bj].in.size()) && ls[i].in.size() + ls[bj].in.size() - best <= 64) { ls[i].mate = bj; ls[bj].mate = (int32_t)i; any = true; }
    }
    if (!any) return false;
    // the union of a pair: the first list's entries in their order, then the second list's new ones; K2 = the longest list after merging
    std::vector<std::vector<int32_t>> uni(G);
    uint32_t K2 = 0;
    for (uint32_t i = 0; i < G; i++) {
        const int32_t m = ls[i].mate;
        if (m >= 0 && (uint32_t)m < i) { uni[i] = uni[m]; continue; }
        for (int32_t id : *ls[i].list) if (id >= 0) uni[i].push_back(id);
        if (m >= 0) for (int32_t id : *ls[m].list) if (id >= 0 && !std::binary_search(ls[i].in.begin(), ls[i].in.end(), id)) uni[i].push_back(id);
        K2 = std::max<uint32_t>(K2, (uint32_t)uni[i].size());
    }
    std::vector<int32_t> g2((size_t)O * K2, -1);
    W2.assign((size_t)O * K2, 0);
    for (uint32_t i = 0; i < G; i++) {
        std::unordered_map<int32_t, uint32_t> pos;
        for (uint32_t x = 0; x < uni[i].size(); x++) pos[uni[i][x]] = x;
        for (uint32_t o : *ls[i].outs) {
            for (uint32_t x = 0; x < uni[i].size(); x++) g2[(size_t)o * K2 + x] = uni[i][x];
            for (uint32_t kk = 0; kk < K; kk++) { const int32_t id = gidx[(size_t)o * K + kk]; if (id >= 0) W2[(size_t)o * K2 + pos[id]] = W[(size_t)o * K + kk]; }
        }
    }
    gidx.swap(g2); K = K2;
    return true;
}

// ---------------------------------------------------------------- grouping
// Outputs that gather the same inputs form a group (PoolLayer: every map of one corner shares its patch; a dense layer: one group), in the order of std::map over
// the gather rows.  KEY: int32_t indices (-1 = padded tap; every negative entry counts as one) or uint64_t device addresses (0 = padded tap) - a tap gathers
// a ciphertext iff its key lies above the type's padding value.  Groups may differ in size (a tiled convolution has smaller tiles at the border): M = the largest,
// the missing members of smaller groups are GEMM_NONE (nothing stored, all-zero weight rows).  Gather rows are padded to Kp entries: the matrix-core form reads 32
// per K step, the VALU kernels 4 at a time and request up to 2 x 8 terms ahead (16 spare entries).
template <class KEY> struct GemmGroups {
    static constexpr KEY PAD = std::is_signed<KEY>::value ? (KEY)-1 : (KEY)0;
    uint32_t O = 0, G = 0, M = 0, K = 0, Kp = 0;
    bool mfma = false;
    std::vector<KEY> rows;                 // [G][Kp]
    std::vector<uint32_t> member;          // [G][M]: the output of (group, m)
    const uint64_t *W = nullptr;           // [O][K] residues mod t
    // clipped + residual form (gemm_residual_form): the K slots of every gather row are permuted, slot kk of group g holds term src[g][kk] of the caller's rows, and the
    // first kres[g] K steps hold every input with a weight beyond +-127
    bool res = false;
    std::vector<uint32_t> src, kres;       // [G][K] (empty: the identity), [G]
    uint32_t term(uint32_t g, uint32_t kk) const { return src.empty() ? kk : src[(size_t)g * K + kk]; }
    bool tap(uint32_t g, uint32_t kk) const { return rows[(size_t)g * Kp + kk] > PAD; }
    const uint64_t *row(uint32_t g, uint32_t m) const { const uint32_t o = member[(size_t)g * M + m]; return o == GEMM_NONE ? nullptr : W + (size_t)o * K; }
    // weight of term kk in the row wr of group g: a padded tap gets the weight 0 whatever the caller passed (k_scalar_gemm_f64 multiplies a valid word by it
    // instead of selecting per lane)
    uint64_t weight(uint32_t g, const uint64_t *wr, uint32_t kk) const { return tap(g, kk) ? wr[term(g, kk)] : 0; }
};
template <class KEY> inline GemmGroups<KEY> gemm_group(const DevConsts &hc, const GemmSwitches &sw, const GemmArith &ar, const KEY *keys, const uint64_t *W, uint32_t O, uint32_t K) {
    const auto groups = gemm_outputs_by_list(keys, O, K);
    GemmGroups<KEY> gr;
    gr.O = O; gr.G = (uint32_t)groups.size(); gr.K = K; gr.W = W;
    for (auto &g : groups) gr.M = std::max<uint32_t>(gr.M, (uint32_t)g.second.size());
    gr.mfma = gemm_mfma_ok(hc, sw, ar, gr.M, K);
    gr.Kp = gr.mfma ? ((K + 31) / 32) * 32 : ((K + 15) & ~15u) + 16;
    gr.rows.assign((size_t)gr.G * gr.Kp, GemmGroups<KEY>::PAD);
    gr.member.assign((size_t)gr.G * gr.M, GEMM_NONE);
    uint32_t g = 0;
    for (auto &kv : groups) {
        memcpy(&gr.rows[(size_t)g * gr.Kp], kv.first.data(), (size_t)K * sizeof(KEY));
        for (uint32_t m = 0; m < kv.second.size(); m++) gr.member[(size_t)g * gr.M + m] = kv.second[m];
        g++;
    }
    return gr;
}

// ---------------------------------------------------------------- weight tiles in kernel layout
// signed doubles [g][mtile][kk < rows][m < tile], zero padded: the small-weight table of k_scalar_gemm_f64 (tile MT, gemm_f64_rows) and the table of k_digit_gemm
// (digit_gemm_tile, digit_gemm_rows)
template <class KEY> inline void pack_gemm_f64(const DevConsts &hc, const GemmGroups<KEY> &gr, uint32_t tile, uint32_t rows, std::vector<char> &bytes) {
    const uint32_t mt = (gr.M + tile - 1) / tile;
    bytes.assign((size_t)gr.G * mt * rows * tile * sizeof(double), 0);
    double *tab = (double *)bytes.data();
    for (uint32_t g = 0; g < gr.G; g++) for (uint32_t m = 0; m < gr.M; m++) {
        const uint64_t *wr = gr.row(g, m);
        if (!wr) continue;
        double *dst = &tab[(((size_t)g * mt + m / tile) * rows) * tile + m % tile];
        for (uint32_t kk = 0; kk < gr.K; kk++) { const uint64_t w = gr.weight(g, wr, kk); dst[(size_t)kk * tile] = w >= hc.t_half ? -(double)(hc.t.q - w) : (double)w; }
    }
}
// lifted residues [j][g][mtile][kk][m < tile], zero padded: k_scalar_gemm
template <class KEY> inline void pack_gemm_int(const DevConsts &hc, const GemmGroups<KEY> &gr, uint32_t tile, std::vector<char> &bytes) {
    const uint32_t mt = (gr.M + tile - 1) / tile, K = gr.K;
    bytes.assign((size_t)hc.k * gr.G * mt * K * tile * sizeof(uint64_t), 0);
    uint64_t *tab = (uint64_t *)bytes.data();
    for (uint32_t j = 0; j < hc.k; j++) for (uint32_t g = 0; g < gr.G; g++) for (uint32_t m = 0; m < gr.M; m++) {
        const uint64_t *wr = gr.row(g, m);
        if (!wr) continue;
        uint64_t *dst = &tab[((((size_t)j * gr.G + g) * mt + m / tile) * K) * tile + m % tile];
        for (uint32_t kk = 0; kk < K; kk++) { const uint64_t w = gr.weight(g, wr, kk); dst[(size_t)kk * tile] = w ? lift_scalar(hc, w, j) : 0; }
    }
}
// fragments [g][p][mtile][kstep][lane][16]: lane l, byte t = digit p of the weight of output row 32 mtile + (l & 31) for term
// 32 kstep + 16 (l >> 5) + t; zero for padded rows / terms / taps
// Clipped + residual form (gr.res, gemm_residual_form; P = 2 here, the kernels' P = 1): plane 0 = c = clamp(w, -127, 127), plane 1 = r = w - c in the same
// fragment layout, the terms in the permuted slot order of gr.rows, r = 0 behind K step kres[g]; then the table kres [G] of 32-bit words, which the kernels read
template <class KEY> inline void pack_gemm_mfma(const DevConsts &hc, const GemmGroups<KEY> &gr, uint32_t P, std::vector<char> &wbytes) {
    const uint32_t mtiles = (gr.M + 31) / 32, ksteps = (gr.K + 31) / 32;
    const uint64_t t = hc.t.q;
    const size_t frags = (size_t)gr.G * P * mtiles * ksteps * 1024;
    wbytes.assign(frags + (gr.res ? gr.G * sizeof(uint32_t) : 0), 0);
    if (gr.res) memcpy(wbytes.data() + frags, gr.kres.data(), gr.G * sizeof(uint32_t));
    for (uint32_t g = 0; g < gr.G; g++) for (uint32_t m = 0; m < gr.M; m++) {
        const uint64_t *wr = gr.row(g, m);
        if (!wr) continue;
        const uint32_t mt = m / 32, r = m % 32;
        for (uint32_t kk = 0; kk < gr.K; kk++) {
            const uint64_t w = gr.weight(g, wr, kk);
            if (!w) continue;
            const int64_t sw = w >= hc.t_half ? -(int64_t)(t - w) : (int64_t)w;
            const int64_t cl = std::min<int64_t>(std::max<int64_t>(sw, -(int64_t)GEMM_RES_CLIP), (int64_t)GEMM_RES_CLIP);
            const uint32_t rec = gr.res ? ((uint32_t)(uint8_t)(int8_t)cl | (uint32_t)(uint8_t)(int8_t)(sw - cl) << 8)
                                        : ((uint32_t)(sw + 0x808080) ^ 0x808080u);   // byte p = signed digit p
            const uint32_t ks = kk / 32, half = (kk % 32) / 16, tt = kk % 16;
            for (uint32_t p = 0; p < P; p++)
                wbytes[((((size_t)g * P + p) * mtiles + mt) * ksteps + ks) * 1024 + (size_t)(half * 32 + r) * 16 + tt] = (char)(uint8_t)(rec >> (8 * p));
        }
    }
}
// the largest sum_k |w_ok| over the gathered terms of any output, or `stop` + 1 as soon as one output exceeds `stop`
template <class KEY> inline uint64_t gemm_row_sum_max(const DevConsts &hc, const GemmGroups<KEY> &gr, uint64_t stop) {
    uint64_t sum_max = 0;
    for (uint32_t g = 0; g < gr.G; g++) for (uint32_t m = 0; m < gr.M; m++) {
        const uint64_t *wr = gr.row(g, m);
        if (!wr) continue;
        uint64_t sum = 0;
        for (uint32_t kk = 0; kk < gr.K; kk++) if (gr.tap(g, kk)) { sum += gemm_abs_weight(hc, wr[gr.term(g, kk)]); if (sum > stop) return stop + 1; }
        sum_max = std::max(sum_max, sum);
    }
    return sum_max;
}
// ---- the clipped + residual form of the matrix-core kernels (k_scalar_gemm_mfma<1, .., GemmResidual>, k_digit_gemm_mfma<1, .., GemmResidual>)
// A trained dense layer has a handful of weights beyond +-127 (CryptoNets 845 -> 100: 48 of 84 500, in 31 input columns, max |w| = 165).  As base-256 digits they cost a
// whole second plane - twice the matrix instructions, a second A fragment per step, one more diagonal of accumulators - that is zero almost everywhere.  Instead
// w = c + r with c = clamp(w, -127, 127) and r = w - c, |r| <= 127 for |w| <= 254: two int8 planes of the SAME weight 256^0, whose products land in the same
// accumulators, and the K slots of every gather row are permuted (index entries and weight fragments alike) so that the inputs with any r != 0 come first: only the
// first kres[g] K steps hold a residual.  The kernels run kres[g] + K steps of the one-plane body (the r fragments of the first kres[g] K steps, then all c
// fragments).  The sum over k is exact integer arithmetic: the order changes no word.
// Gate: a matrix-core plan with 127 < max |w| <= 254 (max as gemm_weight_planes takes it); i32 head-room: a diagonal receives per term (c + r) x digit with
// |c| + |r| = |w| and |digit| <= 128, so |acc| <= 128 R, R = gemm_row_sum_max; 128 R < 2^31 (the digit GEMM receives lo and hi products, (128 + 64) R < 2^31:
// gemm_digit_form; with 3 K < 2^17 and |w| <= 254 both hold for every plan that gets here, R <= 11 097 260 - they are checked all the same); and the share of
// residual steps.  The form is CORRECT up to kres[g] = K steps; it PAYS while (K steps + kres) one-plane steps take less time than K two-plane steps.  Measured per
// step at K = 845 (profiles/gemm_residual_plane.md): one plane 6.52 / 6.21 / 3.40 us (Bsk form, y form, digit GEMM), two planes 7.67 / 6.95 / 5.26 us - break-even
// at kres / K steps = 0.18 / 0.12 / 0.55.  A residual step repeats the gather, recode and LDS exchange of its K step, which is what these kernels wait for, not
// only its matrix instructions.  So the gate is GEMM_RES_SHARE kres[g] <= K steps with GEMM_RES_SHARE = 8: at 1/8 the y form breaks even and the other two still
// gain.  CN_GEMM_RESIDUAL, read whenever a plan is built (A/B; a plan that is cached - cn_gemm_plan_create's, the deferred queue's SgPlan - keeps the form it was
// built in): 0 keeps the base-256 planes, 2 takes the form up to half the K steps (2 kres[g] <= K steps: for measuring where it stops paying, and for tests on
// layers of a few K steps).  Permutes gr.rows in place and fills gr.src / gr.kres.
static const uint32_t GEMM_RES_SHARE = 8;
inline int gemm_residual_mode() { const char *e = getenv("CN_GEMM_RESIDUAL"); return e ? std::min(std::max(atoi(e), 0), 2) : 1; }
template <class KEY> inline void gemm_residual_form(const DevConsts &hc, GemmGroups<KEY> &gr) {
    const int mode = gemm_residual_mode();
    if (!gr.mfma || !mode) return;
    uint64_t amax = 0;
    for (size_t x = 0; x < (size_t)gr.O * gr.K; x++) amax = std::max(amax, gemm_abs_weight(hc, gr.W[x]));
    if (amax <= GEMM_RES_CLIP || amax > GEMM_RES_MAX) return;
    const uint32_t K = gr.K, ksteps = (K + 31) / 32;
    const uint64_t stop = ((1ull << 31) - 1) / 128;
    if (gemm_row_sum_max(hc, gr, stop) > stop) return;
    std::vector<uint32_t> src((size_t)gr.G * K), kres(gr.G);
    for (uint32_t g = 0; g < gr.G; g++) {
        std::vector<uint8_t> big(K, 0);
        for (uint32_t m = 0; m < gr.M; m++) {
            const uint64_t *wr = gr.row(g, m);
            if (wr) for (uint32_t kk = 0; kk < K; kk++) if (gr.tap(g, kk) && gemm_abs_weight(hc, wr[kk]) > GEMM_RES_CLIP) big[kk] = 1;
        }
        uint32_t at = 0;
        for (uint32_t kk = 0; kk < K; kk++) if (big[kk]) src[(size_t)g * K + at++] = kk;
        kres[g] = (at + 31) / 32;
        if ((mode == 2 ? 2 : GEMM_RES_SHARE) * kres[g] > ksteps) return;
        for (uint32_t kk = 0; kk < K; kk++) if (!big[kk]) src[(size_t)g * K + at++] = kk;
    }
    std::vector<KEY> row(K);
    for (uint32_t g = 0; g < gr.G; g++) {
        for (uint32_t kk = 0; kk < K; kk++) row[kk] = gr.rows[(size_t)g * gr.Kp + src[(size_t)g * K + kk]];
        std::copy(row.begin(), row.end(), gr.rows.begin() + (size_t)g * gr.Kp);
    }
    gr.res = true; gr.src.swap(src); gr.kres.swap(kres);
}
// One-limb form of the small-weight kernel: sum_k w_k x_k with x_k < q_max is an exact double as long as (sum_k |w_k| + 1) q_max <= 2^53 for every output row
// (all partial sums are integers below 2^53; the + 1 leaves room for the recentred carry of the fold) - the words are then not split into limbs at all: ONE FMA
// per MAC instead of two, no masks and shifts, one recentring per output.  True for the CryptoNets convolution (row sums <= 373 with the trained weights,
// 44-bit moduli); the dense layers have larger row sums and keep the two-limb form (or the matrix cores).  Needs the whole term list in one block (K <= lazy).
template <class KEY> inline bool gemm_one_limb(const DevConsts &hc, const GemmArith &ar, const GemmGroups<KEY> &gr) {
    static const bool on = !(getenv("CN_GEMM_ONE_LIMB") && !atoi(getenv("CN_GEMM_ONE_LIMB")));
    if (!on || !ar.small || ar.bits > 49 || gr.K > ar.lazy) return false;
    const uint64_t room = (1ull << 53) / cn_mod_range(hc, 0, hc.k).qmax;     // sum |w| + 1 <= room
    return room && gemm_row_sum_max(hc, gr, room - 1) <= room - 1;
}
// kernel form and weight tiles of the grouped GEMM: the matrix cores, or the VALU kernels with FP64 tiles of 1 / 5 / 10 / 20 outputs (small weights) or integer tiles
// of 1 / 5 / 10
template <class KEY> inline void gemm_form_and_pack(const DevConsts &hc, const GemmArith &ar, const GemmGroups<KEY> &gr, GemmLayout &L, std::vector<char> &wbytes) {
    const uint32_t M = gr.M;
    L.K = gr.K; L.Kp = gr.Kp; L.G = gr.G; L.M = M; L.small = ar.small; L.two = ar.two; L.lazy = ar.lazy; L.mfma = gr.mfma;
    if (gr.mfma) {
        L.P = gr.res ? 1 : gemm_weight_planes(hc, gr.W, (size_t)gr.O * gr.K); L.mtiles = (M + 31) / 32; L.ksteps = (gr.K + 31) / 32;
        L.res = gr.res;
        pack_gemm_mfma(hc, gr, gr.res ? 2 : L.P, wbytes);
    } else if (ar.small) {
        L.MT = M >= 16 ? 20 : (M >= 8 ? 10 : (M >= 3 ? 5 : 1));
        pack_gemm_f64(hc, gr, L.MT, gemm_f64_rows(gr.K), wbytes);
        L.one = gemm_one_limb(hc, ar, gr);
    } else {
        L.MT = M >= 8 ? 10 : (M >= 3 ? 5 : 1);
        pack_gemm_int(hc, gr, L.MT, wbytes);
    }
}
// cn_square_gemm: may this layer run on the DIGITS of unrelinearized products (k_digit_gemm)?  Small signed weights and, for every output, sum_k |w| (2^dbc - 1)
// below q_j / 2 for every j and below 2^52: the combined digit polynomial is then an exact double and a recentred lazy value of every limb's FP64 policy.
// Matrix-core form (k_digit_gemm_mfma) where the plan's own GEMM takes the matrix cores (L.mfma: small weights in P <= 3 signed byte digits |w_p| <= 128, M >= 16,
// 3 K < 2^17, rows of 32 K gather entries, fragments at off_w) and a digit splits into two int8 pieces: dg + 128 = (lo + 128) + 256 hi with hi <= 127 needs
// 2^dbc - 1 + 128 < 2^15, dbc <= 14 (then hi <= 64).  i32 head-room: a diagonal receives per term one lo x w_p product (<= 128 * 128) and one hi x w_(p-1) product
// (<= 64 * 128), K <= 43690 terms: 43690 * 24576 = 1 073 725 440 < 2^31.  N a multiple of 256: the column tiles of a slice are dealt to the 8 XCDs.
// A plan in the clipped + residual form (L.res) adds c and r products of one term into the same diagonal: |acc| <= (128 + 64) sum_k |w_k|, which must stay below 2^31.
// Otherwise the FP64 form k_digit_gemm with its own table of signed doubles (dbytes).
// int32 words for S ("digit_i32"): the plan's digit bound sum_max (2^dbc - 1) is at most 2^31 - 1; anything larger keeps doubles
template <class KEY> inline void gemm_digit_form(const DevConsts &hc, const GemmSwitches &sw, const GemmGroups<KEY> &gr, GemmLayout &L, std::vector<char> &dbytes) {
    if (!L.small || hc.k < 2 || hc.dbc < 1 || hc.dbc > 30) return;
    uint64_t qmin = ~0ull; for (uint32_t j = 0; j < hc.k; j++) qmin = std::min(qmin, hc.q[j].q);
    const uint64_t dmax = (1ull << hc.dbc) - 1, lim = std::min<uint64_t>((qmin - 1) / 2, (1ull << 52) - 1) / dmax;      // sum |w| <= lim
    const uint64_t sum_max = gemm_row_sum_max(hc, gr, lim);       // the plan's digit bound is sum_max (2^dbc - 1)
    if (sum_max > lim) return;
    L.dig = true; L.sum_abs_w = sum_max; L.dig_mfma = L.mfma && sw.digit_mfma && hc.dbc <= 14 && !(hc.n & 255) && (!L.res || sum_max * (128 + 64) < (1ull << 31)); L.dig_i32 = sw.digit_i32 && cn_digit_sum_fits_i32(sum_max, hc.dbc);
    if (L.dig_mfma) return;
    L.dMT = digit_gemm_tile(L.M); L.dKw = digit_gemm_rows(L.K);
    pack_gemm_f64(hc, gr, L.dMT, L.dKw, dbytes);
}

// ---------------------------------------------------------------- the image that reaches the device
// [gather | output members | bias entries | weights | digit weights], each on a 256-byte boundary (GemmLayout, cn_policy.h); E: int32_t or uint64_t entries
template <class E> inline void gemm_assemble(const std::vector<E> &gather, const std::vector<E> &outs, const std::vector<E> &bias, const std::vector<char> &wbytes,
                                             const std::vector<char> &dbytes, GemmLayout &L, std::vector<char> &image) {
    L.off_oidx = gemm_al(gather.size() * sizeof(E)); L.off_bidx = L.off_oidx + gemm_al(outs.size() * sizeof(E)); L.off_w = L.off_bidx + gemm_al(bias.size() * sizeof(E));
    L.off_dw = L.off_w + gemm_al(wbytes.size());
    image.assign(L.off_dw + gemm_al(dbytes.size()), 0);
    if (!gather.empty()) memcpy(image.data(), gather.data(), gather.size() * sizeof(E));
    if (!outs.empty()) memcpy(image.data() + L.off_oidx, outs.data(), outs.size() * sizeof(E));
    if (!bias.empty()) memcpy(image.data() + L.off_bidx, bias.data(), bias.size() * sizeof(E));
    if (!wbytes.empty()) memcpy(image.data() + L.off_w, wbytes.data(), wbytes.size());
    if (!dbytes.empty()) memcpy(image.data() + L.off_dw, dbytes.data(), dbytes.size());
}

// ---------------------------------------------------------------- the two planners
// Over indices: idx [O][K] (null: the identity, every output gathers inputs 0 .. K - 1), W [O][K] residues mod t, bias_idx [O] into a plaintext array of bias_count
// polynomials (null: no bias).  validate -> pair -> group -> form -> pack -> assemble; the reference's semantics: zero weights are skipped, an all-zero row is an error.
// max_in: one past the largest input gathered; nnz: non-zero, non-padded terms (statistics)
inline GemmRefusal gemm_plan_indices(const DevConsts &hc, const GemmSwitches &sw, const int32_t *idx, const uint64_t *W, uint32_t O, uint32_t K, const int32_t *bias_idx,
                                     uint32_t bias_count, GemmLayout &L, std::vector<char> &image, uint32_t &max_in, uint64_t &nnz) {
    if (!O || !K || !W) return gemm_refuse("empty scalar GEMM");
    std::vector<int32_t> gidx((size_t)O * K);
    for (uint32_t o = 0; o < O; o++) {
        bool any = false;
        for (uint32_t kk = 0; kk < K; kk++) {
            const int32_t id = idx ? idx[(size_t)o * K + kk] : (int32_t)kk;
            const uint64_t w = W[(size_t)o * K + kk];
            if (w >= hc.t.q) return gemm_refuse("weight >= plain modulus");
            if (id >= 0) max_in = std::max<uint32_t>(max_in, (uint32_t)id + 1);
            if (id >= 0 && w) { any = true; nnz++; }
            gidx[(size_t)o * K + kk] = id;
        }
        if (!any) { GemmRefusal r = gemm_refuse(""); snprintf(r.msg, sizeof r.msg, "output %u has no non-zero term (AddMany of nothing)", o); return r; }
        if (bias_idx && (bias_idx[o] < 0 || (uint32_t)bias_idx[o] >= bias_count)) return gemm_refuse("bias index out of range");
    }
    const GemmArith ar = gemm_arith(hc, sw, gemm_weights_small(hc, W, (size_t)O * K));      // (pairing adds only zero weights: the class stands)
    std::vector<uint64_t> W2;
    if (sw.gemm_pair && ar.small && pair_gather_lists(O, K, gidx, W, W2)) W = W2.data();
    GemmGroups<int32_t> gr = gemm_group(hc, sw, ar, gidx.data(), W, O, K);
    gemm_residual_form(hc, gr);
    std::vector<int32_t> hoidx(gr.member.size(), -1), hbidx(gr.member.size(), 0);           // output members relative to the output base, their bias polynomials
    for (size_t x = 0; x < gr.member.size(); x++) if (gr.member[x] != GEMM_NONE) { hoidx[x] = (int32_t)gr.member[x]; if (bias_idx) hbidx[x] = bias_idx[gr.member[x]]; }
    std::vector<char> wbytes, dbytes;
    gemm_form_and_pack(hc, ar, gr, L, wbytes);
    gemm_digit_form(hc, sw, gr, L, dbytes);
    gemm_assemble(gr.rows, hoidx, hbidx, wbytes, dbytes, L, image);
    return GemmRefusal();
}
// Over device addresses (a flush of the deferred queue): A [O][K] the address of every term (0 = padded tap), W [O][K], out [O] and bias [O] (0: none) the
// addresses of every call's output and folded bias polynomial.  The gather lists are not paired (flush_gemm_group, cn_defer.hip).
// Index tables instead of address tables (round 6).  Every array the library hands out starts on a 256-byte boundary, so the operands of a flush group are 32-bit offsets in units
// of 32 words from the lowest address among them - the INDEX-table kernels of a plan (one 16-byte scalar load per four gather entries, offsets multiplied on the scalar unit)
// instead of the address-table variants (two loads per four, a 64-bit select per term): dense layer 242 -> 221 us alone on the device, convolution 506 -> 492
// (310 with the gather lists paired, profiles/r06_defer_pair_ab.txt); end to end neutral.  Needs rel_on (CN_DEFER_REL), a bias on every output or on none, every offset
// a 256-byte multiple below 2^31 units; otherwise `abs`: the tables hold the addresses themselves
struct GemmAddressPlan {
    GemmLayout L; std::vector<char> image;
    bool abs = false, any_bias = false;
    uint64_t ibase = ~0ull, obase = ~0ull, bbase = ~0ull;        // index-table form: the lowest input / output / bias address
    uint64_t some_input = 0;                                     // address-table form: a valid input (read at padded taps)
};
inline void gemm_plan_addresses(const DevConsts &hc, const GemmSwitches &sw, const uint64_t *A, const uint64_t *W, const uint64_t *out, const uint64_t *bias, uint32_t O, uint32_t K,
                                bool rel_on, GemmAddressPlan &R) {
    const GemmArith ar = gemm_arith(hc, sw, gemm_weights_small(hc, W, (size_t)O * K));
    GemmGroups<uint64_t> gr = gemm_group(hc, sw, ar, A, W, O, K);
    gemm_residual_form(hc, gr);
    std::vector<uint64_t> hoidx(gr.member.size(), 0), hbidx(gr.member.size(), 0);
    bool all_bias = true;
    for (size_t x = 0; x < gr.member.size(); x++) if (gr.member[x] != GEMM_NONE) {
        hoidx[x] = out[gr.member[x]]; hbidx[x] = bias[gr.member[x]];
        R.any_bias = R.any_bias || hbidx[x]; all_bias = all_bias && hbidx[x];
    }
    for (uint64_t a : gr.rows) if (a && !R.some_input) R.some_input = a;
    std::vector<char> wbytes;
    gemm_form_and_pack(hc, ar, gr, R.L, wbytes);
    bool rel = rel_on && (!R.any_bias || all_bias);
    if (rel) {
        for (uint64_t a : gr.rows) if (a) R.ibase = std::min(R.ibase, a);
        for (uint64_t a : hoidx) if (a) R.obase = std::min(R.obase, a);
        for (uint64_t a : hbidx) if (a) R.bbase = std::min(R.bbase, a);
        auto fits = [](uint64_t a, uint64_t base) { return !a || (((a - base) & 255) == 0 && ((a - base) >> 8) < 0x7fffffffull); };
        for (uint64_t a : gr.rows) rel = rel && fits(a, R.ibase);
        for (uint64_t a : hoidx) rel = rel && fits(a, R.obase);
        for (uint64_t a : hbidx) rel = rel && fits(a, R.bbase);
        rel = rel && R.ibase != ~0ull && R.obase != ~0ull;
    }
    R.abs = !rel;
    if (R.abs) { gemm_assemble(gr.rows, hoidx, hbidx, wbytes, {}, R.L, R.image); return; }
    auto relative = [](const std::vector<uint64_t> &a, uint64_t base, int32_t none) {
        std::vector<int32_t> r(a.size(), none);
        for (size_t x = 0; x < a.size(); x++) if (a[x]) r[x] = (int32_t)((a[x] - base) >> 8);
        return r;
    };
    gemm_assemble(relative(gr.rows, R.ibase, -1), relative(hoidx, R.obase, -1), relative(hbidx, R.bbase, 0), wbytes, {}, R.L, R.image);
}
