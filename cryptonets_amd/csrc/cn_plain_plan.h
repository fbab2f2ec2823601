// One plaintext product, decided here and nowhere else: the form a MultiplyPlain of `count` ciphertexts takes, its scratch arrays and what it counts; the SumAllSlots
// sequence and whether it runs as the one-launch chain; the arena of a chained row-dot batch; kernel or composition, accumulator interval and scratch of
// cn_mul_plain_sum and the index work in front of it.  mul_plain_impl, sum_slots_impl, cn_rowdot_batch, cn_sum_slots and cn_mul_plain_sum (cn_eval.hip) read the same
// plans; the deferred flush runs the first two.  Host-only and free of HIP: a plain C++ compiler builds it (tests/cpp/plain_plan.cpp).
#pragma once
#include "cn_policy.h"
#include "cn_ks_plan.h"
#include "cn_rotation.h"
#include <unordered_map>
#include <vector>

// what the decisions read of a context, by value (plain_switches in cn_eval.hip builds it)
struct PlainSwitches {
    int f64, mp_fused, mp_bcast, ks_chain, ptn_order;      // the options of that name (include/cnhip.h)
    bool rr;                                               // the context runs register-radix kernels (rr_kernels)
    KsSwitches ks;
};
inline int plain_policy(const DevConsts &hc, const PlainSwitches &sw) { return cn_policy(cn_mod_range(hc, 0, hc.k), sw.f64 != 0); }

// ---- MultiplyPlain: out[c] = a[c * (a_bcast ? 0 : 1)] * pt[c * pstride]
enum PlainForm {
    PLAIN_BCAST,          // one ciphertext x many plaintexts: the ciphertext transformed once into `ctn`, then k_mul_plain_bcast (it transforms coefficient-form rows itself)
    PLAIN_PTN_FUSED,      // NTT-form plaintexts: k_mul_plain_fused alone, reading the array where it lies
    PLAIN_LIFT_FUSED,     // coefficient-form plaintexts: k_lift_ntt into `lift`, then k_mul_plain_fused
    PLAIN_LEGACY          // "mp_fused" 0, "legacy_ntt", N < 1024: k_lift_plain + transform of the plaintexts, transforms of the ciphertexts around k_dyadic_pt
};
enum PlainArray { PLAIN_CTN, PLAIN_KEEP, PLAIN_LIFT, PLAIN_ARRAYS };      // the transformed ciphertext; the copy of a broadcast source that an output overwrites; the lifted plaintexts
struct PlainCall {
    uint32_t count, polys, pstride; bool ntt;      // pstride: plaintexts apart (0: one for every ciphertext); ntt: rows of an NTT-form array
    bool a_bcast;         // ONE ciphertext against `count` plaintexts
    bool chain;           // a SumAllSlots chain follows and wants sigma(c1) of every product beside it (BcastNext: its arena holds `ctn`, so none is listed here)
    bool alias;           // the broadcast source lies inside the outputs (a pointer fact: the caller computes it)
};
struct PlainPlan {
    PlainForm form; int policy;
    struct { PlainArray id; size_t bytes; } scratch[PLAIN_ARRAYS]; uint32_t arrays;      // what mul_plain_impl allocates, in this order
    uint32_t launches, ptn_bcast;      // what the product itself counts, beside the launches and limbs cn_run_ntt counts for the transforms it runs
    uint64_t fwd_limbs, inv_limbs;
    const char *refusal;               // an internal error: a caller asked for a hand-over the form cannot give
};
// the one-launch product of ONE ciphertext with many plaintexts (also what lets a row-dot batch hand its chain the first link: rowdot_plan)
inline bool plain_takes_bcast(const DevConsts &hc, const PlainSwitches &sw, const PlainCall &c) {
    return sw.mp_fused && sw.rr && c.a_bcast && c.pstride && c.count >= 4 && sw.mp_bcast && !(c.ntt && !cn_plain_wide(plain_policy(hc, sw), hc.logn));
}
inline PlainPlan cn_plain_plan(const DevConsts &hc, const PlainSwitches &sw, const PlainCall &c) {
    const size_t kn = (size_t)hc.k * hc.n, item = c.polys * kn, npt = c.pstride ? c.count : 1;
    const uint64_t limbs = (uint64_t)c.count * c.polys * hc.k;
    PlainPlan p{};
    p.policy = plain_policy(hc, sw);
    auto need = [&](PlainArray id, size_t words) { p.scratch[p.arrays].id = id; p.scratch[p.arrays++].bytes = words * 8; };
    if (!(sw.mp_fused && sw.rr)) {
        p.form = PLAIN_LEGACY;
        if (!c.ntt) need(PLAIN_LIFT, npt * kn);
        p.launches = c.ntt ? 1 : 2;
    } else if (plain_takes_bcast(hc, sw, c)) {
        p.form = PLAIN_BCAST;
        if (!c.chain) need(PLAIN_CTN, item);
        p.launches = 1; p.ptn_bcast = c.ntt;
        p.fwd_limbs = c.ntt ? 0 : limbs; p.inv_limbs = limbs;      // (NTT-form rows: no transform of the plaintexts runs)
    } else if (c.ntt) {
        p.form = PLAIN_PTN_FUSED;
        if (c.a_bcast && c.alias) need(PLAIN_KEEP, item);
        p.launches = 1; p.fwd_limbs = p.inv_limbs = limbs;
    } else {
        p.form = PLAIN_LIFT_FUSED;
        need(PLAIN_LIFT, npt * kn);
        if (c.a_bcast && c.alias) need(PLAIN_KEEP, item);
        p.launches = 2; p.fwd_limbs = npt * hc.k + limbs; p.inv_limbs = limbs;
    }
    if (c.chain && p.form != PLAIN_BCAST) p.refusal = "internal: chained row-dot batch outside the broadcast product";
    return p;
}

// ---- SumAllSlots(length) of AtomicSealBfvVector.cs:888-935: the column swap when length >= N/2, then rotate-and-add by -1, -2, -4 ... below length (0 = all N slots)
struct SumSlotsSeq { bool columns; uint32_t rows; };      // rows: the steps -(1 << i), i < rows
inline SumSlotsSeq sum_slots_seq(uint32_t n, uint32_t length) {
    uint32_t len = length ? length : n;
    SumSlotsSeq s{len >= n / 2, 0};
    if (s.columns) len = n / 2;
    for (uint32_t steps = 1; steps < len; steps *= 2) s.rows++;
    return s;
}
inline std::vector<uint64_t> sum_slots_elts(uint32_t n, uint32_t length) {
    const SumSlotsSeq s = sum_slots_seq(n, length);
    std::vector<uint64_t> elts;
    if (s.columns) elts.push_back(2ull * n - 1);
    for (uint32_t i = 0; i < s.rows; i++) elts.push_back(cn_elt_of_step(n, -(int)(1u << i)));
    return elts;
}
// the elements of the sequence if the whole of it runs on the one-launch key switch with every link handing sigma_next(c1) on (N = 16384, batch); else empty.
// key_form(elt): -1 no key, else the form it was loaded in (KsKey::f64)
template <class KeyForm> inline std::vector<uint64_t> sum_slots_plan(const DevConsts &hc, const PlainSwitches &sw, uint32_t count, uint32_t length, KeyForm key_form) {
    std::vector<uint64_t> elts;
    if (!sw.ks_chain || !count) return elts;
    elts = sum_slots_elts(hc.n, length);
    bool ok = elts.size() >= 2;
    for (size_t i = 0; i < elts.size() && ok; i++) { const int f = key_form(elts[i]); ok = f >= 0 && cn_ks_plan(hc, sw.ks, f != 0, count, 1).form == KS_PAIR14; }
    if (!ok) elts.clear();
    return elts;
}

// ---- cn_rowdot_batch: `rows` broadcast products and their SumAllSlots.  Chained: the product kernel hands the chain its first permuted c1 (no k_galois_limbs pass over
// the products) through ONE arena, sized once and left where it is until the chain has run: at chain_off the chain's ping-pong pair (pp_bytes: rows ciphertexts), behind
// it the transformed ciphertext (ctn_bytes)
struct RowdotPlan {
    std::vector<uint64_t> chain;      // empty: product, then sum_slots_impl on its own
    size_t pp_bytes, ctn_bytes;
    static constexpr size_t chain_off = 0;
};
template <class KeyForm> inline RowdotPlan rowdot_plan(const DevConsts &hc, const PlainSwitches &sw, uint32_t rows, uint32_t length, bool ntt, KeyForm key_form) {
    const size_t ct_bytes = (size_t)2 * hc.k * hc.n * 8;
    RowdotPlan r{{}, rows * ct_bytes, ct_bytes};
    if (length != 1 && plain_takes_bcast(hc, sw, {rows, 2, 1, ntt, true, false, false})) r.chain = sum_slots_plan(hc, sw, rows, length, key_form);
    return r;
}

// ---- cn_mul_plain_sum: G groups, E terms
struct PlainSumPlan {
    bool kernel;          // false: composed of cn_mul_plain per term and AddMany per group ("mp_fused" 0, no register-radix kernels, no wide kernel)
    int policy;
    uint32_t accmax;      // terms between recentrings of the lazy FP64 accumulators (0xffffffff: the integer policy has none)
    uint32_t order;       // k_mul_ptn_sum: workgroup order ("ptn_order")
    size_t src_bytes, grp_bytes, slot_bytes;      // scratch: one transformed source ciphertext (times the distinct sources), the group offsets, the slots
};
inline PlainSumPlan plain_sum_plan(const DevConsts &hc, const PlainSwitches &sw, bool ntt, uint32_t G, uint32_t E) {
    const CnModRange qr = cn_mod_range(hc, 0, hc.k);
    PlainSumPlan p{false, cn_policy(qr, sw.f64 != 0), 0xffffffffu, (uint32_t)sw.ptn_order, (size_t)2 * hc.k * hc.n * 8, ((size_t)G + 1) * 4, (size_t)E * 4};
    p.kernel = sw.mp_fused && sw.rr && cn_plain_wide(p.policy, hc.logn);
    if (p.policy != POL_U64) p.accmax = ntt ? cn_ptn_sum_interval(qr.qmax) : cn_f64_acc_interval(qr.bits);
    return p;
}
// the distinct ciphertexts of the term list in order of first appearance (-> slots of the NTT-form scratch copy), the slot of every term, and the runs of
// neighbouring sources that travel in one copy (baby steps: one run)
struct PlainSumSlots {
    std::vector<uint32_t> slot, src;
    struct Run { uint32_t first, len; };      // slots [first, first + len) hold the ciphertexts src[first], src[first] + 1, ...
    std::vector<Run> runs;
};
inline PlainSumSlots plain_sum_slots(const uint32_t *ct_idx, uint32_t E) {
    PlainSumSlots s;
    s.slot.resize(E);
    std::unordered_map<uint32_t, uint32_t> seen;
    for (uint32_t e = 0; e < E; e++) {
        auto it = seen.find(ct_idx[e]);
        if (it == seen.end()) { it = seen.emplace(ct_idx[e], (uint32_t)s.src.size()).first; s.src.push_back(ct_idx[e]); }
        s.slot[e] = it->second;
    }
    for (uint32_t i = 0, D = (uint32_t)s.src.size(); i < D;) {
        uint32_t r = 1;
        while (i + r < D && s.src[i + r] == s.src[i] + r) r++;
        s.runs.push_back({i, r});
        i += r;
    }
    return s;
}
