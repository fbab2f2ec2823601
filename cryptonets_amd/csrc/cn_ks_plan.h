// One key switch, decided here and nowhere else: the kernel form `cnt` ciphertexts take, the arithmetic policy, the constants the kernels are launched with and the
// bytes of the shared arena (cn_ctx::ks_part) the form writes.  do_keyswitch, the rotations, the two-stream pipeline, the deferred queue and the launchers
// (cn_l_ks.inc.h) all read the same plan.  Host-only and free of HIP: a plain C++ compiler builds it (tests/cpp/ks_plan.cpp).
#pragma once
#include "../../include/cnhip.h"
#include "cn_policy.h"
#include <algorithm>

// what the decision reads of a context, by value (ks_switches in cn_eval.hip builds it)
struct KsSwitches {
    int ks_wide, ks_split14, ks_pair14, ks_xcd, ks_perm_fused;      // the options of that name (include/cnhip.h)
    bool rr;                  // the context runs register-radix kernels (rr_kernels)
    bool half_tables;         // it holds the half-size root tables of N = 16384 (DevConsts::twdh is a device address: only its presence is read)
    // (ciphertext, limb) blocks up to which the two-launch key switch runs one workgroup per DIGIT (above: per source limb; CN_KS_DIGIT_MAX), and up to which a
    // key switch runs as two launches at all (CN_KS_WIDE_MAX).  The fused kernel runs cnt k workgroups: up to 10 of them (1-2 ciphertexts) every digit gets its
    // own workgroup, up to 160 every source limb does; above that the fused kernel fills the chip by itself.
    // 10 since round 3 (32 before): with the four chains of an image on four hardware queues, per-source-limb workgroups cost the chip less for 3-6 ciphertexts
    // too (four chains 5.13-5.24 vs 5.36 ms per image, one chain alone unchanged; 50 / 65: 6.4 / 7.5 ms)
    uint32_t digit_max_blocks, wide_max_blocks;
    size_t arena_max;         // the two-launch forms fall back to the fused one when their partial products would need more bytes than this
};
enum KsForm {
    KS_LEGACY,        // k_keyswitch: radix-2 in LDS (N < 1024, "legacy_ntt"), no fused accumulator
    KS_FUSED,         // k_keyswitch_rr: one launch, a workgroup per (ciphertext, limb)
    KS_DIGIT_MAC,     // two launches: k_ks_digit_mac, a workgroup per (ciphertext, digit, limb), + k_ks_sum_intt
    KS_LIMB_MAC,      // two launches: k_ks_limb_mac, a workgroup per (ciphertext, source limb, limb), + k_ks_sum_intt
    KS_SPLIT14,       // N = 16384: k_keyswitch_split14, two 8192-point halves per limb, + k_ks_combine14
    KS_PAIR14         // N = 16384: k_keyswitch_pair14, both halves of a limb in one workgroup, one launch
};
struct KsPlan {
    KsForm form; int policy;      // policy: cn_policy of the q limbs by the form the key was loaded in (KsKey::f64), not by the "f64" option now
    uint32_t accmax;              // FP64 accumulators: terms between recentrings
    uint32_t xcd_cts;             // fused kernels: ciphertexts (a multiple of 8) placed XCD-aware, see k_keyswitch_rr
    size_t arena_bytes;           // of cn_ctx::ks_part: the partial products of the two-launch forms, the halves of the N = 16384 forms; 0: the form does not touch it
    bool twl;                     // KS_FUSED: the instantiation with LDS-resident forward twiddles
    bool whole;                   // KS_PAIR14: one digit per source limb that covers the limb (the reference's N = 16384 parameter sets, dbc 60): the digit is the word itself
};
// the LDS copy of the twiddle table pays once a workgroup runs enough digit transforms of its modulus
static const uint32_t KS_TWL_MIN_DIGITS = 12;

inline bool ks_two_launch(KsForm f) { return f == KS_DIGIT_MAC || f == KS_LIMB_MAC; }
// the two-launch form of `cnt` ciphertexts, KS_FUSED if they take none: forced by "ks_wide" 1 / 2, automatic (-1) by the (ciphertext, limb) blocks
inline KsForm ks_two_launch_form(const DevConsts &hc, const KsSwitches &sw, uint32_t cnt, int galois) {
    const uint32_t k = hc.k, tot = galois ? hc.gk_tot : hc.rl_tot;
    if (!(sw.rr && (sw.ks_wide > 0 || (sw.ks_wide < 0 && cnt * k <= sw.wide_max_blocks)))) return KS_FUSED;
    // N = 16384: 1024-thread workgroups cannot hold two accumulator sets without spilling -> per-digit only
    const bool limb = sw.ks_wide == 2 || (sw.ks_wide < 0 && cnt * k > sw.digit_max_blocks && hc.logn < 14);
    return (size_t)cnt * (limb ? k : tot) * 2 * k * hc.n * 8 > sw.arena_max ? KS_FUSED : (limb ? KS_LIMB_MAC : KS_DIGIT_MAC);
}
inline KsPlan cn_ks_plan(const DevConsts &hc, const KsSwitches &sw, bool key_f64, uint32_t cnt, int galois) {
    const uint32_t k = hc.k, tot = galois ? hc.gk_tot : hc.rl_tot;
    const size_t ct_bytes = (size_t)2 * k * hc.n * 8;
    const CnModRange qr = cn_mod_range(hc, 0, k);
    KsPlan p{ks_two_launch_form(hc, sw, cnt, galois), cn_policy(qr, key_f64), 0, 0, 0, false, false};
    const bool halves = sw.rr && hc.logn == 14 && sw.half_tables && key_f64 && sw.ks_split14;      // N = 16384 as 8192-point halves (FP64 policies)
    if (!ks_two_launch(p.form)) p.form = halves ? (sw.ks_pair14 ? KS_PAIR14 : KS_SPLIT14) : (sw.rr ? KS_FUSED : KS_LEGACY);
    p.accmax = key_f64 ? cn_f64_acc_interval(qr.bits) : 0xffffffffu;
    p.xcd_cts = sw.ks_xcd == 1 ? (cnt & ~7u) : (sw.ks_xcd == 2 ? 0x80000000u : 0u);
    switch (p.form) {
        case KS_DIGIT_MAC: p.arena_bytes = (size_t)cnt * tot * ct_bytes; break;
        case KS_LIMB_MAC: p.arena_bytes = (size_t)cnt * k * ct_bytes; break;
        case KS_SPLIT14: p.arena_bytes = (size_t)cnt * ct_bytes; break;
        case KS_PAIR14: {
            p.arena_bytes = (size_t)cnt * ct_bytes;
            p.xcd_cts = sw.ks_xcd == 1 ? (cnt & ~7u) : 0u;
            // lazy accumulators of THIS kernel: the forward half-transform (L = 13: five stages behind its one recentring) leaves |v| <= 4.82 q, a term
            // mulmod(v, key) is then at most (1/2 + 0.1875 x 4.82) q = 1.41 q (cn_ntt_core.hip.h), and 2^53 / q >= 16 for q < 2^49: 8 terms (+ the q/2 a recentred
            // accumulator starts from) stay below 11.8 q.  The generic bound above (2.1 q per term, sum below 2^52) allows 2 at 49 bits: a recentring of
            // both accumulator sets every other digit, 2 % of the kernel's FP64 instructions at the reference's N = 16384 parameters.
            if (!qr.light && qr.bits <= 49) p.accmax = std::max(p.accmax, 1u << (52 - qr.bits));
            const int dbc = galois ? hc.gdbc : hc.dbc;
            p.whole = tot == k && dbc < 64 && (qr.qmax >> dbc) == 0;
            break;
        }
        case KS_FUSED: p.twl = p.policy != POL_U64 && hc.logn <= 13 && tot >= KS_TWL_MIN_DIGITS; break;
        case KS_LEGACY: break;
    }
    return p;
}

// ---- readers for the callers around a key switch
// a rotation of `cnt` ciphertexts needs no permutation pass: its key switch takes a two-launch form, whose kernels apply the automorphism while they load c1 and c0
inline bool ks_perm_on_load(const DevConsts &hc, const KsSwitches &sw, uint32_t cnt) { return sw.ks_perm_fused && ks_two_launch(ks_two_launch_form(hc, sw, cnt, 1)); }
// ... and the largest count in [2, bound] of which that holds; 0: none
inline uint32_t ks_largest_perm_on_load(const DevConsts &hc, const KsSwitches &sw, uint32_t bound) {
    for (uint32_t c = bound; c >= 2; c--) if (ks_perm_on_load(hc, sw, c)) return c;
    return 0;
}
// the form keeps data in the context's ONE arena (and may re-allocate it): key switches on two streams must not both take such a form
inline bool ks_writes_arena(const KsPlan &p) { return p.arena_bytes != 0; }
// queued rotations by any step counts run as one launch chain per hop round (rotate_jobs) while they are few: by their blocks alone, whatever "ks_wide" says
inline bool ks_few_rotations(const DevConsts &hc, const KsSwitches &sw, size_t count) { return count * hc.k <= sw.wide_max_blocks; }

// ---- hoisted rotations (cn_rotate_rows_hoisted / cn_apply_galois_hoisted): n rotations of ONE ciphertext share the tot k forward transforms of its digits.
// Two launches: k_ks_digit_ntt, a workgroup per (digit, limb), leaves the transformed digits in the arena; k_ks_hoist_mac, a workgroup per (rotation, limb) - at
// N = 16384, where a 1024-thread workgroup has no room for two accumulator sets, per (rotation, limb, component) - reads them through the rotation's permutation.
// The kernels exist at every register-radix size under all three policies but N = 16384 under the integer policy (cn_ks_hoist_built): beside a 1024-thread
// workgroup's 128 registers per thread the integer inverse transform leaves no room for the rest of k_ks_hoist_mac even with one accumulator set (59 spilled
// registers when built) - refused here, as cn_plain_wide refuses the wide plaintext kernels there; the launchers instantiate by the same predicate.  N < 1024 and
// "legacy_ntt" are refused as well (as cn_encrypt_symmetric refuses them).  The arena is the context's ONE key-switch arena on its own stream: tot k N words,
// whatever n is.
constexpr bool cn_ks_hoist_built(int policy, uint32_t logn) { return logn >= 10 && logn <= 14 && !(policy == POL_U64 && logn == 14); }
struct KsHoistPlan {
    int rc; const char *msg;      // the refusal (0: none)
    int policy;                   // cn_policy of the q limbs by the form the keys were loaded in
    uint32_t accmax;              // FP64 accumulators: terms between recentrings (cn_f64_acc_interval: canonical words times key words, as in the fused kernel)
    size_t arena_bytes;           // of cn_ctx::ks_part: dig[tot][k][N]
    bool per_component;           // second launch: a workgroup per (rotation, limb, component) instead of per (rotation, limb)
    uint32_t blocks_ntt, blocks_mac;      // workgroups of the two launches
    uint64_t fwd_limbs, inv_limbs;        // what the call adds to ntt_forward_limbs / ntt_inverse_limbs
};
inline KsHoistPlan cn_ks_hoist_plan(const DevConsts &hc, const KsSwitches &sw, bool key_f64, uint32_t n) {
    const uint32_t k = hc.k, tot = hc.gk_tot;
    const CnModRange qr = cn_mod_range(hc, 0, k);
    KsHoistPlan p{0, nullptr, cn_policy(qr, key_f64), key_f64 ? cn_f64_acc_interval(qr.bits) : 0xffffffffu, (size_t)tot * k * hc.n * 8, hc.logn == 14, tot * k, 0, (uint64_t)tot * k, (uint64_t)n * 2 * k};
    p.blocks_mac = n * k * (p.per_component ? 2u : 1u);
    auto refuse = [&p](const char *text) { p.rc = CN_ERR_ARG; p.msg = text; p.arena_bytes = 0; p.blocks_ntt = p.blocks_mac = 0; p.fwd_limbs = p.inv_limbs = 0; return p; };
    if (!n) return refuse("hoisted rotations: an empty list");
    if (!sw.rr) return refuse("hoisted rotations need the register-radix kernels (1024 <= N <= 16384, \"legacy_ntt\" off)");
    if (key_f64 && !qr.f64ok) return refuse("internal: FP64 key without FP64 kernel");
    if (!cn_ks_hoist_built(p.policy, hc.logn)) return refuse("hoisted rotations: no kernel under the integer policy at N = 16384 (it does not fit a 1024-thread workgroup's registers)");
    if ((uint64_t)n * k * 2 > 0x7fffffffu) return refuse("hoisted rotations: too many rotations for one launch");
    return p;
}

// ---- summed rotations (cn_rotate_rows_sum / cn_apply_galois_sum): out_g = sum of rotations of DIFFERENT ciphertexts.  A key switch ends in INTT_j(acc) and the
// inverse transform is linear mod q_j, so the NTT-domain partial sums of all terms of an output are added BEFORE one pair of inverse transforms per output limb:
// the words of cn_apply_galois per term + cn_add_many, exactly.  Two launches for the last hop of every term:
//   1. the term MAC, part[term][P][2][k][N] with P partials per term: k_ks_digit_mac (a workgroup per (term, digit, limb), P = gk_tot) or k_ks_limb_mac (per (term,
//      source limb, limb), P = k; N <= 8192) with their KsItem table while the terms are few - they leave exactly these partials -, k_ks_term_mac (per (term, limb);
//      N <= 8192) with P = 1 when they are many;
//   2. k_ks_sum_terms, a workgroup per (output, limb, component): the sum over the output's terms and their P partials, ONE inverse transform, + s_g(c0) of every
//      rotated term (component 0), + both components of every unrotated term.
// Where this does not run the call COMPOSES the literal sequence through a temporary (same words): no register-radix kernels (N < 1024, "legacy_ntt"), the integer
// policy at N = 16384 (cn_ks_sum_built), an arena above KsSwitches::arena_max even at the coarsest granularity.
// The thresholds between the granularities START from digit_max_blocks / wide_max_blocks of the plain key switch, counted in (term, limb) blocks: per digit up to
// the first, per source limb up to the second, per term above.  N = 16384 runs per digit whatever the count: a 1024-thread workgroup (128 registers per thread)
// has no room for two accumulator sets (k_ks_limb_mac) and, beside a 16384-point forward transform, not even for one (cn_ks_term_built) - the 126 giant steps of
// the CIFAR layer (k = 8, 8 digits) are 2 GiB of per-digit partials, inside the default arena_max.  NOBODY HAS MEASURED THEM FOR THIS CALL (tools/rotation_sum_probe.py
// varies them through CN_KS_DIGIT_MAX / CN_KS_WIDE_MAX).  A granularity whose partials exceed arena_max gives way to the next coarser one.
// The settle interval of the second launch: a per-digit partial is ONE lazy product, |x| <= 2.1 q (cn_f64_acc_interval's term), per-limb and per-term partials
// leave recentred, |x| <= q / 2; k_ks_sum_terms recentres every `settle` additions, so its sums stay within q / 2 + settle 2.1 q, and settle =
// cn_f64_acc_interval(bits) = 2^(50 - bits) keeps that below 2^52 for q < 2^bits - the rule of k_ks_sum_intt, whatever the number of terms
// (tests/cpp/ks_sum_plan.cpp sums the worst case).
constexpr bool cn_ks_sum_built(int policy, uint32_t logn) { return logn >= 10 && logn <= 14 && !(policy == POL_U64 && logn == 14); }
constexpr bool cn_ks_term_built(int policy, uint32_t logn) { return cn_ks_sum_built(policy, logn) && logn <= 13; }
enum KsSumForm { KS_SUM_COMPOSE, KS_SUM_DIGIT, KS_SUM_LIMB, KS_SUM_TERM };
static const uint32_t KS_SUM_TERM_MILLI_Q = 2100;      // |partial| <= 2.1 q: what the settle interval rests on
struct KsSumPlan {
    KsSumForm form; const char *why;      // the granularity of the first launch, or "compose" and its reason
    int policy;                           // cn_policy of the q limbs by the form the keys were loaded in
    uint32_t accmax;                      // first launch (k_ks_limb_mac, k_ks_term_mac): terms between recentrings
    uint32_t settle;                      // second launch: additions between recentrings
    uint32_t partials;                    // per term: gk_tot (per digit), k (per source limb) or 1 (per term)
    size_t arena_bytes;                   // of cn_ctx::ks_part: part[rotated][partials][2][k][N]
    uint32_t blocks_mac, blocks_sum;      // workgroups of the two launches
    uint64_t fwd_limbs, inv_limbs;        // what the two launches add to ntt_forward_limbs / ntt_inverse_limbs
};
// rotated: terms with a key switch (their LAST hop runs here); outputs: groups that hold at least one of them
inline KsSumPlan cn_ks_sum_plan(const DevConsts &hc, const KsSwitches &sw, bool key_f64, uint32_t terms, uint32_t rotated, uint32_t outputs) {
    const uint32_t k = hc.k, tot = hc.gk_tot;
    const CnModRange qr = cn_mod_range(hc, 0, k);
    const uint32_t interval = key_f64 ? cn_f64_acc_interval(qr.bits) : 0xffffffffu;
    KsSumPlan p{KS_SUM_COMPOSE, nullptr, cn_policy(qr, key_f64), interval, interval, 0, 0, 0, 0, 0, 0};
    auto compose = [&p](const char *text) { p.why = text; return p; };
    if (!rotated || !outputs || rotated > terms) return compose("no rotated term");
    if (!sw.rr) return compose("no register-radix kernels (N < 1024 or \"legacy_ntt\")");
    if (key_f64 && !qr.f64ok) return compose("FP64 keys without FP64 kernels");
    if (!cn_ks_sum_built(p.policy, hc.logn)) return compose("no kernel under the integer policy at N = 16384");
    if ((uint64_t)rotated * tot * k > 0x7fffffffu) return compose("too many terms for one launch");
    const uint64_t blocks = (uint64_t)rotated * k;
    const size_t ct_bytes = (size_t)2 * k * hc.n * 8;
    auto fits = [&](uint32_t partials) { return (size_t)rotated * partials * ct_bytes <= sw.arena_max; };
    if (blocks <= sw.digit_max_blocks || hc.logn == 14) p.form = KS_SUM_DIGIT;
    else if (blocks <= sw.wide_max_blocks) p.form = KS_SUM_LIMB;
    else p.form = KS_SUM_TERM;
    if (p.form == KS_SUM_DIGIT && !fits(tot) && hc.logn < 14) p.form = KS_SUM_LIMB;      // the coarser granularity first
    if (p.form == KS_SUM_LIMB && !fits(k)) p.form = KS_SUM_TERM;
    if (p.form == KS_SUM_TERM && !cn_ks_term_built(p.policy, hc.logn)) p.form = KS_SUM_COMPOSE;
    p.partials = p.form == KS_SUM_DIGIT ? tot : (p.form == KS_SUM_LIMB ? k : 1);
    if (p.form == KS_SUM_COMPOSE || !fits(p.partials)) { p.form = KS_SUM_COMPOSE; p.partials = 0; return compose("the partial products would not fit the key-switch arena"); }
    p.arena_bytes = (size_t)rotated * p.partials * ct_bytes;
    p.blocks_mac = rotated * p.partials * k; p.blocks_sum = outputs * k * 2;
    p.fwd_limbs = (uint64_t)rotated * tot * k; p.inv_limbs = (uint64_t)outputs * 2 * k;
    return p;
}

// ---- the call shapes a form does not take (internal errors: a caller asked the wrong reader)
struct KsShape { bool dig, perm_elt, items, next_elt; };      // KsCall: ready-made digits; automorphism on load; per-ciphertext operand table; sigma_next(c1) on the side
struct KsRefusal {
    int rc = 0; const char *msg = nullptr;
    explicit operator bool() const { return rc != 0; }
};
inline KsRefusal ks_refusal(const DevConsts &hc, const KsPlan &p, bool key_f64, int galois, const KsShape &s) {
    if (s.dig && !(p.form != KS_LEGACY && key_f64 && hc.logn <= 13 && !galois && !hc.ks_xi)) return {CN_ERR_ARG, "internal: ready-made digits outside the FP64 register-radix key switch"};
    if ((s.perm_elt || s.items || s.next_elt) && !ks_two_launch(p.form) && !(p.form == KS_PAIR14 && !s.items)) return {CN_ERR_ARG, "internal: automorphism inside the fused key switch"};
    if (p.form == KS_LEGACY && key_f64) return {CN_ERR_ARG, "internal: FP64 key without FP64 kernel"};
    return {};
}
