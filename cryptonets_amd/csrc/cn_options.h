// The switches and counters of a context, in one place: the struct of each, the table that gives every switch its option name, range and environment override, the table
// that names every counter, and the three functions over them - defaults for a ring size, environment overrides, set / get by name.  ctx_init, cn_set_option and
// cn_get_option (cn_api.hip) are the callers; a level context copies CnTunables whole (cn_level.hip).  Host-only and free of HIP: a plain C++ compiler builds it
// (tests/cpp/options.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

// Per-context tuning switches, all producing the same words.  Names, ranges and environment overrides: kOptions below (cn_set_option / cn_get_option,
// include/cnhip.h); a level context copies them from its parent whole.  Booleans are 0 / 1.
// Switches removed after their variants measured no gain: staggered squaring groups in the flush (profiles/r06_stagger_ab.txt), the q side of a batched squaring on the
// second stream (profiles/r06_square_overlap.txt), the 128-VGPR fused key switch (profiles/HISTORY.md, round 1).
struct CnTunables {
    int f64 = 1;              // transforms of moduli < 2^49 and key switching in exact FP64; 0 (CN_NO_F64=1): integer (Shoup) transforms everywhere
    int legacy_ntt = 0;       // 1: radix-2 LDS kernels (the only ones below N = 1024)
    int gemm_order = 1;       // scalar GEMM (VALU kernels): 1 = slice-major workgroup order (every input slice fetched once per XCD), 0 = group-major
    int ks_perm_fused = 1;    // rotations through the two-launch key switch apply the automorphism while loading (no k_galois_lds pass)
    int ks_xcd = 0;           // fused key switch, workgroup order: 0 (ciphertext, limb); 1 the k workgroups of a ciphertext on one XCD (share its source limbs in
                              // that L2); 2 limb-major (one key slice per XCD L2 at a time).  Default by N (cn_option_defaults)
    int sq_fused = 1;         // squarings: forward transforms + tensor + inverse transforms in one kernel; 0 = separate launches
    int sq_lds = 1;           // fused squaring with the NTT-form operand parked in LDS (N <= 8192) - HBM traffic = the algorithmic 2 reads + 3 writes per
                              // block (profiles/r02_pmc_square_gemm.txt); 0: parked in the outputs' place (two workgroups per CU)
    int sq_pipe = 1;          // 1: fused squaring of a batch (>= 4 blocks per resident workgroup) on the pipelined resident kernel k_square_pipe; 0: k_square_fused; 2: k_square_pipe for any count (tests)
    int sq_halves = 1;        // Multiply + Relinearize of >= 512 ciphertexts (N <= 8192) in parts software-pipelined over the context's two streams (pipelined_halves,
                              // cn_api_shared.h).  1: the batched entry point cn_mul_relin; 2: also the queued per-ciphertext calls of a flush (measured slower there); 0: off
    int enc_fused = 2;        // 2: a block per (ciphertext, component, limb) - k_encrypt_split, two workgroups per CU: 420 against 542 us per 784 ciphertexts; 1: one block per
                              // (ciphertext, limb) behind the samplers (k_encrypt_fused, N <= 8192); 0: expand + batched transform + k_encrypt_tail
    int fold_zero = 1;        // queued fresh encryptions of zero whose only reader is a queued scalar product and which have been released: folded by linearity (k_encrypt_fold); 0: materialised
    int gemm_mfma = 1;        // scalar GEMMs with >= 16 outputs per gather list on the int8 matrix cores (exact); 0: FP64 kernel
    int gemm_pair = 1;        // planned scalar GEMMs: gather lists that share at least half of their inputs are merged in pairs (pair_gather_lists); 0: the caller's lists
    int mp_fused = 1;         // dense MultiplyPlain as k_lift_ntt + k_mul_plain_fused; 0 = the six separate launches
    int ks_wide = -1;         // -1 auto (small batches), 0 fused kernel, 1 two-launch with a workgroup per digit, 2 two-launch per source limb
    int ks_split14 = 1;       // N = 16384: key switch as two 8192-point halves per limb (no register spills); 0 = fused 1024-thread kernel
    int ks_pair14 = 1;        // ... both halves in ONE launch per rotation (k_keyswitch_pair14); 0 = k_keyswitch_split14 + k_ks_combine14 (+ k_galois_lds)
    int ks_chain = 1;         // SumAllSlots at N = 16384: every link of the rotate-and-add chain hands sigma_next(c1) to the next one (no permutation pass between links)
    int mp_bcast = 1;         // one ciphertext x many plaintexts (row-dot batches) as ONE launch that transforms the plaintexts (k_mul_plain_bcast); 0: k_lift_ntt + k_mul_plain_fused
    int mul_sum = 1;          // cn_mul_relin_sum sums the unrelinearized products and runs one key switch per output where it can (k_product_sum, the same words); 0: always
                              // Multiply + Relinearize per term and AddMany
    int digit_mfma = 1;       // plans made from now on run their digit GEMM on the int8 matrix cores where they can (k_digit_gemm_mfma, exact); 0: always the FP64 kernel k_digit_gemm
    int digit_i32 = 1;        // plans made from now on (and cn_mul_relin_sum calls) hand their digit sums S to the key switch as int32 words where the bound allows it
                              // (cn_digit_sum_fits_i32, cn_policy.h: half the bytes of S); 0: always doubles
    int defer_square_gemm = 0;   // (default 0: its effect on the literal call sequence has not been measured, profiles/deferred_square_gemm.md): queued squarings launched by a
                              // layer-boundary flush keep their relinearisation back; scalar products that read nothing else run as cn_square_gemm's second half - one key switch
                              // per dense OUTPUT (cn_defer.hip); 0: every queued squaring relinearises at once
    int sg_prefloor = 1;      // cn_square_gemm - 1 = components 0 and 1 take ONE floor tail per dense output where square_gemm_prefloor_ok allows (cn_mul_plan.h: layers of at
                              // least SG_PREFLOOR_MIN_K terms); 0 = every product is floored (the old form); 2 = the new form for any K (tests).  The same words
    int ptn_order = 0;        // k_mul_ptn_sum, workgroup order: 0 limb-major, 1 limb = workgroup index mod k (a limb per XCD at k = 8)
};
// What a context counts, each read back under its name in kCounters
struct CnCounters {
    uint64_t folded_zero = 0;     // zero encryptions folded so far
    uint64_t mr_pipelined = 0;    // cn_mul_relin chunks and flushed Multiply + Relinearize groups that ran through pipelined_halves
    uint64_t sg_fused = 0;        // cn_square_gemm calls that ran the one-key-switch-per-output form
    uint64_t sg_prefloor = 0;     // ... of which in the pre-floor form: one floor tail per dense output for components 0 and 1
    uint64_t dsg_fused = 0;       // groups of queued scalar products that ran on deferred squarings in the one-key-switch-per-output form
    uint64_t dg_mfma = 0;         // digit GEMMs launched in the matrix-core form
    uint64_t ms_fused = 0;        // cn_mul_relin_sum calls that ran one key switch per output
    uint64_t ks_dig_i32 = 0;      // key switches launched on int32 digit sums
    uint64_t ptn_sum = 0, ptn_bcast = 0;       // launches of k_mul_ptn_sum / of k_mul_plain_bcast on NTT-form plaintexts
    uint64_t diag_scan = 0, diag_encode = 0;   // launches of k_diag_scan / of k_diag_gather
};

// A flag stores "non-zero = on"; an enumerated switch refuses a value outside lo..hi, its environment override (read at creation) is clamped into the range.
// replan: plans made earlier were built under the old value and must be dropped (the switches build_gemm_plan reads: gemm_switches, cn_eval.hip).
struct OptionSpec { const char *name; int CnTunables::*member; int lo, hi; bool flag; const char *env; bool replan; };
static const OptionSpec kOptions[] = {
    {"f64",               &CnTunables::f64,               0, 1, true,  nullptr,         true},    // environment: CN_NO_F64 (cn_options_from_env); affects keys uploaded AFTER the call
    {"legacy_ntt",        &CnTunables::legacy_ntt,        0, 1, true,  "CN_LEGACY_NTT", false},
    {"gemm_order",        &CnTunables::gemm_order,        0, 1, false, "CN_GEMM_ORDER", false},
    {"ks_perm_fused",     &CnTunables::ks_perm_fused,     0, 1, true,  nullptr,         false},
    {"ks_xcd",            &CnTunables::ks_xcd,            0, 2, false, "CN_KS_XCD",     false},   // default by N (cn_option_defaults)
    {"sq_fused",          &CnTunables::sq_fused,          0, 1, true,  "CN_SQ_FUSED",   false},
    {"sq_lds",            &CnTunables::sq_lds,            0, 1, true,  "CN_SQ_LDS",     false},
    {"sq_pipe",           &CnTunables::sq_pipe,           0, 2, false, "CN_SQ_PIPE",    false},
    {"sq_halves",         &CnTunables::sq_halves,         0, 2, false, "CN_SQ_HALVES",  false},
    {"enc_fused",         &CnTunables::enc_fused,         0, 2, false, "CN_ENC_FUSED",  false},
    {"fold_zero",         &CnTunables::fold_zero,         0, 1, true,  "CN_FOLD_ZERO",  false},
    {"gemm_mfma",         &CnTunables::gemm_mfma,         0, 1, true,  "CN_GEMM_MFMA",  true},    // affects GEMMs planned AFTER the call
    {"gemm_pair",         &CnTunables::gemm_pair,         0, 1, true,  "CN_GEMM_PAIR",  true},    // likewise
    {"mp_fused",          &CnTunables::mp_fused,          0, 1, true,  "CN_MP_FUSED",   false},
    {"ks_wide",           &CnTunables::ks_wide,          -1, 2, false, nullptr,         false},
    {"ks_split14",        &CnTunables::ks_split14,        0, 1, true,  nullptr,         false},
    {"ks_pair14",         &CnTunables::ks_pair14,         0, 1, true,  "CN_KS_PAIR14",  false},
    {"ks_chain",          &CnTunables::ks_chain,          0, 1, true,  "CN_KS_CHAIN",   false},
    {"mp_bcast",          &CnTunables::mp_bcast,          0, 1, true,  nullptr,         false},
    {"mul_sum",           &CnTunables::mul_sum,           0, 1, true,  nullptr,         false},
    {"digit_mfma",        &CnTunables::digit_mfma,        0, 1, true,  nullptr,         true},    // the digit GEMM of plans made AFTER the call
    {"digit_i32",         &CnTunables::digit_i32,         0, 1, true,  nullptr,         true},    // the digit sums of plans made AFTER the call (and of cn_mul_relin_sum)
    {"defer_square_gemm", &CnTunables::defer_square_gemm, 0, 1, true,  nullptr,         false},   // (cn_set_option's lock has settled what the queue held back under the old value)
    {"sg_prefloor",       &CnTunables::sg_prefloor,       0, 2, false, nullptr,         false},
    {"ptn_order",         &CnTunables::ptn_order,         0, 1, false, "CN_PTN_ORDER",  false},
};
struct CounterSpec { const char *name; uint64_t CnCounters::*member; };
static const CounterSpec kCounters[] = {
    {"folded_zero_encryptions", &CnCounters::folded_zero}, {"mul_relin_pipelined", &CnCounters::mr_pipelined}, {"square_gemm_fused", &CnCounters::sg_fused},
    {"square_gemm_prefloor", &CnCounters::sg_prefloor}, {"defer_square_gemm_fused", &CnCounters::dsg_fused}, {"digit_gemm_mfma", &CnCounters::dg_mfma},
    {"mul_sum_fused", &CnCounters::ms_fused}, {"ks_digits_i32", &CnCounters::ks_dig_i32}, {"ptn_sum", &CnCounters::ptn_sum}, {"ptn_bcast", &CnCounters::ptn_bcast},
    {"diag_scan", &CnCounters::diag_scan}, {"diag_encode", &CnCounters::diag_encode},
};

// the switches of a new context of N = 2^logn
// fused key switch, workgroup order: limb-major up to N = 8192 (one key slice per XCD L2 at a time: 2.34 GiB fetched per 845-ciphertext launch against 3.99 GiB in
// (ciphertext, limb) order and 3.0 GiB with the limbs of a ciphertext on one XCD, same kernel time - profiles/r03_pmc_keyswitch_orders.txt); at N = 16384, where
// limb-major measured 30 % slower in round 1 (k_keyswitch_pair14): the k workgroups of a ciphertext on one XCD - they share its source limbs in that L2 (34.3 vs
// 35.1 ms per 5488-ciphertext link)
inline CnTunables cn_option_defaults(uint32_t logn) { CnTunables t; t.ks_xcd = logn <= 13 ? 2 : 1; return t; }
// the environment overrides, read through env(name) -> text or null (ctx_init: getenv)
template <class Env> void cn_options_from_env(CnTunables &t, Env env) {
    if (const char *e = env("CN_NO_F64")) t.f64 = !atoi(e);
    for (const OptionSpec &o : kOptions)
        if (const char *e = o.env ? env(o.env) : nullptr) t.*o.member = o.flag ? atoi(e) != 0 : std::max(o.lo, std::min(o.hi, atoi(e)));
}
inline const OptionSpec *cn_find_option(const char *name) {
    for (const OptionSpec &o : kOptions) if (!strcmp(name, o.name)) return &o;
    return nullptr;
}
// set by name: null = no switch of that name; *refused: the value lies outside the row's range and nothing changed
inline const OptionSpec *cn_option_set(CnTunables &t, const char *name, int value, bool *refused) {
    const OptionSpec *o = cn_find_option(name);
    *refused = o && !o->flag && (value < o->lo || value > o->hi);
    if (o && !*refused) t.*o->member = o->flag ? value != 0 : value;
    return o;
}
// get by name, a switch or a counter (which saturates); false = neither
inline bool cn_option_get(const CnTunables &t, const CnCounters &cnt, const char *name, int *value) {
    if (const OptionSpec *o = cn_find_option(name)) { *value = t.*o->member; return true; }
    for (const CounterSpec &c : kCounters) if (!strcmp(name, c.name)) { *value = (int)std::min<uint64_t>(cnt.*c.member, 0x7fffffff); return true; }
    return false;
}
