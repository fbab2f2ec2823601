// The two decisions every launch starts from, taken here and nowhere else: the arithmetic policy of a modulus range and whether a ring size has the
// register-radix kernels.  Host-only and free of HIP: a plain C++ compiler builds it (tests/cpp/policy_table.cpp).
#pragma once
#include "cn_internal.h"

enum { POL_U64 = 0, POL_F64 = 1, POL_F64L = 2 };       // ArU64 (Shoup, any modulus), ArF64 (< 2^49.4), ArF64L (<= 44 bits: no forward recentring)

// Moduli [base_off, base_off + nmod) in the order of the twiddle tables: m < k is q_m, k <= m < k + kb is bsk_(m-k), k + kb is the plain modulus t.  The unit of
// decision is the range, not the context: c3 takes ArF64L for its q limbs and for t, ArF64 for its 49-bit BEHZ auxiliary base
struct CnModRange {
    bool f64ok;        // every modulus has its FP64 tables (DevConsts::f64ok: below 2^49, and t only when batching)
    bool light;        // no modulus has a bit at or above bit 44
    int bits;          // bit length of qmax (0: empty range)
    uint64_t qmax;     // the largest modulus
};
inline CnModRange cn_mod_range(const DevConsts &hc, uint32_t base_off, uint32_t nmod) {
    CnModRange r{true, true, 0, 0};
    for (uint32_t m = base_off; m < base_off + nmod; m++) {
        const uint64_t q = m < hc.k ? hc.q[m].q : (m < hc.k + hc.kb ? hc.bsk[m - hc.k].q : hc.t.q);
        r.f64ok = r.f64ok && hc.f64ok[m];
        if (q > r.qmax) r.qmax = q;
    }
    r.light = !(r.qmax >> 44);
    r.bits = r.qmax ? 64 - __builtin_clzll(r.qmax) : 0;
    return r;
}
// use_f64: the "f64" option as it stands now - or, for a key switch, the form its key was loaded in (KsKey::f64)
inline int cn_policy(const CnModRange &r, bool use_f64) { return !(use_f64 && r.f64ok) ? POL_U64 : (r.light ? POL_F64L : POL_F64); }
// Digit sums S = sum_k w_k dig_k of cn_square_gemm / cn_mul_relin_sum (|dig| <= 2^dbc - 1, sum_abs_w = the largest sum_k |w_k| of any output; K for unit
// weights): do they fit a signed 32-bit word, sum_abs_w (2^dbc - 1) <= 2^31 - 1?  Then the producers store int32 words and the key switch reads half the bytes
inline bool cn_digit_sum_fits_i32(uint64_t sum_abs_w, int dbc) {
    if (dbc < 1 || dbc > 31) return false;
    return (unsigned __int128)sum_abs_w * ((1ull << dbc) - 1) <= 0x7fffffffull;
}
// cn_square_gemm's pre-floor form runs ONE floor tail per dense output on the weighted sums of the inputs' floor operands.  Its Shenoy-Kumaresan
// conversion returns V_o = sum_k w_ok W_k exactly iff |V_o| < B m_sk / 2, where W_k = floor(t d_k / q) - a_k is the integer the per-input floor computes: |d| <= 2 N q^2
// for a coefficient of the cross term of operands below q, so |W| < 4 t N q and |V_o| < 4 R t N q with R = sum_abs_w.  One-sided: true implies 8 R t N q <= B m_sk / 2
// (a bit to spare) - the logarithms are doubles whose errors (below 2^-40 in the sum) the margin 2^-20 covers; false may be a near miss.  Also true only if the exact
// sums Y_oj = sum_k w_ok y_kj (|y| < q_j) stay below 2^63, R q_j < 2^63 for every j: the GEMM forms them in two's complement 64-bit words.
inline bool cn_prefloor_bound_ok(uint64_t sum_abs_w, uint64_t t, uint32_t n, const uint64_t *q, uint32_t k, const uint64_t *base, uint32_t kb) {
    if (!sum_abs_w || !t || !n || !k || !kb) return false;
    double lhs = __builtin_log2((double)sum_abs_w) + __builtin_log2((double)t) + __builtin_log2((double)n) + 3.0, rhs = -1.0;
    for (uint32_t j = 0; j < k; j++) {
        if (!q[j] || (unsigned __int128)sum_abs_w * q[j] >= ((unsigned __int128)1 << 63)) return false;
        lhs += __builtin_log2((double)q[j]);
    }
    for (uint32_t b = 0; b < kb; b++) { if (base[b] < 2) return false; rhs += __builtin_log2((double)base[b]); }
    return lhs + 0x1p-20 <= rhs;
}
// The tables of a planned scalar GEMM (HOT LOOP A), as the planner (cn_gemm_plan.h) writes them and the launchers (cn_l_gemm.hip) read them.
// k_scalar_gemm_f64: rows of the weight table per (group, output tile) - K terms + zero rows up to a multiple of 16 + 16: the kernel's sets of 4 (or 8) terms run past K
// and multiply whatever word the padded gather entry reads by these zeros
inline uint32_t gemm_f64_rows(uint32_t K) { return ((K + 15) & ~15u) + 16; }
inline uint32_t digit_gemm_tile(uint32_t M) { return M > 2 ? 10u : 2u; }
inline uint32_t digit_gemm_rows(uint32_t K) { return ((K + 7) & ~7u) + 8; }        // K terms + zero rows: the kernel's sets of four terms run past K
// image: [gather rows G x Kp | output members G x M | bias entries G x M | weights | digit-GEMM weights], every table on a 256-byte boundary; 4-byte entries (indices,
// -1 = padded tap / no output) or 8-byte ones (device addresses, 0 likewise: the deferred queue's address-table form)
struct GemmLayout {
    uint32_t K = 0, Kp = 0, G = 0, M = 0, MT = 0, lazy = 0;
    bool small = false, two = false, one = false, mfma = false;
    uint32_t P = 0, mtiles = 0, ksteps = 0;  // matrix-core form: weight digit planes, 32-row output tiles, 32-term steps
    // res: the clipped + residual form (gemm_residual_form, cn_gemm_plan.h) - P = 1, the fragments hold two planes c and r of weight 256^0 and the table kres [G] behind
    // them (the leading K steps with a residual, per gather list), the K slots of the gather rows are permuted
    bool res = false;
    // cn_square_gemm: the layer may run on the digits of the unrelinearized products (square_gemm_fused_ok) - signed weights [G][mtiles][dKw][dMT] at off_dw
    // dig_mfma: the digit GEMM runs on the matrix cores from the fragments at off_w (no table at off_dw)
    // dig_i32: every digit sum fits a signed 32-bit word (cn_digit_sum_fits_i32 of the largest row, "digit_i32" on): S is stored and read as int32 words
    bool dig = false, dig_mfma = false, dig_i32 = false; uint32_t dMT = 0, dKw = 0;
    size_t off_oidx = 0, off_bidx = 0, off_w = 0, off_dw = 0;
    uint64_t sum_abs_w = 0;                  // with `dig`: the largest sum_k |w_ok| of any output (the plan's digit bound is sum_abs_w (2^dbc - 1)); 0 = not known: no pre-floor form
    template <class E> const E *gather(const char *image) const { return (const E *)image; }                  // [G][Kp]
    template <class E> const E *members(const char *image) const { return (const E *)(image + off_oidx); }    // [G][M]
};
// Sums over NTT-form plaintexts on the FP64 policies (k_mul_ptn_sum, cn_k_ptn.hip.h): a term is ArF64T::mulmod of two canonical words below q < 2^50, exact with
// |term| <= q/2 + 3 q^2 / 2^53 (the quotient is rint of a product rounded three times).  cn_ptn_term_bound rounds that up to an integer; cn_ptn_sum_interval is how
// many terms the lazy accumulators take between two recentrings: the largest count with count x bound < 2^52 (a recentred accumulator adds at most q/2 + 1 < 2^49:
// every partial sum stays below 2^53), capped at CN_PTN_INTERVAL_CAP, which *capped reports (the counter is a 32-bit word; small moduli would allow millions).
static const uint32_t CN_PTN_INTERVAL_CAP = 1u << 16;
inline uint64_t cn_ptn_term_bound(uint64_t q) {
    const unsigned __int128 sq = (unsigned __int128)3 * q * q;
    return q / 2 + 1 + (uint64_t)((sq + (((unsigned __int128)1 << 53) - 1)) >> 53);
}
inline uint32_t cn_ptn_sum_interval(uint64_t qmax, bool *capped = nullptr) {
    const uint64_t fit = ((1ull << 52) - 1) / cn_ptn_term_bound(qmax);
    if (capped) *capped = fit > CN_PTN_INTERVAL_CAP;
    return fit > CN_PTN_INTERVAL_CAP ? CN_PTN_INTERVAL_CAP : (fit ? (uint32_t)fit : 1u);
}
// The wide plaintext kernels - k_mul_plain_bcast on NTT-form rows, k_mul_plain_sum, k_mul_ptn_sum - exist at every register-radix size but N = 16384 under the integer
// policy: beside a 1024-thread workgroup's 128 registers per thread the integer transform leaves no room for their accumulators or row loads (25, 50 and 2 spilled
// registers when built).  There the row-dot batch runs k_mul_plain_fused alone and cn_mul_plain_sum composes cn_mul_plain and AddMany (cn_plain_plan.h); the launchers
// instantiate by the same predicate, so a kernel the plan picks is a kernel that was built.
constexpr bool cn_plain_wide(int policy, uint32_t logn) { return !(policy == POL_U64 && logn == 14); }
// Lazy FP64 accumulators of products of canonical words (the key switch's digit sums, k_mul_plain_sum): |term| <= 2.1 q, so this many terms between two recentrings
// keep the sum below 2^52
inline uint32_t cn_f64_acc_interval(int bits) { return bits >= 50 ? 1u : 1u << (50 - bits < 10 ? 50 - bits : 10); }
// the ring sizes of the register-radix kernels: 1024 <= N <= 16384, or N <= 8192 (max_logn = 13) for the kernels that stop there
inline bool cn_rr_size(uint32_t logn, uint32_t max_logn = 14) { return logn >= 10 && logn <= max_logn; }
