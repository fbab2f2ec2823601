// One ciphertext product, decided here and nowhere else: the tensor kernels a BEHZ multiply of `cnt` ciphertexts launches, what its base extension and floor are
// told, the scratch arrays of the chain, how a batch of products is cut into chunks under the scratch limit at each of the sites that run one, the gates of the
// one-key-switch-per-output forms (cn_square_gemm, cn_mul_relin_sum, the deferred square + dense layer) and the parts of a pipelined Multiply + Relinearize.
// do_multiply, run_mul_relin and the entry points around them (cn_eval.hip), the deferred queue (cn_defer.hip) and the launchers (cn_l_rr.inc.h, cn_l_behz.hip) read
// the same plan.  Host-only and free of HIP: a plain C++ compiler builds it (tests/cpp/mul_plan.cpp).
#pragma once
#include "cn_policy.h"
#include "cn_ks_plan.h"

// what the decisions read of a context, by value (mul_switches in cn_eval.hip builds it)
struct MulSwitches {
    int f64, sq_fused, sq_pipe, sq_lds, sq_halves;      // the options of that name (include/cnhip.h)
    bool mul_sum, digit_i32, defer_square_gemm;         // ... set by name
    bool rr, rr13;            // the context runs register-radix kernels (rr_kernels), and those that stop at N = 8192
    int cus;                  // compute units of the device
    bool capturing;           // a graph is being recorded
    size_t smax;              // the scratch limit (CN_SCRATCH_GB)
    bool rlk, rlk_f64;        // a relinearisation key is present; it was loaded in FP64 form (KsKey::f64)
    KsSwitches ks;
    int sg_prefloor = 0;      // "sg_prefloor": 0 = cn_square_gemm floors every product (the old form), 1 = the pre-floor form where square_gemm_prefloor_ok says so, 2 = ... for any K (tests)
};
inline size_t mul_al(size_t b) { return (b + 255) & ~(size_t)255; }      // the scratch arena hands out multiples of 256 bytes (al, salloc)

// ---- one product launch chain: extend, [transforms,] tensor, [inverse transforms,] floor
enum MulForm {
    MUL_SQUARE_FUSED,     // squaring on the FP64 policies: forward transforms, tensor and inverse transforms of one (ciphertext, limb) in ONE kernel per base; its q side reads
                          // the input ciphertexts in place, so the base extension only has to produce the Bsk limbs
    MUL_INTT_TENSOR,      // forward transforms, then k_intt_tensor: the tensor product fused into the inverse transform (register-radix sizes)
    MUL_ELEMENTWISE       // forward transforms, k_tensor, inverse transforms ("legacy_ntt", N < 1024)
};
enum SqKernel {
    SQ_PLAIN,             // k_square_fused: the NTT-form operand parked in the outputs' place (two workgroups per CU)
    SQ_LDS,               // k_square_fused<.., true>: parked in LDS (one workgroup per CU; N <= 8192)
    SQ_PIPE               // k_square_pipe: `per_limb` resident workgroups per modulus for the whole launch; pays once a workgroup squares several blocks (N <= 8192)
};
enum MulArray { MUL_AQ, MUL_AB, MUL_BQ, MUL_BB, MUL_DQ, MUL_DB, MUL_ARRAYS };      // operands a, b extended to q / Bsk, the tensor d on q / Bsk
struct MulBase {                                                                    // policy: cn_policy of the base under "f64"; sq, per_limb: MUL_SQUARE_FUSED only
    int policy; SqKernel sq; uint32_t per_limb;
    bool ntt01 = false;   // SQ_LDS / SQ_PIPE: components 0 and 1 leave in NTT form (canonical words, tail_index layout) - the Bsk side of cn_square_gemm's pre-floor form
};
struct MulPlan {
    MulForm form;
    bool lazy;            // the tensor leaves as lazy-FP64 hand-off words (lazy_word, cn_dev_common.hip.h) and the floor is told so: the tensor kernels of BOTH bases and the
                          // floor are on the FP64 policy - the fused squaring always, k_intt_tensor when behz_f64 holds; k_tensor writes canonical words
    bool behz_f64;        // base extension and floor run their FP64 kernels: every data and auxiliary prime below 2^49 (DevConsts::behz_f64) and "f64" on
    MulBase q, bsk;
    struct { MulArray id; size_t bytes; } scratch[MUL_ARRAYS]; uint32_t arrays;      // what do_multiply allocates, in this order
};
inline MulBase mul_base(const DevConsts &hc, const MulSwitches &sw, MulForm form, uint32_t cnt, uint32_t base_off, uint32_t Lm) {
    MulBase b{cn_policy(cn_mod_range(hc, base_off, Lm), sw.f64 != 0), SQ_PLAIN, 0};
    if (form != MUL_SQUARE_FUSED || hc.logn > 13) return b;
    b.per_limb = std::min<uint32_t>((uint32_t)std::max(1, sw.cus) / Lm, cnt);
    if (b.per_limb >= 1 && (sw.sq_pipe == 2 || (sw.sq_pipe && cnt >= 4 * b.per_limb))) b.sq = SQ_PIPE;
    else if (sw.sq_lds) b.sq = SQ_LDS;
    return b;
}
inline MulPlan cn_mul_plan(const DevConsts &hc, const MulSwitches &sw, bool square, uint32_t cnt) {
    const size_t n = hc.n, k = hc.k, kb = hc.kb;
    MulPlan p{};
    p.behz_f64 = hc.behz_f64 && sw.f64;
    const bool sq_ok = sw.sq_fused && sw.f64 && sw.rr && cn_mod_range(hc, 0, hc.k).f64ok && cn_mod_range(hc, hc.k, hc.kb).f64ok;
    p.form = square && hc.behz_f64 && sq_ok ? MUL_SQUARE_FUSED : (sw.rr ? MUL_INTT_TENSOR : MUL_ELEMENTWISE);
    p.lazy = p.form != MUL_ELEMENTWISE && p.behz_f64;      // (behz_f64 puts every modulus of both bases on an FP64 policy: no kernel is missing for a lazy tensor)
    p.q = mul_base(hc, sw, p.form, cnt, 0, hc.k); p.bsk = mul_base(hc, sw, p.form, cnt, hc.k, hc.kb);
    auto need = [&](MulArray id, size_t words) { p.scratch[p.arrays].id = id; p.scratch[p.arrays++].bytes = words * 8; };
    if (p.form != MUL_SQUARE_FUSED) need(MUL_AQ, cnt * 2 * k * n);
    need(MUL_AB, cnt * 2 * kb * n);
    if (!square) { need(MUL_BQ, cnt * 2 * k * n); need(MUL_BB, cnt * 2 * kb * n); }
    need(MUL_DQ, cnt * 3 * k * n); need(MUL_DB, cnt * 3 * kb * n);
    return p;
}
// The bytes of one chain per ciphertext as CHUNKING counts them: both operands on both bases, the tensor, 1024 for the roundings.  This is not the sum of
// MulPlan::scratch - a fused squaring allocates no MUL_AQ and is counted as if it did.  It stays so on purpose: chunk boundaries, and with them launch counts, follow it.
inline size_t mul_chain_bytes(const DevConsts &hc, bool square) {
    const size_t kk = (size_t)hc.k + hc.kb;
    return mul_al(((square ? 1 : 2) * 2 * kk * hc.n + 3 * kk * hc.n) * 8) + 1024;
}

// ---- chunking: a batch of `count` products runs `chunk` at a time so that a chunk's scratch stays inside the limit (one product at least)
inline uint32_t cn_chunk_of(size_t smax, size_t per, uint32_t count) { return (uint32_t)std::min<size_t>(std::max<size_t>(1, smax / per), count); }      // (also the queued encryptions' rule)
enum MulSite {
    MUL_AT_MULTIPLY,      // cn_multiply: the chain
    MUL_AT_MUL_RELIN,     // cn_mul_relin: + the size-3 product
    MUL_AT_PARK,          // parked squarings of a boundary flush: + one operand address (the products go to the context's product array)
    MUL_AT_DEFERRED,      // queued cn_mul_relin calls of a flush: + the size-3 product and three addresses
    MUL_AT_SQUARE_GEMM,   // cn_square_gemm: ALL `count` products and the digit sums of `outputs` outputs beside the chain of a chunk
    MUL_AT_SUM_GROUP      // one group of cn_mul_relin_sum: its `count` products, the digit sums of `outputs` outputs and two address tables beside the chain of a chunk
};
struct MulBatch {
    size_t per, fixed, slack; uint32_t tables;      // bytes per ciphertext of a chunk; beside the chunks; roundings; address tables of one entry per ciphertext of a chunk
    uint32_t chunk;
    bool fits;                                      // MUL_AT_SQUARE_GEMM: `fixed` and one chain fit the limit (else: the two steps as they are)
    size_t ensure(uint32_t c) const { return fixed + per * c + tables * mul_al((size_t)c * 8) + slack; }      // the arena of a chunk of c
};
inline MulBatch mul_batch(const DevConsts &hc, const MulSwitches &sw, MulSite site, uint32_t count, bool square, uint32_t outputs = 0, bool s32 = false) {
    const size_t kn = (size_t)hc.k * hc.n, chain = mul_chain_bytes(hc, square), sums = mul_al((size_t)outputs * hc.rl_tot * hc.n * (s32 ? 4 : 8));
    MulBatch b{chain, 0, 8192, 0, 0, true};
    switch (site) {
        case MUL_AT_MULTIPLY: b.slack = 4096; break;
        case MUL_AT_MUL_RELIN: b.per += mul_al(3 * kn * 8); break;
        case MUL_AT_PARK: b.per += 8 + 64; b.tables = 1; break;
        case MUL_AT_DEFERRED: b.per += mul_al(3 * kn * 8) + 3 * 8 + 64; b.tables = 3; break;
        case MUL_AT_SQUARE_GEMM:
            b.fixed = mul_al((size_t)count * 3 * kn * 8) + sums + 8192; b.slack = 4096;
            b.fits = !(b.fixed + b.per > sw.smax);
            b.chunk = b.fits ? (uint32_t)std::min<size_t>(count, (sw.smax - b.fixed) / b.per) : 0;
            return b;
        case MUL_AT_SUM_GROUP:
            b.fixed = mul_al((size_t)count * 3 * kn * 8) + sums + 2 * mul_al((size_t)count * 8) + 8192; b.slack = 4096;
            b.chunk = (uint32_t)std::min<size_t>(count, std::max<size_t>(1, (sw.smax - std::min(sw.smax, b.fixed)) / b.per));
            return b;
    }
    b.chunk = cn_chunk_of(sw.smax, b.per, count);
    return b;
}
// cn_mul_relin_sum of `count` outputs of K products each: outputs per group (0: not even one output fits beside one chain - the literal sequence) and whether the digit
// sums are int32 words (unit weights: K (2^dbc - 1) <= 2^31 - 1, "digit_i32" on).  A group holds the products [output][term][3][k][N], S [output][rl_tot][N] and the
// two address tables of a group beside the scratch of one product
struct MulSumBatch { bool s32; uint32_t group; };
inline MulSumBatch mul_sum_batch(const DevConsts &hc, const MulSwitches &sw, uint32_t K, uint32_t count) {
    const size_t kn = (size_t)hc.k * hc.n, per = mul_chain_bytes(hc, false), slack = 4 * 256 + 8192;
    MulSumBatch b{sw.digit_i32 && cn_digit_sum_fits_i32(K, hc.dbc), 0};
    const size_t per_out = (size_t)K * 3 * kn * 8 + (size_t)hc.rl_tot * hc.n * (b.s32 ? 4 : 8) + (size_t)K * 16;
    b.group = (uint32_t)std::min<size_t>(count, sw.smax > per + slack ? (sw.smax - per - slack) / per_out : 0);
    return b;
}
// the deferred square + dense layer of a planned group with O outputs: temporary [O][2][k][N], S, the gather / member / output tables (sg_run, cn_defer.hip)
inline size_t mul_sg_scratch(const DevConsts &hc, const GemmLayout &L, uint32_t O) {
    return mul_al((size_t)O * 2 * hc.k * hc.n * 8) + mul_al((size_t)O * hc.rl_tot * hc.n * (L.dig_i32 ? 4 : 8)) + mul_al((size_t)L.G * L.Kp * 4) + mul_al((size_t)L.G * L.M * 4) +
           mul_al((size_t)O * 8) + 8192;
}

// ---- the gates of the one-key-switch-per-output forms
// cn_mul_relin_sum: the smallest K that takes the one-key-switch-per-output form (cn_get_option "mul_sum_min_k").  2 = every sum of products: at C3, K = 2 takes
// 0.53 (one output) and 0.69 (eight outputs) of the literal sequence's time, the spreads of the two sides apart (profiles/mul_relin_sum.md, tools/mul_sum_probe.py)
static const uint32_t MUL_SUM_MIN_K = 2;
static const uint32_t PRODUCT_SUM_MAX_DIGITS = 8;      // k_product_sum keeps the digits of one source limb in registers (cn_k_gemm.hip.h)
// everything but the plan: "f64" on, every q limb and the key on an FP64 policy, the register-radix kernels up to N = 8192, the plain decomposition.  The deferred queue
// asks it (with the switch and a key: mul_defers_square_gemm) before it holds the relinearisation of queued squarings back
inline bool square_gemm_ctx_ok(const DevConsts &hc, const MulSwitches &sw) { return sw.f64 && sw.rr13 && !hc.ks_xi && sw.rlk_f64 && cn_mod_range(hc, 0, hc.k).f64ok; }
inline bool square_gemm_fused_ok(const DevConsts &hc, const MulSwitches &sw, const GemmLayout &L) { return L.dig && square_gemm_ctx_ok(hc, sw); }
inline bool mul_defers_square_gemm(const DevConsts &hc, const MulSwitches &sw) { return sw.defer_square_gemm && square_gemm_ctx_ok(hc, sw) && sw.rlk; }
// cn_square_gemm's pre-floor form ("One floor tail per dense output"): components 0 and 1 of the products are never floored per input - their Bsk words
// are summed in NTT form on the matrix cores, the canonical y of their q words as exact integers, and ONE floor tail per output gives the words of the old form.
// Runs when "sg_prefloor" is on, the old fused form would run (square_gemm_fused_ok) with the plan's GEMM on the matrix cores, the products come from the fused squaring
// kernels with the operand parked in LDS or registers (MUL_SQUARE_FUSED, lazy hand-off, "sq_lds": no SQ_PLAIN launch at any chunk size), the weights have one or two signed byte digits (|w| <= 32639: the
// three-plane instantiation of the y GEMM would spill registers), every auxiliary prime is below
// 2^49 (seven signed byte digits), the bound on |V_o| holds (cn_prefloor_bound_ok, cn_policy.h) and the layer has at least SG_PREFLOOR_MIN_K terms ("sg_prefloor" 2: any).
// SG_PREFLOOR_MIN_K: measured at C3 with 100 outputs, both forms alternating in one process - K = 64, 128, 256: the old form is faster (the new one pays two more GEMM launches,
// a transform and a floor launch whatever K is); K = 512 and 845: the new form's slowest repetition beats the old form's fastest (profiles/square_gemm_prefloor.md)
static const uint32_t SG_PREFLOOR_MIN_K = 512;
inline bool square_gemm_prefloor_ok(const DevConsts &hc, const MulSwitches &sw, const GemmLayout &L) {
    if (!sw.sg_prefloor || !L.mfma || !L.P || L.P > 2 || !square_gemm_fused_ok(hc, sw, L) || (sw.sg_prefloor < 2 && L.K < SG_PREFLOOR_MIN_K)) return false;
    const MulPlan p = cn_mul_plan(hc, sw, true, 1);
    if (p.form != MUL_SQUARE_FUSED || !p.lazy || !p.behz_f64 || !sw.sq_lds || hc.logn > 13 || hc.kb != hc.k + 1 || cn_mod_range(hc, hc.k, hc.kb).bits > 49) return false;
    uint64_t q[CN_MAXK], b[CN_MAXK + 1];
    for (uint32_t j = 0; j < hc.k; j++) q[j] = hc.q[j].q;
    for (uint32_t j = 0; j < hc.kb; j++) b[j] = hc.bsk[j].q;
    return cn_prefloor_bound_ok(L.sum_abs_w, hc.t.q, hc.n, q, hc.k, b, hc.kb);
}
// what the form keeps beside the old form's arrays for the whole call: the tensor words of ALL `count` products on both bases (the GEMMs read them after the last
// chunk), X and Y of the `outputs` outputs.  cn_square_gemm adds the total to MulBatch::fixed before it asks whether the call fits
enum SgArray { SG_DQ, SG_DB, SG_X, SG_Y, SG_ARRAYS };
struct SgPrefloorScratch { struct { SgArray id; size_t bytes; } scratch[SG_ARRAYS]; size_t total; };
inline SgPrefloorScratch square_gemm_prefloor_scratch(const DevConsts &hc, uint32_t count, uint32_t outputs) {
    const size_t n = hc.n, k = hc.k, kb = hc.kb;
    SgPrefloorScratch s{{{SG_DQ, mul_al(count * 3 * k * n * 8)}, {SG_DB, mul_al(count * 3 * kb * n * 8)}, {SG_X, mul_al(outputs * 2 * kb * n * 8)}, {SG_Y, mul_al(outputs * 2 * k * n * 8)}}, 0};
    for (const auto &a : s.scratch) s.total += a.bytes;
    return s;
}
// cn_mul_relin_sum: "mul_sum" on, K >= MUL_SUM_MIN_K, S is a lazy value the KsDigits kernels take (K (2^dbc - 1) below every q_j / 2 and below 2^52), the kernel's
// 64-bit accumulators hold the sums of components 0 and 1 exactly (K (q_max - 1) < 2^64: PRODUCT_SUM_MAX_TERMS), its digit registers hold every limb's digits (at
// most PRODUCT_SUM_MAX_DIGITS of at most 31 bits) and its blocks of 512 coefficients tile the ring
inline bool mul_sum_fused_ok(const DevConsts &hc, const MulSwitches &sw, uint32_t K) {
    if (!sw.mul_sum || K < MUL_SUM_MIN_K || !square_gemm_ctx_ok(hc, sw)) return false;
    if (hc.dbc < 1 || hc.dbc > 31) return false;
    const unsigned __int128 s = (unsigned __int128)K * ((1ull << hc.dbc) - 1);
    if (s >= ((unsigned __int128)1 << 52)) return false;
    for (uint32_t j = 0; j < hc.k; j++) if (s >= hc.q[j].q / 2 || hc.rl_dig[j] > PRODUCT_SUM_MAX_DIGITS) return false;
    return (unsigned __int128)K * (cn_mod_range(hc, 0, hc.k).qmax - 1) < ((unsigned __int128)1 << 64) && !(hc.n & 511);
}

// ---- "sq_halves": Multiply + Relinearize of a batch in parts over the context's two streams (pipelined_halves, cn_api_shared.h)
static const uint32_t SQ_HALVES_MIN = 512;       // (the 100-ciphertext layer of CryptoNets pipelined as well: 12.35 -> 13.4 ms per batch, visit AY)
// the parts of a pipelined batch of c ciphertexts: part i = [first[i], first[i + 1]); returns the number of parts P = min(3, max(1, c / 128)) (first[] holds P + 1
// entries).  Three parts are cut at 30 and 70 %, two at the half; every cut is rounded up to a multiple of 8.
inline uint32_t pipeline_cuts(uint32_t c, uint32_t first[4]) {
    const uint32_t P = std::min<uint32_t>(3, std::max<uint32_t>(1, c / 128));
    first[0] = 0; first[P] = c;
    if (P == 2) first[1] = (c / 2 + 7) & ~7u;
    if (P == 3) { first[1] = (uint32_t)(((uint64_t)c * 3 / 10 + 7) & ~7ull); first[2] = (uint32_t)(((uint64_t)c * 7 / 10 + 7) & ~7ull); }
    return P;
}
// the parts in which a Multiply + Relinearize of c ciphertexts runs through pipelined_halves ("sq_halves" at least sq_halves_min), 0: it does not.  Only if no part's key
// switch writes the context's ONE arena ks_part (the two-launch forms keep their partial products there and may re-allocate it), which the parts on the two streams
// would share.  The caller still needs the second stream (aux_stream_ready)
inline uint32_t mul_pipeline_parts(const DevConsts &hc, const MulSwitches &sw, uint32_t c, int sq_halves_min, uint32_t first[4]) {
    if (sw.sq_halves < sq_halves_min || hc.logn > 13 || c < SQ_HALVES_MIN || sw.capturing) return 0;
    const uint32_t P = pipeline_cuts(c, first);
    for (uint32_t i = 0; i < P; i++) if (ks_writes_arena(cn_ks_plan(hc, sw.ks, sw.rlk_f64, first[i + 1] - first[i], 0))) return 0;
    return P >= 2 ? P : 0;
}
