// HOT LOOP B: the element-wise BEHZ steps between the batched transforms (base extension q -> Bsk, fast floor + Shenoy-Kumaresan).
// Included by cn_l_behz.hip only.
#pragma once
#include "cn_dev_common.hip.h"

// ------------------------------------------------------------------ HOT LOOP B: BEHZ multiply
// Step 0/1 (fastbconv_mtilde + mont_rq): q -> Bsk, removing q-overflows via m~ = 2^32.
// src ciphertext c = src + c*stride*ctw, or src_tab[c] (deferred per-ciphertext calls: every ciphertext is its own array);
// writes the q copy (for the q-side NTT) and Bsk.
template <int K, int NB = K>
__global__ void __launch_bounds__(256) k_behz_extend(const uint64_t *__restrict__ src, uint32_t stride, const uint64_t *const *__restrict__ src_tab,
                                                     uint64_t *__restrict__ aq, uint64_t *__restrict__ ab, const DevConsts *__restrict__ C, uint32_t chunks) {
    const uint32_t n = C->n;
    const uint32_t cp = blockIdx.x / chunks, i = (blockIdx.x % chunks) * blockDim.x + threadIdx.x;   // cp = ct*2 + poly
    const uint32_t ct = cp >> 1, p = cp & 1;
    const NTT_GLOBAL uint64_t *x = (const NTT_GLOBAL uint64_t *)(src_tab ? src_tab[ct] : src + (size_t)ct * stride * 2 * K * n) + (size_t)p * K * n + i;   // src_tab: one address per ciphertext
    uint64_t *oq = aq + (size_t)cp * K * n + i, *ob = ab + (size_t)cp * (NB + 1) * n + i;
    uint64_t y[K], mt = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        uint64_t v = x[(size_t)j * n];
        oq[(size_t)j * n] = v;
        y[j] = mulmod(v, C->mt_inv_qhat_q[j], C->q[j]);
        mt += y[j] * C->qhat_mt[j];
    }
    mt &= 0xffffffffull;
    const uint64_t r = (0 - mt * C->inv_q_mt) & 0xffffffffull;      // r = -x q^{-1} mod m~
#pragma unroll
    for (int b = 0; b <= NB; b++) {
        const DMod bm = C->bsk[b];
        const uint64_t rr = r >= 0x80000000ull ? r + bm.q - 0x100000000ull : r;     // centred r as a residue mod b
        u128 acc = (u128)rr * C->ex_R_bsk[b];                                      // (x_b + q*r) * m~^-1 with the factors folded:
#pragma unroll
        for (int j = 0; j < K; j++) acc += (u128)y[j] * C->ex_Q_bsk[b][j];         // one lazy accumulation, one Barrett reduction
        ob[(size_t)b * n] = bred128(acc, bm);
    }
}
// The same two element-wise steps in exact FP64 (DevConsts::behz_f64: every data and auxiliary prime < 2^49).  The integer
// versions spend ~2700 / ~1450 VALU instructions per coefficient, mostly in 128-bit Barrett reductions and 64x64->128
// products assembled from 32-bit pieces; here a term of a base conversion is ArF64::mulmod (6 FP64 instructions, |r| <= 2.1 p), a
// conversion of <= 6 terms is summed exactly in one double and reduced once.  Representatives: the CRT coefficients
// y_j = [x (q/q_j)^-1]_{q_j} MUST be canonical (another representative changes the q-overflow count and with it the words
// SEAL produces); residues that are only re-reduced (f_b, z_j, alpha) may stay lazy - z_j + s b_j shifts the Shenoy-Kumaresan
// sum by s B and alpha by s, which cancels.
template <int K, int NB = K>
__global__ void __launch_bounds__(256) k_behz_extend_f64(const uint64_t *__restrict__ src, uint32_t stride, const uint64_t *const *__restrict__ src_tab,
                                                         uint64_t *__restrict__ aq, uint64_t *__restrict__ ab, const DevConsts *__restrict__ C, uint32_t chunks) {
    const uint32_t n = C->n;
    const uint32_t cp = blockIdx.x / chunks, i = (blockIdx.x % chunks) * blockDim.x + threadIdx.x;   // cp = ct*2 + poly
    const uint32_t ct = cp >> 1, p = cp & 1;
    const NTT_GLOBAL uint64_t *x = (const NTT_GLOBAL uint64_t *)(src_tab ? src_tab[ct] : src + (size_t)ct * stride * 2 * K * n) + (size_t)p * K * n + i;   // src_tab: one address per ciphertext
    uint64_t *oq = aq + (size_t)cp * K * n + i, *ob = ab + (size_t)cp * (NB + 1) * n + i;
    double y[K];
    uint32_t mt = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const uint64_t v = x[(size_t)j * n];
        if (aq) oq[(size_t)j * n] = v;             // aq == nullptr: the fused squaring kernel reads the q limbs from the ciphertext itself
        const BzF::Mod mq = {C->qd[j], C->qinvd[j]};
        y[j] = bz_canon(BzF::mulmod(BzF::from_u64(v), C->bd.mt_inv_qhat_q[j], mq), mq);       // canonical: feeds the mod-m~ sum
        mt += (uint32_t)__double_as_longlong(__dadd_rn(y[j], 4503599627370496.0)) * (uint32_t)C->qhat_mt[j];   // low 32 bits of y (exact integer < 2^49)
    }
    const double r = (double)(int32_t)(0u - mt * (uint32_t)C->inv_q_mt);                       // centred r = -x q^-1 mod m~ = 2^32
#pragma unroll
    for (int b = 0; b <= NB; b++) {
        const BzF::Mod mb = {C->qd[K + b], C->qinvd[K + b]};
        double acc = BzF::mulmod(r, C->bd.ex_R_bsk[b], mb);
#pragma unroll
        for (int j = 0; j < K; j++) {
            acc = __dadd_rn(acc, BzF::mulmod(y[j], C->bd.ex_Q_bsk[b][j], mb));
            if (K >= 7 && j == 3) acc = BzF::center(acc, mb);          // more than 7 terms of 2.1 b would pass 2^53
        }
        ob[(size_t)b * n] = BzF::to_u64(acc, mb);
    }
}
// LZ: the tensor limbs arrive in the lazy-FP64 hand-off format (lazy_word, cn_dev_common.hip.h): doubles without the 1/N factor, |x| <= 8.5 p, and the
// two input constants carry N^-1 (bd.fl_c1n_q, bd.fl_Tn_bsk).  Every later step is the same; so are the words written.
// The floor's tail on f_b = W mod b (any representative, |f| <= 12.6 b): alpha_sk, z_l and the Shenoy-Kumaresan conversion Bsk -> q.  r[j] == W (mod q_j), lazy (to_u64 canonicalises).
// The tail of k_behz_floor_f64 below, step for step, for k_behz_floor_out (that kernel keeps its own text: its instantiations are tuned as they stand)
template <int K, int NB> DEV void behz_floor_tail(const double (&f)[NB + 1], const DevConsts *__restrict__ C, double (&r)[K]) {
    double z[NB];
    const BzF::Mod msk = {C->qd[K + NB], C->qinvd[K + NB]};
    double acc = BzF::mulmod(-f[NB], C->bd.inv_B_msk, msk);
#pragma unroll
    for (int j = 0; j < NB; j++) {
        const BzF::Mod mb = {C->qd[K + j], C->qinvd[K + j]};
        z[j] = BzF::mulmod(f[j], C->bd.inv_bhat_b[j], mb);
        acc = __dadd_rn(acc, BzF::mulmod(z[j], C->bd.fl_A_msk[j], msk));
        if (NB >= 7 && j == 3) acc = BzF::center(acc, msk);
    }
    const double alpha = BzF::center(acc, msk);                                                        // centred alpha_sk
#pragma unroll
    for (int j = 0; j < K; j++) {
        const BzF::Mod mq = {C->qd[j], C->qinvd[j]};
        double a2 = BzF::mulmod(-alpha, C->bd.B_q[j], mq);
#pragma unroll
        for (int l = 0; l < NB; l++) {
            a2 = __dadd_rn(a2, BzF::mulmod(z[l], C->bd.bhat_q[j][l], mq));
            if (NB >= 7 && l == 3) a2 = BzF::center(a2, mq);
        }
        r[j] = a2;
    }
}
// COMP (cn_square_gemm's pre-floor form: component 2 alone): block group u works on polynomial cp = u * cstride + cbase of the arrays instead of cp = u.
// (A pack of at most one tag type, FloorComp: the whole-product forms keep their names k_behz_floor_f64<K, NB, LZ>.)
struct FloorComp {};
template <int K, int NB = K, bool LZ = false, class... COMP_>
__global__ void __launch_bounds__(256) k_behz_floor_f64(const uint64_t *__restrict__ dq, const uint64_t *__restrict__ db, uint64_t *__restrict__ out,
                                                        const DevConsts *__restrict__ C, uint32_t chunks, uint32_t cbase = 0, uint32_t cstride = 1) {
    constexpr bool COMP = sizeof...(COMP_) != 0;
    const uint32_t n = C->n;
    const uint32_t cp = COMP ? (blockIdx.x / chunks) * cstride + cbase : blockIdx.x / chunks, i = (blockIdx.x % chunks) * blockDim.x + threadIdx.x;   // cp = ct*3 + poly
    const uint64_t *xq = dq + (size_t)cp * K * n + i, *xb = db + (size_t)cp * (NB + 1) * n + i;
    uint64_t *o = out + (size_t)cp * K * n + i;
    double y[K], f[NB + 1], z[NB];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const BzF::Mod mq = {C->qd[j], C->qinvd[j]};
        const double x = LZ ? lazy_value(xq[(size_t)j * n]) : BzF::from_u64(xq[(size_t)j * n]);
        y[j] = bz_canon(BzF::mulmod(x, LZ ? C->bd.fl_c1n_q[j] : C->bd.fl_c1_q[j], mq), mq);           // [x t (q/q_j)^-1]_{q_j}, canonical
    }
#pragma unroll
    for (int b = 0; b <= NB; b++) {
        const BzF::Mod mb = {C->qd[K + b], C->qinvd[K + b]};
        const double x = LZ ? lazy_value(xb[(size_t)b * n]) : BzF::from_u64(xb[(size_t)b * n]);
        double acc = BzF::mulmod(x, LZ ? C->bd.fl_Tn_bsk[b] : C->bd.fl_T_bsk[b], mb);                 // (x_b t - conv_b) q^-1, folded
#pragma unroll
        for (int j = 0; j < K; j++) {
            acc = __dadd_rn(acc, BzF::mulmod(y[j], C->bd.fl_N_bsk[b][j], mb));
            if (K >= 7 && j == 3) acc = BzF::center(acc, mb);          // (sums of more than 7 terms of 2.1 b would pass 2^53)
        }
        f[b] = acc;                                                                                    // |f| <= 12.6 b < 2^53
    }
    const BzF::Mod msk = {C->qd[K + NB], C->qinvd[K + NB]};
    double acc = BzF::mulmod(-f[NB], C->bd.inv_B_msk, msk);
#pragma unroll
    for (int j = 0; j < NB; j++) {
        const BzF::Mod mb = {C->qd[K + j], C->qinvd[K + j]};
        z[j] = BzF::mulmod(f[j], C->bd.inv_bhat_b[j], mb);
        acc = __dadd_rn(acc, BzF::mulmod(z[j], C->bd.fl_A_msk[j], msk));
        if (NB >= 7 && j == 3) acc = BzF::center(acc, msk);
    }
    const double alpha = BzF::center(acc, msk);                                                        // centred alpha_sk
#pragma unroll
    for (int j = 0; j < K; j++) {
        const BzF::Mod mq = {C->qd[j], C->qinvd[j]};
        double a2 = BzF::mulmod(-alpha, C->bd.B_q[j], mq);
#pragma unroll
        for (int l = 0; l < NB; l++) {
            a2 = __dadd_rn(a2, BzF::mulmod(z[l], C->bd.bhat_q[j][l], mq));
            if (NB >= 7 && l == 3) a2 = BzF::center(a2, mq);
        }
        o[(size_t)j * n] = BzF::to_u64(a2, mq);
    }
}
// The floor tail once per dense OUTPUT (cn_square_gemm's pre-floor form): block group = (slot s of the plan's member table, component c < 2).  With
// f_kb = T_b x_kb + sum_j N_bj y_kj (mod b) the per-input floor's Bsk value, sum_k w_k f_kb == T_b X_b + sum_j N_bj Y_j (mod b) for X_b = sum_k w_k x_kb mod b
// (X [output][2][NB + 1][N]: canonical coefficients - the Bsk GEMM of the NTT-form tensor words, transformed back by k_ntt_rr, N^-1 included) and the EXACT integers
// Y_j = sum_k w_k y_kj (Y [output][2][K][N], two's complement, |Y| < 2^63: k_scalar_gemm_mfma<.., GemmYForm>).  The tail turns those residues of V = sum_k w_k W_k into
// V mod q_j - word for word sum_k w_k floor_k mod q_j as long as |V| < B m_sk / 2 (cn_prefloor_bound_ok) - then the Delta-scaled bias (component 0), canonical words
// into output obase + oidx[s] of out [..][2][K][N].  oidx / bidx: the plan's member and bias tables ([slots], oidx < 0: no output); bias null: none
template <int K, int NB = K>
__global__ void __launch_bounds__(256) k_behz_floor_out(const uint64_t *__restrict__ X, const uint64_t *__restrict__ Y, const int32_t *__restrict__ oidx,
                                                        const uint64_t *__restrict__ bias, const int32_t *__restrict__ bidx, uint64_t *__restrict__ out, uint32_t obase,
                                                        const DevConsts *__restrict__ C, uint32_t chunks) {
    const uint32_t n = C->n;
    const uint32_t u = blockIdx.x / chunks, s = u >> 1, c = u & 1, i = (blockIdx.x % chunks) * blockDim.x + threadIdx.x;
    const int32_t oo = oidx[s];
    if (oo < 0) return;                                                                                // (uniform)
    const uint64_t *xb = X + ((size_t)oo * 2 + c) * (NB + 1) * n + i, *yq = Y + ((size_t)oo * 2 + c) * K * n + i;
    uint64_t *o = out + ((size_t)(obase + (uint32_t)oo) * 2 + c) * K * n + i;
    double yh[K], yl[K], f[NB + 1], r[K];
#pragma unroll
    for (int j = 0; j < K; j++) {                                                                      // Y = yh 2^32 + yl, |yh| <= 2^31
        const int64_t v = (int64_t)yq[(size_t)j * n];
        yh[j] = (double)(int32_t)(v >> 32); yl[j] = (double)(uint32_t)v;
    }
#pragma unroll
    for (int b = 0; b <= NB; b++) {
        const BzF::Mod mb = {C->qd[K + b], C->qinvd[K + b]};
        double acc = BzF::mulmod(BzF::from_u64(xb[(size_t)b * n]), C->bd.fl_T_bsk[b], mb);
#pragma unroll
        for (int j = 0; j < K; j++) {
            const double yb = __dadd_rn(BzF::mulmod(yh[j], 4294967296.0, mb), yl[j]);                  // Y_j mod b, |yb| <= 2.1 b + 2^32 < 3 b (b > 2^40)
            acc = __dadd_rn(acc, BzF::mulmod(yb, C->bd.fl_N_bsk[b][j], mb));
            if (K >= 7 && j == 3) acc = BzF::center(acc, mb);
        }
        f[b] = acc;
    }
    behz_floor_tail<K, NB>(f, C, r);
    const uint64_t bv = bias && c == 0 ? bias[(size_t)bidx[s] * n + i] : 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const BzF::Mod mq = {C->qd[j], C->qinvd[j]};
        uint64_t w = BzF::to_u64(r[j], mq);
        if (bv) w = addmod(w, scale_plain(C, bv, j), C->q[j].q);
        o[(size_t)j * n] = w;
    }
}
// Steps 3/4 (x t, fast_floor: q u Bsk -> Bsk, fastbconv_sk: Bsk -> q) per coefficient.
template <int K, int NB = K>
__global__ void __launch_bounds__(256) k_behz_floor(const uint64_t *__restrict__ dq, const uint64_t *__restrict__ db, uint64_t *__restrict__ out,
                                                    const DevConsts *__restrict__ C, uint32_t chunks) {
    const uint32_t n = C->n;
    const uint32_t cp = blockIdx.x / chunks, i = (blockIdx.x % chunks) * blockDim.x + threadIdx.x;   // cp = ct*3 + poly
    const uint64_t *xq = dq + (size_t)cp * K * n + i, *xb = db + (size_t)cp * (NB + 1) * n + i;
    uint64_t *o = out + (size_t)cp * K * n + i;
    uint64_t y[K], f[NB + 1], z[NB];
#pragma unroll
    for (int j = 0; j < K; j++) y[j] = mulmod(xq[(size_t)j * n], C->fl_c1_q[j], C->q[j]);           // x * t * (q/q_j)^-1
#pragma unroll
    for (int b = 0; b <= NB; b++) {
        const DMod bm = C->bsk[b];
        u128 acc = (u128)xb[(size_t)b * n] * C->fl_T_bsk[b];                                       // (x_b*t - conv_b) * q^-1, folded
#pragma unroll
        for (int j = 0; j < K; j++) acc += (u128)y[j] * C->fl_N_bsk[b][j];
        f[b] = bred128(acc, bm);
    }
    const DMod sk = C->bsk[NB];
    u128 acc = (u128)(sk.q - f[NB]) * C->inv_B_msk;
#pragma unroll
    for (int j = 0; j < NB; j++) { z[j] = mulmod(f[j], C->inv_bhat_b[j], C->bsk[j]); acc += (u128)z[j] * C->fl_A_msk[j]; }
    const uint64_t alpha = bred128(acc, sk);
    const bool neg = alpha > (sk.q >> 1);
#pragma unroll
    for (int j = 0; j < K; j++) {
        const DMod qm = C->q[j];
        u128 a2 = neg ? (u128)C->B_q[j] * (sk.q - alpha) : (u128)(qm.q - C->B_q[j]) * alpha;        // -alpha*B (centred alpha)
#pragma unroll
        for (int l = 0; l < NB; l++) a2 += (u128)z[l] * C->bhat_q[j][l];
        o[(size_t)j * n] = bred128(a2, qm);
    }
}
