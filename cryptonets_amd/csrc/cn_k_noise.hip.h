// Invariant noise norm (cn_noise_norm): for every ciphertext the exact centred infinity norm of v = t (c0 + c1 s [+ c2 s^2]) mod q, as K
// little-endian 64-bit words.  SEAL's Decryptor.InvariantNoiseBudget needs nothing else: budget = bitlen(q) - bitlen(norm) - 1.
//
// One workgroup per ciphertext; thread i takes coefficients i, i + NN_THREADS, ...  Per coefficient, in registers:
//   y_j = [(c0_j + acc_j) fl_c1_q[j]]_{q_j} = [x_j (q/q_j)^-1]_{q_j},   x_j = [t (c0_j + acc_j)]_{q_j}
//         (acc = c1 s [+ c2 s^2] in coefficient form, decrypt_phase; fl_c1_q[j] = [t inv_qhat_q[j]]_{q_j} with the context's own inv_qhat_q)
//   S   = sum_j y_j (q/q_j)                  K words (DevConsts::nn_qhat): S < K q < 2^(61 K + 4) <= 2^(64 K) for K >= 2; K = 1: S = y_0 < q
//   X   = S - alpha q = [v]_q,               alpha = floor(S / q) = floor(sum_j y_j / q_j)
// Exactness of the reduction: alpha is estimated in FP64 as a = floor(sum_j y_j * (1/q_j)).  Every term lies in [0, 1) and carries a relative
// error of at most 3 * 2^-53 (the conversion of y_j, the rounded reciprocal nn_qinv, the fused product-sum), and the K running sums stay below
// K <= 12: the estimate is off by less than 2^-40 < 1, so a is alpha - 1, alpha or alpha + 1 and S - a q lies in [-q, 2q).  a <= K, so
// a q < 2^(64 K) fits the K words.  ONE correction then gives the exact X in [0, q): a borrow out of the K-word subtraction (S < a q) adds q
// back, otherwise a result >= q loses one q.  (tests/noise_norm_model.py checks both corrections with a forced off-by-one estimate.)
// Centred: |X| = X if X <= q - X (the host's 2X <= q), else q - X.  The maximum over the N coefficients: per thread, across the wave (cross-lane
// shuffles), across the waves (LDS); one lane writes the K words.
#pragma once
#include "cn_dev_common.hip.h"

#define NN_THREADS 512

typedef const NTT_GLOBAL uint64_t *NnIn;
typedef NTT_GLOBAL uint64_t *NnOut;
typedef const __attribute__((address_space(4))) DevConsts *NnConsts;   // the constants: wave-uniform, scalar loads

// C, opaque to the compiler: the loads through the result are not hoisted above this point.  Wave-uniform (scalar loads).
DEV NnConsts nn_launder(const DevConsts *C) {
    uint64_t cp = (uint64_t)C;
    asm volatile("" : "+s"(cp));
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)cp), hi = (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(cp >> 32));
    return (NnConsts)(((uint64_t)hi << 32) | lo);                     // (readfirstlane returns int: widened unsigned, not sign-extended)
}
// a < b as K-word integers: the highest word in which they differ decides
template <int K> DEV bool nn_less(const uint64_t (&a)[K], const uint64_t (&b)[K]) {
    bool lt = false;
#pragma unroll
    for (int w = 0; w < K; w++) lt = a[w] < b[w] || (a[w] == b[w] && lt);
    return lt;
}
template <int K> DEV void nn_take_max(uint64_t (&best)[K], const uint64_t (&v)[K]) {
    const bool more = nn_less<K>(best, v);
#pragma unroll
    for (int w = 0; w < K; w++) best[w] = more ? v[w] : best[w];
}

// c0: first polynomial of ciphertext ct at c0_ + ct * ct_stride; acc: [count][K][N]; out: [count][K] words
template <int K>
__global__ void __launch_bounds__(NN_THREADS) k_noise_norm(const uint64_t *__restrict__ c0_, size_t ct_stride, const uint64_t *__restrict__ acc_,
                                                            uint64_t *__restrict__ out_, const DevConsts *__restrict__ C) {
    const uint32_t n = C->n, ct = blockIdx.x, tid = threadIdx.x;
    const NnIn c0 = (NnIn)c0_ + (size_t)ct * ct_stride, acc = (NnIn)acc_ + (size_t)ct * K * n;
    uint64_t best[K];
#pragma unroll
    for (int w = 0; w < K; w++) best[w] = 0;
    for (uint32_t i = tid; i < n; i += NN_THREADS) {
        // the constants are loaded again in every iteration (scalar loads that hit the scalar cache): hoisted out of the loop, the
        // K (K - 1) words of q/q_j would not fit the SGPRs and spill
        NnConsts Ci = nn_launder(C);
        uint64_t X[K];
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < K; w++) X[w] = 0;
#pragma unroll
        for (int j = 0; j < K; j++) {
            Ci = nn_launder(C);                                               // (and per limb: the SGPRs hold one limb's constants at a time)
            const DMod qm = {Ci->q[j].q, Ci->q[j].r0, Ci->q[j].r1};
            const uint64_t y = mulmod(addmod(c0[(size_t)j * n + i], acc[(size_t)j * n + i], qm.q), Ci->fl_c1_q[j], qm);
            if constexpr (K == 1) {
                X[0] = y;
            } else {
                s = fma((double)y, Ci->nn_qinv[j], s);
                uint64_t carry = 0;
#pragma unroll
                for (int w = 0; w < K - 1; w++) {
                    const u128 p = (u128)y * Ci->nn_qhat[j][w] + X[w] + carry;
                    X[w] = (uint64_t)p; carry = (uint64_t)(p >> 64);
                }
                X[K - 1] += carry;
            }
        }
        if constexpr (K > 1) {
            const uint64_t a = (uint64_t)s;                                   // s >= 0: truncation = floor
            uint64_t mc = 0, br = 0;
#pragma unroll
            for (int w = 0; w < K; w++) {                                     // X -= a q, borrow out in br
                const u128 p = (u128)a * Ci->nn_q[w] + mc;
                const uint64_t sub = (uint64_t)p, d = X[w] - sub;
                mc = (uint64_t)(p >> 64);
                const uint64_t b1 = X[w] < sub;
                X[w] = d - br; br = b1 | (uint64_t)(d < br);
            }
            uint64_t qw[K];
#pragma unroll
            for (int w = 0; w < K; w++) qw[w] = Ci->nn_q[w];
            if (br) {                                                         // S < a q: X + q (mod 2^(64 K)) is in [0, q)
                uint64_t cy = 0;
#pragma unroll
                for (int w = 0; w < K; w++) { const uint64_t u = X[w] + qw[w]; const uint64_t c1 = u < X[w]; X[w] = u + cy; cy = c1 | (uint64_t)(X[w] < u); }
            } else if (!nn_less<K>(X, qw)) {                                  // X in [q, 2q)
                uint64_t bw = 0;
#pragma unroll
                for (int w = 0; w < K; w++) { const uint64_t d = X[w] - qw[w]; const uint64_t b1 = X[w] < qw[w]; X[w] = d - bw; bw = b1 | (uint64_t)(d < bw); }
            }
        }
        uint64_t D[K], bw = 0;                                                // D = q - X > 0
#pragma unroll
        for (int w = 0; w < K; w++) { const uint64_t qw = Ci->nn_q[w], d = qw - X[w]; const uint64_t b1 = qw < X[w]; D[w] = d - bw; bw = b1 | (uint64_t)(d < bw); }
        const bool far = nn_less<K>(D, X);                                    // X > q - X
#pragma unroll
        for (int w = 0; w < K; w++) X[w] = far ? D[w] : X[w];
        nn_take_max<K>(best, X);
    }
    constexpr int WAVES = NN_THREADS / 64;
    __shared__ uint64_t red[WAVES][K];
    const uint32_t lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        uint64_t o[K];
#pragma unroll
        for (int w = 0; w < K; w++) o[w] = __shfl_xor(best[w], off);
        nn_take_max<K>(best, o);
    }
    if (lane == 0) {
#pragma unroll
        for (int w = 0; w < K; w++) red[wave][w] = best[w];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 0; w < K; w++) best[w] = lane < WAVES ? red[lane][w] : 0;
#pragma unroll
    for (int off = WAVES / 2; off >= 1; off >>= 1) {
        uint64_t o[K];
#pragma unroll
        for (int w = 0; w < K; w++) o[w] = __shfl_xor(best[w], off);
        nn_take_max<K>(best, o);
    }
    if (lane == 0) {
        const NnOut out = (NnOut)out_ + (size_t)ct * K;
#pragma unroll
        for (int w = 0; w < K; w++) out[w] = best[w];
    }
}
