// Modulus switching (cn_mod_switch): SEAL 3.2's mod_switch_scale_to_next applied KS - KD times, as ONE streaming pass.
//
// Each thread owns two consecutive coefficients of one (ciphertext, poly) item: it loads the KS source limbs with 16-byte global loads,
// performs every drop in registers (successive single drops, as SEAL's mod_switch_to loops - not one rounding by the product of the dropped
// primes) and stores the KD limbs that remain.  Dropping prime p (p = KS-1 .. KD):
//   r = (x_p + h_p) mod q_p,   x_i' = (x_i - (r mod q_i) + (h_p mod q_i)) q_p^-1 mod q_i   (i < p),   h_p = floor(q_p / 2)
// The constants (DevConsts::ms_inv / ms_invs / ms_h) are wave-uniform: scalar loads.  Arithmetic: r mod q_i by one-word Barrett
// (floor(2^64/q_i) = DMod::r1, quotient off by at most one), the product by Shoup's method; every step ends canonical.
#pragma once
#include "cn_dev_common.hip.h"

typedef uint64_t ms_u64x2 __attribute__((ext_vector_type(2)));   // 16-byte global load / store
typedef const NTT_GLOBAL ms_u64x2 *MsIn;
typedef NTT_GLOBAL ms_u64x2 *MsOut;

// x mod q for any 64-bit x: q < 2^62, r1 = floor(2^64 / q) - the quotient estimate is low by at most one
DEV uint64_t ms_reduce(uint64_t x, const DMod &m) {
    const uint64_t r = x - __umul64hi(x, m.r1) * m.q;
    return r >= m.q ? r - m.q : r;
}
DEV uint64_t ms_one(uint64_t xi, uint64_t r, uint64_t hi, uint64_t inv, uint64_t invs, const DMod &m) {
    const uint64_t q = m.q;
    uint64_t v = submod(xi, ms_reduce(r, m), q);
    v = addmod(v, hi, q);
    const uint64_t y = shoup_lazy(v, inv, invs, q);
    return y >= q ? y - q : y;
}

// items = (ciphertext, poly) pairs; src item i at src + i * KS * N, dst item i at dst + i * KD * N
template <int KS, int KD>
__global__ void __launch_bounds__(256) k_mod_switch(const uint64_t *__restrict__ src_, uint64_t *__restrict__ dst_, const DevConsts *__restrict__ C,
                                                     uint32_t items, uint32_t logn) {
    static_assert(KD >= 1 && KD < KS, "a switch drops at least one prime and keeps at least one");
    const uint32_t half_logn = logn - 1;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;          // one pair of coefficients
    if (g >= ((uint64_t)items << half_logn)) return;
    const uint32_t item = (uint32_t)(g >> half_logn), pair = (uint32_t)(g & ((1u << half_logn) - 1));
    const size_t n2 = (size_t)1 << half_logn;                                     // 16-byte pairs per limb
    MsIn src = (MsIn)src_ + (size_t)item * KS * n2 + pair;
    MsOut dst = (MsOut)dst_ + (size_t)item * KD * n2 + pair;
    uint64_t x[KS], y[KS];
#pragma unroll
    for (int j = 0; j < KS; j++) { const ms_u64x2 v = src[(size_t)j * n2]; x[j] = v.x; y[j] = v.y; }
#pragma unroll
    for (int p = KS - 1; p >= KD; p--) {
        const DMod mp = C->q[p];
        const uint64_t h = mp.q >> 1;
        const uint64_t rx = addmod(x[p], h, mp.q), ry = addmod(y[p], h, mp.q);
#pragma unroll
        for (int i = 0; i < p; i++) {
            const DMod mi = C->q[i];
            const uint64_t inv = C->ms_inv[p][i], invs = C->ms_invs[p][i], hi = C->ms_h[p][i];
            x[i] = ms_one(x[i], rx, hi, inv, invs, mi);
            y[i] = ms_one(y[i], ry, hi, inv, invs, mi);
        }
    }
#pragma unroll
    for (int j = 0; j < KD; j++) { ms_u64x2 v; v.x = x[j]; v.y = y[j]; dst[(size_t)j * n2] = v; }
}
