// Modulus switching in exact FP64 (cn_mod_switch on chains whose moduli are all below 2^49): the same successive single drops as
// k_mod_switch (cn_k_modswitch.hip.h), the same words, with every modular step on the FP64 pipe instead of 64-bit integer products.
//
// Dropping prime p (p = KS-1 .. KD):  r = (x_p + h_p) mod q_p,  x_i' = (x_i - r + (h_p mod q_i)) q_p^-1 mod q_i  (i < p).
// Every residue is a canonical double (an exact integer below 2^49).  v = x_i - r + h_i needs no reduction of r modulo q_i: |v| < 3 * 2^49.
// ArF64::mulmod (the product of the transforms and key switches, cn_ntt_core.hip.h) is exact for it, and with the constant centred
// (|w| <= q_i / 2) the quotient estimate of v w / q_i is off by at most 1/2 + 3 2^-53 |v| / 2 < 0.79: the result r' = v w - h q_i is exact
// with |r'| < q_i, and one conditional add of q_i makes it canonical.  The integer kernel's result is the same canonical residue: identical
// words.
// The constants (DevConsts::qd / qinvd / ms_invd / ms_hd) are wave-uniform: scalar loads.  Loads and stores: 16 B per lane, global.
#pragma once
#include "cn_dev_common.hip.h"
#include "cn_k_modswitch.hip.h"

DEV double msd_canon(double r, double q) { return r < 0.0 ? __dadd_rn(r, q) : r; }           // |r| < q -> [0, q)

// items = (ciphertext, poly) pairs; src item i at src + i * KS * N, dst item i at dst + i * KD * N
template <int KS, int KD>
__global__ void __launch_bounds__(256) k_mod_switch_f64(const uint64_t *__restrict__ src_, uint64_t *__restrict__ dst_, const DevConsts *__restrict__ C,
                                                         uint32_t items, uint32_t logn) {
    static_assert(KD >= 1 && KD < KS, "a switch drops at least one prime and keeps at least one");
    const uint32_t half_logn = logn - 1;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;          // one pair of coefficients
    if (g >= ((uint64_t)items << half_logn)) return;
    const uint32_t item = (uint32_t)(g >> half_logn), pair = (uint32_t)(g & ((1u << half_logn) - 1));
    const size_t n2 = (size_t)1 << half_logn;                                     // 16-byte pairs per limb
    MsIn src = (MsIn)src_ + (size_t)item * KS * n2 + pair;
    MsOut dst = (MsOut)dst_ + (size_t)item * KD * n2 + pair;
    double x[KS], y[KS];
#pragma unroll
    for (int j = 0; j < KS; j++) { const ms_u64x2 v = src[(size_t)j * n2]; x[j] = ArF64::from_u64(v.x); y[j] = ArF64::from_u64(v.y); }
#pragma unroll
    for (int p = KS - 1; p >= KD; p--) {
        const double qp = C->qd[p], hp = C->ms_hd[p][p];
        double rx = __dadd_rn(x[p], hp), ry = __dadd_rn(y[p], hp);               // < 2 q_p: exact
        rx = rx >= qp ? __dadd_rn(rx, -qp) : rx;
        ry = ry >= qp ? __dadd_rn(ry, -qp) : ry;
#pragma unroll
        for (int i = 0; i < p; i++) {
            const ArF64::Mod mi = {C->qd[i], C->qinvd[i]};
            const double inv = C->ms_invd[p][i], hi = C->ms_hd[p][i];
            x[i] = msd_canon(ArF64::mulmod(__dadd_rn(__dadd_rn(x[i], hi), -rx), inv, mi), mi.q);
            y[i] = msd_canon(ArF64::mulmod(__dadd_rn(__dadd_rn(y[i], hi), -ry), inv, mi), mi.q);
        }
    }
#pragma unroll
    for (int j = 0; j < KD; j++) {
        ms_u64x2 v;                                               // canonical doubles below 2^49: the integer is the value
        v.x = (uint64_t)__double_as_longlong(__dadd_rn(x[j], 4503599627370496.0)) & 0x000FFFFFFFFFFFFFull;
        v.y = (uint64_t)__double_as_longlong(__dadd_rn(y[j], 4503599627370496.0)) & 0x000FFFFFFFFFFFFFull;
        dst[(size_t)j * n2] = v;
    }
}
