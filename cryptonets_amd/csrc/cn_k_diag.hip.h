// Sums of plaintext x ciphertext products on the register-radix core (cn_mul_plain_sum; N = 2^L, L = 10..14): the inner loop of a generalized-diagonal
// (baby-step giant-step) matrix-vector product, DESIGN §6g.  Included by cn_l_diag.hip.
#pragma once
#include "cn_dev_common.hip.h"

// out[g] = sum_{e in [grp_off[g], grp_off[g + 1])} MultiplyPlain(ct[slot[e]], pt[e]) in ONE kernel: block = (group g, poly p, limb j).  The distinct ciphertexts
// arrive in NTT form (ctn: [slot][2][k][N], canonical - transformed once per call like the one ciphertext of k_mul_plain_bcast); per term the block lifts the
// plaintext into q_j while loading it (k_lift_ntt: t_half, lift_inc), transforms IT, multiplies by the ciphertext's NTT words at the positions the thread holds
// (16 B/lane) and accumulates in registers - canonical sums under the integer policy, lazy doubles recentred every `accmax` terms under the FP64 policies (the
// accumulators of the key switch: a term mulmod(v, word) of a lazy transform output and a canonical word is at most 2.1 q).  ONE inverse transform, N^-1 and one
// store per block: no NTT-form product and no lifted plaintext ever exists in HBM, and the words are those of MultiplyPlain + Add in any order (exact modular
// arithmetic, canonical results).
// A block per POLYNOMIAL (the plaintext is transformed by both blocks of a group): the transform's 16 values and one set of 16 accumulators fit the 128 registers
// a 1024-thread workgroup (N = 16384) leaves a thread; two accumulator sets in FP64 do not.
// The image of a term's transform is reused by the next term's: the "image is free again" barrier sits behind the next first pass (ntt_forward_regs<.., PRE>).
template <class AR> struct DiagMac;
template <> struct DiagMac<ArU64> {
    static DEV void mac(uint64_t &acc, uint64_t x, uint64_t w, const DMod &qm, const ArCtx<ArU64> &) { acc = addmod(acc, mulmod(canon4(x, qm.q), w, qm), qm.q); }
    static DEV void settle(uint64_t (&)[16], const ArCtx<ArU64> &) {}
};
template <int RN> struct DiagMac<ArF64T<RN>> {
    typedef ArF64T<RN> ArF64;
    static DEV void mac(double &acc, double x, uint64_t w, const DMod &, const ArCtx<ArF64> &A) { acc = __dadd_rn(acc, ArF64::mulmod(x, ArF64::from_u64(w), A.m)); }
    static DEV void settle(double (&a)[16], const ArCtx<ArF64> &A) { ArF64::renorm(a, A.m); }
};
template <int L, class AR>
__global__ void __launch_bounds__(NttPlan<L>::NT) k_mul_plain_sum(const uint64_t *__restrict__ pt, const uint64_t *__restrict__ ctn, const uint32_t *__restrict__ grp_off,
                                                                  const uint32_t *__restrict__ slot, uint64_t *__restrict__ out, const DevConsts *__restrict__ C, uint32_t accmax) {
    typedef typename AR::T T;
    extern __shared__ __align__(16) unsigned char smem[];
    T *s = reinterpret_cast<T *>(smem);
    constexpr uint32_t n = 1u << L;
    constexpr int SA = NttPlan<L>::SA;
    const uint32_t tid = threadIdx.x, k = C->k, j = blockIdx.x % k, gp = blockIdx.x / k, g = gp >> 1, p = gp & 1;
    const DMod qm = C->q[j];
    const ArCtx<AR> A(C, j);
    const uint64_t th = C->t_half, inc = C->lift_inc[j];
    const uint32_t e0 = grp_off[g], e1 = grp_off[g + 1];
    T acc[16];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0;
    uint32_t terms = 0;
#pragma unroll 1
    for (uint32_t e = e0; e < e1; e++) {
        uint32_t tl = tid;
        asm volatile("" : "+v"(tl));                   // one transform's address math / twiddles live at a time (see k_keyswitch_rr)
        const uint64_t *x = pt + (size_t)e * n;
        const uint64_t *w = ctn + (((size_t)slot[e] * 2 + p) * k + j) * n;
        T v[16];
#pragma unroll
        for (int r = 0; r < 16; r++) { const uint64_t m = x[pass_index<L, SA, 0>(tl, r)]; v[r] = A.load(m >= th ? m + inc : m); }
        ntt_forward_regs<AR, L, true>(v, s, A.fw, A.m, tl);
        // the ciphertext words in sets of WS 16-byte loads: all eight in flight beside v and acc are the whole register file of a 1024-thread workgroup
        constexpr int WS = std::is_same<T, uint64_t>::value ? 1 : (L == 14 ? 4 : 8);
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 2 * WS) {
            if (WS < 8) __builtin_amdgcn_sched_barrier(0);
            ulonglong2 y[WS];
#pragma unroll
            for (int i = 0; i < WS; i++) y[i] = *reinterpret_cast<const ulonglong2 *>(w + tail_index<L>(tl, r0 + 2 * i));
#pragma unroll
            for (int i = 0; i < WS; i++) { DiagMac<AR>::mac(acc[r0 + 2 * i], v[r0 + 2 * i], y[i].x, qm, A); DiagMac<AR>::mac(acc[r0 + 2 * i + 1], v[r0 + 2 * i + 1], y[i].y, qm, A); }
        }
        if (++terms == accmax) { terms = 0; DiagMac<AR>::settle(acc, A); }
    }
    if (!ntt_tail_local<L>()) __syncthreads();         // (block-local tail: the inverse starts inside the wave's own blocks)
    uint32_t ti = tid;
    asm volatile("" : "+v"(ti));
    ntt_inverse_regs<AR, L>(acc, s, A.iv, A.m, ti);
    uint64_t *o = out + ((size_t)gp * k + j) * n;
#pragma unroll
    for (int r = 0; r < 16; r++) o[pass_index<L, SA, 0>(ti, r)] = A.scaled(acc[r]);
}
