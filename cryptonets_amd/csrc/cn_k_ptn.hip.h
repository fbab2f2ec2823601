// Sums of products with NTT-form weight plaintexts (cn_mul_plain_sum on a kind-4 array, N = 2^L, L = 10..14).  Included by cn_l_ptn.hip.
#pragma once
#include "cn_dev_common.hip.h"

// out[g] = INTT( sum_{e in [grp_off[g], grp_off[g + 1])} ptn[e] . ctn[slot[e]] ): the plaintexts arrive as Evaluator.TransformToNtt left them (cn_pt_transform:
// ptn [e][k][N], canonical words NTT_j(lift_j(m_e)) in the order k_lift_ntt writes), the distinct ciphertexts transformed once per call (ctn [slot][2][k][N],
// canonical) - so a term is loads, one modular product and one addition per word at the positions the inverse transform starts from (tail_index).  The loop has
// no transform, no LDS traffic and no barrier; ONE inverse transform per polynomial, N^-1 and one store end the block.  Same words as k_mul_plain_sum and as
// MultiplyPlain + Add in any order (exact modular arithmetic, canonical results).
// Block = (limb j, group g) with BOTH polynomials (NP = 2: a plaintext limb is read once per term), or (limb j, group g, poly p) (NP = 1) where two accumulator
// sets do not fit the registers (cn_l_ptn.hip says which size has which).  The block index is limb-major (j = blockIdx.x / units): all groups of a diagonal plan
// walk the same rotated inputs, so the blocks in flight share ONE limb of the D ciphertexts (D x 2 x 8N bytes: 4 MiB of the 32 MiB at CIFAR shapes).  The other order
// ("ptn_order" = 1: limb = block index mod k, a limb per XCD at k = 8) measured the same at CIFAR shapes (profiles/ntt_weights.md); limb-major is the default.
// Latency is hidden by loads in flight, not by waves: a term is cut into chunks of WS register pairs, and the 16-byte loads of the chunk D ahead (of the next term
// behind the last chunks) are requested before the arithmetic of the current one.  With ONE chunk of one pair ahead at N = 16384 the kernel ran at one memory
// round trip per chunk (5.6 ms per CIFAR layer and prime, 1024 blocks x 128 terms x 8 chunks x 1.4 us over 256 CUs); two ahead is what its 128 registers allow.
//
// The lazy FP64 accumulators.  A term is mulmod(x, w) of two CANONICAL words 0 <= x, w < q < 2^49.4 (k_mul_plain_sum multiplies a lazy transform output, up to
// 6.3 q, by a canonical word: its "2.1 q" does not apply here).  ArF64T::mulmod returns r = x w - h q EXACTLY, h = rint(fl(fl(x w) fl(1/q))): three roundings,
// |h - x w / q| <= 1/2 + 3 2^-53 x w / q < 1/2 + 3 q 2^-53, hence
//     |term| <= q/2 + 3 q^2 / 2^53          (0.69 q at 49 bits, 0.5 q + 1 up to 26 bits; cn_ptn_term_bound, cn_policy.h, rounds it up to an integer).
// `interval` terms are added between two recentrings (cn_ptn_sum_interval: the largest count with interval x bound < 2^52); a recentred accumulator is at most
// q/2 + 1 < 2^49, so every partial sum stays below 2^52 + 2^49 < 2^53: exact integers in a double, and ArF64T::center / ntt_inverse_regs (which recentres first)
// accept any |x| < 2^53.  The integer policy keeps canonical sums (addmod) and never settles.
template <class AR> struct PtnMac;
template <> struct PtnMac<ArU64> {
    static DEV void mac(uint64_t &acc, uint64_t x, uint64_t w, const DMod &qm, const ArCtx<ArU64> &) { acc = addmod(acc, mulmod(x, w, qm), qm.q); }
    static DEV void settle(uint64_t (&)[16], const ArCtx<ArU64> &) {}
};
template <int RN> struct PtnMac<ArF64T<RN>> {
    typedef ArF64T<RN> ArF64;
    static DEV void mac(double &acc, uint64_t x, uint64_t w, const DMod &, const ArCtx<ArF64> &A) {
        acc = __dadd_rn(acc, ArF64::mulmod(ArF64::from_u64(x), ArF64::from_u64(w), A.m));
    }
    static DEV void settle(double (&a)[16], const ArCtx<ArF64> &A) { ArF64::renorm(a, A.m); }
};
// the words of one chunk: WS register pairs of the plaintext limb and of NP ciphertext limbs
template <int NP, int WS> struct PtnChunk { ulonglong2 x[WS], y[NP][WS]; };
template <int L, int NP, int WS, int H> DEV void ptn_load(PtnChunk<NP, WS> &c, const uint64_t *__restrict__ x, const uint64_t *__restrict__ w, size_t wpoly, uint32_t tl) {
#pragma unroll
    for (int i = 0; i < WS; i++) {
        const uint32_t at = tail_index<L>(tl, 2 * (H * WS + i));
        c.x[i] = *reinterpret_cast<const ulonglong2 *>(x + at);
#pragma unroll
        for (int p = 0; p < NP; p++) c.y[p][i] = *reinterpret_cast<const ulonglong2 *>(w + p * wpoly + at);
    }
}
template <class AR, int NP, int WS, int H> DEV void ptn_mac(typename AR::T (&acc)[NP][16], const PtnChunk<NP, WS> &c, const DMod &qm, const ArCtx<AR> &A) {
#pragma unroll
    for (int i = 0; i < WS; i++) {
        const int r = 2 * (H * WS + i);
#pragma unroll
        for (int p = 0; p < NP; p++) { PtnMac<AR>::mac(acc[p][r], c.x[i].x, c.y[p][i].x, qm, A); PtnMac<AR>::mac(acc[p][r + 1], c.x[i].y, c.y[p][i].y, qm, A); }
    }
}
// chunk H of the term at (x, w): request the chunk D ahead (`xn`, `wn`: the next term, behind the last chunks) into the slot this chunk leaves, then the arithmetic of
// this one - D chunks are in flight while one is multiplied (D divides the chunks of a term, so a chunk's slot H mod D is the same in every term)
template <int L, class AR, int NP, int WS, int D, int H> DEV void ptn_term(typename AR::T (&acc)[NP][16], PtnChunk<NP, WS> (&q)[D], const uint64_t *__restrict__ x,
                                                                           const uint64_t *__restrict__ w, const uint64_t *__restrict__ xn, const uint64_t *__restrict__ wn,
                                                                           size_t wpoly, uint32_t tl, const DMod &qm, const ArCtx<AR> &A) {
    constexpr int CH = 8 / WS;
    PtnChunk<NP, WS> nxt;
    if constexpr (H + D < CH) ptn_load<L, NP, WS, H + D>(nxt, x, w, wpoly, tl); else ptn_load<L, NP, WS, H + D - CH>(nxt, xn, wn, wpoly, tl);
    ptn_mac<AR, NP, WS, H>(acc, q[H % D], qm, A);
    q[H % D] = nxt;
    if constexpr (H + 1 < CH) ptn_term<L, AR, NP, WS, D, H + 1>(acc, q, x, w, xn, wn, wpoly, tl, qm, A);
}
template <int L, int NP, int WS, int D, int H> DEV void ptn_prime(PtnChunk<NP, WS> (&q)[D], const uint64_t *__restrict__ x, const uint64_t *__restrict__ w, size_t wpoly, uint32_t tl) {
    ptn_load<L, NP, WS, H>(q[H], x, w, wpoly, tl);
    if constexpr (H + 1 < D) ptn_prime<L, NP, WS, D, H + 1>(q, x, w, wpoly, tl);
}
// one accumulator set -> coefficients: inverse transform, N^-1, canonical store
template <int L, class AR> DEV void ptn_finish(typename AR::T (&acc)[16], typename AR::T *s, const ArCtx<AR> &A, uint64_t *__restrict__ o, uint32_t tid) {
    uint32_t ti = tid;
    asm volatile("" : "+v"(ti));
    ntt_inverse_regs<AR, L>(acc, s, A.iv, A.m, ti);
#pragma unroll
    for (int r = 0; r < 16; r++) o[pass_index<L, NttPlan<L>::SA, 0>(ti, r)] = A.scaled(acc[r]);
}
template <int L, class AR, int NP, int WS, int D>
__global__ void __launch_bounds__(NttPlan<L>::NT) k_mul_ptn_sum(const uint64_t *__restrict__ ptn, const uint64_t *__restrict__ ctn, const uint32_t *__restrict__ grp_off,
                                                                const uint32_t *__restrict__ slot, uint64_t *__restrict__ out, const DevConsts *__restrict__ C, uint32_t interval,
                                                                uint32_t units, uint32_t by_xcd) {
    typedef typename AR::T T;
    static_assert((NP == 1 || NP == 2) && (WS == 1 || WS == 2 || WS == 4 || WS == 8) && D >= 1 && (8 / WS) % D == 0,
                  "k_mul_ptn_sum: one or two polynomials, chunks of 1, 2, 4 or 8 register pairs, a depth that divides the chunks of a term");
    extern __shared__ __align__(16) unsigned char smem[];
    T *s = reinterpret_cast<T *>(smem);
    constexpr uint32_t n = 1u << L;
    // block order ("ptn_order"): 0 limb-major; 1 limb = blockIdx.x mod k - with k = 8 the blocks of a limb share an XCD (its L2), the idea of the key switch's "ks_xcd"
    const uint32_t tid = threadIdx.x, k = C->k, j = by_xcd ? blockIdx.x % k : blockIdx.x / units, u = by_xcd ? blockIdx.x / k : blockIdx.x % units;
    const uint32_t g = NP == 2 ? u : u >> 1, p0 = NP == 2 ? 0u : u & 1u;
    const DMod qm = C->q[j];
    const ArCtx<AR> A(C, j);
    const size_t wpoly = (size_t)k * n;                                     // from poly 0 to poly 1 of a transformed ciphertext
    const uint32_t e0 = grp_off[g], e1 = grp_off[g + 1];
    T acc[NP][16];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[p][r] = 0;
    uint32_t tl = tid;
    asm volatile("" : "+v"(tl));                                            // the loop's address math apart from the inverse transform's
    const uint64_t *x = ptn + ((size_t)e0 * k + j) * n;
    const uint64_t *w = ctn + (((size_t)slot[e0] * 2 + p0) * k + j) * n;
    PtnChunk<NP, WS> q[D];
    ptn_prime<L, NP, WS, D, 0>(q, x, w, wpoly, tl);
    uint32_t terms = 0;
#pragma unroll 1
    for (uint32_t e = e0; e < e1; e++) {
        const uint32_t en = e + 1 < e1 ? e + 1 : e;                        // (behind the last term: its own first chunks again - in bounds, never used)
        const uint64_t *xn = ptn + ((size_t)en * k + j) * n;
        const uint64_t *wn = ctn + (((size_t)slot[en] * 2 + p0) * k + j) * n;
        ptn_term<L, AR, NP, WS, D, 0>(acc, q, x, w, xn, wn, wpoly, tl, qm, A);
        x = xn; w = wn;
        if (++terms == interval) {
            terms = 0;
#pragma unroll
            for (int p = 0; p < NP; p++) PtnMac<AR>::settle(acc[p], A);
        }
    }
    ptn_finish<L, AR>(acc[0], s, A, out + (((size_t)g * 2 + p0) * k + j) * n, tid);
    if constexpr (NP == 2) {
        __syncthreads();                                                    // everybody has taken poly 0's coefficients out of the image
        ptn_finish<L, AR>(acc[1], s, A, out + (((size_t)g * 2 + 1) * k + j) * n, tid);
    }
}
