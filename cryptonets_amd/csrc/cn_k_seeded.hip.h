// Seeded symmetric ciphertexts (include/cnhip.h: cn_encrypt_symmetric, cn_ct_expand): c1 of a fresh secret-key encryption is INTT(a) for a uniform a that
// anybody regenerates from 32 public bytes, so only c0 has to travel.
//
//   a_j (limb j of item i) = sample_uniform8(a_seed, a_nonce, CN_STREAM_A, a_item0 + i, j * (N/8) + b, q_j), b = 0 .. N/8 - 1: the layout k_sample_uniform gives
//   the `a` of a key, read as the NTT form in the library's transform order.  c1 = INTT(a), c0 = INTT(-a . s) + e + Delta m (the embedding of EncTail).
//
// One kernel, block = (ciphertext, component p, limb j), NT = N/16 threads:
//   * the draw: a ChaCha20 block is 8 CONSECUTIVE positions of a, while the inverse transform starts from pairs that lie 64 positions apart (tail_index) - a thread
//     that drew "its own" 16 registers would compute 8 blocks and drop three quarters of each.  So thread tid draws blocks 2 tid and 2 tid + 1 (positions 16 tid ..
//     16 tid + 15), puts them into the exchange image and takes its 16 registers out of it in the layout of the inverse transform.  For N <= 8192 the positions a
//     thread draws and the positions it starts from lie in the same 512-position block, which one half-wave owns (tail_index): that exchange is wave-local like
//     the transform's own.  a never exists in HBM.
//   * p = 1: inverse transform, N^-1, store: c1.  p = 0: times s (NTT form, 16 B per lane at the thread's positions), negated, inverse transform and the epilogue
//     of the public-key encryption kernels (EncTail: N^-1, + e from the int8 noise polynomial, + Delta m, ONE canonicalisation): c0.
//   * cn_ct_expand launches the p = 1 blocks alone; cn_encrypt_symmetric launches both components, so the draw runs twice per (ciphertext, limb): two inverse
//     transforms per (ciphertext, limb) against the four transforms of cn_encrypt.  Measured (profiles/seeded_probe.txt): the expansion takes 2.08 x (N = 8192) /
//     1.73 x (N = 16384) its inverse transforms alone - a draw costs about a transform - and the encryption 0.99 x / 0.91 x cn_encrypt.  A kernel that keeps a in
//     registers for both components (one draw less, one workgroup per CU) has not been built or measured.
//   * N = 16384 runs on the plain NttPlan<14> (one 1024-thread workgroup, 106-118 VGPRs, no scratch), not as two 8192-point halves.
//   * stores: 8 B per lane, coalesced, through pass_index like every inverse-transform epilogue here; s and the exchange image move 16 B per lane.
// The reduction of a 64-bit word mod q_j is the Barrett reduction of the context (exact: the same residue as the % of sample_uniform8, tests/seeded_model.py).
#pragma once
#include "cn_k_rr.hip.h"

// sample_uniform8 (cn_dev_common.hip.h) with the context's Barrett constants in place of the two 64-bit divisions per word: the same 8 residues
DEV void seeded_uniform8(const RngKey &key, uint64_t nonce, uint64_t item, uint32_t blk, const DMod &qm, uint64_t (&out)[8]) {
    const uint64_t lim = ~0ull - bred128(~0ull, 0, qm) - 1;
    uint32_t pending = 0xff;
    for (uint32_t trial = 0; pending; trial++) {
        uint32_t w[16];
        chacha20_block(key, rng_counter(item, CN_STREAM_A, trial, blk), nonce, w);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const uint64_t v = ((uint64_t)w[2 * c] << 32) | w[2 * c + 1];
            if ((pending & (1u << c)) && v <= lim) { out[c] = bred128(v, 0, qm); pending &= ~(1u << c); }
        }
    }
}

// out: poly 0 of ciphertext ct at out + ct * ct_stride; comp0 = 1: the p = 1 blocks only (expansion).  sk, noise, pt are read by the p = 0 blocks only.
template <int L, class AR>
__global__ void __launch_bounds__(NttPlan<L>::NT, 4) k_seeded(uint64_t *__restrict__ out, size_t ct_stride, const DevConsts *__restrict__ C, RngKey akey, uint64_t a_nonce, uint64_t a_item0,
                                                           uint32_t comp0, const uint64_t *__restrict__ sk, const int8_t *__restrict__ noise, const uint64_t *__restrict__ pt,
                                                           uint32_t pt_stride_words) {
    typedef typename AR::T T;
    extern __shared__ __align__(16) unsigned char smem[];
    T *s = reinterpret_cast<T *>(smem);
    constexpr uint32_t n = 1u << L;
    constexpr int SA = NttPlan<L>::SA;
    const uint32_t k = C->k, tid = threadIdx.x, comps = 2 - comp0, j = blockIdx.x % k, p = comp0 + (blockIdx.x / k) % comps, ct = blockIdx.x / (comps * k);
    const ArCtx<AR> A(C, j);
    const DMod qm = C->q[j];
    struct alignas(16) P2 { T a, b; };
#pragma unroll 1
    for (uint32_t h = 0; h < 2; h++) {                                       // one block's words live at a time
        uint64_t w[8];
        const uint32_t blk = 2 * tid + h;
        seeded_uniform8(akey, a_nonce, a_item0 + ct, j * (n / 8) + blk, qm, w);
#pragma unroll
        for (int c = 0; c < 8; c += 2) *reinterpret_cast<P2 *>(s + lds_pos(8 * blk + c)) = P2{A.load(w[c]), A.load(w[c + 1])};
    }
    if (ntt_tail_local<L>()) ntt_wave_sync(); else __syncthreads();
    T v[16];
    lds_get_tail<T, L>(v, s, tid);
    if (p == 0) {                                                            // -a . s at the positions the thread holds
        const TensorOps<AR> ops(C, j);
        const uint64_t *ss = sk + (size_t)j * n;                             // (a kernel argument: global, not flat, loads)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const ulonglong2 y = *reinterpret_cast<const ulonglong2 *>(ss + tail_index<L>(tid, r));
            if constexpr (std::is_same<T, double>::value) { v[r] = -ops.mul(v[r], A.load(y.x), A); v[r + 1] = -ops.mul(v[r + 1], A.load(y.y), A); }
            else { v[r] = negmod(ops.mul(v[r], y.x, A), qm.q); v[r + 1] = negmod(ops.mul(v[r + 1], y.y, A), qm.q); }
        }
    }
    if (!ntt_tail_local<L>()) __syncthreads();                               // everybody has taken its words out of the image
    ntt_inverse_regs<AR, L>(v, s, A.iv, A.m, tid);
    NTT_GLOBAL uint64_t *o = (NTT_GLOBAL uint64_t *)out + (size_t)ct * ct_stride + ((size_t)p * k + j) * n;
    if (p == 1) {
#pragma unroll
        for (int r = 0; r < 16; r++) o[pass_index<L, SA, 0>(tid, r)] = A.scaled(v[r]);
        return;
    }
    const NTT_GLOBAL uint64_t *m = pt ? (const NTT_GLOBAL uint64_t *)pt + (size_t)ct * pt_stride_words : nullptr;
    const NTT_GLOBAL int8_t *ee = (const NTT_GLOBAL int8_t *)noise + (size_t)ct * n;
    const EncTail<AR> tail(A, C, j, qm.q);
    const bool has_m = m != nullptr;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const uint32_t e = pass_index<L, SA, 0>(tid, r);
        o[e] = tail.word(v[r], ee[e], has_m, has_m ? m[e] : 0);
    }
}
