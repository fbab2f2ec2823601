// Galois keys for a caller's own list of elements in ONE launch (include/cnhip.h: cn_keygen_galois).  cn_keygen builds a key-switch key as a host loop over its
// (l, d) entries - uniform draw, noise draw, expansion, forward transform, k_key_b per entry, and INTT -> k_galois -> NTT of the secret key per element; this
// kernel makes every entry of every listed element at once and produces the SAME words:
//
//   entry e = (l, d) of the g-th listed element, limb j:   a = sample_uniform8(sampler key, seed, stream 3, item0 + 2 (g tot + e), j (N/8) + b, q_j)   [k_sample_uniform]
//                                                          e^ = NTT(noise polynomial of stream 1, item0 + 2 (g tot + e) + 1)                          [k_sample_small]
//                                                          b = -(a . s_j + e^) + f_j . sigma_g(s)_j,   f = the KeyFactors of gen_ksk (zero unless j = l)
//
// Block = (element g, entry e, limb j), NT = N/16 threads, on the register-radix NttPlan:
//   * the draw of a comes first and follows k_seeded: thread tid draws blocks 2 tid and 2 tid + 1 (positions 16 tid .. 16 tid + 15) into the exchange image and
//     takes its 16 words out in the tail layout - wave-local for N <= 8192 (both position sets lie in the 512-position block the half-wave owns).  The image
//     carries the raw 64-bit words whatever the arithmetic policy (bit casts, no conversion).  a leaves for the key at once and the thread reads its own 16 words
//     back in the last step: nothing but the transform's registers is live during the transform (a kept in registers across it: spills at 128 VGPRs).
//   * then the noise arrives as the int8 polynomials of ONE k_sample_small launch over all entries (drawn once per coefficient, like encrypt_chain's), becomes residues
//     mod q_j in registers and takes the ONE forward transform of the block; the canonical words stay in 16 registers at the positions of tail_index.
//   * sigma_g(s) needs no transform: in NTT form x -> x^g permutes the evaluation points.  Slot i of the library's order (minimal primitive root psi, bit-reversed)
//     holds the value at psi^(2 brev(i) + 1), so sigma_g(s)[i] = s[brev(((2 brev(i) + 1) g mod 2N - 1) / 2)] (tests/test_galois_steps_model.py derives it against
//     INTT -> automorphism -> NTT).  The host builds that index table once per element (uint16: N <= 16384) and the blocks with j = l gather s_j through it.
//   * the pointwise part runs in 64-bit integers for every policy (32 modular products per thread against the ~100 butterflies of the transform): exact, so the words
//     do not depend on the policy.  Stores: 16 B per lane, a half-wave covers 512 contiguous bytes (tail_index); the FP64 image of a context that keeps its keys
//     as doubles (keys_as_f64) is written by the kernel itself.
#pragma once
#include "cn_dev_common.hip.h"

typedef uint64_t ksk_u64x2 __attribute__((ext_vector_type(2)));
struct KskOut { NTT_GLOBAL uint64_t *key; };                 // one key per listed element: [(l,d)][2][k][N]
struct KskFactors { uint64_t f[CN_MAXK]; };                  // per entry: the message factor of every limb (gen_ksk)

// sample_uniform8 (cn_dev_common.hip.h) with the context's Barrett constants in place of the two 64-bit divisions per word: the same 8 residues
DEV void ksk_uniform8(const RngKey &key, uint64_t nonce, uint32_t stream, uint64_t item, uint32_t blk, const DMod &qm, uint64_t (&out)[8]) {
    const uint64_t lim = ~0ull - bred128(~0ull, 0, qm) - 1;
    uint32_t pending = 0xff;
    for (uint32_t trial = 0; pending; trial++) {
        uint32_t w[16];
        chacha20_block(key, rng_counter(item, stream, trial, blk), nonce, w);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const uint64_t v = ((uint64_t)w[2 * c] << 32) | w[2 * c + 1];
            if ((pending & (1u << c)) && v <= lim) { out[c] = bred128(v, 0, qm); pending &= ~(1u << c); }
        }
    }
}
template <class T> DEV T ksk_bits_in(uint64_t v);
template <> DEV uint64_t ksk_bits_in<uint64_t>(uint64_t v) { return v; }
template <> DEV double ksk_bits_in<double>(uint64_t v) { return __longlong_as_double((long long)v); }
DEV uint64_t ksk_bits_out(uint64_t v) { return v; }
DEV uint64_t ksk_bits_out(double v) { return (uint64_t)__double_as_longlong(v); }
DEV uint64_t ksk_unword(uint64_t w, bool f64) { return f64 ? (uint64_t)(long long)__longlong_as_double((long long)w) : w; }
DEV uint64_t ksk_word(uint64_t v, bool f64) { return f64 ? (uint64_t)__double_as_longlong((double)(long long)v) : v; }      // (exact: keys_as_f64 means residues < 2^49)

template <int L, class AR>
__global__ void __launch_bounds__(NttPlan<L>::NT, 4) k_ksk_gen(const KskOut *__restrict__ outs, const KskFactors *__restrict__ fac, const uint16_t *__restrict__ perm,
                                                            const int8_t *__restrict__ noise, const uint64_t *__restrict__ sk, const DevConsts *__restrict__ C,
                                                            RngKey key, uint64_t nonce, uint64_t item0, uint32_t tot, uint32_t f64out) {
    typedef typename AR::T T;
    extern __shared__ __align__(16) unsigned char smem[];
    T *s = reinterpret_cast<T *>(smem);
    constexpr uint32_t n = 1u << L;
    constexpr int SA = NttPlan<L>::SA;
    const uint32_t k = C->k, tid = threadIdx.x, j = blockIdx.x % k, ge = blockIdx.x / k, e = ge % tot, g = ge / tot;
    const ArCtx<AR> A(C, j);
    const DMod qm = C->q[j];
    const bool f64 = f64out != 0;
    NTT_GLOBAL uint64_t *ob = outs[g].key + ((size_t)e * 2 * k + j) * n, *oa = ob + (size_t)k * n;
    struct alignas(16) P2 { T a, b; };
#pragma unroll 1
    for (uint32_t h = 0; h < 2; h++) {                                       // one block's words live at a time
        uint64_t w[8];
        const uint32_t blk = 2 * tid + h;
        ksk_uniform8(key, nonce, 3u, item0 + 2ull * ge, j * (n / 8) + blk, qm, w);
#pragma unroll
        for (int c = 0; c < 8; c += 2) *reinterpret_cast<P2 *>(s + lds_pos(8 * blk + c)) = P2{ksk_bits_in<T>(w[c]), ksk_bits_in<T>(w[c + 1])};
    }
    if (ntt_tail_local<L>()) ntt_wave_sync(); else __syncthreads();
    {   // a leaves in the tail layout: 16 B per lane, a half-wave covers 512 contiguous bytes.  The thread reads ITS OWN words back in the last step.
        T ab[16];
        lds_get_tail<T, L>(ab, s, tid);
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            ksk_u64x2 va;
            va.x = ksk_word(ksk_bits_out(ab[r]), f64); va.y = ksk_word(ksk_bits_out(ab[r + 1]), f64);
            *reinterpret_cast<NTT_GLOBAL ksk_u64x2 *>(oa + tail_index<L>(tid, r)) = va;
        }
    }
    __syncthreads();                                                         // everybody has taken its words out of the image
    T v[16];                                                                 // NTT(noise) mod q_j at tail_index(tid, r), lazy
    {
        const int8_t *ee = noise + (size_t)ge * n;
#pragma unroll
        for (int r = 0; r < 16; r++) { const int32_t x = ee[pass_index<L, SA, 0>(tid, r)]; v[r] = A.load(x >= 0 ? (uint64_t)x : qm.q - (uint64_t)(-x)); }
        ntt_forward_regs<AR, L>(v, s, A.fw, A.m, tid);
    }
    uint32_t tl = tid;
    asm volatile("" : "+v"(tl));                                             // the addresses of the last step are formed anew (carried across the transform they spill)
    const uint64_t f = fac[e].f[j];
    const uint64_t *ss = sk + (size_t)j * n;                                 // (kernel arguments: global, not flat, loads)
    const uint16_t *pp = perm + (size_t)g * n;
    if constexpr (std::is_same<T, double>::value) {
        // FP64 policies: the lazy transform output (|x| <= 6.3 q) takes part as it is - |-(a s + e^) + f sigma(s)| <= (2.1 + 6.3 + 2.1) q < 16 q, ONE canonicalisation
        const double fd = A.load(f);
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            const uint32_t pos = tail_index<L>(tl, r);
            const ksk_u64x2 va = *reinterpret_cast<const NTT_GLOBAL ksk_u64x2 *>(oa + pos);
            const double a0 = f64 ? ksk_bits_in<double>(va.x) : A.load(va.x), a1 = f64 ? ksk_bits_in<double>(va.y) : A.load(va.y);
            const ulonglong2 y = *reinterpret_cast<const ulonglong2 *>(ss + pos);
            double b0 = -__dadd_rn(AR::mulmod(a0, A.load(y.x), A.m), v[r]), b1 = -__dadd_rn(AR::mulmod(a1, A.load(y.y), A.m), v[r + 1]);
            if (f) {                                                         // (uniform: the blocks of limb l of entry (l, d))
                const ushort2 ix = *reinterpret_cast<const ushort2 *>(pp + pos);
                b0 = __dadd_rn(b0, AR::mulmod(A.load(ss[ix.x]), fd, A.m)); b1 = __dadd_rn(b1, AR::mulmod(A.load(ss[ix.y]), fd, A.m));
            }
            ksk_u64x2 vb;
            vb.x = ksk_word(A.canon(b0), f64); vb.y = ksk_word(A.canon(b1), f64);
            *reinterpret_cast<NTT_GLOBAL ksk_u64x2 *>(ob + pos) = vb;
        }
    } else {
        // integer policy: e^ waits in b's place (canonical; the thread reads its own words back), so that the Barrett products below have the registers to themselves
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            ksk_u64x2 ve;
            ve.x = A.canon(v[r]); ve.y = A.canon(v[r + 1]);
            *reinterpret_cast<NTT_GLOBAL ksk_u64x2 *>(ob + tail_index<L>(tl, r)) = ve;
        }
#pragma unroll 1
        for (int r = 0; r < 16; r += 2) {
            const uint32_t pos = tail_index<L>(tl, r);
            const ksk_u64x2 va = *reinterpret_cast<const NTT_GLOBAL ksk_u64x2 *>(oa + pos), ve = *reinterpret_cast<const NTT_GLOBAL ksk_u64x2 *>(ob + pos);
            const ulonglong2 y = *reinterpret_cast<const ulonglong2 *>(ss + pos);
            uint64_t b0 = negmod(addmod(mulmod(va.x, y.x, qm), ve.x, qm.q), qm.q), b1 = negmod(addmod(mulmod(va.y, y.y, qm), ve.y, qm.q), qm.q);
            if (f) {
                const ushort2 ix = *reinterpret_cast<const ushort2 *>(pp + pos);
                b0 = addmod(b0, mulmod(ss[ix.x], f, qm), qm.q); b1 = addmod(b1, mulmod(ss[ix.y], f, qm), qm.q);
            }
            ksk_u64x2 vb;
            vb.x = b0; vb.y = b1;
            *reinterpret_cast<NTT_GLOBAL ksk_u64x2 *>(ob + pos) = vb;
        }
    }
}
