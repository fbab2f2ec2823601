// Reply path on the device (cn_decrypt_join): CRT join of the decoded plaintexts of P plaintext-prime contexts - EncryptedSealBfvVector.JoinSplitNumbers
// (EncryptedSealBfvVector.cs:381-411) - centring, conversion to a double, division by the scale, and the arg max over the ciphertexts of a slot.
//
// Per value, in registers (W = cn_join_words <= 4 words, M = t_0 .. t_{P-1} < 2^255):
//   Garner   x = a_0 + a_1 t_0 + a_2 t_0 t_1 + ..,  a_j = [(v_j - x_j) (t_0 .. t_{j-1})^-1]_{t_j} with x_j = the partial sum so far reduced mod t_j (a Horner pass over
//            its W words, one Barrett reduction per word); the digit times the W-word product t_0 .. t_{j-1} is added with 64 x 64 -> 128-bit multiply-adds.
//            x is the unique integer in [0, M) with x == v_j (mod t_j): every a_j < t_j, so the mixed-radix sum stays below M.
//   sign     CN_JOIN_SIGNED: x - M replaces x when 2x > M (2x < 2^(64 W): W counts the bit above bit_length(M)); the W words are two's complement from then on.
//   double   round-to-nearest-even of the exact integer: the top 64 bits of |x| and a sticky bit for everything below them decide the 53-bit mantissa - what
//            Python's float(int) computes; the quotient by the scale is the IEEE division.
// The per-value functions are plain C++ (__host__ __device__ under hipcc): tests/cpp/crt_join_model.cpp runs them on the CPU against Python's integers.
// The kernels read the P residues of a value straight out of the transformed plaintexts [P][count][N] through the BatchEncoder index map (no gather pass), take the
// call's constants (JoinTab, a few hundred bytes) through scalar loads and use neither LDS nor scratch.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "cn_internal.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CNJ_HD __host__ __device__ inline
#else
#define CNJ_HD inline
#endif

#define CNJ_MAXP 8
#define CNJ_MAXW 4
#define CNJ_SIGNED 1u          // = CN_JOIN_SIGNED (include/cnhip.h)
#define CNJ_COEFF0 2u          // = CN_JOIN_COEFF0

typedef unsigned __int128 cnj_u128;

// the constants of one call: moduli with their Barrett words, Garner's inverses and partial products, M, the scale
struct JoinTab {
    uint32_t P, W, flags, pad;
    DMod t[CNJ_MAXP];
    uint64_t inv[CNJ_MAXP];                    // inv[j] = (t_0 .. t_{j-1})^-1 mod t_j (inv[0] unused)
    uint64_t prod[CNJ_MAXP][CNJ_MAXW];         // prod[j] = t_0 .. t_{j-1}, little-endian words (prod[0] = 1)
    uint64_t M[CNJ_MAXW];
    double scale;
};

// ---------------------------------------------------------------- per-value arithmetic (host and device)
CNJ_HD uint64_t cnj_mulhi(uint64_t a, uint64_t b) { return (uint64_t)(((cnj_u128)a * b) >> 64); }
// Barrett reduction of x = x1:x0 < 2^128 (the mulmod of cn_dev_common.hip.h, SEAL's barrett_reduce_128) with a second conditional subtraction: the quotient
// estimate is short by at most 2, and 3 t < 2^64 for every modulus below 2^62
CNJ_HD uint64_t cnj_bred128(uint64_t x0, uint64_t x1, const DMod &m) {
    uint64_t carry = cnj_mulhi(x0, m.r0);
    const uint64_t t2lo = x0 * m.r1, t2hi = cnj_mulhi(x0, m.r1);
    const uint64_t tmp1 = t2lo + carry, tmp3 = t2hi + (uint64_t)(tmp1 < carry);
    const uint64_t t3lo = x1 * m.r0, t3hi = cnj_mulhi(x1, m.r0);
    const uint64_t s = tmp1 + t3lo;
    carry = t3hi + (uint64_t)(s < tmp1);
    const uint64_t qhat = x1 * m.r1 + tmp3 + carry;
    uint64_t r = x0 - qhat * m.q;
    r = r >= m.q ? r - m.q : r;
    return r >= m.q ? r - m.q : r;
}
CNJ_HD uint64_t cnj_mulmod(uint64_t a, uint64_t b, const DMod &m) { return cnj_bred128(a * b, cnj_mulhi(a, b), m); }
// x (W words) mod t: Horner from the top word, r 2^64 + x[w] < 2^126
template <int W> CNJ_HD uint64_t cnj_reduce(const uint64_t (&x)[W], const DMod &m) {
    uint64_t r = 0;
#pragma unroll
    for (int w = W - 1; w >= 0; w--) r = cnj_bred128(x[w], r, m);
    return r;
}
// Garner's mixed-radix recombination: v[j] < t_j -> x in [0, M), W words
template <int P, int W> CNJ_HD void cnj_garner(const uint64_t (&v)[P], const JoinTab &T, uint64_t (&x)[W]) {
    x[0] = v[0];
#pragma unroll
    for (int w = 1; w < W; w++) x[w] = 0;
#pragma unroll
    for (int j = 1; j < P; j++) {
        const DMod m = T.t[j];
        const uint64_t r = cnj_reduce<W>(x, m);
        const uint64_t d = v[j] >= r ? v[j] - r : v[j] + m.q - r;
        const uint64_t a = cnj_mulmod(d, T.inv[j], m);
        uint64_t carry = 0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            const cnj_u128 p = (cnj_u128)a * T.prod[j][w] + x[w] + carry;
            x[w] = (uint64_t)p; carry = (uint64_t)(p >> 64);
        }
    }
}
// the sign step: x in [0, M) -> x - M (two's complement) when 2x > M
template <int W> CNJ_HD void cnj_centre(uint64_t (&x)[W], const uint64_t (&M)[CNJ_MAXW]) {
    bool gt = false;                               // 2x > M: the highest word in which they differ decides
    uint64_t low = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        const uint64_t d = (x[w] << 1) | low;
        low = x[w] >> 63;
        gt = d > M[w] || (d == M[w] && gt);
    }
    if (!gt) return;
    uint64_t bw = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        const uint64_t d = x[w] - M[w];
        const uint64_t b1 = x[w] < M[w];
        x[w] = d - bw; bw = b1 | (uint64_t)(d < bw);
    }
}
// two's-complement W words -> the nearest double, ties to even (|x| < 2^255: no overflow, no subnormals)
template <int W> CNJ_HD double cnj_to_double(const uint64_t (&x)[W]) {
    const bool neg = (x[W - 1] >> 63) != 0;
    uint64_t mag[W], cy = 1;
#pragma unroll
    for (int w = 0; w < W; w++) {
        const uint64_t f = neg ? ~x[w] : x[w];
        mag[w] = neg ? f + cy : f;
        cy = neg ? (uint64_t)(mag[w] < cy) : 0;
    }
    // top: the highest non-zero word (index h); below: the word under it; rest: OR of every word under that (static indices only: registers)
    uint64_t top = 0, below = 0, rest = 0, pre = 0; int h = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
        const bool nz = mag[w] != 0;
        const uint64_t under = w > 0 ? mag[w - 1] : 0;
        top = nz ? mag[w] : top; below = nz ? under : below; rest = nz ? pre : rest; h = nz ? w : h;
        pre |= under;
    }
    if (top == 0) return 0.0;
    const int lz = __builtin_clzll(top);
    const uint64_t top64 = lz ? (top << lz) | (below >> (64 - lz)) : top;          // the 64 bits from the leading one down
    const uint64_t sticky = (lz ? below << lz : below) | rest;                      // anything below them
    const int e = 64 * h + 63 - lz;                                                 // 2^e <= |x| < 2^(e + 1)
    uint64_t mant = top64 >> 11;                                                    // 53 bits, bit 52 set
    const uint64_t rem = top64 & 0x7ffull;
    mant += (uint64_t)(rem > 0x400ull || (rem == 0x400ull && (sticky != 0 || (mant & 1))));
    // a mantissa that rounded up to 2^53 carries into the exponent field
    const uint64_t bits = ((uint64_t)neg << 63) | ((((uint64_t)(e + 1023)) << 52) + (mant - (1ull << 52)));
    double d;
    __builtin_memcpy(&d, &bits, 8);
    return d;
}
// one joined value: residues -> words (two's complement under the signed flag) and the double
template <int P, int W> CNJ_HD double cnj_join_value(const uint64_t (&v)[P], const JoinTab &T, uint64_t (&x)[W]) {
    cnj_garner<P, W>(v, T, x);
    if (T.flags & CNJ_SIGNED) cnj_centre<W>(x, T.M);
    return cnj_to_double<W>(x) / T.scale;
}
// a > b as two's-complement W-word integers
template <int W> CNJ_HD bool cnj_greater(const uint64_t (&a)[W], const uint64_t (&b)[W]) {
    bool gt = false;
#pragma unroll
    for (int w = 0; w < W - 1; w++) gt = a[w] > b[w] || (a[w] == b[w] && gt);
    const int64_t ta = (int64_t)a[W - 1], tb = (int64_t)b[W - 1];
    return ta > tb || (ta == tb && gt);
}

// ---------------------------------------------------------------- the constants of a call (host)
static inline uint64_t cnj_host_powmod(uint64_t b, uint64_t e, uint64_t q) {
    cnj_u128 r = 1, x = b % q;
    for (; e; e >>= 1) { if (e & 1) r = r * x % q; x = x * x % q; }
    return (uint64_t)r;
}
// T for the moduli t[0 .. P): 0, or -1 when P is out of range, two moduli are equal, a modulus is below 2 or not below 2^62, or M >= 2^255.
// The moduli must be prime (the inverses are Fermat powers); the caller checks that.
static inline int cnj_build_tab(const uint64_t *t, uint32_t P, uint32_t flags, double scale, JoinTab *T) {
    if (P < 1 || P > CNJ_MAXP) return -1;
    *T = JoinTab();
    T->P = P; T->flags = flags; T->scale = scale;
    uint64_t acc[CNJ_MAXW] = {1, 0, 0, 0};
    for (uint32_t j = 0; j < P; j++) {
        if (t[j] < 2 || (t[j] >> 62)) return -1;
        for (uint32_t i = 0; i < j; i++) if (t[i] == t[j]) return -1;
        const cnj_u128 one = (cnj_u128)1 << 64, q1 = one / t[j], rem = one % t[j];
        T->t[j].q = t[j]; T->t[j].r1 = (uint64_t)q1; T->t[j].r0 = (uint64_t)((rem << 64) / t[j]);       // floor(2^128 / t_j)
        for (int w = 0; w < CNJ_MAXW; w++) T->prod[j][w] = acc[w];
        if (j) {
            cnj_u128 r = 0;
            for (int w = CNJ_MAXW - 1; w >= 0; w--) r = ((r << 64) | acc[w]) % t[j];
            T->inv[j] = cnj_host_powmod((uint64_t)r, t[j] - 2, t[j]);
        }
        uint64_t carry = 0;
        for (int w = 0; w < CNJ_MAXW; w++) { const cnj_u128 p = (cnj_u128)acc[w] * t[j] + carry; acc[w] = (uint64_t)p; carry = (uint64_t)(p >> 64); }
        if (carry || (acc[CNJ_MAXW - 1] >> 63)) return -1;
    }
    int bits = 0;
    for (int w = 0; w < CNJ_MAXW; w++) { T->M[w] = acc[w]; if (acc[w]) bits = 64 * w + 64 - __builtin_clzll(acc[w]); }
    T->W = (uint32_t)((bits + 1 + 63) / 64);
    return 0;
}

// ---------------------------------------------------------------- kernels
#if defined(__HIPCC__)
#define CNJ_GLOBAL __attribute__((address_space(1)))
#define CNJ_THREADS 256

template <int W> __device__ __forceinline__ void cnj_store_words(CNJ_GLOBAL uint64_t *dst, const uint64_t (&x)[W]) {
    if constexpr (W % 2 == 0) {                                         // 16-byte stores (the rows are 16 W bytes apart from a 256-byte aligned base)
        typedef uint64_t v2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int w = 0; w < W; w += 2) { v2 p; p.x = x[w]; p.y = x[w + 1]; *(CNJ_GLOBAL v2 *)(dst + w) = p; }
    } else {
#pragma unroll
        for (int w = 0; w < W; w++) dst[w] = x[w];
    }
}
template <int W> __device__ __forceinline__ void cnj_load_words(const CNJ_GLOBAL uint64_t *src, uint64_t (&x)[W]) {
    if constexpr (W % 2 == 0) {
        typedef uint64_t v2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int w = 0; w < W; w += 2) { const v2 p = *(const CNJ_GLOBAL v2 *)(src + w); x[w] = p.x; x[w + 1] = p.y; }
    } else {
#pragma unroll
        for (int w = 0; w < W; w++) x[w] = src[w];
    }
}
// One thread per (ciphertext c, slot s), c * nslots + s < total = count * nslots.  plain: the transformed plaintexts [P][count][N] (coefficient form under
// CN_JOIN_COEFF0); index_map: slot -> position (entries < N; not read under CN_JOIN_COEFF0, where nslots = 1 and position 0 is taken);
// values [count][nslots] doubles or null; words [count][nslots][W] or null.
template <int P, int W>
__global__ void __launch_bounds__(CNJ_THREADS) k_crt_join(const uint64_t *__restrict__ plain_, const uint32_t *__restrict__ index_map_, const JoinTab *__restrict__ tab_,
                                                          double *__restrict__ values_, uint64_t *__restrict__ words_, uint32_t n, uint32_t count, uint32_t nslots) {
    const uint64_t total = (uint64_t)count * nslots, id = (uint64_t)blockIdx.x * CNJ_THREADS + threadIdx.x;
    if (id >= total) return;
    const JoinTab &T = *tab_;                                          // kernel-uniform, read-only: scalar loads
    const uint32_t c = (uint32_t)(id / nslots), s = (uint32_t)(id - (uint64_t)c * nslots);
    const uint32_t pos = (T.flags & CNJ_COEFF0) ? 0u : ((const CNJ_GLOBAL uint32_t *)index_map_)[s];
    const CNJ_GLOBAL uint64_t *plain = (const CNJ_GLOBAL uint64_t *)plain_ + (size_t)c * n + pos;
    uint64_t v[P], x[W];
#pragma unroll
    for (int p = 0; p < P; p++) v[p] = plain[(size_t)p * count * n];
    const double d = cnj_join_value<P, W>(v, T, x);
    if (values_) ((CNJ_GLOBAL double *)values_)[id] = d;
    if (words_) cnj_store_words<W>((CNJ_GLOBAL uint64_t *)words_ + id * W, x);
}
// One thread per slot: the lowest c whose integer words[c][s] is largest (signed W-word compare)
template <int W>
__global__ void __launch_bounds__(CNJ_THREADS) k_join_argmax(const uint64_t *__restrict__ words_, int32_t *__restrict__ argmax_, uint32_t count, uint32_t nslots) {
    const uint32_t s = blockIdx.x * CNJ_THREADS + threadIdx.x;
    if (s >= nslots) return;
    const CNJ_GLOBAL uint64_t *words = (const CNJ_GLOBAL uint64_t *)words_;
    uint64_t best[W];
    cnj_load_words<W>(words + (size_t)s * W, best);
    int32_t arg = 0;
    for (uint32_t c = 1; c < count; c++) {
        uint64_t x[W];
        cnj_load_words<W>(words + ((size_t)c * nslots + s) * W, x);
        const bool gt = cnj_greater<W>(x, best);
#pragma unroll
        for (int w = 0; w < W; w++) best[w] = gt ? x[w] : best[w];
        arg = gt ? (int32_t)c : arg;
    }
    ((CNJ_GLOBAL int32_t *)argmax_)[s] = arg;
}
#endif
