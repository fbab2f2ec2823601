// Request path on the device (cn_split_encode / cn_split_encrypt): EncryptedSealBfvVector.SplitBigNumbers (EncryptedSealBfvVector.cs:352-365) and the value
// mapping of VectorToPlaintext (AtomicSealBfvVector.cs:1114-1232) for P plaintext-prime contexts at once - scaling, rounding, the range test, the residue of
// every prime, and the scatter into BatchEncoder's slot order.
//
// Per value, in registers:
//   f64   r = rint(x * scale): ONE IEEE double multiply, then round to nearest even; out of range when r is NaN, infinite or |r| >= 2^62; w = (int64) r
//   i64   w is the element (every int64, INT64_MIN included)
//   v_i   w mod t_i in [0, t_i): a 64-bit Barrett reduction of |w| (cnj_bred128 of cn_k_join.hip.h with a zero high word), t_i - r for a negative w with r != 0.
//         |w| is taken in unsigned arithmetic: 0 - (uint64) w is 2^63 for INT64_MIN, and no signed negation happens.
// The per-value functions are plain C++ (__host__ __device__ under hipcc): tests/cpp/crt_split_model.cpp runs them on the CPU against Python's integers.
// The kernel maps one thread to one (plaintext, position) pair in tiles of CSP_TC plaintexts x CSP_TS slots; an image-major input (stride_ct = 1) is read with
// the lanes along the plaintexts and turned through one LDS tile, so either layout is read in contiguous segments.
#pragma once
#include "cn_k_join.hip.h"

#define CSP_I64 1u             // = CN_SPLIT_I64 (include/cnhip.h)
#define CSP_COEFF0 2u          // = CN_SPLIT_COEFF0
#define CSP_TILED 0x100u       // launcher's own: turn the input through the LDS tile (the lanes read along stride_ct)

// the constants of one launch: the moduli with their Barrett words, the first plaintext row of every context
struct SplitTab {
    DMod t[CNJ_MAXP];
    uint64_t *dst[CNJ_MAXP];
};

// ---------------------------------------------------------------- per-value arithmetic (host and device)
// the 64 bits of an input element -> w; false when the f64 kind's value does not fit (NaN, infinite, |rint(x scale)| >= 2^62)
CNJ_HD bool csp_convert(uint64_t bits, uint32_t flags, double scale, int64_t &w) {
    if (flags & CSP_I64) { w = (int64_t)bits; return true; }
    double x;
    __builtin_memcpy(&x, &bits, 8);
    const double r = __builtin_rint(x * scale);
    const bool ok = __builtin_fabs(r) < 4611686018427387904.0;          // false for NaN
    w = ok ? (int64_t)r : 0;
    return ok;
}
// w mod t as the representative in [0, t)
CNJ_HD uint64_t csp_residue(int64_t w, const DMod &m) {
    const bool neg = w < 0;
    const uint64_t mag = neg ? 0ull - (uint64_t)w : (uint64_t)w;
    const uint64_t r = cnj_bred128(mag, 0, m);
    return (neg && r) ? m.q - r : r;
}
// Barrett words of a modulus 2 <= t < 2^62 (floor(2^128 / t), as cnj_build_tab)
static inline DMod csp_dmod(uint64_t t) {
    const cnj_u128 one = (cnj_u128)1 << 64, q1 = one / t, rem = one % t;
    DMod m; m.q = t; m.r1 = (uint64_t)q1; m.r0 = (uint64_t)((rem << 64) / t);
    return m;
}

// ---------------------------------------------------------------- kernel
#if defined(__HIPCC__)
#define CSP_THREADS 256
#define CSP_TS 64              // slots of a tile: one wave
#define CSP_TC 16              // plaintexts of a tile: 128 contiguous bytes of an image-major row

// Grid (ceil(n / CSP_TS), ceil(count / CSP_TC)).  Thread (lane tx, wave ty) handles position blockIdx.x CSP_TS + tx of the plaintexts blockIdx.y CSP_TC + ty + 4 r.
// values: element (c, s) at values[c stride_ct + s stride_slot] for c < count, s < nvalues (nothing else is read).  Dense: slot s goes to position index_map[s]
// of row c of every context, 0 for s >= nvalues; CSP_COEFF0: position s itself (nvalues = 1: the constant row).  nz [P][nz_stride]: word [i][c] OR-ed with 1 where plaintext c
// of context i has a non-zero coefficient; bad: OR-ed with 1 when a value does not fit.  Both are zeroed by the caller.
template <int P>
__global__ void __launch_bounds__(CSP_THREADS) k_crt_split(const uint64_t *__restrict__ values_, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues,
                                                           uint32_t flags, double scale, const SplitTab tab, const uint32_t *__restrict__ index_map_, uint32_t n,
                                                           uint32_t *__restrict__ nz_, uint32_t nz_stride, uint32_t *__restrict__ bad_) {
    __shared__ uint64_t tile[CSP_TS][CSP_TC + 1];
    const CNJ_GLOBAL uint64_t *values = (const CNJ_GLOBAL uint64_t *)values_;
    const uint32_t tx = threadIdx.x & (CSP_TS - 1), ty = threadIdx.x / CSP_TS;
    const uint32_t s0 = blockIdx.x * CSP_TS, c0 = blockIdx.y * CSP_TC, s = s0 + tx;
    const bool tiled = (flags & CSP_TILED) != 0;                       // (kernel-uniform)
    if (tiled) {
        const uint32_t lc = threadIdx.x & (CSP_TC - 1), ls = threadIdx.x / CSP_TC, c = c0 + lc;
#pragma unroll
        for (uint32_t r = 0; r < CSP_TS * CSP_TC / CSP_THREADS; r++) {
            const uint32_t sl = ls + r * (CSP_THREADS / CSP_TC), sg = s0 + sl;
            if (c < count && sg < nvalues) tile[sl][lc] = values[(int64_t)c * stride_ct + (int64_t)sg * stride_slot];
        }
        __syncthreads();
    }
    const uint32_t pos = (s < n && !(flags & CSP_COEFF0)) ? ((const CNJ_GLOBAL uint32_t *)index_map_)[s] : s;
    bool any_bad = false;
#pragma unroll
    for (uint32_t r = 0; r < CSP_TC * CSP_TS / CSP_THREADS; r++) {
        const uint32_t cl = ty + r * (CSP_THREADS / CSP_TS), c = c0 + cl;
        if (c >= count) break;                                         // (wave-uniform: a wave is one plaintext row)
        const bool have = s < nvalues;
        uint64_t bits = 0;
        if (have) bits = tiled ? tile[tx][cl] : values[(int64_t)c * stride_ct + (int64_t)s * stride_slot];
        int64_t w;
        const bool ok = csp_convert(bits, have ? flags : CSP_I64, scale, w);
        any_bad |= !ok;
#pragma unroll
        for (int i = 0; i < P; i++) {
            const uint64_t v = csp_residue(w, tab.t[i]);
            if (s < n) ((CNJ_GLOBAL uint64_t *)tab.dst[i])[(size_t)c * n + pos] = v;
            if (__ballot(v != 0) && tx == 0) atomicOr(nz_ + (size_t)i * nz_stride + c, 1u);
        }
    }
    if (__ballot(any_bad) && tx == 0) atomicOr(bad_, 1u);
}
#endif
