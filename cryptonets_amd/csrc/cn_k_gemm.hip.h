// HOT LOOP A: scalar GEMM kernels (AtomicSealBfvVector.cs:434-521).  Included by cn_l_gemm.hip only.
#pragma once
#include "cn_dev_common.hip.h"

// ------------------------------------------------------------------ HOT LOOP A: scalar GEMM
// Workgroup -> (coefficient chunk, limb, output tile mt, group g).  The mtiles output tiles of one (chunk, limb, g) read the SAME
// input elements; workgroup ids are dealt round-robin to the 8 XCDs (each with its own L2), so the tiles take ids b, b+8, b+16, ...
// - same XCD, adjacent in time: the K input elements are fetched from HBM once and re-read from that XCD's L2 (dense 845->100:
// 5 tiles; without this every tile streamed the 528 MB of input ciphertexts again).
// order 1 (slice-major): a SLICE = (limb, chunk of 256 coefficients) of every ciphertext is 2 KiB per ciphertext - all 784 inputs of the CryptoNets
// convolution are 1.5 MiB, which an XCD's 4 MiB L2 holds.  XCD x (blocks b = x mod 8) walks through ALL groups of slice x, then of slice x + 8, ...:
// every input slice is fetched once per launch, whatever the overlap of the gather lists (5x5 windows at stride 2 share each pixel 6.25 times; in
// group-major order only the horizontal overlap survived in L2: FETCH_SIZE 2.3 x the input bytes, profiles/r02_pmc_square_gemm.txt).
// order 1 is launched as a 2-D grid (8 * mtiles * G, slices / 8) - x fastest, so workgroup (x, y) still lands on XCD x mod 8: the coordinates of the
// convolution's workgroups (mtiles = 1; chunks is a power of two) come out of shifts and masks.  (As one linear id they took three divisions by run-time
// values - ~100 vector instructions of the ~860 a convolution workgroup issues, on a kernel that is bound by its issue slots.)
DEV void gemm_block_coords(uint32_t bx, uint32_t by, uint32_t chunks, uint32_t limbs, uint32_t mtiles, uint32_t G, uint32_t &chunk, uint32_t &limb, uint32_t &mt, uint32_t &g,
                           uint32_t order = 0) {
    if (order == 1) {
        const uint32_t x = bx & 7, r = bx >> 3;
        if (mtiles == 1) { mt = 0; g = r; } else { mt = r % mtiles; g = r / mtiles; }
        const uint32_t sl = by * 8 + x;
        chunk = sl & (chunks - 1); limb = sl >> (__ffs((int)chunks) - 1);
        return;
    }
    const uint32_t b = bx, D = chunks * limbs * G;
    uint32_t d;
    if ((D & 7) == 0) { const uint32_t r = b >> 3; mt = r % mtiles; d = (r / mtiles) * 8 + (b & 7); }
    else { d = b % D; mt = b / D; }
    chunk = d % chunks; limb = (d / chunks) % limbs; g = d / (chunks * limbs);
}
// Group g gathers K input ciphertexts idx[g][:] once and produces M outputs (register tile MT):
//   out[out_idx[g][m]] = sum_k Wl[j][g][m][k] * in[idx[g][k]]  (+ scaled bias)   per limb j, coefficient i.
// Products accumulate lazily in 128 bits; one Barrett reduction per `lazy` terms.
// ABS: the gather / output / bias tables hold DEVICE ADDRESSES (u64, 0 = padded tap / no output / no bias) instead of indices relative
// to `in` / `out` / `bias` - the form the deferred per-ciphertext calls arrive in, where every ciphertext is its own array.
// A device address read from a table is a GLOBAL address: said so, the access is global_load / global_store.  As a generic pointer it is
// flat_load - counted on lgkmcnt as well, so every wait for a scalar weight load also drained the input loads in flight (the address-table
// kernels of the deferred calls ran 30-60 % behind their index-table twins).
DEV const NTT_GLOBAL uint64_t *gmem(uint64_t a) { return (const NTT_GLOBAL uint64_t *)a; }
DEV NTT_GLOBAL uint64_t *gmem_w(uint64_t a) { return (NTT_GLOBAL uint64_t *)a; }
// Index units of the table-driven (non-ABS) kernels, in words: input / output index x unit = word offset from `in` / `out`, bias index x unit from `bias`.  0 = the defaults (one
// ciphertext / one plaintext per index: the arrays of a plan).  The deferred per-ciphertext calls - every ciphertext its own array - hand in 32-bit offsets in units of 32 words
// (256 B: the allocation granule) from the lowest address of their flush group (round 6): the same index-table kernels as a plan instead of 64-bit address tables.
struct GemmUnits { uint32_t in, out, bias; };
template <bool ABS> struct GemmTab { typedef int32_t T; };
template <> struct GemmTab<true> { typedef uint64_t T; };
template <int MT, bool ABS = false>
__global__ void __launch_bounds__(256) k_scalar_gemm(const uint64_t *__restrict__ in, const void *__restrict__ idx_, const uint64_t *__restrict__ Wl,
                                                     const void *__restrict__ out_idx_, const uint64_t *__restrict__ bias, const void *__restrict__ bias_idx_,
                                                     uint64_t *__restrict__ out, const DevConsts *__restrict__ C, uint32_t chunks, uint32_t G, uint32_t M,
                                                     uint32_t K, uint32_t mtiles, uint32_t lazy, uint32_t Kp, uint32_t obase, uint32_t polys, uint32_t order, GemmUnits U) {
    typedef typename GemmTab<ABS>::T TT;
    const TT *idx = (const TT *)idx_, *out_idx = (const TT *)out_idx_, *bias_idx = (const TT *)bias_idx_;
    const uint32_t n = C->n, k = C->k, limbs = polys * k;       // polys = ciphertext size: 2, or 3 for unrelinearized products (Evaluator::multiply_plain / add accept both)
    uint32_t chunk, limb, mt, g;
    gemm_block_coords(blockIdx.x, blockIdx.y, chunks, limbs, mtiles, G, chunk, limb, mt, g, order);
    const uint32_t j = limb % k, i = chunk * blockDim.x + threadIdx.x;
    const size_t ctw = (size_t)limbs * n, e = (size_t)limb * n + i;
    const size_t iu = U.in ? U.in : ctw, ou = U.out ? U.out : ctw, bu = U.bias ? U.bias : n;
    const DMod qm = C->q[j];
    u128 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m] = 0;
    const TT *gi = idx + (size_t)g * Kp;                                                 // row pitch Kp: 16 B aligned, -1 (ABS: 0) beyond K
    const uint64_t *gw = Wl + (((size_t)j * G + g) * mtiles + mt) * (size_t)K * MT;      // [kk][m]: the MT weights of a term are contiguous
    const uint32_t mcnt = min((uint32_t)MT, M - mt * MT);
    for (uint32_t k0 = 0; k0 < K; k0 += lazy) {            // reduction between blocks of `lazy` terms (see k_scalar_gemm_f64)
        const uint32_t k1 = min(K, k0 + lazy);
        for (uint32_t kk = k0; kk < k1; kk++) {
            uint64_t x;
            if constexpr (ABS) { const uint64_t a = gi[kk]; if (!a) continue; x = gmem(a)[e]; }
            else { const int32_t id = gi[kk]; if (id < 0) continue; x = in[(size_t)id * iu + e]; }
#pragma unroll
            for (int m = 0; m < MT; m++) acc[m] += (u128)x * gw[(size_t)kk * MT + m];       // zero-padded beyond mcnt
        }
        if (k1 < K) {
#pragma unroll
            for (int m = 0; m < MT; m++) acc[m] = bred128(acc[m], qm);
        }
    }
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const uint32_t o = g * M + mt * MT + m;
        // bias: a PoolLayer bias is the constant polynomial (BatchEncoder of a constant vector) - every coefficient but one is zero and
        // scales to zero: the 128-bit multiply + Barrett of scale_plain is skipped there (wave-uniformly almost everywhere)
        if constexpr (ABS) {
            if ((uint32_t)m < mcnt && out_idx[o]) {
                uint64_t r = bred128(acc[m], qm);
                if (bias_idx && bias_idx[o] && limb < k) { const uint64_t bv = gmem(bias_idx[o])[i]; if (bv) r = addmod(r, scale_plain(C, bv, j), qm.q); }
                gmem_w(out_idx[o])[e] = r;
            }
        } else if ((uint32_t)m < mcnt && out_idx[o] >= 0) {                     // -1: padding member of a smaller group
            uint64_t r = bred128(acc[m], qm);
            if (bias && limb < k) { const uint64_t bv = bias[(size_t)bias_idx[o] * bu + i]; if (bv) r = addmod(r, scale_plain(C, bv, j), qm.q); }
            out[(size_t)(obase + (uint32_t)out_idx[o]) * ou + e] = r;
        }
    }
}

// FP64 variant of the scalar GEMM for SMALL SIGNED weights (|w| < 2^20 after centring mod t - every PoolLayer weight
// round(w*scale) is): the input residue x < 2^(NL*LW) is split into NL limbs of LW bits, each limb times the weight is an
// exact double (< 2^(LW+20)), and up to 2^(52-LW-20) such terms accumulate exactly in one v_fma_f64 per limb - two half-rate
// FMAs per MAC instead of a 64x64->128-bit integer multiply-add (~12 half-rate instructions).  The signed weight is the same
// for every limb j, so the table is k times smaller as well.  Folded back with one 128-bit Barrett reduction per `lazy` terms.
// Weights through the vector memory path (MT = 20): a wave-uniform weight as a scalar operand means s_load, and scalar loads return
// out of order - the only possible wait is lgkmcnt(0), and ~70 free SGPRs hold less than two terms of 20 weights, so every other term
// exposed an L2 round trip (the 135 KB weight tile of a block never fits the 16 KB scalar cache).  Instead lanes 0..15 of every
// row of 16 load 16 consecutive table entries (5 coalesced 8 B loads per 4 terms, in-order vmcnt, requested two steps ahead) and
// the FMA takes its weight through DPP: v_fmac_f64_dpp ... row_newbcast:i reads src0 from lane i of the own row - the one DPP
// control gfx90a+ allows on FP64 instructions, at no extra issue slot.  (Through __builtin_amdgcn_update_dpp the compiler emits a
// separate v_mov_b64_dpp per weight, +50 % FP64-rate instructions - hence inline assembly; "s_nop 1" covers the 2 wait states a
// DPP read needs after a VALU write of its source, in case the register allocator put a copy right in front.)
#ifndef GEMM_DPP_W
#define GEMM_DPP_W 1
#endif
// limb l of a canonical residue (below 2^(NL LW)) as an exact double; the top limb needs no mask.  NL = 1: the WHOLE word (v | 2^52's exponent, minus 2^52: two
// instructions) - the launcher picks that form when every row's sum of |weights| times q_max stays below 2^53 (gemm_one_limb): one FMA per MAC and nothing to fold
template <int NL, int LW> DEV double gemm_limb(uint64_t x, int l) {
    if constexpr (NL == 1) return BzF::from_u64(x & 0x000FFFFFFFFFFFFFull);   // (masked: a padded tap multiplies whatever word it reads by the weight 0 - an unwritten array
                                                                               // may hold bits 52..62, which would land in the exponent: 0 x NaN poisons the sum; one v_and_b32 per term)
    else return (double)(uint32_t)(l == NL - 1 ? x >> (l * LW) : (x >> (l * LW)) & ((1ull << LW) - 1));
}
template <int LANE> DEV void fmac_bcast(double &acc, double w, double x) {
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(w), "v"(x), "n"(LANE));
}
DEV void fmac_bcast_lane(int lane, double &acc, double w, double x) {          // `lane` is a constant after unrolling
    switch (lane) {
    case 0: fmac_bcast<0>(acc, w, x); break;   case 1: fmac_bcast<1>(acc, w, x); break;   case 2: fmac_bcast<2>(acc, w, x); break;   case 3: fmac_bcast<3>(acc, w, x); break;
    case 4: fmac_bcast<4>(acc, w, x); break;   case 5: fmac_bcast<5>(acc, w, x); break;   case 6: fmac_bcast<6>(acc, w, x); break;   case 7: fmac_bcast<7>(acc, w, x); break;
    case 8: fmac_bcast<8>(acc, w, x); break;   case 9: fmac_bcast<9>(acc, w, x); break;   case 10: fmac_bcast<10>(acc, w, x); break; case 11: fmac_bcast<11>(acc, w, x); break;
    case 12: fmac_bcast<12>(acc, w, x); break; case 13: fmac_bcast<13>(acc, w, x); break; case 14: fmac_bcast<14>(acc, w, x); break; default: fmac_bcast<15>(acc, w, x); break;
    }
}
// (178 VGPRs = 2 waves per SIMD.  Forcing 168 VGPRs for 3 waves costs 4 spilled registers and measured 16.3 vs 15.3 ms per batch.)
template <int MT, int NL, int LW, bool ABS = false>
__global__ void __launch_bounds__(256) k_scalar_gemm_f64(const uint64_t *__restrict__ in, const void *__restrict__ idx_, const double *__restrict__ Wd,
                                                         const void *__restrict__ out_idx_, const uint64_t *__restrict__ bias, const void *__restrict__ bias_idx_,
                                                         uint64_t *__restrict__ out, const DevConsts *__restrict__ C, uint32_t chunks, uint32_t G, uint32_t M,
                                                         uint32_t K, uint32_t mtiles, uint32_t lazy, uint32_t Kp, uint32_t obase, uint32_t polys, uint32_t order, uint32_t Kw, GemmUnits U) {
    typedef typename GemmTab<ABS>::T TT;
    const TT *idx = (const TT *)idx_, *out_idx = (const TT *)out_idx_, *bias_idx = (const TT *)bias_idx_;
    const uint32_t n = C->n, k = C->k, limbs = polys * k;       // polys = ciphertext size: 2, or 3 for unrelinearized products (Evaluator::multiply_plain / add accept both)
    uint32_t chunk, limb, mt, g;
    gemm_block_coords(blockIdx.x, blockIdx.y, chunks, limbs, mtiles, G, chunk, limb, mt, g, order);
    const uint32_t j = limb % k, i = chunk * blockDim.x + threadIdx.x;
    const size_t ctw = (size_t)limbs * n, e = (size_t)limb * n + i;
    const size_t iu = U.in ? U.in : ctw, ou = U.out ? U.out : ctw, bu = U.bias ? U.bias : n;
    const DMod qm = C->q[j];
    double acc[NL][MT], res[MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
        res[m] = 0.0;
#pragma unroll
        for (int l = 0; l < NL; l++) acc[l][m] = 0.0;
    }
    const TT *gi = idx + (size_t)g * Kp;                                                 // row pitch Kp: 16 B aligned, -1 (ABS: 0) beyond K
    const double *gw = Wd + ((size_t)g * mtiles + mt) * (size_t)Kw * MT;                 // [kk < Kw][m]: zero rows behind the K terms (gemm_f64_rows)
    const uint32_t mcnt = min((uint32_t)MT, M - mt * MT);
    // fold: value = sum_l acc[l] * 2^(l*LW) mod q_j, in exact FP64 (q_j < 2^49): Horner with one modular multiply per limb.  (The
    // 128-bit integer version - double -> int128 conversions and a Barrett reduction per output - cost more instructions than the 25
    // terms of a convolution window.)
    const BzF::Mod mq = {C->qd[j], C->qinvd[j]};
    auto fold = [&]() {
#pragma unroll
        for (int m = 0; m < MT; m++) {
            double r = acc[NL - 1][m];
            acc[NL - 1][m] = 0.0;
#pragma unroll
            for (int l = NL - 2; l >= 0; l--) { r = __dadd_rn(BzF::mulmod(r, (double)(1u << LW), mq), acc[l][m]); acc[l][m] = 0.0; }
            res[m] = BzF::center(__dadd_rn(res[m], r), mq);       // |res| <= q/2 between folds, |r| < 2^53 - q
        }
    };
    // blocks of `lazy` terms with the fold BETWEEN the inner loops: a fold test inside the term loop gets if-converted by the
    // compiler (the whole 128-bit fold executed every iteration under v_cndmask - 30x the instructions of the 2*MT FMAs)
    // Software pipeline: a term is one dependent scalar load (gather index) + one global load, ~1 us of latency against
    // 2*MT*NL FMAs.  Two register sets ping-pong: the input elements of the NEXT PF terms are requested before the FMAs of the
    // current PF terms are issued.  The requests are branch-free (padded taps and terms past K multiply a valid word by the weight 0: every
    // (group, tile) of the table ends in zero rows, gemm_f64_rows), so the waits stay exact.
#ifndef GEMM_PF_SMALL
#define GEMM_PF_SMALL 4       // terms requested ahead per register set for MT <= 5 (convolution windows: 25 taps, 5 maps).  8 - two gather lists of four in flight per
                              // thread, VERDICT r03 next #7 - was measured in round 4 and is NOT the default: 91 instead of 66 VGPRs (5 instead of 7 waves per SIMD),
                              // 476 against 462 us for the CryptoNets convolution (profiles/HISTORY.md, round 4); again on the round-5 kernel (80 VGPRs, 26 spilled
                              // SGPRs for the weights of a set): 451-455 against 382-386 us
#endif
    constexpr int PF = (MT <= 5) ? GEMM_PF_SMALL : 4;
    static_assert(PF % 4 == 0, "gather indices travel in 16 B scalar loads of four");
    // A padded tap (-1 / address 0 in the gather row) and a term past K carry the WEIGHT 0 in the table (pack_gemm_f64) and read a valid word (element
    // 0 / the fallback ciphertext); a block of `lazy` terms ends on a multiple of 2 PF unless it ends at K: no per-lane select on the 64-bit words.
    auto fetch = [&](uint64_t (&x)[PF], uint32_t kk) {
        // ONE 16 B scalar load per four gather indices (four dependent s_load_dword + wait chains cost more than the FMAs)
        const uint32_t kc = min(kk, Kp - PF);
        if constexpr (ABS) {               // addresses: two 16 B scalar loads per four; a padded tap reads (and multiplies by 0) the fallback ciphertext `in`
#pragma unroll
            for (int c = 0; c < PF; c += 4) {
                const ulonglong2 a01 = *reinterpret_cast<const ulonglong2 *>(__builtin_assume_aligned(gi + kc + c, 16));
                const ulonglong2 a23 = *reinterpret_cast<const ulonglong2 *>(__builtin_assume_aligned(gi + kc + c + 2, 16));
                const uint64_t ad[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
                for (int p = 0; p < 4; p++) x[c + p] = gmem(ad[p] ? ad[p] : (uint64_t)in)[e];
            }
        } else {
#pragma unroll
            for (int c = 0; c < PF; c += 4) {
                const int4 ids = *reinterpret_cast<const int4 *>(__builtin_assume_aligned(gi + kc + c, 16));
                const int32_t id[4] = {ids.x, ids.y, ids.z, ids.w};
#pragma unroll
                for (int p = 0; p < 4; p++) x[c + p] = in[(size_t)max(id[p], 0) * iu + e];
            }
        }
    };
    // the weights of WB terms (up to 20 doubles = 40 SGPRs) are contiguous: requested together (wide scalar loads, ONE wait) before the first product.
    // WSET (the whole set fits: MT <= 5): they are requested BEFORE the gather entries of the set behind it (wload in front of fetch), so that the one
    // lgkmcnt(0) in front of that set's input requests covers them too - one scalar round trip per set on a wave's chain of dependent requests instead of two
    constexpr int WB = MT >= 20 ? 1 : (MT * PF <= 20 ? PF : 20 / MT);
    constexpr bool WSET = WB == PF;
    auto wload = [&](double (&w)[WB * MT], uint32_t kk) {
        const double *wp = gw + (size_t)kk * MT;
#pragma unroll
        for (int q = 0; q < WB * MT; q++) w[q] = wp[q];
    };
    auto terms = [&](const uint64_t (&x)[PF], uint32_t kk, const double (&w0)[WB * MT]) {
#pragma unroll
        for (int p0 = 0; p0 < PF; p0 += WB) {
            double w[WB * MT];
            if constexpr (WSET) {
#pragma unroll
                for (int q = 0; q < WB * MT; q++) w[q] = w0[q];
            } else wload(w, kk + p0);
#pragma unroll
            for (int p = p0; p < p0 + WB; p++) {
                double xl[NL];
#pragma unroll
                for (int l = 0; l < NL; l++) xl[l] = gemm_limb<NL, LW>(x[p], l);
#pragma unroll
                for (int m = 0; m < MT; m++) {
#pragma unroll
                    for (int l = 0; l < NL; l++) acc[l][m] = __fma_rn(xl[l], w[(p - p0) * MT + m], acc[l][m]);
                }
            }
        }
    };
    constexpr bool DPPW = GEMM_DPP_W && MT == 20 && PF == 4;
    constexpr int WV = DPPW ? PF * MT / 16 : 1;                    // 4 terms x 20 weights = 5 registers of 16 lanes
    auto wfetch = [&](double (&wv)[WV], uint32_t kk) {             // rows min(kk, K + 4) .. + 3: inside the zero rows behind the K terms
        const double *wp = gw + (size_t)min(kk, K + 4) * MT + (threadIdx.x & 15);
#pragma unroll
        for (int v = 0; v < WV; v++) wv[v] = wp[16 * v];
    };
    auto terms_dpp = [&](const uint64_t (&x)[PF], double (&wv)[WV]) {
#pragma unroll
        for (int p = 0; p < PF; p++) {
            double xl[NL];
#pragma unroll
            for (int l = 0; l < NL; l++) xl[l] = gemm_limb<NL, LW>(x[p], l);
            asm volatile("s_nop 1");
#pragma unroll
            for (int m = 0; m < MT; m++) {
                const int f = p * MT + m;
#pragma unroll
                for (int l = 0; l < NL; l++) fmac_bcast_lane(f & 15, acc[l][m], wv[(f >> 4) % WV], xl[l]);
            }
        }
    };
    for (uint32_t k0 = 0; k0 < K; k0 += lazy) {
        const uint32_t k1 = min(K, k0 + lazy);
        uint64_t xa[PF], xb[PF];
        if constexpr (DPPW) {
            double wa[WV], wb[WV];
            fetch(xa, k0); wfetch(wa, k0);
            for (uint32_t kk = k0; kk < k1; kk += 2 * PF) {
                fetch(xb, kk + PF); wfetch(wb, kk + PF);
                terms_dpp(xa, wa);
                fetch(xa, kk + 2 * PF); wfetch(wa, kk + 2 * PF);
                terms_dpp(xb, wb);
            }
        } else {
            // sets of PF terms in pairs, then the odd set: a window of 25 taps is 7 sets of four, not 8.  ONE exit at the end of the pair loop and no branch
            // inside it - at a join the compiler's wait counts assume the path with the fewest requests in flight and drain the set requested ahead.
            const uint32_t sets = (k1 - k0 + PF - 1) / PF;
            uint32_t kk = k0;
            double wa[WB * MT], wb[WB * MT];
            fetch(xa, k0);
            for (uint32_t it = sets >> 1; it; it--, kk += 2 * PF) {
                if constexpr (WSET) { wload(wa, kk); __builtin_amdgcn_sched_barrier(0); }      // (the scheduler sinks the request behind the input requests otherwise)
                fetch(xb, kk + PF);
                terms(xa, kk, wa);
                if constexpr (WSET) { wload(wb, kk + PF); __builtin_amdgcn_sched_barrier(0); }
                fetch(xa, kk + 2 * PF);
                terms(xb, kk + PF, wb);
            }
            if (sets & 1) { if constexpr (WSET) wload(wa, kk); terms(xa, kk, wa); }
        }
        fold();
    }
    // Outputs in sets of OB: the table entries of a set (scalar loads), then its bias words (all requested before the first is used), then the arithmetic and
    // the stores - one exposed round trip per kind and set.  (One output at a time it was three dependent round trips per output: table entry -> bias entry ->
    // bias word, ~8 us of a convolution workgroup's ~19 us.)
    constexpr int OB = MT < 5 ? MT : 5;
    const uint32_t olast = G * M - 1;
    const bool hb = (ABS ? bias_idx != nullptr : bias != nullptr) && limb < k;
#pragma unroll
    for (int m0 = 0; m0 < MT; m0 += OB) {
        uint32_t oo[OB];
        TT oi[OB], bi[OB];
        bool st[OB];
        uint64_t bv[OB];
#pragma unroll
        for (int u = 0; u < OB; u++) oo[u] = min(g * M + mt * MT + m0 + u, olast);
#pragma unroll
        for (int u = 0; u < OB; u++) { oi[u] = out_idx[oo[u]]; bi[u] = 0; bv[u] = 0; }
        if (hb) {
#pragma unroll
            for (int u = 0; u < OB; u++) bi[u] = bias_idx[oo[u]];
        }
#pragma unroll
        for (int u = 0; u < OB; u++) st[u] = (uint32_t)(m0 + u) < mcnt && (ABS ? oi[u] != 0 : (int64_t)oi[u] >= 0);
        if (hb) {
#pragma unroll
            for (int u = 0; u < OB; u++) {
                if constexpr (ABS) bv[u] = gmem(st[u] && bi[u] ? bi[u] : (uint64_t)in)[i];          // no bias: any readable word, discarded below
                else bv[u] = bias[(size_t)(st[u] ? bi[u] : (TT)0) * bu + i];
            }
#pragma unroll
            for (int u = 0; u < OB; u++) if (!(st[u] && (ABS ? bi[u] != 0 : true))) bv[u] = 0;
        }
#pragma unroll
        for (int u = 0; u < OB; u++) {
            if (!st[u]) continue;
            // res left the last fold recentred (|res| <= q/2 + 1 ulp of the quotient): canonical residue without a second quotient
            const double rc = res[m0 + u] < 0.0 ? __dadd_rn(res[m0 + u], mq.q) : res[m0 + u];
            uint64_t r = (uint64_t)__double_as_longlong(__dadd_rn(rc, 4503599627370496.0)) & 0x000FFFFFFFFFFFFFull;
            // bias: a PoolLayer bias is the constant polynomial - every coefficient but one is zero and scales to zero (skipped wave-uniformly almost everywhere)
            if (bv[u]) r = addmod(r, scale_plain(C, bv[u], j), qm.q);
            if constexpr (ABS) gmem_w(oi[u])[e] = r;
            else out[(size_t)(obase + (uint32_t)oi[u]) * ou + e] = r;
        }
    }
}

// ------------------------------------------------------------------ scalar GEMM on the int8 matrix cores (exact)
// out[o][e] = sum_k W[o][k] * x[k][e] mod q_j is an integer contraction over K input ciphertexts: M = outputs, N = coefficients, K = inputs.
// With SMALL signed weights it maps onto v_mfma_i32_32x32x32_i8 EXACTLY: the residue x < 2^46 is recoded into 6 signed base-256 digits
// (x + 0x80..80 has bytes b_i; b_i - 128 = b_i ^ 0x80 as int8), the weight into P <= 3 signed digits the same way; digit x digit products
// (<= 2^14) accumulate in i32 over K P < 2^17 terms without overflow, products of equal weight 256^(i+p) share one accumulator
// ("diagonal"), and the 6 + P - 1 diagonals are folded mod q_j in exact FP64 at the end.
// Workgroup = 4 waves = 32 coefficient columns x up to four 32-row output tiles (wave w: m-tile 4 mg + w).  The B operand (digits of 32
// inputs x 32 columns per K step) is the same for the four waves, so they build it TOGETHER: wave w loads the input words of K slots
// 4w .. 4w+3 of its lanes' half (4 loads of 256 contiguous bytes per half-wave instead of 16), recodes them, transposes their bytes with
// v_perm_b32 into one dword per digit plane, and publishes the six dwords in LDS; after one barrier every wave reads its complete
// fragments back as 16 B per lane and plane.  Three LDS buffers and a ring of three register sets keep one barrier per K step with the input words and
// the A fragments (weight digits, laid out in fragment order by the plan: one 16 B load per lane and plane) of the next TWO steps in flight; the gather-table
// entries of a wave's slots are wave-uniform and arrive through the scalar cache, a step ahead of the loads that use them (round 5).
// K-slot convention: lane l, byte t of an operand <-> k = 32 ks + 16 (l >> 5) + t for BOTH operands (the instruction pairs equal slots,
// so any convention shared by A and B is correct).  C/D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v16i_t __attribute__((ext_vector_type(16)));
DEV uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }   // byte n of the result = byte sel[n] of {hi: 4..7, lo: 0..3}
#ifndef GEMM_MFMA_DEPTH
#define GEMM_MFMA_DEPTH 2          // K steps of input words in flight beside the one being multiplied (1 or 2)
#endif
// FORM (the pre-floor form of cn_square_gemm, relative addressing only; the same weight fragments and tables):
//   GEMM_BSK: the limbs are those of the auxiliary base Bsk (kb per polynomial, moduli k .. k + kb - 1, below 2^49: SEVEN signed digits), canonical words in,
//             canonical words out, no bias - X_o = sum_k w_ok x_k mod b on the NTT-form tensor words of components 0 and 1;
//   GEMM_Y:   the inputs are the lazy-FP64 hand-off words of the q-side tensor; the load path forms the floor's canonical y = [x t (q/q_j)^-1]_{q_j} (k_behz_floor_f64's
//             own expression) and the diagonals are folded to the EXACT signed 64-bit integer Y_o = sum_k w_ok y_k (two's complement; no modular fold, no bias).
// (A pack of at most one form tag: the ciphertext form keeps its name k_scalar_gemm_mfma<P, ABS>.)
// GemmResidual (a further tag, P = 1 only): the plan's clipped + residual form (gemm_residual_form, cn_gemm_plan.h).  Wf holds TWO int8 planes of the same weight
// 256^0 - c = clamp(w, -127, 127) and r = w - c, laid out as the planes of P = 2 - and behind them the table kres [G]; the K slots are sorted so that r = 0 behind
// K step kres[g].  The kernel runs kres[g] + ksteps steps of the ONE-plane body: step v < kres multiplies the r fragment of K step v, step v >= kres the c fragment
// of K step v - kres, into the same accumulators (same weight; the integer sum does not care about the order).  Which plane and which K step a step reads is
// scalar address arithmetic in the request lambdas: no second loop, no branch around loads in flight, no register beyond those of P = 1 (a second loop for the
// residual phase, which would save the kres repeated B operands, doubled the live accumulators at its joins: the pre-floor forms spilled; the ciphertext form, 240
// VGPRs without a spill, was not measured).  A residual step costs a whole step here, which is what the plan's gate on kres counts (GEMM_RES_SHARE, cn_gemm_plan.h).
// Accumulators, fold and epilogue are those of P = 1: |acc| <= 128 sum_k |w_k| < 2^31 by the plan's gate.  kres = 0 is the P = 1 kernel step for step.
enum { GEMM_CT = 0, GEMM_BSK = 1, GEMM_Y = 2 };
struct GemmBskForm { static constexpr int form = GEMM_BSK; static constexpr bool res = false; };
struct GemmYForm { static constexpr int form = GEMM_Y; static constexpr bool res = false; };
struct GemmResidual { static constexpr int form = GEMM_CT; static constexpr bool res = true; };
template <int P, bool ABS, class... FORM_>
__global__ void __launch_bounds__(256, 2) k_scalar_gemm_mfma(const uint64_t *__restrict__ in, const void *__restrict__ idx_, const int8_t *__restrict__ Wf,
                                                             const void *__restrict__ out_idx_, const uint64_t *__restrict__ bias, const void *__restrict__ bias_idx_,
                                                             uint64_t *__restrict__ out, const DevConsts *__restrict__ C, uint32_t G, uint32_t M, uint32_t mtiles,
                                                             uint32_t ksteps, uint32_t obase, uint32_t polys, GemmUnits U) {
    constexpr int FORM = (GEMM_CT + ... + FORM_::form);
    constexpr bool RES = (false || ... || FORM_::res);
    constexpr int PW = RES ? 2 : P;                                // weight planes in Wf
    static_assert(sizeof...(FORM_) <= (RES ? 2 : 1) && FORM <= GEMM_Y && (FORM == GEMM_CT || !ABS), "the pre-floor forms use relative addressing");
    static_assert(!RES || P == 1, "clipped + residual weights: one plane and its residual");
    typedef typename GemmTab<ABS>::T TT;
    const TT *idx = (const TT *)idx_, *out_idx = (const TT *)out_idx_, *bias_idx = (const TT *)bias_idx_;
    constexpr int ND = FORM == GEMM_BSK ? 7 : 6, D = ND + P - 1, NB = GEMM_MFMA_DEPTH + 1;
    __shared__ __align__(16) uint32_t frag[NB][ND][64][4];         // [buffer][digit plane][lane][slot group q]: 6 (7) KiB each
    const uint32_t n = C->n, k = FORM == GEMM_BSK ? C->kb : C->k, limbs = polys * k, ctiles = n >> 5;
    // the wave number as a SCALAR: the gather-table entries of a wave's K slots are then wave-uniform and travel through the scalar cache (lgkmcnt).  As vector
    // loads they sat on vmcnt IN FRONT of the input loads that need them: every step waited for the table (vmcnt(0) - which also drained whatever input words
    // were still in flight), then for the inputs: two exposed round trips per K step, 1.9 us of them against 0.2 us of matrix instructions.
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), half = lane >> 5, col = lane & 31;
    uint32_t b = blockIdx.x;
    const uint32_t ctile = b % ctiles; b /= ctiles;
    const uint32_t limb = b % limbs; b /= limbs;
    const uint32_t mgroups = (mtiles + 3) >> 2, mg = b % mgroups, g = b / mgroups;
    const uint32_t mt = mg * 4 + wave;
    const bool active = mt < mtiles;                           // a wave without an output tile still loads its share of the B operand
    const uint32_t j = limb % k;
    const size_t ctw = (size_t)limbs * n, e = (size_t)limb * n + (size_t)ctile * 32 + col;
    const size_t iu = U.in ? U.in : ctw, ou = U.out ? U.out : ctw, bu = U.bias ? U.bias : n;
    const uint32_t Kp = ksteps * 32;
    const TT *gi = idx + (size_t)g * Kp + 4 * wave;            // + 32 ks + 16 half + u
    const int8_t *wf = Wf + ((((size_t)g * PW) * mtiles + (active ? mt : 0)) * ksteps) * 1024 + (size_t)lane * 16;      // + (p * mtiles * ksteps + ks) * 1024
    v16i_t acc[D];
#pragma unroll
    for (int d = 0; d < D; d++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[d][r] = 0;
    const uint64_t BIAS = FORM == GEMM_BSK ? 0x0080808080808080ull : 0x0000808080808080ull;
    // Requests behind the last step are NOT skipped but repeat the last step (a few words re-read from L2): with a branch around the loads the compiler's wait
    // counts at the join assume the path WITHOUT them - "at most 5 younger loads" where 11 are in flight - and every step drained the sets requested ahead.
    const uint32_t klast = ksteps - 1;
    // clipped + residual form: step v of vsteps = kres + ksteps reads plane r of K step v (v < kres) or plane c of K step v - kres; `fragment`: its A fragment, in
    // units of 1024 bytes from wf.  Otherwise step v is K step v
    uint32_t kres = 0;
    if constexpr (RES) kres = reinterpret_cast<const uint32_t *>(Wf + (size_t)G * PW * mtiles * ksteps * 1024)[g];
    const uint32_t vsteps = RES ? ksteps + kres : ksteps;
    auto kstep = [&](uint32_t v) { if constexpr (RES) { const uint32_t vv = min(v, vsteps - 1); return vv < kres ? vv : vv - kres; } else return min(v, klast); };
    auto fragment = [&](uint32_t v) { if constexpr (RES) return min(v, vsteps - 1) < kres ? mtiles * ksteps + kstep(v) : kstep(v); else return min(v, klast); };
    auto load_idx = [&](TT (&s)[8], uint32_t ks) {              // table entries of slots 4 wave .. + 3 (lanes 0..31) and 16 + 4 wave .. + 3 (lanes 32..63): scalar loads
        const TT *t = gi + (size_t)kstep(ks) * 32;
#pragma unroll
        for (int u = 0; u < 4; u++) { s[u] = t[u]; s[4 + u] = t[16 + u]; }
    };
    auto load_x = [&](uint64_t (&x)[4], const TT (&s)[8]) {     // the 4 input words of this lane's slots
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if constexpr (ABS) {
                const uint64_t a0 = s[u] ? s[u] : (uint64_t)in, a1 = s[4 + u] ? s[4 + u] : (uint64_t)in;      // padded tap: any readable word (its weight digits are 0)
                x[u] = gmem(half ? a1 : a0)[e];
            } else {
                // both products on the scalar unit, THEN the per-lane choice (left alone the compiler chooses first and multiplies per lane: two quarter-rate
                // v_mad_u64_u32 per word)
                size_t o0 = (size_t)max(s[u], 0) * iu, o1 = (size_t)max(s[4 + u], 0) * iu;
                asm volatile("" : "+s"(o0), "+s"(o1));
                x[u] = in[(half ? o1 : o0) + e];
            }
        }
    };
    auto load_a = [&](v4i_t (&af)[P], uint32_t ks) {
#pragma unroll
        for (int p = 0; p < P; p++) af[p] = *reinterpret_cast<const v4i_t *>(wf + ((size_t)p * mtiles * ksteps + fragment(ks)) * 1024);
    };
    // x / af: NB register sets in a ring - set (ks mod NB) holds step ks, requested GEMM_MFMA_DEPTH steps ahead; `nidx` = the table entries of the step whose
    // inputs are requested next (asked for one step before they are needed; refilled right after use)
    uint64_t xs[NB][4];
    v4i_t afs[NB][P];
    TT nidx[8];
    load_idx(nidx, 0);
#pragma unroll
    for (int s = 0; s < GEMM_MFMA_DEPTH; s++) { load_x(xs[s], nidx); load_a(afs[s], s); load_idx(nidx, s + 1); }
    auto step = [&](uint64_t (&x)[4], v4i_t (&af)[P], uint64_t (&xn)[4], v4i_t (&afn)[P], uint32_t ks, uint32_t (*fb)[64][4]) {
        // recode: byte i of y = signed digit i; transpose the 4 words into one dword per digit plane; publish
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            uint64_t xw = x[u];
            if constexpr (FORM == GEMM_Y) {                                // the floor's canonical y of a lazy tensor word (an exact integer below q_j < 2^47)
                const BzF::Mod mq = {C->qd[j], C->qinvd[j]};
                const double yv = bz_canon(BzF::mulmod(lazy_value(xw), C->bd.fl_c1n_q[j], mq), mq);
                xw = (uint64_t)__double_as_longlong(__dadd_rn(yv, 4503599627370496.0)) & 0x000FFFFFFFFFFFFFull;
            }
            const uint64_t y = (xw + BIAS) ^ BIAS; lo[u] = (uint32_t)y; hi[u] = (uint32_t)(y >> 32);
        }
        const uint32_t ab02 = byte_perm(lo[1], lo[0], 0x06020400u), cd02 = byte_perm(lo[3], lo[2], 0x06020400u);     // (a0 b0 a2 b2), (c0 d0 c2 d2)
        const uint32_t ab13 = byte_perm(lo[1], lo[0], 0x07030501u), cd13 = byte_perm(lo[3], lo[2], 0x07030501u);     // (a1 b1 a3 b3), (c1 d1 c3 d3)
        const uint32_t hab = byte_perm(hi[1], hi[0], 0x05010400u), hcd = byte_perm(hi[3], hi[2], 0x05010400u);       // (a4 b4 a5 b5), (c4 d4 c5 d5)
        fb[0][lane][wave] = byte_perm(cd02, ab02, 0x05040100u);          // a0 b0 c0 d0
        fb[1][lane][wave] = byte_perm(cd13, ab13, 0x05040100u);
        fb[2][lane][wave] = byte_perm(cd02, ab02, 0x07060302u);          // a2 b2 c2 d2
        fb[3][lane][wave] = byte_perm(cd13, ab13, 0x07060302u);
        fb[4][lane][wave] = byte_perm(hcd, hab, 0x05040100u);
        fb[5][lane][wave] = byte_perm(hcd, hab, 0x07060302u);
        if constexpr (ND == 7) {                                         // (a6 b6 . .), (c6 d6 . .) -> a6 b6 c6 d6
            const uint32_t hab6 = byte_perm(hi[1], hi[0], 0x06020602u), hcd6 = byte_perm(hi[3], hi[2], 0x06020602u);
            fb[ND - 1][lane][wave] = byte_perm(hcd6, hab6, 0x05040100u);
        }
        load_x(xn, nidx); load_a(afn, ks + GEMM_MFMA_DEPTH);             // in flight over the barriers and matrix instructions of the next GEMM_MFMA_DEPTH steps
        load_idx(nidx, ks + GEMM_MFMA_DEPTH + 1);
        __syncthreads();
        if (active) {
            v4i_t bf[ND];
#pragma unroll
            for (int i = 0; i < ND; i++) bf[i] = *reinterpret_cast<const v4i_t *>(&fb[i][lane][0]);
            // P x 6 matrix instructions; equal digit weights share an accumulator
#pragma unroll
            for (int p = 0; p < P; p++)
#pragma unroll
                for (int i = 0; i < ND; i++) acc[i + p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[p], bf[i], acc[i + p], 0, 0, 0);
        }
    };
    // the set that step ks refills is the one step ks - 1 consumed
    // (for the same reason the loop has ONE exit, at its end: whole turns of the ring, then the ksteps mod NB steps left over)
    uint32_t ks = 0;
    for (; ks + NB <= vsteps; ks += NB) {
#pragma unroll
        for (int s = 0; s < NB; s++) step(xs[s], afs[s], xs[(s + GEMM_MFMA_DEPTH) % NB], afs[(s + GEMM_MFMA_DEPTH) % NB], ks + s, frag[s]);
    }
#pragma unroll
    for (int s = 0; s < NB - 1; s++)
        if (ks + s < vsteps) step(xs[s], afs[s], xs[(s + GEMM_MFMA_DEPTH) % NB], afs[(s + GEMM_MFMA_DEPTH) % NB], ks + s, frag[s]);
    if (!active) return;
    if constexpr (FORM == GEMM_Y) {
        // ---- the exact integer: sum_d acc_d 256^d in two's complement (|Y| < 2^63 by the plan's gate - cn_prefloor_bound_ok, cn_policy.h - so the wrapped sum is Y)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const uint32_t row = (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * half, o = g * M + mt * 32 + row;
            if (mt * 32 + row >= M) continue;
            uint64_t v = 0;
#pragma unroll
            for (int d = 0; d < D; d++) v += (uint64_t)(int64_t)acc[d][r] << (8 * d);
            if (out_idx[o] < 0) continue;
            out[(size_t)(obase + (uint32_t)out_idx[o]) * ou + e] = v;
        }
        return;
    }
    // ---- fold the diagonals: value = sum_d acc_d 256^d mod q_j (exact FP64), bias, store
    const uint32_t jm = FORM == GEMM_BSK ? C->k + j : j;
    const BzF::Mod mq = {C->qd[jm], C->qinvd[jm]};
    const DMod qm = C->q[FORM == GEMM_BSK ? 0 : j];
    // three neighbouring diagonals at a time: a_d + 256 a_(d+1) + 65536 a_(d+2) is an exact double (|a| < 2^31: below 2^47.1), so a row costs two modular
    // products (by 2^24 and 2^48 mod q_j) instead of one per diagonal
    const double c24 = BzF::center(16777216.0, mq), c48 = BzF::center(__dmul_rn(c24, 16777216.0), mq);       // exact: |c24| <= 2^24
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const uint32_t row = (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * half, o = g * M + mt * 32 + row;
        if (mt * 32 + row >= M) continue;
        auto group = [&](int d0) {
            double t = (double)acc[d0][r];
            if (d0 + 1 < D) t = __fma_rn((double)acc[d0 + 1 < D ? d0 + 1 : d0][r], 256.0, t);
            if (d0 + 2 < D) t = __fma_rn((double)acc[d0 + 2 < D ? d0 + 2 : d0][r], 65536.0, t);
            return t;
        };
        double v = __dadd_rn(group(0), BzF::mulmod(group(3), c24, mq));
        if (D > 6) v = __dadd_rn(v, BzF::mulmod(group(6), c48, mq));
        uint64_t res = BzF::to_u64(v, mq);
        if constexpr (ABS) {
            if (!out_idx[o]) continue;
            if (bias_idx && bias_idx[o] && limb < k) { const uint64_t bv = gmem(bias_idx[o])[(size_t)ctile * 32 + col]; if (bv) res = addmod(res, scale_plain(C, bv, j), qm.q); }
            gmem_w(out_idx[o])[e] = res;
        } else {
            if (out_idx[o] < 0) continue;
            if (FORM == GEMM_CT && bias && limb < k) { const uint64_t bv = bias[(size_t)bias_idx[o] * bu + (size_t)ctile * 32 + col]; if (bv) res = addmod(res, scale_plain(C, bv, j), qm.q); }
            out[(size_t)(obase + (uint32_t)out_idx[o]) * ou + e] = res;
        }
    }
}

// ------------------------------------------------------------------ digit GEMM (cn_square_gemm)
// The dense layer behind a squaring layer, applied to the DIGITS of the unrelinearized component: S[o][g][i] = sum_k w[o][k] * dig_g(in[idx[k]][l][i]) for the
// digit g = (source limb l, digit d) of the key-switch decomposition, dig = (word >> dbc d) & (2^dbc - 1).  Digit extraction is the only step of a key switch that
// is not linear, and it happens here, per input, before the weights: everything behind it (transforms, key products, inverse transforms, the mod q_j reductions)
// commutes with the weighted sum, so ONE key switch per output fed with S gives the words of one key switch per input followed by the scalar GEMM.  S is a plain
// signed integer (|S| <= max_o sum_k |w_ok| (2^dbc - 1) < 2^52, checked when the plan is built), the same for every output limb j: exact in one FMA per term.
// Workgroup = (256 coefficients, source limb l, group of DG digits, output tile mt, gather list g); in = component 2 of product 0, products in_unit words apart.
// Weights [g][mt][kk < Kw][MT] signed doubles, zero rows behind the K terms and zero for padded taps (which read a valid word: product 0); gather rows as in
// k_scalar_gemm_f64.  The output tiles of a slice take block ids 8 apart: one XCD, adjacent in time, the slice is re-read from that L2 (gemm_block_coords).
// Element type of S (all three producers): doubles - k_digit_gemm<MT, DG> - or, where the plan's digit bound is at most 2^31 - 1 (GemmPlan::dig_i32), int32 words -
// k_digit_gemm<MT, DG, int32_t>: the same exact integer in half the bytes, read by the KsDigits<AR, int32_t> key switch.  (A parameter pack: the double forms keep their names.)
template <class... E> struct DigitWord { typedef double type; };
template <> struct DigitWord<int32_t> { typedef int32_t type; };
template <> struct DigitWord<GemmResidual> { typedef double type; };                  // (k_digit_gemm_mfma alone: the plan's clipped + residual weights)
template <> struct DigitWord<int32_t, GemmResidual> { typedef int32_t type; };
template <int MT, int DG, class... E>
__global__ void __launch_bounds__(256) k_digit_gemm(const uint64_t *__restrict__ in, size_t in_unit, const int32_t *__restrict__ idx, const double *__restrict__ Wd,
                                                    const int32_t *__restrict__ out_idx, typename DigitWord<E...>::type *__restrict__ S, const DevConsts *__restrict__ C, uint32_t G, uint32_t M,
                                                    uint32_t K, uint32_t mtiles, uint32_t Kp, uint32_t Kw, uint32_t ndg) {
    const uint32_t n = C->n, k = C->k, chunks = n >> 8;
    uint32_t chunk, lj, mt, g;
    gemm_block_coords(blockIdx.x, 0, chunks, k * ndg, mtiles, G, chunk, lj, mt, g);
    const uint32_t l = lj % k, d0 = (lj / k) * DG, nd = C->rl_dig[l];
    if (d0 >= nd) return;
    uint32_t g0 = 0;                                           // index of the first digit of limb l in the key
    for (uint32_t x = 0; x < l; x++) g0 += C->rl_dig[x];
    const uint32_t i = chunk * 256 + threadIdx.x, dbc = (uint32_t)C->dbc, mask = (1u << dbc) - 1;
    const size_t e = (size_t)l * n + i;
    uint32_t sh[DG];
#pragma unroll
    for (int d = 0; d < DG; d++) sh[d] = min(dbc * (d0 + (uint32_t)d), 63u);
    double acc[DG][MT];
#pragma unroll
    for (int d = 0; d < DG; d++)
#pragma unroll
        for (int m = 0; m < MT; m++) acc[d][m] = 0.0;
    const int32_t *gi = idx + (size_t)g * Kp;
    const double *gw = Wd + ((size_t)g * mtiles + mt) * (size_t)Kw * MT;
    constexpr int PF = 4, WB = MT > 10 ? 1 : 2;
    auto fetch = [&](uint64_t (&x)[PF], uint32_t kk) {         // branch-free: terms past K and padded taps carry the weight 0
        const int4 ids = *reinterpret_cast<const int4 *>(__builtin_assume_aligned(gi + min(kk, Kp - PF), 16));
        const int32_t id[4] = {ids.x, ids.y, ids.z, ids.w};
#pragma unroll
        for (int p = 0; p < PF; p++) x[p] = in[(size_t)max(id[p], 0) * in_unit + e];
    };
    auto terms = [&](const uint64_t (&x)[PF], uint32_t kk) {
#pragma unroll
        for (int p0 = 0; p0 < PF; p0 += WB) {
            double w[WB * MT];
            const double *wp = gw + (size_t)(kk + p0) * MT;
#pragma unroll
            for (int q = 0; q < WB * MT; q++) w[q] = wp[q];
#pragma unroll
            for (int p = p0; p < p0 + WB; p++) {
                double dg[DG];
#pragma unroll
                for (int d = 0; d < DG; d++) dg[d] = (double)((uint32_t)(x[p] >> sh[d]) & mask);
#pragma unroll
                for (int m = 0; m < MT; m++)
#pragma unroll
                    for (int d = 0; d < DG; d++) acc[d][m] = __fma_rn(dg[d], w[(p - p0) * MT + m], acc[d][m]);
            }
        }
    };
    {   // sets of PF terms in pairs, two register sets ping-pong (k_scalar_gemm_f64); ONE exit at the end of the pair loop
        const uint32_t sets = (K + PF - 1) / PF;
        uint32_t kk = 0;
        uint64_t xa[PF], xb[PF];
        fetch(xa, 0);
        for (uint32_t it = sets >> 1; it; it--, kk += 2 * PF) {
            fetch(xb, kk + PF);
            terms(xa, kk);
            fetch(xa, kk + 2 * PF);
            terms(xb, kk + PF);
        }
        if (sets & 1) terms(xa, kk);
    }
    const uint32_t tot = C->rl_tot;
#pragma unroll
    for (int m = 0; m < MT; m++) {
        const uint32_t mm = mt * MT + (uint32_t)m;
        if (mm >= M) break;
        const int32_t o = out_idx[g * M + mm];
        if (o < 0) continue;                                   // padding member of a smaller group
#pragma unroll
        for (int d = 0; d < DG; d++)
            if (d0 + (uint32_t)d < nd) S[((size_t)o * tot + g0 + d0 + (uint32_t)d) * n + i] = (typename DigitWord<E...>::type)acc[d][m];
    }
}

// ------------------------------------------------------------------ digit GEMM on the int8 matrix cores (exact)
// The same sums S[o][(l, d)][i] = sum_k w[o][k] * dig_d(in[idx[k]][l][i]) as k_digit_gemm, as an integer contraction on v_mfma_i32_32x32x32_i8 with the structure of
// k_scalar_gemm_mfma: workgroup = 4 waves = 32 coefficient columns of one source limb l x up to four 32-row output tiles (wave w: tile 4 mg + w) x a group of DG digits;
// the waves build the B operand together through LDS (one barrier per K step, ring of three register sets, gather-table entries as scalar loads - see there for why).
// A operand: the plan's weight fragments as they are (pack_gemm_mfma: P signed base-256 digits w_p of every weight, zero for padded taps / rows / terms).
// B operand: a digit dg < 2^dbc, dbc <= 14, is split as dg = lo + 256 hi with t = dg + 128, lo = (t & 255) - 128 in -128..127 (the byte (t & 255) ^ 0x80 read as int8)
// and hi = t >> 8 in 0..64 - exact by construction, both int8.  Products lo w_p have weight 256^p, hi w_p weight 256^(p + 1): P + 1 diagonals per digit,
//   S = sum_j 256^j acc_j,   acc_j = sum_k (lo_k w_(k,j) + hi_k w_(k,j-1)).
// A diagonal receives at most two products per term, together at most 128 * 128 + 64 * 128 = 24576 in magnitude; the plan takes this form only with 3 K < 2^17
// (gemm_mfma_ok), K <= 43690 terms: |acc_j| <= 1 073 725 440 < 2^31 (the bound is enforced where the plan is built, cn_gemm_plan.h).
// Fold in FP64, lowest diagonal first: every partial sum is an integer below 2^53 in magnitude - acc_0 + 256 acc_1 + 65536 acc_2 < 2^47.1 for any i32 values, and the top
// diagonal of P = 3 holds only hi w_2 products (|w_2| <= 128: |acc_3| < 2^28.5, 2^24 |acc_3| < 2^52.5) - so each FMA is exact and the result is the S of k_digit_gemm
// (|S| < 2^52 by the plan's digit check), stored where that kernel stores it.  An accumulator register holds 32 consecutive coefficients per half-wave: 256 B per store.
// Digit groups: 16 (P + 1) DG accumulator registers per wave; all five digits of a CryptoNets limb (240 at P = 2) do not fit two workgroups per CU, so a workgroup takes
// DG of them and the groups of a slice take block ids 8 apart - one XCD, adjacent in time: the second group reads the slice from that L2.  Limbs with fewer digits
// skip the absent ones (rl_dig), a group without any digit leaves at once.
// int32 words (k_digit_gemm_mfma<P, DG, int32_t>): |S| <= 2^31 - 1, so the fold runs in 32-bit integers - exact modulo 2^32 whatever the partial sums do - and
// the word is stored as it is: no conversion, half the bytes (an accumulator register then stores 128 B per half-wave).
// Clipped + residual weights (k_digit_gemm_mfma<1, DG, .., GemmResidual>; gemm_residual_form, cn_gemm_plan.h): as in k_scalar_gemm_mfma the kernel runs kres[g] + ksteps
// steps of the one-plane body - the r fragments of the first kres[g] K steps, then the c fragments of all of them - into the SAME two diagonals (r has the weight 256^0
// of c).  A diagonal then receives (c + r) lo or (c + r) hi with |c| + |r| = |w|: |acc_j| <= (128 + 64) sum_k |w_k| < 2^31 by the plan's gate (gemm_digit_form).
// With 32 accumulator registers per digit instead of 48 this form takes DG = DIGIT_GEMM_RES_GROUP = 5 digits per workgroup - every digit of a CryptoNets limb: the slice
// is read once and the B operand built once instead of twice (207 VGPRs, two workgroups per CU; 95 us against 109 us with DG = 3 at 146 VGPRs, profiles/gemm_residual_plane.md).
constexpr int DIGIT_GEMM_RES_GROUP = 5;
template <int P, int DG, class... E>
__global__ void __launch_bounds__(256, 2) k_digit_gemm_mfma(const uint64_t *__restrict__ in, size_t in_unit, const int32_t *__restrict__ idx, const int8_t *__restrict__ Wf,
                                                            const int32_t *__restrict__ out_idx, typename DigitWord<E...>::type *__restrict__ S, const DevConsts *__restrict__ C, uint32_t G,
                                                            uint32_t M, uint32_t mtiles, uint32_t ksteps, uint32_t ndg) {
    constexpr int NP = 2 * DG, D = P + 1, NB = GEMM_MFMA_DEPTH + 1;
    constexpr bool RES = (false || ... || std::is_same<E, GemmResidual>::value);
    constexpr int PW = RES ? 2 : P;                                // weight planes in Wf
    static_assert(!RES || P == 1, "clipped + residual weights: one plane and its residual");
    __shared__ __align__(16) uint32_t frag[NB][NP][64][4];         // [buffer][digit, piece][lane][slot group q]
    const uint32_t n = C->n, k = C->k, ctiles = n >> 5;            // n is a multiple of 256 (launcher)
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), half = lane >> 5, col = lane & 31;
    uint32_t b = blockIdx.x;
    const uint32_t x8 = b & 7; b >>= 3;
    const uint32_t dgi = b % ndg; b /= ndg;
    const uint32_t ctile = (b % (ctiles >> 3)) * 8 + x8; b /= ctiles >> 3;
    const uint32_t l = b % k; b /= k;
    const uint32_t mgroups = (mtiles + 3) >> 2, mg = b % mgroups, g = b / mgroups;
    const uint32_t d0 = dgi * DG, nd = C->rl_dig[l];
    if (d0 >= nd) return;
    const uint32_t cnt = min((uint32_t)DG, nd - d0);
    uint32_t g0 = 0;                                           // index of the first digit of limb l in the key
    for (uint32_t x = 0; x < l; x++) g0 += C->rl_dig[x];
    const uint32_t mt = mg * 4 + wave;
    const bool active = mt < mtiles;                           // a wave without an output tile still loads its share of the B operand
    const uint32_t dbc = (uint32_t)C->dbc, mask = (1u << dbc) - 1;
    uint32_t sh[DG];
#pragma unroll
    for (int d = 0; d < DG; d++) sh[d] = min(dbc * (d0 + (uint32_t)d), 63u);
    const size_t e = (size_t)l * n + (size_t)ctile * 32 + col;
    const uint32_t Kp = ksteps * 32;
    const int32_t *gi = idx + (size_t)g * Kp + 4 * wave;       // + 32 ks + 16 half + u
    const int8_t *wf = Wf + ((((size_t)g * PW) * mtiles + (active ? mt : 0)) * ksteps) * 1024 + (size_t)lane * 16;      // + (p * mtiles * ksteps + ks) * 1024
    v16i_t acc[DG][D];
#pragma unroll
    for (int d = 0; d < DG; d++)
#pragma unroll
        for (int j = 0; j < D; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[d][j][r] = 0;
    // requests behind the last step repeat the last step, as in k_scalar_gemm_mfma (no branch around loads in flight)
    const uint32_t klast = ksteps - 1;
    // clipped + residual form: step v of vsteps = kres + ksteps reads plane r of K step v (v < kres) or plane c of K step v - kres (k_scalar_gemm_mfma)
    uint32_t kres = 0;
    if constexpr (RES) kres = reinterpret_cast<const uint32_t *>(Wf + (size_t)G * PW * mtiles * ksteps * 1024)[g];
    const uint32_t vsteps = RES ? ksteps + kres : ksteps;
    auto kstep = [&](uint32_t v) { if constexpr (RES) { const uint32_t vv = min(v, vsteps - 1); return vv < kres ? vv : vv - kres; } else return min(v, klast); };
    auto fragment = [&](uint32_t v) { if constexpr (RES) return min(v, vsteps - 1) < kres ? mtiles * ksteps + kstep(v) : kstep(v); else return min(v, klast); };
    auto load_idx = [&](int32_t (&s)[8], uint32_t ks) {
        const int32_t *t = gi + (size_t)kstep(ks) * 32;
#pragma unroll
        for (int u = 0; u < 4; u++) { s[u] = t[u]; s[4 + u] = t[16 + u]; }
    };
    auto load_x = [&](uint64_t (&x)[4], const int32_t (&s)[8]) {   // a padded tap reads product 0 (its weight digits are 0)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            size_t o0 = (size_t)max(s[u], 0) * in_unit, o1 = (size_t)max(s[4 + u], 0) * in_unit;
            asm volatile("" : "+s"(o0), "+s"(o1));
            x[u] = in[(half ? o1 : o0) + e];
        }
    };
    auto load_a = [&](v4i_t (&af)[P], uint32_t ks) {
#pragma unroll
        for (int p = 0; p < P; p++) af[p] = *reinterpret_cast<const v4i_t *>(wf + ((size_t)p * mtiles * ksteps + fragment(ks)) * 1024);
    };
    uint64_t xs[NB][4];
    v4i_t afs[NB][P];
    int32_t nidx[8];
    load_idx(nidx, 0);
#pragma unroll
    for (int s = 0; s < GEMM_MFMA_DEPTH; s++) { load_x(xs[s], nidx); load_a(afs[s], s); load_idx(nidx, s + 1); }
    auto step = [&](uint64_t (&x)[4], v4i_t (&af)[P], uint64_t (&xn)[4], v4i_t (&afn)[P], uint32_t ks, uint32_t (*fb)[64][4]) {
        // digits of the 4 words, + 128: byte 0 = lo + 128, byte 1 = hi; transposed into one dword per (digit, piece); published
#pragma unroll
        for (int d = 0; d < DG; d++) {
            uint32_t t[4];
#pragma unroll
            for (int u = 0; u < 4; u++) t[u] = ((uint32_t)(x[u] >> sh[d]) & mask) + 128u;
            const uint32_t ab = byte_perm(t[1], t[0], 0x05010400u), cd = byte_perm(t[3], t[2], 0x05010400u);      // (a.lo b.lo a.hi b.hi), (c.lo d.lo c.hi d.hi)
            fb[2 * d][lane][wave] = byte_perm(cd, ab, 0x05040100u) ^ 0x80808080u;
            fb[2 * d + 1][lane][wave] = byte_perm(cd, ab, 0x07060302u);
        }
        load_x(xn, nidx); load_a(afn, ks + GEMM_MFMA_DEPTH);
        load_idx(nidx, ks + GEMM_MFMA_DEPTH + 1);
        __syncthreads();
        if (active) {
#pragma unroll
            for (int d = 0; d < DG; d++) {
                if ((uint32_t)d >= cnt) continue;
                const v4i_t blo = *reinterpret_cast<const v4i_t *>(&fb[2 * d][lane][0]), bhi = *reinterpret_cast<const v4i_t *>(&fb[2 * d + 1][lane][0]);
#pragma unroll
                for (int p = 0; p < P; p++) acc[d][p] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[p], blo, acc[d][p], 0, 0, 0);
#pragma unroll
                for (int p = 0; p < P; p++) acc[d][p + 1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[p], bhi, acc[d][p + 1], 0, 0, 0);
            }
        }
    };
    uint32_t ks = 0;
    for (; ks + NB <= vsteps; ks += NB) {
#pragma unroll
        for (int s = 0; s < NB; s++) step(xs[s], afs[s], xs[(s + GEMM_MFMA_DEPTH) % NB], afs[(s + GEMM_MFMA_DEPTH) % NB], ks + s, frag[s]);
    }
#pragma unroll
    for (int s = 0; s < NB - 1; s++)
        if (ks + s < vsteps) step(xs[s], afs[s], xs[(s + GEMM_MFMA_DEPTH) % NB], afs[(s + GEMM_MFMA_DEPTH) % NB], ks + s, frag[s]);
    if (!active) return;
    // ---- fold the diagonals of every digit to one exact double and store it: the table entries of the 16 rows first (one round trip)
    const uint32_t tot = C->rl_tot, olast = G * M - 1;
    int32_t oo[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const uint32_t mm = mt * 32 + (uint32_t)(r & 3) + 8u * (uint32_t)(r >> 2) + 4u * half;
        oo[r] = out_idx[min(g * M + mm, olast)];
        if (mm >= M) oo[r] = -1;
    }
#pragma unroll
    for (int d = 0; d < DG; d++) {
        if ((uint32_t)d >= cnt) continue;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            if (oo[r] < 0) continue;                               // row past M, or padding member of a smaller group
            typename DigitWord<E...>::type *dst = S + ((size_t)oo[r] * tot + g0 + d0 + (uint32_t)d) * n + (size_t)ctile * 32 + col;
            if constexpr (std::is_same<typename DigitWord<E...>::type, int32_t>::value) {
                uint32_t v = (uint32_t)acc[d][D - 1][r];
#pragma unroll
                for (int j = D - 2; j >= 0; j--) v = (v << 8) + (uint32_t)acc[d][j][r];
                *dst = (int32_t)v;
            } else {
                double v = (double)acc[d][0][r];
#pragma unroll
                for (int j = 1; j < D; j++) v = __fma_rn((double)acc[d][j][r], (double)(1u << (8 * j)), v);
                *dst = v;
            }
        }
    }
}

// ------------------------------------------------------------------ sum of K unrelinearized products (cn_mul_relin_sum)
// out = sum_k Relinearize(Multiply(a_k, b_k)) needs ONE key switch, by the identity of k_digit_gemm with unit weights: this kernel is the sum in front of it.  A
// streaming reduction over the K size-3 products of one output, prod[o][term][3][k][N] (canonical words, cn_l_behz_floor):
//   out[o][c][l] = sum_k prod[o][k][c][l] mod q_l (c = 0, 1: canonical words - the add0 / add1 of the key switch, which reads them where it then writes the result),
//   S[o][g0(l) + d] = sum_k dig_d(prod[o][k][2][l]),   dig_d(w) = (w >> dbc d) & (2^dbc - 1)   (exact doubles, where k_digit_gemm stores them).
// Workgroup = (512 coefficients, source limb l, output o); a thread owns two consecutive coefficients and reads them with 16-byte global loads (k_mod_switch), the
// limb-l words of all three components of a term: every product word comes from HBM exactly once - 3 K k N 8 bytes per output, the kernel's whole cost.  All ND
// digits of the limb live in the thread (ND >= every rl_dig[l], chosen by the launcher; <= 8).  A wider decomposition has to loop digit groups in here, not split
// them over workgroups: components 0 and 1 would be summed twice.  Terms in sets of four, two register sets ping-pong (k_digit_gemm): twelve 16-byte loads per
// thread in flight before the first use; whole pairs of sets run without a branch, the at most seven terms behind them in a tail; a load behind the last term repeats it.
// Accumulators are plain 64-bit integers: the host admits K (q_l - 1) < 2^64 for every l (components 0 and 1, one reduction mod q_l per stored word) and
// K (2^dbc - 1) < 2^52 (digit sums: exact as doubles, lazy values the KsDigits kernels take) - PRODUCT_SUM_MAX_TERMS / mul_sum_fused_ok, cn_mul_plan.h.
typedef uint64_t ps_u64x2 __attribute__((ext_vector_type(2)));
typedef double ps_f64x2 __attribute__((ext_vector_type(2)));
DEV uint64_t ps_reduce(uint64_t x, const DMod &m) {              // x mod q for any 64-bit x: r1 = floor(2^64 / q), the quotient estimate is low by at most one
    const uint64_t r = x - __umul64hi(x, m.r1) * m.q;
    return r >= m.q ? r - m.q : r;
}
// int32 words (k_product_sum<ND, int32_t>, K (2^dbc - 1) <= 2^31 - 1): the two sums of a thread leave as one 8-byte store.
typedef int32_t ps_i32x2 __attribute__((ext_vector_type(2)));
template <int ND, class... E>
__global__ void __launch_bounds__(256) k_product_sum(const uint64_t *__restrict__ prod_, uint32_t K, uint64_t *__restrict__ out_, typename DigitWord<E...>::type *__restrict__ S_,
                                                     const DevConsts *__restrict__ C) {
    typedef const NTT_GLOBAL ps_u64x2 *In;
    constexpr int PF = 4;
    const uint32_t n = C->n, k = C->k, n2 = n >> 1, tiles = n >> 9;
    uint32_t b = blockIdx.x;
    const uint32_t tile = b % tiles; b /= tiles;
    const uint32_t l = b % k, o = b / k;
    const uint32_t p = tile * 256 + threadIdx.x;                 // pair of coefficients
    const uint32_t dbc = (uint32_t)C->dbc, mask = (1u << dbc) - 1, nd = C->rl_dig[l];
    uint32_t g0 = 0;                                             // index of the first digit of limb l in the key
    for (uint32_t x = 0; x < l; x++) g0 += C->rl_dig[x];
    uint32_t sh[ND];
#pragma unroll
    for (int d = 0; d < ND; d++) sh[d] = min(dbc * (uint32_t)d, 63u);
    const size_t comp = (size_t)k * n2, unit = 3 * comp;         // in 16-byte pairs
    // a wave-uniform base per (term, component) and ONE 32-bit lane offset: the loads take the scalar-base form and need no address registers of their own
    const NTT_GLOBAL char *src = (const NTT_GLOBAL char *)prod_ + (size_t)o * K * unit * 16;
    const uint32_t lane_off = (l * n2 + p) * 16;                 // < 8 k N bytes
    uint64_t c0x = 0, c0y = 0, c1x = 0, c1y = 0, dx[ND], dy[ND];
#pragma unroll
    for (int d = 0; d < ND; d++) { dx[d] = 0; dy[d] = 0; }
    auto fetch = [&](ps_u64x2 (&x)[PF][3], uint32_t kk) {
#pragma unroll
        for (int t = 0; t < PF; t++) {
            const NTT_GLOBAL char *s = src + (size_t)min(kk + (uint32_t)t, K - 1) * unit * 16;
#pragma unroll
            for (int c = 0; c < 3; c++) x[t][c] = *(In)(s + (size_t)c * comp * 16 + lane_off);
        }
    };
    auto term = [&](const ps_u64x2 (&x)[3]) {
        c0x += x[0].x; c0y += x[0].y; c1x += x[1].x; c1y += x[1].y;
#pragma unroll
        for (int d = 0; d < ND; d++) { dx[d] += (uint32_t)(x[2].x >> sh[d]) & mask; dy[d] += (uint32_t)(x[2].y >> sh[d]) & mask; }
    };
    auto terms = [&](const ps_u64x2 (&x)[PF][3]) {                 // a whole set: no branch
#pragma unroll
        for (int t = 0; t < PF; t++) term(x[t]);
    };
    auto tail = [&](const ps_u64x2 (&x)[PF][3], uint32_t nv) {     // the first nv terms of a set (wave-uniform)
#pragma unroll
        for (int t = 0; t < PF; t++) if ((uint32_t)t < nv) term(x[t]);
    };
    {   // whole sets in pairs, two register sets ping-pong (k_digit_gemm); the at most seven terms behind the last pair in a tail of their own
        uint32_t kk = 0;
        ps_u64x2 xa[PF][3], xb[PF][3];
        fetch(xa, 0);
        for (uint32_t it = K / (2 * PF); it; it--, kk += 2 * PF) {
            fetch(xb, kk + PF);
            terms(xa);
            fetch(xa, kk + 2 * PF);
            terms(xb);
        }
        const uint32_t r = K - kk;                                   // 0 .. 7
        if (r > PF) fetch(xb, kk + PF);
        tail(xa, min(r, (uint32_t)PF));
        if (r > PF) tail(xb, r - PF);
    }
    const DMod m = C->q[l];
    typedef NTT_GLOBAL ps_u64x2 *Out;
    Out dst = (Out)out_ + (size_t)o * 2 * comp + (size_t)l * n2 + p;
    ps_u64x2 v;
    v.x = ps_reduce(c0x, m); v.y = ps_reduce(c0y, m); dst[0] = v;
    v.x = ps_reduce(c1x, m); v.y = ps_reduce(c1y, m); dst[comp] = v;
    typedef typename DigitWord<E...>::type SE;
    typedef typename std::conditional<std::is_same<SE, int32_t>::value, ps_i32x2, ps_f64x2>::type SV;
    typedef NTT_GLOBAL SV *OutS;
    OutS sd = (OutS)S_ + ((size_t)o * C->rl_tot + g0) * n2 + p;
#pragma unroll
    for (int d = 0; d < ND; d++)
        if ((uint32_t)d < nd) { SV w; w.x = (SE)dx[d]; w.y = (SE)dy[d]; sd[(size_t)d * n2] = w; }
}
