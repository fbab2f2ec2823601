// Packed rows (include/cnhip.h: cn_ct_upload_packed, cn_ct_download_packed): the wire form of a polynomial limb without padding bits.
//
//   b_j = bit_length(q_j).  The N residues of limb j are one little-endian bit stream: coefficient i is bits [i b_j, (i + 1) b_j) of the row, bit p of the row is bit
//   p % 64 of word p / 64, a row is N b_j / 64 words.  A packed ciphertext is its rows in [poly][limb] order, a batch [ciphertext][poly][limb].
//
// Both kernels are streaming kernels, one workgroup of 256 threads per TILE = 1024 coefficients of one row (N >= 1024 is a multiple of it): a tile is 16 b_j packed
// words (a multiple of 128 B, so every tile of every row starts 16-byte aligned) and 1024 array words.
//   * k_unpack_rows: the tile's packed words go HBM -> LDS with 16 B per lane (8 b_j <= 480 accesses, at most two per thread), then thread t extracts the coefficient
//     pairs (2 t, 2 t + 1) and (512 + 2 t, 513 + 2 t) - two LDS words per coefficient at an address that depends on the INDEX only - and, last of all, stores each
//     pair with one 16-byte access.  q_j < 2^b_j, so a stream can carry v >= q_j: the kernel stores v - q_j (< q_j, because 2^b_j <= 2 q_j) and ORs 1 into the call's flag word,
//     one atomic per workgroup that saw one.
//   * k_pack_rows: the tile's 1024 words go HBM -> LDS with 16 B per lane, then thread t builds the packed word pairs 2 u, 2 u + 1 (u = t, t + 256 < 8 b_j) from
//     the coefficients that overlap them (at most ceil(64 / b_j) + 1 per word) and stores each pair with one 16-byte access.  Words are masked to b_j bits.
// One instantiation serves every ring size and modulus: b_j and q_j come from DevConsts (workgroup-uniform: scalar registers).  No scratch, no flat accesses.
#pragma once
#include "cn_dev_common.hip.h"

static constexpr uint32_t PK_TILE = 1024, PK_NT = 256, PK_MAXB = 60;

DEV uint32_t pk_bits(uint64_t q) { return 64u - (uint32_t)__builtin_clzll(q); }
// where the workgroup works: (item, poly, limb, tile) from the block id, the packed words of its tile and the array words of its tile
struct PkPlace { uint32_t b; uint64_t q; size_t packed_off, arr_off; };
DEV PkPlace pk_place(const DevConsts *__restrict__ C, uint32_t polys, size_t item_words) {
    const uint32_t n = C->n, k = C->k, tiles = n / PK_TILE;
    uint32_t id = blockIdx.x;
    const uint32_t tile = id % tiles; id /= tiles;
    const uint32_t j = id % k; id /= k;
    const uint32_t p = id % polys, item = id / polys;
    uint32_t before = 0, all = 0;                             // bits per coefficient of the limbs in front of j, and of all limbs
    for (uint32_t i = 0; i < k; i++) { const uint32_t bi = pk_bits(C->q[i].q); all += bi; before += i < j ? bi : 0; }
    PkPlace w;
    w.q = C->q[j].q; w.b = pk_bits(w.q);
    w.packed_off = ((size_t)item * polys + p) * (n / 64) * all + (size_t)(n / 64) * before + (size_t)tile * (PK_TILE / 64) * w.b;
    w.arr_off = (size_t)item * item_words + ((size_t)p * k + j) * n + (size_t)tile * PK_TILE;
    return w;
}

// packed: [cnt][polys][limb] rows; arr: poly 0 of item 0, items item_words apart ([poly][limb][N]); grid = cnt * polys * k * N / 1024
__global__ void __launch_bounds__(PK_NT) k_unpack_rows(const uint64_t *__restrict__ packed, uint64_t *__restrict__ arr, size_t item_words, uint32_t polys,
                                                       const DevConsts *__restrict__ C, uint32_t *__restrict__ flag) {
    __shared__ __align__(16) uint64_t s[PK_TILE / 64 * PK_MAXB + 2];      // (a coefficient that ends on a word boundary still reads the word behind it: masked away)
    const PkPlace w = pk_place(C, polys, item_words);
    const uint32_t tid = threadIdx.x, b = w.b;
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(packed + w.packed_off);
#pragma unroll
    for (uint32_t r = 0; r < 2; r++) {
        const uint32_t u = tid + r * PK_NT;
        if (u < 8 * b) *reinterpret_cast<ulonglong2 *>(s + 2 * u) = src[u];
    }
    __syncthreads();
    const uint64_t mask = (1ull << b) - 1;
    int bad = 0;
    uint64_t v[4];                                                           // the pairs (2 t, 2 t + 1) and (512 + 2 t, 513 + 2 t)
#pragma unroll
    for (uint32_t e = 0; e < 4; e++) {
        const uint32_t bit = (2 * (tid + (e >> 1) * PK_NT) + (e & 1)) * b, wd = bit >> 6, sh = bit & 63;
        const uint64_t lo = s[wd], hi = s[wd + 1];
        uint64_t x = ((lo >> sh) | (sh ? hi << (64 - sh) : 0)) & mask;
        if (x >= w.q) { x -= w.q; bad = 1; }
        v[e] = x;
    }
    // Invariant: every LDS access - the flag's reduction included - comes before the two 16-byte stores, and nothing follows them.  The workgroup barriers of the
    // reduction sit between the last LDS read and the first store, so no schedule moves one across the other.
    if (__syncthreads_or(bad) && tid == 0) atomicOr(flag, 1u);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(arr + w.arr_off);
    dst[tid] = make_ulonglong2(v[0], v[1]);
    dst[tid + PK_NT] = make_ulonglong2(v[2], v[3]);
}

// the inverse: arr -> packed
__global__ void __launch_bounds__(PK_NT) k_pack_rows(const uint64_t *__restrict__ arr, size_t item_words, uint64_t *__restrict__ packed, uint32_t polys,
                                                     const DevConsts *__restrict__ C) {
    __shared__ __align__(16) uint64_t s[PK_TILE];
    const PkPlace w = pk_place(C, polys, item_words);
    const uint32_t tid = threadIdx.x, b = w.b;
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(arr + w.arr_off);
#pragma unroll
    for (uint32_t r = 0; r < 2; r++) {
        const uint32_t u = tid + r * PK_NT;
        *reinterpret_cast<ulonglong2 *>(s + 2 * u) = src[u];
    }
    __syncthreads();
    const uint64_t mask = (1ull << b) - 1;
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(packed + w.packed_off);
#pragma unroll
    for (uint32_t r = 0; r < 2; r++) {
        const uint32_t u = tid + r * PK_NT;
        if (u >= 8 * b) break;
        uint64_t o[2];
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t bit0 = (2 * u + h) * 64;            // the word covers bits [bit0, bit0 + 64) of the tile's stream
            uint64_t x = 0;
            for (uint32_t i = bit0 / b; i < PK_TILE && i * b < bit0 + 64; i++) {
                const uint64_t v = s[i] & mask;
                const int32_t pos = (int32_t)(i * b) - (int32_t)bit0;       // -59 .. 63
                x |= pos >= 0 ? v << pos : v >> -pos;
            }
            o[h] = x;
        }
        dst[u] = make_ulonglong2(o[0], o[1]);
    }
}
