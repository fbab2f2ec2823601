// Building a generalized-diagonal dense-layer plan on the device (cn_diag_scan, cn_diag_encode).  Included by cn_l_diagplan.hip.
//
// Both kernels read the slot-order weight matrix S [R][N] the entry points decode the row plaintexts into: S[r][x] = W[r, x] (residues mod t), of which only r < R and
// x < dim are ever touched - everything outside reads as zero without a memory access.  m = N / 2, slot s = h m + p.
//
//   k_diag_scan    flag (c, i) is set iff diag_(c,i)[h, p] = W[h m + p, (h ^ c) m + (p + i) mod m] has a non-zero slot: every non-zero W[h_r m + p_r, h_c m + x] sets
//                  flag (h_r ^ h_c, (x - p_r) mod m).  One streaming pass: a workgroup takes DSC_ROWS rows, its lanes run along the columns (16 bytes a lane), the 2 m flags
//                  live in LDS as bytes (N bytes) and are set with plain stores - every writer stores 1 - and the set ones go to the global array as plain byte stores of 1.
//   k_diag_gather  out[term e][index_map[h m + p]] = pre_(c,J,b)[h, p] = W[(h ^ c) m + (p - J) mod m, h m + (p + b) mod m] for the terms of one RUN: up to DGA_T terms with the
//                  same (c, J) and consecutive b = b0 + db.  A workgroup owns (run, h, DGA_T consecutive p = p0 + dp): element (dp, db) is column h m + (p0 + dp + b0 + db) mod m of
//                  matrix row (h ^ c) m + (p0 + dp - J) mod m - for one dp the `len` columns of a run are ONE contiguous row segment (two where it wraps at m), 256 bytes at
//                  len = 32.  Half a wave loads one segment and stores it as row dp of the LDS tile (pitch DGA_T + 1 words); then the lanes run along dp for one db, which the
//                  odd pitch keeps conflict-free (bank pair (dp + db) mod 32), and make the scattered 8-byte store k_encode_scatter makes.  A term with a non-zero value gets
//                  its byte nz[e] = 1, one plain store per half wave.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static constexpr uint32_t DSC_THREADS = 256, DSC_ROWS = 8;
static constexpr uint32_t DGA_THREADS = 256, DGA_T = 32, DGA_PITCH = DGA_T + 1;
// a run of the term list: terms [first, first + len) are (c, J, b0 + db), db < len <= DGA_T, b0 + len <= m
struct DiagRun { uint32_t c, J, b0, len, first; };

__device__ __forceinline__ void dsc_mark(uint8_t *flags, uint64_t w, uint32_t r, uint32_t x, uint32_t m, uint32_t logm) {
    if (w) flags[((((r >> logm) ^ (x >> logm)) & 1u) << logm) + ((x - r) & (m - 1))] = 1;
}
// grid: ceil(R / DSC_ROWS) workgroups of DSC_THREADS; dynamic LDS: N bytes (a whole number of words); nonzero [2][m] zeroed by the caller
__global__ void __launch_bounds__(DSC_THREADS) k_diag_scan(const uint64_t *__restrict__ S, uint32_t R, uint32_t dim, uint32_t logn, uint8_t *__restrict__ nonzero) {
    extern __shared__ uint32_t dsc_lds[];
    uint8_t *flags = (uint8_t *)dsc_lds;
    const uint32_t n = 1u << logn, logm = logn - 1, m = n >> 1, tid = threadIdx.x;
    const uint32_t words = (n + 3) / 4;
    for (uint32_t i = tid; i < words; i += DSC_THREADS) dsc_lds[i] = 0;
    __syncthreads();
    const uint32_t r0 = blockIdx.x * DSC_ROWS, r1 = min(r0 + DSC_ROWS, R);
    for (uint32_t r = r0; r < r1; r++) {
        const uint64_t *row = S + (size_t)r * n;
        for (uint32_t x = 2 * tid; x < dim; x += 2 * DSC_THREADS) {
            if (x + 1 < dim) {                                       // (N is even and a row starts at a multiple of N words: the pair is 16-byte aligned)
                const ulonglong2 w = *reinterpret_cast<const ulonglong2 *>(row + x);
                dsc_mark(flags, w.x, r, x, m, logm); dsc_mark(flags, w.y, r, x + 1, m, logm);
            } else dsc_mark(flags, row[x], r, x, m, logm);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < words; i += DSC_THREADS) {            // (flags at n and above, where n < 4, are never set)
        const uint32_t f = dsc_lds[i];
        if (f & 0x000000ffu) nonzero[4 * i] = 1;
        if (f & 0x0000ff00u) nonzero[4 * i + 1] = 1;
        if (f & 0x00ff0000u) nonzero[4 * i + 2] = 1;
        if (f & 0xff000000u) nonzero[4 * i + 3] = 1;
    }
}

// grid: (ceil(m / DGA_T), 2, runs) workgroups of DGA_THREADS; out: plaintext 0 of the launch ([term][N] words, every word of every term of the runs is written);
// nz: byte 0 of the launch, zeroed by the caller
__global__ void __launch_bounds__(DGA_THREADS) k_diag_gather(const uint64_t *__restrict__ S, uint32_t R, uint32_t dim, uint32_t logn, const DiagRun *__restrict__ runs,
                                                             const uint32_t *__restrict__ index_map, uint64_t *__restrict__ out, uint8_t *__restrict__ nz) {
    __shared__ uint64_t tile[DGA_T * DGA_PITCH];
    const uint32_t n = 1u << logn, m = n >> 1, tid = threadIdx.x;
    const DiagRun run = runs[blockIdx.z];
    const uint32_t h = blockIdx.y, p0 = blockIdx.x * DGA_T;
    {   // load: lane db of a half wave takes column db of the segment of row dp
        const uint32_t db = tid & (DGA_T - 1);
        for (uint32_t dp = tid / DGA_T; dp < DGA_T; dp += DGA_THREADS / DGA_T) {
            const uint32_t p = p0 + dp;
            if (p < m && db < run.len) {
                const uint32_t r = (h ^ run.c) * m + ((p - run.J) & (m - 1)), x = h * m + ((p + run.b0 + db) & (m - 1));
                tile[dp * DGA_PITCH + db] = (r < R && x < dim) ? S[(size_t)r * n + x] : 0;
            }
        }
    }
    __syncthreads();
    {   // store: lane dp of a half wave takes slot p0 + dp of term db
        const uint32_t dp = tid & (DGA_T - 1), p = p0 + dp;
        const uint32_t pos = p < m ? index_map[h * m + p] : 0;
        for (uint32_t db = tid / DGA_T; db < run.len; db += DGA_THREADS / DGA_T) {      // (uniform per half wave)
            const uint32_t e = run.first + db;
            uint64_t v = 0;
            if (p < m) { v = tile[dp * DGA_PITCH + db]; out[(size_t)e * n + pos] = v; }
            const uint64_t any = __ballot(v != 0);
            if (dp == 0 && ((any >> (tid & 32u)) & 0xffffffffull)) nz[e] = 1;
        }
    }
}
