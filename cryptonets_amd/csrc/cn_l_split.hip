// Launcher of the request-path kernel (cn_k_split.hip.h): k_crt_split per number of plaintext primes P.
#include "cn_runtime.h"
#include "cn_k_split.hip.h"

template <int P> static void launch_split(hipStream_t st, dim3 grid, const uint64_t *values, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues, uint32_t flags,
                                          double scale, const SplitTab &tab, const uint32_t *index_map, uint32_t n, uint32_t *nz, uint32_t nz_stride, uint32_t *bad) {
    hipLaunchKernelGGL((k_crt_split<P>), grid, dim3(CSP_THREADS), 0, st, values, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad);
}

// `count` plaintexts of `nvalues` values on c's stream: element (ct, s) at values[ct stride_ct + s stride_slot] (device memory, 8 bytes each; flags: CN_SPLIT_*), row ct
// of context i at dst[i] + ct N; index_map may be null under CN_SPLIT_COEFF0.  nz [P][nz_stride] and bad [1] are zeroed by the caller and OR-ed into.
int cn_l_crt_split(cn_ctx *c, const void *values, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues, uint32_t flags, double scale,
                   const uint64_t *t, uint64_t *const *dst, uint32_t P, const uint32_t *index_map, uint32_t *nz, uint32_t nz_stride, uint32_t *bad) {
    const uint32_t n = c->hc.n;
    const uint32_t gy = (count + CSP_TC - 1) / CSP_TC;
    if (P < 1 || P > CNJ_MAXP || nvalues < 1 || nvalues > n || gy > 65535 || (flags & ~(CSP_I64 | CSP_COEFF0)) || (!(flags & CSP_COEFF0) && !index_map))
        return cn_fail(CN_ERR_ARG, "internal: split of %u x %u values over %u primes", count, nvalues, P);
    if (!count) return 0;
    SplitTab tab{};
    for (uint32_t i = 0; i < P; i++) {
        if (t[i] < 2 || (t[i] >> 62)) return cn_fail(CN_ERR_ARG, "internal: split modulo a plain modulus outside [2, 2^62)");
        tab.t[i] = csp_dmod(t[i]); tab.dst[i] = dst[i];
    }
    // the lanes run along the slots unless the plaintexts are the contiguous dimension of the input
    if (stride_ct == 1 && stride_slot != 1 && count > 1 && nvalues > 1) flags |= CSP_TILED;
    const dim3 grid((n + CSP_TS - 1) / CSP_TS, gy);
    const uint64_t *v = (const uint64_t *)values;
    switch (P) {
        case 1: launch_split<1>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
        case 2: launch_split<2>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
        case 3: launch_split<3>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
        case 4: launch_split<4>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
        case 5: launch_split<5>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
        case 6: launch_split<6>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
        case 7: launch_split<7>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
        default: launch_split<8>(c->stream, grid, v, stride_ct, stride_slot, count, nvalues, flags, scale, tab, index_map, n, nz, nz_stride, bad); break;
    }
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
