// Launchers of k_diag_scan and k_diag_gather (cn_k_diagplan.hip.h): the device side of cn_diag_scan / cn_diag_encode (cn_api.hip).
#include "cn_runtime.h"
#include "cn_k_diagplan.hip.h"

static_assert(sizeof(DiagRunHost) == sizeof(DiagRun), "the run table is uploaded as the host wrote it");

// flags [2][N / 2] bytes, zeroed by the caller, of the slot matrix S [R][N] (columns below dim)
int cn_l_diag_scan(cn_ctx *c, const uint64_t *S, uint32_t R, uint32_t dim, uint8_t *flags) {
    if (!R) return 0;
    hipLaunchKernelGGL(k_diag_scan, dim3((R + DSC_ROWS - 1) / DSC_ROWS), dim3(DSC_THREADS), (size_t)((c->hc.n + 3) & ~3u), c->stream, S, R, dim, c->hc.logn, flags);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    c->cnt.diag_scan++;
    return 0;
}
// the terms of `nruns` runs (device table; DiagRun::first counts from out / nz) into out [term][N], slot order -> SEAL's coefficient positions (index_map)
int cn_l_diag_gather(cn_ctx *c, const uint64_t *S, uint32_t R, uint32_t dim, const DiagRunHost *runs, uint32_t nruns, const uint32_t *index_map, uint64_t *out, uint8_t *nz) {
    if (!nruns) return 0;
    const uint32_t m = c->hc.n / 2;
    if (nruns > CN_DIAG_MAX_RUNS) return cn_fail(CN_ERR_ARG, "internal: %u runs in one launch of k_diag_gather", nruns);
    hipLaunchKernelGGL(k_diag_gather, dim3((m + DGA_T - 1) / DGA_T, 2, nruns), dim3(DGA_THREADS), 0, c->stream, S, R, dim, c->hc.logn, (const DiagRun *)runs, index_map, out, nz);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    c->cnt.diag_encode++;
    return 0;
}
