// Launchers of the packed-row kernels (cn_k_packed.hip.h): one instantiation each, whatever the ring size and the moduli.
#include "cn_runtime.h"
#include "cn_k_packed.hip.h"

size_t cn_packed_row_words(const cn_ctx *c) {           // words of one packed polynomial: (N / 64) * sum_j bit_length(q_j); 0 when the context has no packed form
    if (c->hc.n < PK_TILE) return 0;
    size_t bits = 0;
    for (uint32_t j = 0; j < c->hc.k; j++) bits += 64u - (uint32_t)__builtin_clzll(c->hc.q[j].q);
    return (size_t)(c->hc.n / 64) * bits;
}
static int packed_grid(cn_ctx *c, uint32_t cnt, uint32_t polys, uint32_t *grid) {
    if (c->hc.n < PK_TILE) return cn_fail(CN_ERR_ARG, "packed rows need N >= 1024");
    const uint64_t g = (uint64_t)cnt * polys * c->hc.k * (c->hc.n / PK_TILE);
    if (g >> 31) return cn_fail(CN_ERR_ARG, "too many packed rows for one call");
    *grid = (uint32_t)g;
    return 0;
}
int cn_l_unpack_rows(cn_ctx *c, const uint64_t *packed, uint64_t *arr, size_t item_words, uint32_t cnt, uint32_t polys, uint32_t *flag, hipStream_t stream) {
    if (!cnt) return 0;
    uint32_t grid; CHECK(packed_grid(c, cnt, polys, &grid));
    hipLaunchKernelGGL(k_unpack_rows, dim3(grid), dim3(PK_NT), 0, stream ? stream : c->stream, packed, arr, item_words, polys, c->dc, flag);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
int cn_l_pack_rows(cn_ctx *c, const uint64_t *arr, size_t item_words, uint64_t *packed, uint32_t cnt, uint32_t polys, hipStream_t stream) {
    if (!cnt) return 0;
    uint32_t grid; CHECK(packed_grid(c, cnt, polys, &grid));
    hipLaunchKernelGGL(k_pack_rows, dim3(grid), dim3(PK_NT), 0, stream ? stream : c->stream, arr, item_words, packed, polys, c->dc);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
