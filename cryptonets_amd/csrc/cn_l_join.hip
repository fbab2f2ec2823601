// Launchers of the reply-path kernels (cn_k_join.hip.h): k_crt_join per (plaintext primes P, words W), k_join_argmax per W.
#include "cn_runtime.h"
#include "cn_k_join.hip.h"
#include <utility>

typedef void (*JoinLaunch)(hipStream_t s, const uint64_t *plain, const uint32_t *index_map, const JoinTab *tab, double *values, uint64_t *words, uint32_t n, uint32_t count, uint32_t nslots);
template <int P, int W> static void launch_join(hipStream_t s, const uint64_t *plain, const uint32_t *index_map, const JoinTab *tab, double *values, uint64_t *words, uint32_t n,
                                                uint32_t count, uint32_t nslots) {
    const uint64_t total = (uint64_t)count * nslots;
    hipLaunchKernelGGL((k_crt_join<P, W>), dim3((unsigned)((total + CNJ_THREADS - 1) / CNJ_THREADS)), dim3(CNJ_THREADS), 0, s, plain, index_map, tab, values, words, n, count, nslots);
}
template <int P, int... W> static constexpr void fill_row(JoinLaunch (&row)[CNJ_MAXW + 1], std::integer_sequence<int, W...>) {
    ((row[W + 1] = &launch_join<P, W + 1>), ...);
}
template <int... P> static constexpr void fill(JoinLaunch (&t)[CNJ_MAXP + 1][CNJ_MAXW + 1], std::integer_sequence<int, P...>) {
    (fill_row<P + 1>(t[P + 1], std::make_integer_sequence<int, CNJ_MAXW>{}), ...);
}
static const struct JoinTable {
    JoinLaunch t[CNJ_MAXP + 1][CNJ_MAXW + 1] = {};
    JoinTable() { fill(t, std::make_integer_sequence<int, CNJ_MAXP>{}); }
} join_table;

// `count` x `nslots` values on c's stream: plain [P][count][N] (all of it behind c's stream by now), tab = the call's JoinTab on the device; values / words may be null
int cn_l_crt_join(cn_ctx *c, const uint64_t *plain, const uint32_t *index_map, const void *tab, uint32_t P, uint32_t W, double *values, uint64_t *words, uint32_t count, uint32_t nslots) {
    if (P < 1 || P > CNJ_MAXP || W < 1 || W > CNJ_MAXW || nslots < 1 || nslots > c->hc.n) return cn_fail(CN_ERR_ARG, "internal: join of %u primes in %u words over %u slots", P, W, nslots);
    if (!count) return 0;
    join_table.t[P][W](c->stream, plain, index_map, (const JoinTab *)tab, values, words, c->hc.n, count, nslots);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
// argmax[s] = the lowest ciphertext whose words [count][nslots][W] are largest in slot s
int cn_l_join_argmax(cn_ctx *c, const uint64_t *words, uint32_t W, int32_t *argmax, uint32_t count, uint32_t nslots) {
    if (W < 1 || W > CNJ_MAXW) return cn_fail(CN_ERR_ARG, "internal: arg max over %u words", W);
    if (!count || !nslots) return 0;
    const dim3 grid((nslots + CNJ_THREADS - 1) / CNJ_THREADS), block(CNJ_THREADS);
    switch (W) {
        case 1: hipLaunchKernelGGL((k_join_argmax<1>), grid, block, 0, c->stream, words, argmax, count, nslots); break;
        case 2: hipLaunchKernelGGL((k_join_argmax<2>), grid, block, 0, c->stream, words, argmax, count, nslots); break;
        case 3: hipLaunchKernelGGL((k_join_argmax<3>), grid, block, 0, c->stream, words, argmax, count, nslots); break;
        default: hipLaunchKernelGGL((k_join_argmax<4>), grid, block, 0, c->stream, words, argmax, count, nslots); break;
    }
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
