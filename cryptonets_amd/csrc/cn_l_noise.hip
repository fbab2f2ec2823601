// Launcher of the invariant-noise-norm kernel (cn_k_noise.hip.h): one instantiation per limb count, 1 <= K <= CN_MAXK.
#include "cn_runtime.h"
#include "cn_k_noise.hip.h"
#include <utility>

typedef void (*NnLaunch)(hipStream_t s, const uint64_t *c0, size_t ct_stride, const uint64_t *acc, uint64_t *out, const DevConsts *C, uint32_t count);
template <int K> static void launch_nn(hipStream_t s, const uint64_t *c0, size_t ct_stride, const uint64_t *acc, uint64_t *out, const DevConsts *C, uint32_t count) {
    hipLaunchKernelGGL((k_noise_norm<K>), dim3(count), dim3(NN_THREADS), 0, s, c0, ct_stride, acc, out, C);
}
template <int... K> static constexpr void fill(NnLaunch (&t)[CN_MAXK + 1], std::integer_sequence<int, K...>) {
    ((t[K + 1] = &launch_nn<K + 1>), ...);
}
static const struct NnTable {
    NnLaunch t[CN_MAXK + 1] = {};
    NnTable() { fill(t, std::make_integer_sequence<int, CN_MAXK>{}); }
} nn_table;

// `count` ciphertexts on c's stream: c0 of ciphertext i at c0 + i * ct_stride, acc [count][k][N] (decrypt_phase), out [count][k] words
int cn_l_noise_norm(cn_ctx *c, const uint64_t *c0, size_t ct_stride, const uint64_t *acc, uint64_t *out, uint32_t count) {
    const uint32_t k = c->hc.k;
    if (k < 1 || k > CN_MAXK) return cn_fail(CN_ERR_ARG, "internal: noise norm of %u limbs", k);
    if (!count) return 0;
    nn_table.t[k](c->stream, c0, ct_stride, acc, out, c->dc, count);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
