// Launcher of the exact-FP64 modulus-switching kernel (cn_k_modswitch_f64.hip.h): one instantiation per (source limbs, target limbs) pair,
// 2 <= KS <= CN_MAXK; cn_l_mod_switch (cn_l_modswitch.hip) decides which form runs.
#include "cn_runtime.h"
#include "cn_k_modswitch_f64.hip.h"
#include <utility>

typedef void (*MsLaunch)(hipStream_t s, const uint64_t *src, uint64_t *dst, const DevConsts *C, uint32_t items, uint32_t logn);
template <int KS, int KD> static void launch_ms_f64(hipStream_t s, const uint64_t *src, uint64_t *dst, const DevConsts *C, uint32_t items, uint32_t logn) {
    const uint64_t threads = (uint64_t)items << (logn - 1);
    hipLaunchKernelGGL((k_mod_switch_f64<KS, KD>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, src, dst, C, items, logn);
}
template <int KS, int... KD> static constexpr void fill_row(MsLaunch (&row)[CN_MAXK + 1], std::integer_sequence<int, KD...>) {
    ((row[KD + 1] = &launch_ms_f64<KS, KD + 1>), ...);
}
template <int... KS> static constexpr void fill(MsLaunch (&t)[CN_MAXK + 1][CN_MAXK + 1], std::integer_sequence<int, KS...>) {
    (fill_row<KS + 2>(t[KS + 2], std::make_integer_sequence<int, KS + 1>{}), ...);
}
static const struct MsF64Table {
    MsLaunch t[CN_MAXK + 1][CN_MAXK + 1] = {};
    MsF64Table() { fill(t, std::make_integer_sequence<int, CN_MAXK - 1>{}); }
} ms_f64_table;

void cn_l_mod_switch_f64(hipStream_t s, const uint64_t *src, uint64_t *dst, const DevConsts *src_consts, uint32_t ks, uint32_t kd, uint32_t items, uint32_t logn) {
    ms_f64_table.t[ks][kd](s, src, dst, src_consts, items, logn);
}
