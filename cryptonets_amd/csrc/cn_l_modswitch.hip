// Launcher of the modulus-switching kernel (cn_k_modswitch.hip.h): one instantiation per (source limbs, target limbs) pair, 2 <= KS <= CN_MAXK.
#include "cn_runtime.h"
#include "cn_k_modswitch.hip.h"
#include <utility>

typedef void (*MsLaunch)(hipStream_t s, const uint64_t *src, uint64_t *dst, const DevConsts *C, uint32_t items, uint32_t logn);
template <int KS, int KD> static void launch_ms(hipStream_t s, const uint64_t *src, uint64_t *dst, const DevConsts *C, uint32_t items, uint32_t logn) {
    const uint64_t threads = (uint64_t)items << (logn - 1);
    hipLaunchKernelGGL((k_mod_switch<KS, KD>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, src, dst, C, items, logn);
}
// table[KS][KD] (KD < KS), null elsewhere
template <int KS, int... KD> static constexpr void fill_row(MsLaunch (&row)[CN_MAXK + 1], std::integer_sequence<int, KD...>) {
    ((row[KD + 1] = &launch_ms<KS, KD + 1>), ...);
}
template <int... KS> static constexpr void fill(MsLaunch (&t)[CN_MAXK + 1][CN_MAXK + 1], std::integer_sequence<int, KS...>) {
    (fill_row<KS + 2>(t[KS + 2], std::make_integer_sequence<int, KS + 1>{}), ...);
}
static const struct MsTable {
    MsLaunch t[CN_MAXK + 1][CN_MAXK + 1] = {};
    MsTable() { fill(t, std::make_integer_sequence<int, CN_MAXK - 1>{}); }
} ms_table;

void cn_l_mod_switch_f64(hipStream_t s, const uint64_t *src, uint64_t *dst, const DevConsts *src_consts, uint32_t ks, uint32_t kd, uint32_t items, uint32_t logn);

// The (KS, KD) pairs where the exact-FP64 kernel measured faster than the integer one on the MI355X (profiles/level_schedule_probe.txt): every
// drop of two or more primes, 0.41-0.89 of the integer time on the C3 and 9-limb chains.  A single drop stays on the integer path: both forms
// run at 1.5-1.8x the HBM floor there, within 0-5 % of each other.  CN_MS_F64_ALL=1 (the probe's A/B build only) makes every pair eligible.
#ifndef CN_MS_F64_ALL
#define CN_MS_F64_ALL 0
#endif
bool cn_ms_f64_pair(uint32_t ks, uint32_t kd) {
    if (CN_MS_F64_ALL) return true;
    return ks - kd >= 2;
}

// `items` (ciphertext, poly) pairs: src [items][ks][N] -> dst [items][kd][N] on the stream of `c` (the target context), constants of `src_consts`.
// f64: the FP64 form is allowed (the "f64" option is on and every modulus of the source chain is below 2^49); it runs where cn_ms_f64_pair holds.
// *ran_f64 (may be null): which form ran.
int cn_l_mod_switch(cn_ctx *c, const uint64_t *src, uint64_t *dst, const DevConsts *src_consts, uint32_t ks, uint32_t kd, uint32_t items, uint32_t logn,
                    bool f64, bool *ran_f64) {
    if (ks > CN_MAXK || kd == 0 || kd >= ks || logn < 1) return cn_fail(CN_ERR_ARG, "internal: mod switch %u -> %u limbs", ks, kd);
    const bool use_f64 = f64 && cn_ms_f64_pair(ks, kd);
    if (ran_f64) *ran_f64 = use_f64;
    if (!items) return 0;
    if (use_f64) cn_l_mod_switch_f64(c->stream, src, dst, src_consts, ks, kd, items, logn);
    else ms_table.t[ks][kd](c->stream, src, dst, src_consts, items, logn);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
