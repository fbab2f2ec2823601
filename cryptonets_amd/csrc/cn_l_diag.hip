// Launchers of k_mul_plain_sum (cn_k_diag.hip.h) for the three arithmetic policies (cn_policy.h) and the five register-radix sizes.
#include "cn_runtime.h"
#include "cn_policy.h"
#include "cn_k_diag.hip.h"

template <class K> static int diag_big_lds(K kern, size_t bytes) {
    HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
// instantiated where cn_plain_wide (cn_policy.h) says so: the plan (cn_plain_plan.h) composes the existing calls elsewhere
template <int L, class AR> static constexpr bool diag_has() { return cn_plain_wide(std::is_same<typename AR::T, uint64_t>::value ? POL_U64 : POL_F64, L); }
template <int L> static int diag_attrs_l(size_t bytes) {
    if constexpr (diag_has<L, ArU64>()) CHECK(diag_big_lds(k_mul_plain_sum<L, ArU64>, bytes));
    CHECK(diag_big_lds(k_mul_plain_sum<L, ArF64>, bytes)); CHECK(diag_big_lds(k_mul_plain_sum<L, ArF64L>, bytes));
    return 0;
}
// transforms whose padded LDS image exceeds the default dynamic-LDS limit (N >= 8192)
int cn_l_diag_set_attrs(uint32_t logn, size_t bytes) {
    if (logn == 13) return diag_attrs_l<13>(bytes);
    if (logn == 14) return diag_attrs_l<14>(bytes);
    return 0;
}
template <int L, class AR> static bool l_mul_plain_sum(cn_ctx *c, const MulPlainSumLaunch &a) {
    if constexpr (!diag_has<L, AR>()) return false;
    else hipLaunchKernelGGL((k_mul_plain_sum<L, AR>), dim3(a.groups * 2 * c->hc.k), dim3(NttPlan<L>::NT), (size_t)ntt_lds_words(1u << L) * 8, c->stream, a.pt, a.ctn, a.grp_off, a.slot, a.out,
                       c->dc, a.accmax);
    return true;
}
template <class AR> static bool by_size(cn_ctx *c, const MulPlainSumLaunch &a) {
    switch (c->hc.logn) {
        case 10: return l_mul_plain_sum<10, AR>(c, a); case 11: return l_mul_plain_sum<11, AR>(c, a); case 12: return l_mul_plain_sum<12, AR>(c, a);
        case 13: return l_mul_plain_sum<13, AR>(c, a); case 14: return l_mul_plain_sum<14, AR>(c, a); default: return false;
    }
}
int cn_l_mul_plain_sum(cn_ctx *c, int policy, const MulPlainSumLaunch &a) {
    if (!a.groups) return 0;
    const bool ok = policy == POL_U64 ? by_size<ArU64>(c, a) : (policy == POL_F64 ? by_size<ArF64>(c, a) : by_size<ArF64L>(c, a));
    if (!ok) return cn_fail(CN_ERR_ARG, "internal: cn_mul_plain_sum without a kernel for N = 2^%u", c->hc.logn);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    return 0;
}
