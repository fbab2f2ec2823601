// Launchers of k_mul_ptn_sum (cn_k_ptn.hip.h) for the three arithmetic policies (cn_policy.h) and the five register-radix sizes.
#include "cn_runtime.h"
#include "cn_policy.h"
#include "cn_k_ptn.hip.h"

// The form of a block per (size, policy), decided from the build report (tests/test_ptn_resources.py holds the register counts): NP = polynomials per block,
// WS = register pairs per chunk of loads in flight.  Both polynomials in one block (a plaintext limb read once per term) at every size that has a kernel: the FP64
// policies at N <= 8192 with chunks of four pairs, one ahead (128 registers), at N = 16384 with chunks of one pair, two ahead (126 / 128 of the 128 a 1024-thread
// workgroup leaves a thread; chunks of two pairs, one ahead, spill 9), the integer policy at N <= 8192 with chunks of two (163 - 168).  Instantiated where cn_plain_wide
// (cn_policy.h) says so: under the integer policy at N = 16384 it spills 50 registers with both polynomials and still 2 with one (the integer inverse transform alone takes 116).
template <int L, class AR> struct PtnForm {
    static constexpr bool f64 = std::is_same<typename AR::T, double>::value;
    static constexpr int NP = 2;
    static constexpr int WS = f64 ? (L == 14 ? 1 : 4) : 2;
    static constexpr int D = (f64 && L == 14) ? 2 : 1;                 // chunks requested ahead
    static constexpr bool has = cn_plain_wide(f64 ? POL_F64 : POL_U64, L);
};
template <class K> static int ptn_big_lds(K kern, size_t bytes) {
    HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
template <int L, class AR> static int ptn_attr(size_t bytes) {
    if constexpr (PtnForm<L, AR>::has) return ptn_big_lds(k_mul_ptn_sum<L, AR, PtnForm<L, AR>::NP, PtnForm<L, AR>::WS, PtnForm<L, AR>::D>, bytes);
    else return 0;
}
template <int L> static int ptn_attrs_l(size_t bytes) {
    CHECK((ptn_attr<L, ArU64>(bytes))); CHECK((ptn_attr<L, ArF64>(bytes))); CHECK((ptn_attr<L, ArF64L>(bytes)));
    return 0;
}
// the inverse transform's padded LDS image exceeds the default dynamic-LDS limit (N >= 8192)
int cn_l_ptn_set_attrs(uint32_t logn, size_t bytes) {
    if (logn == 13) return ptn_attrs_l<13>(bytes);
    if (logn == 14) return ptn_attrs_l<14>(bytes);
    return 0;
}
template <int L, class AR> static bool l_mul_ptn_sum(cn_ctx *c, const MulPlainSumLaunch &a) {
    if constexpr (!PtnForm<L, AR>::has) return false;
    else {
        constexpr int NP = PtnForm<L, AR>::NP;
        const uint32_t units = a.groups * (2 / NP);                        // blocks per limb; the block index is limb-major
        hipLaunchKernelGGL((k_mul_ptn_sum<L, AR, NP, PtnForm<L, AR>::WS, PtnForm<L, AR>::D>), dim3(units * c->hc.k), dim3(NttPlan<L>::NT), (size_t)ntt_lds_words(1u << L) * 8, c->stream, a.pt, a.ctn,
                           a.grp_off, a.slot, a.out, c->dc, a.accmax, units, a.order);
        return true;
    }
}
template <class AR> static bool by_size(cn_ctx *c, const MulPlainSumLaunch &a) {
    switch (c->hc.logn) {
        case 10: return l_mul_ptn_sum<10, AR>(c, a); case 11: return l_mul_ptn_sum<11, AR>(c, a); case 12: return l_mul_ptn_sum<12, AR>(c, a);
        case 13: return l_mul_ptn_sum<13, AR>(c, a); case 14: return l_mul_ptn_sum<14, AR>(c, a); default: return false;
    }
}
// a.pt: the NTT-form words of term 0 ([term][k][N]); a.accmax: the recentring interval (cn_ptn_sum_interval); a.order: the workgroup order ("ptn_order")
int cn_l_mul_ptn_sum(cn_ctx *c, int policy, const MulPlainSumLaunch &a) {
    if (!a.groups) return 0;
    const bool ok = policy == POL_U64 ? by_size<ArU64>(c, a) : (policy == POL_F64 ? by_size<ArF64>(c, a) : by_size<ArF64L>(c, a));
    if (!ok) return cn_fail(CN_ERR_ARG, "internal: cn_mul_plain_sum (NTT-form plaintexts) without a kernel for N = 2^%u", c->hc.logn);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    c->cnt.ptn_sum++;
    return 0;
}
