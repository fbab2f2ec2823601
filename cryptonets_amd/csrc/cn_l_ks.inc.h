// Launchers of the key-switch kernels for ONE arithmetic policy (KS_POLICY, KS_NAME): included by cn_l_ks_u64.hip, cn_l_ks_f64.hip
// and cn_l_ks_f64l.hip, so that the three policies compile in parallel.
#include "cn_runtime.h"
#include "cn_k_ks.hip.h"

typedef KS_POLICY AR;
static constexpr bool kF64 = std::is_same<typename AR::T, double>::value;

static constexpr size_t PAIR14_LDS = (size_t)ntt_lds_words(8192) * 8 + 65536;      // k_keyswitch_pair14: exchange image + 64 KiB (the parked next digit / staging window)
template <class K> static int big_lds(K kern, size_t bytes) {
    HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
// dynamic LDS of the fused key switch with LDS-resident forward twiddles: exchange image + table
template <int L> static size_t ks_twl_lds() { return ((size_t)ntt_lds_words(1u << L) + (1u << L)) * 8; }
// int32 digit sums: the rings do_keyswitch admits ready-made digits for (N <= 8192) - no instantiation of the 1024-thread kernels, which nobody launches
template <int L> static constexpr bool kDig32 = kF64 && L <= 13;
// the instantiations that read ready-made digits (KsArgs::dig), as doubles (DS = KsDigits<AR>) or int32 words (KsDigits<AR, int32_t>)
template <int L, class DS> static int set_attrs_dig(size_t bytes) {
    CHECK(big_lds(k_keyswitch_rr<L, DS, 1, false, false>, bytes));
    if constexpr (KsFwd<AR, L>::lds) CHECK(big_lds(k_keyswitch_rr<L, DS, 1, true, false>, ks_twl_lds<L>()));
    CHECK(big_lds(k_ks_digit_mac<L, DS>, bytes)); CHECK(big_lds(k_ks_limb_mac<L, DS>, bytes));
    return 0;
}
// hoisted rotations: the instantiations the planner's predicate admits (cn_ks_hoist_built, cn_ks_plan.h)
template <int L> static constexpr bool kHoist = cn_ks_hoist_built(kF64 ? POL_F64 : POL_U64, L);
// summed rotations: the instantiations the planner's predicate admits (cn_ks_sum_built, cn_ks_plan.h)
template <int L> static constexpr bool kSum = cn_ks_sum_built(kF64 ? POL_F64 : POL_U64, L);
template <int L> static constexpr bool kTerm = cn_ks_term_built(kF64 ? POL_F64 : POL_U64, L);
template <int L> static int set_attrs_l(size_t bytes) {
    CHECK(big_lds(k_keyswitch_rr<L, AR>, bytes)); CHECK(big_lds(k_keyswitch_rr<L, AR, 1, false, true>, bytes));
    if constexpr (KsFwd<AR, L>::lds) { CHECK(big_lds(k_keyswitch_rr<L, AR, 1, true>, ks_twl_lds<L>())); CHECK(big_lds(k_keyswitch_rr<L, AR, 1, true, true>, ks_twl_lds<L>())); }
    CHECK(big_lds(k_ks_digit_mac<L, AR>, bytes)); CHECK(big_lds(k_ks_limb_mac<L, AR>, bytes)); CHECK(big_lds(k_ks_sum_intt<L, AR>, bytes));
    if constexpr (kSum<L>) CHECK(big_lds(k_ks_sum_terms<L, AR>, bytes));
    if constexpr (kTerm<L>) CHECK(big_lds(k_ks_term_mac<L, AR>, bytes));
    if constexpr (kHoist<L>) { CHECK(big_lds(k_ks_digit_ntt<L, AR>, bytes)); CHECK(big_lds(k_ks_hoist_mac<L, AR, L == 14>, bytes)); }
    if constexpr (kF64) { CHECK((set_attrs_dig<L, KsDigits<AR>>(bytes))); if constexpr (kDig32<L>) CHECK((set_attrs_dig<L, KsDigits<AR, int32_t>>(bytes))); }
    return 0;
}
static int set_attrs(uint32_t logn, size_t bytes) {
    if constexpr (kF64) { if (logn == 12) { CHECK(big_lds(k_keyswitch_rr<12, AR, 1, true>, ks_twl_lds<12>())); CHECK(big_lds(k_keyswitch_rr<12, AR, 1, true, true>, ks_twl_lds<12>()));
                                           CHECK(big_lds(k_keyswitch_rr<12, KsDigits<AR>, 1, true, false>, ks_twl_lds<12>()));
                                           CHECK(big_lds(k_keyswitch_rr<12, KsDigits<AR, int32_t>, 1, true, false>, ks_twl_lds<12>())); } }   // N = 4096: image + LDS twiddle table = 66.5 KiB
    if (logn == 13) CHECK(set_attrs_l<13>(bytes));
    if (logn == 14) {
        CHECK(set_attrs_l<14>(bytes));
        if constexpr (kF64) {
            CHECK(big_lds(k_keyswitch_split14<AR>, (size_t)ntt_lds_words(8192) * 8)); CHECK(big_lds(k_keyswitch_split14<AR, true>, (size_t)ntt_lds_words(8192) * 8));
            CHECK(big_lds(k_keyswitch_pair14<AR, false, false>, PAIR14_LDS)); CHECK(big_lds(k_keyswitch_pair14<AR, true, false>, PAIR14_LDS));
            CHECK(big_lds(k_keyswitch_pair14<AR, false, true>, PAIR14_LDS)); CHECK(big_lds(k_keyswitch_pair14<AR, true, true>, PAIR14_LDS));
        }
    }
    return 0;
}
template <int L, bool XI, class ARS = AR> static void launch_fused_x(cn_ctx *c, const KsArgs &a) {
    const uint32_t tot = a.galois ? c->hc.gk_tot : c->hc.rl_tot;
    constexpr bool DIG = KsSrc<ARS>::dig;
    const uint64_t *tgt = DIG ? (const uint64_t *)a.dig : a.target;
    const size_t tstride = DIG ? (size_t)tot * c->hc.n : a.tstride;
    if constexpr (KsFwd<AR, L>::lds) {
        if (a.plan.twl) {
            hipLaunchKernelGGL((k_keyswitch_rr<L, ARS, 1, true, XI>), dim3(a.cnt * c->hc.k), dim3(NttPlan<L>::NT), ks_twl_lds<L>(), c->stream, tgt, tstride, a.add0, a.add1,
                               a.astride, (const void *)a.key, a.out, c->dc, a.galois, a.plan.accmax, a.extra, a.xstride, a.out_tab, a.plan.xcd_cts);
            return;
        }
    }
    hipLaunchKernelGGL((k_keyswitch_rr<L, ARS, 1, false, XI>), dim3(a.cnt * c->hc.k), dim3(NttPlan<L>::NT), (size_t)ntt_lds_words(1u << L) * 8, c->stream, tgt, tstride,
                       a.add0, a.add1, a.astride, (const void *)a.key, a.out, c->dc, a.galois, a.plan.accmax, a.extra, a.xstride, a.out_tab, a.plan.xcd_cts);
}
template <int L> static void launch_fused(cn_ctx *c, const KsArgs &a) {
    if constexpr (kF64) {
        if (a.dig) {
            if constexpr (kDig32<L>) { if (a.dig_i32) { launch_fused_x<L, false, KsDigits<AR, int32_t>>(c, a); return; } }
            launch_fused_x<L, false, KsDigits<AR>>(c, a); return;
        }
    }
    if (c->hc.ks_xi) launch_fused_x<L, true>(c, a);
    else launch_fused_x<L, false>(c, a);
}
// first launch of the two-launch forms from ready-made digit polynomials (DS: KsDigits<AR> or KsDigits<AR, int32_t>)
template <int L, class DS> static void launch_dig_mac(cn_ctx *c, const KsArgs &a, uint32_t tot, size_t lds) {
    const uint32_t k = c->hc.k;
    if (a.plan.form == KS_LIMB_MAC) hipLaunchKernelGGL((k_ks_limb_mac<L, DS>), dim3(a.cnt * k * k), dim3(NttPlan<L>::NT), lds, c->stream, (const uint64_t *)a.dig, (size_t)tot * c->hc.n,
                                        (const void *)a.key, c->ks_part, c->dc, a.galois, a.plan.accmax, 0u, (const KsItem *)nullptr);
    else hipLaunchKernelGGL((k_ks_digit_mac<L, DS>), dim3(a.cnt * tot * k), dim3(NttPlan<L>::NT), lds, c->stream, (const uint64_t *)a.dig, (size_t)tot * c->hc.n,
                            (const void *)a.key, c->ks_part, c->dc, a.galois, tot, 0u, (const KsItem *)nullptr);
}
template <int L> static void launch_two_phase(cn_ctx *c, const KsArgs &a) {
    const uint32_t tot = a.galois ? c->hc.gk_tot : c->hc.rl_tot, k = c->hc.k;
    const size_t lds = (size_t)ntt_lds_words(1u << L) * 8;
    const bool limb = a.plan.form == KS_LIMB_MAC;
    bool dig = false;
    if constexpr (kF64) dig = a.dig != nullptr;
    if (dig) {                      // ready-made digit polynomials: the same two forms, first launch from KsArgs::dig
        if constexpr (kF64) {
            bool i32 = false;
            if constexpr (kDig32<L>) i32 = a.dig_i32;
            if constexpr (kDig32<L>) { if (i32) launch_dig_mac<L, KsDigits<AR, int32_t>>(c, a, tot, lds); }
            if (!i32) launch_dig_mac<L, KsDigits<AR>>(c, a, tot, lds);
        }
        hipLaunchKernelGGL((k_ks_sum_intt<L, AR>), dim3(a.cnt * k * 2), dim3(NttPlan<L>::NT), lds, c->stream, (const void *)c->ks_part, a.add0, a.add1, a.astride,
                           a.out, c->dc, limb ? k : tot, limb ? 0xffffffffu : a.plan.accmax, a.extra, a.xstride, a.out_tab, a.perm_elt, a.items);
    } else if (limb) {              // one partial per (ct, source limb): k*k workgroups per ciphertext, k partials to sum
        hipLaunchKernelGGL((k_ks_limb_mac<L, AR>), dim3(a.cnt * k * k), dim3(NttPlan<L>::NT), lds, c->stream, a.target, a.tstride, (const void *)a.key, c->ks_part,
                           c->dc, a.galois, a.plan.accmax, a.perm_elt, a.items);
        hipLaunchKernelGGL((k_ks_sum_intt<L, AR>), dim3(a.cnt * k * 2), dim3(NttPlan<L>::NT), lds, c->stream, (const void *)c->ks_part, a.add0, a.add1, a.astride,
                           a.out, c->dc, k, 0xffffffffu, a.extra, a.xstride, a.out_tab, a.perm_elt, a.items);
    } else {                        // one partial per (ct, digit)
        hipLaunchKernelGGL((k_ks_digit_mac<L, AR>), dim3(a.cnt * tot * k), dim3(NttPlan<L>::NT), lds, c->stream, a.target, a.tstride, (const void *)a.key, c->ks_part,
                           c->dc, a.galois, tot, a.perm_elt, a.items);
        hipLaunchKernelGGL((k_ks_sum_intt<L, AR>), dim3(a.cnt * k * 2), dim3(NttPlan<L>::NT), lds, c->stream, (const void *)c->ks_part, a.add0, a.add1, a.astride,
                           a.out, c->dc, tot, a.plan.accmax, a.extra, a.xstride, a.out_tab, a.perm_elt, a.items);
    }
    cn_launch_count(c);
}
template <int L> static void launch_rr(cn_ctx *c, const KsArgs &a) {
    if (ks_two_launch(a.plan.form)) { launch_two_phase<L>(c, a); return; }
    launch_fused<L>(c, a);
}
// N = 16384 as two 8192-point halves per limb: partial halves into c->ks_part (the caller runs k_ks_combine14 behind it)
static bool split14(cn_ctx *c, const KsArgs &a) {
    if constexpr (kF64) {
        if (c->hc.ks_xi)
            hipLaunchKernelGGL((k_keyswitch_split14<AR, true>), dim3(a.cnt * c->hc.k * 2), dim3(NttPlan<13>::NT), (size_t)ntt_lds_words(8192) * 8, c->stream, a.target, a.tstride,
                               (const void *)a.key, (uint64_t *)c->ks_part, c->dc, a.galois, a.plan.accmax);
        else
            hipLaunchKernelGGL((k_keyswitch_split14<AR>), dim3(a.cnt * c->hc.k * 2), dim3(NttPlan<13>::NT), (size_t)ntt_lds_words(8192) * 8, c->stream, a.target, a.tstride,
                               (const void *)a.key, (uint64_t *)c->ks_part, c->dc, a.galois, a.plan.accmax);
        return true;
    }
    return false;
}
// N = 16384 in one launch: both halves per (ciphertext, output limb) workgroup (k_keyswitch_pair14); a.target = sigma(c1) for rotations
template <bool XI, bool WHOLE> static void launch_pair14(cn_ctx *c, const KsArgs &a) {
    if constexpr (kF64)
        hipLaunchKernelGGL((k_keyswitch_pair14<AR, XI, WHOLE>), dim3(a.cnt * c->hc.k), dim3(NttPlan<13>::NT), PAIR14_LDS, c->stream, a.target, a.tstride, a.add0, a.add1, a.astride,
                           (const void *)a.key, a.out, (double *)c->ks_part, c->dc, a.galois, a.plan.accmax, a.extra, a.xstride, a.out_tab, a.perm_elt, a.next_elt, a.next_out, a.plan.xcd_cts);
}
static bool pair14(cn_ctx *c, const KsArgs &a) {
    if constexpr (kF64) {
        if (c->hc.ks_xi) { if (a.plan.whole) launch_pair14<true, true>(c, a); else launch_pair14<true, false>(c, a); }
        else { if (a.plan.whole) launch_pair14<false, true>(c, a); else launch_pair14<false, false>(c, a); }
        return true;
    }
    return false;
}
// the kernels of a.plan.form (cn_ks_plan.h); false: this policy or ring size has no instantiation of it
static bool launch(cn_ctx *c, const KsArgs &a) {
    switch (a.plan.form) {
        case KS_LEGACY: return false;           // (k_keyswitch is launched by do_keyswitch itself)
        case KS_SPLIT14: return split14(c, a);
        case KS_PAIR14: return pair14(c, a);
        default: break;
    }
    switch (c->hc.logn) {
        case 10: launch_rr<10>(c, a); return true;
        case 11: launch_rr<11>(c, a); return true;
        case 12: launch_rr<12>(c, a); return true;
        case 13: launch_rr<13>(c, a); return true;
        case 14: launch_rr<14>(c, a); return true;
        default: return false;
    }
}
// hoisted rotations: the digit transforms of the one input into c->ks_part, then every rotation's permuted read, key product and inverse transforms (KsHoistPlan;
// its per_component is N = 16384, which is the kernel's template argument here)
template <int L> static bool launch_hoist(cn_ctx *c, const KsHoistArgs &a) {
    if constexpr (kHoist<L>) {
        const size_t lds = (size_t)ntt_lds_words(1u << L) * 8, kn = (size_t)c->hc.k << L;
        hipLaunchKernelGGL((k_ks_digit_ntt<L, AR>), dim3(a.plan.blocks_ntt), dim3(NttPlan<L>::NT), lds, c->stream, a.in + kn, c->ks_part, c->dc, c->hc.gk_tot);
        hipLaunchKernelGGL((k_ks_hoist_mac<L, AR, L == 14>), dim3(a.plan.blocks_mac), dim3(NttPlan<L>::NT), lds, c->stream, (const void *)c->ks_part, a.in, a.items, c->dc, c->hc.gk_tot,
                           a.plan.accmax);
        cn_launch_count(c, 2);
        return true;
    }
    return false;
}
static bool hoist(cn_ctx *c, const KsHoistArgs &a) {
    switch (c->hc.logn) {
        case 10: return launch_hoist<10>(c, a);
        case 11: return launch_hoist<11>(c, a);
        case 12: return launch_hoist<12>(c, a);
        case 13: return launch_hoist<13>(c, a);
        case 14: return launch_hoist<14>(c, a);
        default: return false;
    }
}
// summed rotations: the partial products of every rotated term into c->ks_part (per digit, per source limb or per term, operand, key and element from the KsItem table, the automorphism applied on load), then per (output, limb, component) their sum, one inverse transform and the addends (KsSumPlan)
template <int L> static bool launch_sum(cn_ctx *c, const KsSumArgs &a) {
    if constexpr (kSum<L>) {
        const size_t lds = (size_t)ntt_lds_words(1u << L) * 8;
        if (a.plan.form == KS_SUM_LIMB)
            hipLaunchKernelGGL((k_ks_limb_mac<L, AR>), dim3(a.plan.blocks_mac), dim3(NttPlan<L>::NT), lds, c->stream, (const uint64_t *)nullptr, (size_t)0, (const void *)nullptr, c->ks_part,
                               c->dc, 1, a.plan.accmax, 0u, a.items);
        else if (a.plan.form == KS_SUM_DIGIT)
            hipLaunchKernelGGL((k_ks_digit_mac<L, AR>), dim3(a.plan.blocks_mac), dim3(NttPlan<L>::NT), lds, c->stream, (const uint64_t *)nullptr, (size_t)0, (const void *)nullptr, c->ks_part,
                               c->dc, 1, c->hc.gk_tot, 0u, a.items);
        else if (a.plan.form == KS_SUM_TERM) {
            if constexpr (kTerm<L>) hipLaunchKernelGGL((k_ks_term_mac<L, AR>), dim3(a.plan.blocks_mac), dim3(NttPlan<L>::NT), lds, c->stream, c->ks_part, c->dc, a.plan.accmax, a.items);
            else return false;
        } else return false;
        hipLaunchKernelGGL((k_ks_sum_terms<L, AR>), dim3(a.plan.blocks_sum), dim3(NttPlan<L>::NT), lds, c->stream, (const void *)c->ks_part, a.outs, a.terms, c->dc, a.plan.partials,
                           a.plan.settle);
        cn_launch_count(c, 2);
        return true;
    }
    return false;
}
static bool sum(cn_ctx *c, const KsSumArgs &a) {
    switch (c->hc.logn) {
        case 10: return launch_sum<10>(c, a);
        case 11: return launch_sum<11>(c, a);
        case 12: return launch_sum<12>(c, a);
        case 13: return launch_sum<13>(c, a);
        case 14: return launch_sum<14>(c, a);
        default: return false;
    }
}
#ifndef __HIP_DEVICE_COMPILE__      // host-side table (in the device pass a const global would be emitted as device data)
extern const KsOps KS_NAME = {set_attrs, launch, hoist, sum};
#endif
