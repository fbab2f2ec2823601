// Launcher of the seeded-ciphertext kernel (cn_k_seeded.hip.h): one instantiation per transform size and arithmetic policy.
#include "cn_runtime.h"
#include "cn_k_seeded.hip.h"

template <int L, class AR> static int launch_seeded(cn_ctx *c, const SeededArgs &a) {
    const size_t lds = (size_t)ntt_lds_words(1u << L) * 8;
    if (lds > 48 * 1024)                      // N >= 8192: the padded image exceeds the default dynamic-LDS limit (per device: set at every launch, a host-side table write)
        HIPCHK(hipFuncSetAttribute((const void *)k_seeded<L, AR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RngKey key; memcpy(key.k, a.a_seed32, 32);
    const uint32_t comps = a.expand_only ? 1 : 2;
    hipLaunchKernelGGL((k_seeded<L, AR>), dim3(a.cnt * comps * c->hc.k), dim3(NttPlan<L>::NT), lds, c->stream, a.out, a.ct_stride, c->dc, key, a.a_nonce, a.a_item0,
                       a.expand_only ? 1u : 0u, c->sk, a.noise, a.pt, a.pt_stride_words);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    c->st.ntt_inverse_limbs += (uint64_t)a.cnt * comps * c->hc.k;
    return 0;
}
template <class AR> static int by_size(cn_ctx *c, const SeededArgs &a) {
    switch (c->hc.logn) {
        case 10: return launch_seeded<10, AR>(c, a); case 11: return launch_seeded<11, AR>(c, a); case 12: return launch_seeded<12, AR>(c, a);
        case 13: return launch_seeded<13, AR>(c, a); case 14: return launch_seeded<14, AR>(c, a);
    }
    return cn_fail(CN_ERR_ARG, "seeded ciphertexts need 1024 <= N <= 16384");
}
// the policy of the context's coefficient moduli, chosen like the public-key encryption's (encrypt_chain)
int cn_l_seeded(cn_ctx *c, const SeededArgs &a) {
    if (!a.cnt) return 0;
    switch (cn_policy(cn_mod_range(c->hc, 0, c->hc.k), c->opt.f64)) {
        case POL_F64L: return by_size<ArF64L>(c, a);
        case POL_F64: return by_size<ArF64>(c, a);
    }
    return by_size<ArU64>(c, a);
}
