// Launcher of the Galois-key generation kernel (cn_k_keygen.hip.h): one instantiation per transform size and arithmetic policy.
#include "cn_runtime.h"
#include "cn_k_keygen.hip.h"

template <int L, class AR> static int launch_ksk_gen(cn_ctx *c, const KskGenArgs &a) {
    const size_t lds = (size_t)ntt_lds_words(1u << L) * 8;
    if (lds > 48 * 1024)                      // N >= 8192: the padded image exceeds the default dynamic-LDS limit (per device: set at every launch, a host-side table write)
        HIPCHK(hipFuncSetAttribute((const void *)k_ksk_gen<L, AR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    RngKey key; memcpy(key.k, c->rng_key, sizeof key.k);
    hipLaunchKernelGGL((k_ksk_gen<L, AR>), dim3(a.elts * a.tot * c->hc.k), dim3(NttPlan<L>::NT), lds, c->stream, (const KskOut *)a.outs, (const KskFactors *)a.fac, a.perm, a.noise,
                       c->sk, c->dc, key, a.seed, a.item0, a.tot, a.f64out ? 1u : 0u);
    HIPCHK(hipGetLastError()); cn_launch_count(c);
    c->st.ntt_forward_limbs += (uint64_t)a.elts * a.tot * c->hc.k;
    return 0;
}
template <class AR> static int by_size(cn_ctx *c, const KskGenArgs &a) {
    switch (c->hc.logn) {
        case 10: return launch_ksk_gen<10, AR>(c, a); case 11: return launch_ksk_gen<11, AR>(c, a); case 12: return launch_ksk_gen<12, AR>(c, a);
        case 13: return launch_ksk_gen<13, AR>(c, a); case 14: return launch_ksk_gen<14, AR>(c, a);
    }
    return cn_fail(CN_ERR_ARG, "cn_keygen_galois needs 1024 <= N <= 16384");
}
// the policy of the context's coefficient moduli, chosen like the encryption's (encrypt_chain)
int cn_l_ksk_gen(cn_ctx *c, const KskGenArgs &a) {
    if (!a.elts || !a.tot) return 0;
    switch (cn_policy(cn_mod_range(c->hc, 0, c->hc.k), c->opt.f64)) {
        case POL_F64L: return by_size<ArF64L>(c, a);
        case POL_F64: return by_size<ArF64>(c, a);
    }
    return by_size<ArU64>(c, a);
}
