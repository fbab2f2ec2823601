// CPU run of the host-only planner of the hoisted rotations (cn_ks_hoist_plan, cryptonets_amd/csrc/cn_ks_plan.h) over real context tables (cn_tables.cpp), for
// tests/test_ks_hoist_plan.py.  Input (argv[1]), one parameter set per line of text (the format of ks_plan.cpp):
//     name n t dbc gdbc k q_0 .. q_{k-1}          (hex moduli; k = 0: the default coefficient modulus of n)
// Output per set:
//     set name n logn k gk_tot gdbc f64ok m_0 .. m_{k-1}
//     h key_f64 rr n : rc policy accmax arena_bytes per_component blocks_ntt blocks_mac fwd_limbs inv_limbs | text          (text: the refusal, - = none)
//     b policy logn : built                          (cn_ks_hoist_built over every policy and log N = 9 .. 15, once, before the first set)
#include "../../cryptonets_amd/csrc/cn_ks_plan.h"
#include <cstdio>
#include <vector>

static const char *POLICY[] = {"U64", "F64", "F64L"};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    for (int pol = POL_U64; pol <= POL_F64L; pol++) for (uint32_t logn = 9; logn <= 15; logn++) printf("b %s %u : %d\n", POLICY[pol], logn, (int)cn_ks_hoist_built(pol, logn));
    char name[64]; unsigned n, k; unsigned long long t; int dbc, gdbc;
    while (fscanf(f, "%63s %u %llu %d %d %u", name, &n, &t, &dbc, &gdbc, &k) == 6) {
        if (k > CN_MAXK) return 3;
        uint64_t q[CN_MAXK];
        for (unsigned j = 0; j < k; j++) { unsigned long long x; if (fscanf(f, "%llx", &x) != 1) return 3; q[j] = x; }
        if (!k) { const int cnt = cn_default_coeff_modulus_impl(n, q); if (cnt <= 0) return 3; k = (unsigned)cnt; }
        static DevConsts hc;
        std::vector<uint64_t> tw((size_t)(2 * k + 3) * 4 * n);
        std::vector<double> twd((size_t)(2 * k + 3) * 2 * n);
        std::vector<uint32_t> index_map(n);
        char err[256];
        if (cn_build_consts(&hc, n, q, k, t, dbc, gdbc, tw.data(), index_map.data(), err, sizeof err)) { fprintf(stderr, "%s: %s\n", name, err); return 4; }
        cn_build_f64_tables(&hc, tw.data(), twd.data());
        const bool f64ok = cn_mod_range(hc, 0, hc.k).f64ok;
        printf("set %s %u %u %u %u %d %d", name, hc.n, hc.logn, hc.k, hc.gk_tot, hc.gdbc, (int)f64ok);
        for (uint32_t j = 0; j < hc.k; j++) printf(" %llx", (unsigned long long)hc.q[j].q);
        printf("\n");
        const uint32_t counts[] = {0, 1, 3, 12, 127, 0x20000000u};
        for (int key_f64 = 0; key_f64 < 2; key_f64++) for (int rr = 0; rr < 2; rr++) for (uint32_t cnt : counts) {
            const KsSwitches sw{-1, 1, 1, 0, 1, rr != 0, true, 10, 160, (size_t)24 << 30};
            const KsHoistPlan p = cn_ks_hoist_plan(hc, sw, key_f64 != 0, cnt);
            printf("h %d %d %u : %d %s %u %zu %d %u %u %llu %llu | %s\n", key_f64, rr, cnt, p.rc, POLICY[p.policy], p.accmax, p.arena_bytes, (int)p.per_component, p.blocks_ntt,
                   p.blocks_mac, (unsigned long long)p.fwd_limbs, (unsigned long long)p.inv_limbs, p.rc ? p.msg : "-");
        }
    }
    fclose(f);
    return 0;
}
