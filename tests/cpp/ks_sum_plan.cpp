// CPU run of the host-only planner of the summed rotations (cn_ks_sum_plan, cryptonets_amd/csrc/cn_ks_plan.h) over real context tables (cn_tables.cpp), for
// tests/test_ks_sum_plan.py.  Input (argv[1]), one parameter set per line of text (the format of ks_plan.cpp):
//     name n t dbc gdbc k q_0 .. q_{k-1}          (hex moduli; k = 0: the default coefficient modulus of n)
// Output per set:
//     set name n logn k gk_tot gdbc f64ok m_0 .. m_{k-1}
//     s key_f64 rr arena_max rotated : form policy accmax settle partials arena_bytes blocks_mac blocks_sum fwd_limbs inv_limbs | text
//                                                            (text: why it composes, - = it does not)
//     w key_f64 : settle milli_q worst_hi worst_lo          (the exact worst case of k_ks_sum_terms' lazy sums at the widest modulus, times 2000, as two 64-bit halves)
//     b policy logn : built term_built                      (cn_ks_sum_built / cn_ks_term_built over every policy and log N = 9 .. 15, once, before the first set)
// Every plan is asked with terms = rotated + 2 and outputs = (rotated + 1) / 2 (0 rotated terms: 1 output).
#include "../../cryptonets_amd/csrc/cn_ks_plan.h"
#include <cstdio>
#include <vector>

static const char *POLICY[] = {"U64", "F64", "F64L"};
static const char *FORM[] = {"compose", "digit", "limb", "term"};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    for (int pol = POL_U64; pol <= POL_F64L; pol++) for (uint32_t logn = 9; logn <= 15; logn++) printf("b %s %u : %d %d\n", POLICY[pol], logn, (int)cn_ks_sum_built(pol, logn), (int)cn_ks_term_built(pol, logn));
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
        const CnModRange qr = cn_mod_range(hc, 0, hc.k);
        printf("set %s %u %u %u %u %d %d", name, hc.n, hc.logn, hc.k, hc.gk_tot, hc.gdbc, (int)qr.f64ok);
        for (uint32_t j = 0; j < hc.k; j++) printf(" %llx", (unsigned long long)hc.q[j].q);
        printf("\n");
        const uint32_t counts[] = {0, 1, 3, 4, 40, 53, 54, 126};
        const size_t arenas[] = {(size_t)24 << 30, (size_t)3 << 20, (size_t)1 << 20};
        for (int key_f64 = 0; key_f64 < 2; key_f64++) for (int rr = 0; rr < 2; rr++) for (size_t arena : arenas) for (uint32_t rot : counts) {
            const KsSwitches sw{-1, 1, 1, 0, 1, rr != 0, true, 10, 160, arena};
            const KsSumPlan p = cn_ks_sum_plan(hc, sw, key_f64 != 0, rot + 2, rot, rot ? (rot + 1) / 2 : 1);
            printf("s %d %d %zu %u : %s %s %u %u %u %zu %u %u %llu %llu | %s\n", key_f64, rr, arena, rot, FORM[p.form], POLICY[p.policy], p.accmax, p.settle, p.partials, p.arena_bytes,
                   p.blocks_mac, p.blocks_sum, (unsigned long long)p.fwd_limbs, (unsigned long long)p.inv_limbs, p.why ? p.why : "-");
        }
        for (int key_f64 = 0; key_f64 < 2; key_f64++) {
            const KsSwitches sw{-1, 1, 1, 0, 1, true, true, 10, 160, (size_t)24 << 30};
            const KsSumPlan p = cn_ks_sum_plan(hc, sw, key_f64 != 0, 1, 1, 1);
            // a recentred sum (|x| <= q / 2) and `settle` partials of at most KS_SUM_TERM_MILLI_Q / 1000 q each, times 2000: q (1000 + 2 settle milli_q)
            const unsigned __int128 worst = (unsigned __int128)qr.qmax * (1000 + 2 * (unsigned __int128)p.settle * KS_SUM_TERM_MILLI_Q);
            printf("w %d : %u %u %llu %llu\n", key_f64, p.settle, KS_SUM_TERM_MILLI_Q, (unsigned long long)(worst >> 64), (unsigned long long)worst);
        }
    }
    fclose(f);
    return 0;
}
