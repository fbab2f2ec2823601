// CPU run of the host-only key-switch planner (cryptonets_amd/csrc/cn_ks_plan.h) over real context tables (cn_tables.cpp), for tests/test_ks_plan.py.
// Input (argv[1]), one parameter set per line of text (the format of policy_table.cpp):
//     name n t dbc gdbc k q_0 .. q_{k-1}          (hex moduli; k = 0: the default coefficient modulus of n)
// Output per set:
//     set name n logn k rl_tot gk_tot dbc gdbc f64ok arena_small m_0 .. m_{k-1}
//     p key_f64 galois ks_wide ks_split14 ks_pair14 rr half_tables ks_xcd small cnt : form policy accmax xcd_cts arena_bytes twl whole writes_arena
//     r ks_wide rr ks_perm_fused small : perm_on_load at every count of the grid | largest (bound 64) largest (bound 3) | few_rotations at every count
//     x form key_f64 galois ks_xi shape : rc text          (shape: bit 0 ready-made digits, 1 perm_elt, 2 items, 3 next_elt)
// small = 1: arena_max is arena_small (the bytes of eight ciphertexts), else 24 GiB.  The block thresholds are the defaults, 10 and 160.
#include "../../cryptonets_amd/csrc/cn_ks_plan.h"
#include <cstdio>
#include <vector>

static const char *FORM[] = {"LEGACY", "FUSED", "DIGIT_MAC", "LIMB_MAC", "SPLIT14", "PAIR14"};
static const char *POLICY[] = {"U64", "F64", "F64L"};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
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
        const size_t arena_small = (size_t)8 * 2 * hc.k * hc.n * 8, arena_big = (size_t)24 << 30;
        printf("set %s %u %u %u %u %u %d %d %d %zu", name, hc.n, hc.logn, hc.k, hc.rl_tot, hc.gk_tot, hc.dbc, hc.gdbc, (int)f64ok, arena_small);
        for (uint32_t j = 0; j < hc.k; j++) printf(" %llx", (unsigned long long)hc.q[j].q);
        printf("\n");
        const uint32_t counts[] = {10 / hc.k, 10 / hc.k + 1, 160 / hc.k, 160 / hc.k + 1, 1, 3, 511, 512, 845, 5488};
        for (int key_f64 = 0; key_f64 <= (f64ok ? 1 : 0); key_f64++) for (int galois = 0; galois < 2; galois++) for (int wide = -1; wide <= 2; wide++)
        for (int split = 0; split < 2; split++) for (int pair = 0; pair < 2; pair++) for (int rr = 0; rr < 2; rr++) for (int half = 0; half < 2; half++)
        for (int xcd = 0; xcd < 3; xcd++) for (int small = 0; small < 2; small++) for (uint32_t cnt : counts) {
            const KsSwitches sw{wide, split, pair, xcd, 1, rr != 0, half != 0, 10, 160, small ? arena_small : arena_big};
            const KsPlan p = cn_ks_plan(hc, sw, key_f64 != 0, cnt, galois);
            printf("p %d %d %d %d %d %d %d %d %d %u : %s %s %u %u %zu %d %d %d\n", key_f64, galois, wide, split, pair, rr, half, xcd, small, cnt, FORM[p.form], POLICY[p.policy],
                   p.accmax, p.xcd_cts, p.arena_bytes, (int)p.twl, (int)p.whole, (int)ks_writes_arena(p));
        }
        for (int wide = -1; wide <= 2; wide++) for (int rr = 0; rr < 2; rr++) for (int perm = 0; perm < 2; perm++) for (int small = 0; small < 2; small++) {
            const KsSwitches sw{wide, 1, 1, 0, perm, rr != 0, true, 10, 160, small ? arena_small : arena_big};
            printf("r %d %d %d %d :", wide, rr, perm, small);
            for (uint32_t cnt : counts) printf(" %d", (int)ks_perm_on_load(hc, sw, cnt));
            printf(" | %u %u |", ks_largest_perm_on_load(hc, sw, 64), ks_largest_perm_on_load(hc, sw, 3));
            for (uint32_t cnt : counts) printf(" %d", (int)ks_few_rotations(hc, sw, cnt));
            printf("\n");
        }
        for (int form = KS_LEGACY; form <= KS_PAIR14; form++) for (int key_f64 = 0; key_f64 < 2; key_f64++) for (int galois = 0; galois < 2; galois++)
        for (uint32_t xi = 0; xi < 2; xi++) for (int shape = 0; shape < 16; shape++) {
            hc.ks_xi = xi;
            const KsPlan p{(KsForm)form, POL_U64, 0, 0, 0, false, false};
            const KsRefusal no = ks_refusal(hc, p, key_f64 != 0, galois, {(shape & 1) != 0, (shape & 2) != 0, (shape & 4) != 0, (shape & 8) != 0});
            printf("x %s %d %d %u %d : %d %s\n", FORM[form], key_f64, galois, xi, shape, no.rc, no ? no.msg : "-");
        }
        hc.ks_xi = 0;
    }
    fclose(f);
    return 0;
}
