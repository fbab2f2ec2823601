// CPU run of the host-only policy header (cryptonets_amd/csrc/cn_policy.h) over real context tables (cn_tables.cpp), for tests/test_policy_table.py.
// Input (argv[1]), one parameter set per line of text:
//     name n t dbc gdbc k q_0 .. q_{k-1}          (hex moduli; k = 0: the default coefficient modulus of n)
// Output per set:
//     set name n t batching k kb
//     then for use_f64 = 0, 1 and every range asked below one line
//     r use_f64 base_off nmod f64ok light bits qmax policy m_0 .. m_{nmod-1}      (the moduli the program read out of the tables, hex like qmax)
#include "../../cryptonets_amd/csrc/cn_policy.h"
#include <cstdio>
#include <vector>

static const char *policy_name(int pol) {
    switch (pol) { case POL_U64: return "U64"; case POL_F64: return "F64"; case POL_F64L: return "F64L"; }
    return "?";
}
static void print_range(const DevConsts &hc, int use_f64, uint32_t base_off, uint32_t nmod) {
    const CnModRange r = cn_mod_range(hc, base_off, nmod);
    printf("r %d %u %u %d %d %d %llx %s", use_f64, base_off, nmod, (int)r.f64ok, (int)r.light, r.bits, (unsigned long long)r.qmax, policy_name(cn_policy(r, use_f64 != 0)));
    for (uint32_t m = base_off; m < base_off + nmod; m++)
        printf(" %llx", (unsigned long long)(m < hc.k ? hc.q[m].q : (m < hc.k + hc.kb ? hc.bsk[m - hc.k].q : hc.t.q)));
    printf("\n");
}

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
        printf("set %s %u %llu %u %u %u\n", name, hc.n, (unsigned long long)hc.t.q, hc.batching, hc.k, hc.kb);
        const uint32_t all = hc.k + hc.kb + (hc.batching ? 1 : 0);
        for (int use_f64 = 0; use_f64 < 2; use_f64++) {
            for (uint32_t j = 1; j <= hc.k; j++) print_range(hc, use_f64, 0, j);       // the q limbs (j = k) and every prefix of them (the lower levels of a chain)
            print_range(hc, use_f64, hc.k, hc.kb);
            print_range(hc, use_f64, 0, hc.k + hc.kb);
            if (hc.batching) print_range(hc, use_f64, hc.k + hc.kb, 1);
            for (uint32_t m = 0; m < all; m++) print_range(hc, use_f64, m, 1);
            print_range(hc, use_f64, 0, 0);                      // never asked today: no moduli, bits 0
        }
    }
    fclose(f);
    return 0;
}
