// CPU run of the per-value arithmetic of cn_decrypt_join (cryptonets_amd/csrc/cn_k_join.hip.h: the functions the kernel k_crt_join calls), for
// tests/test_crt_join_model.py.  Input (argv[1]), one group per line of text:
//     P flags scale-as-hex-bits nvalues t_0 .. t_{P-1}
//     followed by nvalues lines of P residues (hex)
// Output: per group "W <words>", then per value its W words (hex, little-endian) and the bits of the double.
#include "../../cryptonets_amd/csrc/cn_k_join.hip.h"
#include <cstdio>
#include <cstring>
#include <vector>

template <int P, int W> static void run_group(const JoinTab &T, const std::vector<uint64_t> &res, size_t nvals) {
    for (size_t i = 0; i < nvals; i++) {
        uint64_t v[P], x[W];
        for (int p = 0; p < P; p++) v[p] = res[i * P + p];
        const double d = cnj_join_value<P, W>(v, T, x);
        uint64_t bits; memcpy(&bits, &d, 8);
        for (int w = 0; w < W; w++) printf("%016llx ", (unsigned long long)x[w]);
        printf("%016llx\n", (unsigned long long)bits);
    }
}
template <int P> static void run_p(const JoinTab &T, const std::vector<uint64_t> &res, size_t nvals) {
    switch (T.W) {
        case 1: run_group<P, 1>(T, res, nvals); break;
        case 2: run_group<P, 2>(T, res, nvals); break;
        case 3: run_group<P, 3>(T, res, nvals); break;
        default: run_group<P, 4>(T, res, nvals); break;
    }
}
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned P, flags; unsigned long long sbits, nvals;
    while (fscanf(f, "%u %u %llx %llu", &P, &flags, &sbits, &nvals) == 4) {
        if (P < 1 || P > CNJ_MAXP) return 3;
        uint64_t t[CNJ_MAXP];
        for (unsigned p = 0; p < P; p++) { unsigned long long x; if (fscanf(f, "%llx", &x) != 1) return 3; t[p] = x; }
        double scale; uint64_t sb = sbits; memcpy(&scale, &sb, 8);
        JoinTab T;
        if (cnj_build_tab(t, P, flags, scale, &T)) { printf("refused\n"); return 4; }
        std::vector<uint64_t> res((size_t)nvals * P);
        for (auto &r : res) { unsigned long long x; if (fscanf(f, "%llx", &x) != 1) return 3; r = x; }
        printf("W %u\n", T.W);
        switch (P) {
            case 1: run_p<1>(T, res, nvals); break; case 2: run_p<2>(T, res, nvals); break; case 3: run_p<3>(T, res, nvals); break; case 4: run_p<4>(T, res, nvals); break;
            case 5: run_p<5>(T, res, nvals); break; case 6: run_p<6>(T, res, nvals); break; case 7: run_p<7>(T, res, nvals); break; default: run_p<8>(T, res, nvals); break;
        }
    }
    fclose(f);
    return 0;
}
