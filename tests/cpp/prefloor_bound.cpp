// cn_prefloor_bound_ok (cryptonets_amd/csrc/cn_policy.h) on the CPU: reads cases "R t n k q_0 .. q_(k-1) kb b_0 .. b_(kb-1)" (decimal, one per line) from the file
// named on the command line and prints the answer (0 / 1) per line.  tests/test_square_gemm_prefloor_model.py checks every answer against Python integers.
#include <cinttypes>
#include <cstdio>
#include "../../cryptonets_amd/csrc/cn_policy.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    uint64_t R, t, q[CN_MAXK], b[CN_MAXK + 1];
    uint32_t n, k, kb;
    while (fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu32, &R, &t, &n, &k) == 4) {
        if (k > CN_MAXK) return 3;
        for (uint32_t j = 0; j < k; j++) if (fscanf(f, "%" SCNu64, &q[j]) != 1) return 3;
        if (fscanf(f, "%" SCNu32, &kb) != 1 || kb > CN_MAXK + 1) return 3;
        for (uint32_t j = 0; j < kb; j++) if (fscanf(f, "%" SCNu64, &b[j]) != 1) return 3;
        printf("%d\n", (int)cn_prefloor_bound_ok(R, t, n, q, k, b, kb));
    }
    fclose(f);
    return 0;
}
