// cn_ptn_term_bound / cn_ptn_sum_interval (cryptonets_amd/csrc/cn_policy.h) on the CPU: reads moduli (decimal, one per line) from the file named on the command
// line and prints "q bound interval capped" per line.  tests/test_ptn_accumulate_bound.py recomputes every figure with Python integers.
#include <cinttypes>
#include <cstdio>
#include "../../cryptonets_amd/csrc/cn_policy.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    uint64_t q;
    while (fscanf(f, "%" SCNu64, &q) == 1) {
        bool capped = false;
        const uint32_t interval = cn_ptn_sum_interval(q, &capped);
        printf("%" PRIu64 " %" PRIu64 " %u %d\n", q, cn_ptn_term_bound(q), interval, (int)capped);
    }
    fclose(f);
    return 0;
}
