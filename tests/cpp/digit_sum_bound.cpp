// cn_digit_sum_fits_i32 (cryptonets_amd/csrc/cn_policy.h) on the CPU: reads "sum_abs_w dbc" pairs (decimal) from the file named on the command line and prints
// "sum_abs_w dbc answer" per line.  tests/test_digit_sum_bound.py recomputes every answer with Python integers.
#include <cinttypes>
#include <cstdio>
#include "../../cryptonets_amd/csrc/cn_policy.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    uint64_t s; int dbc;
    while (fscanf(f, "%" SCNu64 " %d", &s, &dbc) == 2) printf("%" PRIu64 " %d %d\n", s, dbc, (int)cn_digit_sum_fits_i32(s, dbc));
    fclose(f);
    return 0;
}
