// Prints the 19 thresholds of the device noise sampler as the library computes them (cryptonets_amd/csrc/cn_noise_table.h, host code only), one
// hexadecimal word per line: tests/test_sampler_model.py compares them with the exact values.
#include <cstdio>
#include "../../cryptonets_amd/csrc/cn_noise_table.h"

int main() {
    const NoiseTab t = cn_noise_table_compute();
    for (int i = 0; i < 19; i++) printf("%llx\n", (unsigned long long)t.thr[i]);
    return 0;
}
