// Thresholds of the noise sampler (sample_noise8, cn_dev_common.hip.h).  Host code only, nothing of HIP: the library computes the table once per process
// (cn_noise_table(), cn_client.hip) and tests/cpp/noise_table.cpp prints it for the comparison with the exact values (tests/test_sampler_model.py).
#pragma once
#include <cmath>
#include <cstdint>

struct NoiseTab { uint64_t thr[19]; };
// cumulative distribution of |x|, x ~ N(0, 3.2^2) conditioned on |x| <= 19.2 (SEAL 3.2: noise_standard_deviation 3.20, noise_max_deviation 6 sigma):
// thr[i] = floor(2^63 P(|x| < i + 1 | clipped)), long double erf
inline NoiseTab cn_noise_table_compute() {
    NoiseTab t;
    const long double sigma = 3.2L, root2 = 1.41421356237309504880168872420969808L, norm = erfl(19.2L / (sigma * root2));
    for (int i = 0; i < 19; i++) {
        const long double c = erfl((long double)(i + 1) / (sigma * root2)) / norm;             // P(|x| < i + 1 | clipped)
        t.thr[i] = c >= 1.0L ? 0x7fffffffffffffffull : (uint64_t)floorl(c * 9223372036854775808.0L);
    }
    return t;
}
