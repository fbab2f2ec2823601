// CPU run of the per-value arithmetic of cn_split_encode / cn_split_encrypt (cryptonets_amd/csrc/cn_k_split.hip.h: the functions the kernel k_crt_split calls), for
// tests/test_crt_split_model.py.  Input (argv[1]), one group per line of text:
//     P flags scale-as-hex-bits nvalues t_0 .. t_{P-1}
//     followed by nvalues lines, each the 64 bits of one input element (hex): a double, or an int64 under flag 1
// Output: per value its P residues (hex), or "bad" when the value does not fit.
#include "../../cryptonets_amd/csrc/cn_k_split.hip.h"
#include <cstdio>
#include <cstring>

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned P, flags; unsigned long long sbits, nvals;
    while (fscanf(f, "%u %u %llx %llu", &P, &flags, &sbits, &nvals) == 4) {
        if (P < 1 || P > CNJ_MAXP) return 3;
        DMod t[CNJ_MAXP];
        for (unsigned p = 0; p < P; p++) { unsigned long long x; if (fscanf(f, "%llx", &x) != 1 || x < 2 || (x >> 62)) return 3; t[p] = csp_dmod(x); }
        double scale; uint64_t sb = sbits; memcpy(&scale, &sb, 8);
        for (unsigned long long i = 0; i < nvals; i++) {
            unsigned long long bits;
            if (fscanf(f, "%llx", &bits) != 1) return 3;
            int64_t w;
            if (!csp_convert(bits, flags, scale, w)) { printf("bad\n"); continue; }
            for (unsigned p = 0; p < P; p++) printf("%llx%c", (unsigned long long)csp_residue(w, t[p]), p + 1 < P ? ' ' : '\n');
        }
    }
    fclose(f);
    return 0;
}
