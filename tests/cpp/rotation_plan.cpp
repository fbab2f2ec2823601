// CPU run of the host-only rotation planner (cryptonets_amd/csrc/cn_rotation.h), for tests/test_rotation_plan.py.
// Input (argv[1]), one key set per line of text: name n count elt_0 .. elt_{count-1} (the Galois elements whose keys exist).  Output per set: "set name n", then for
// every step count in [-n/2 - 1, n/2 + 1] one line "s steps own plan elt_0 .. elt_{hops-1}" (own = cn_elt_of_step(n, steps); the elements in execution order) or
// "s steps own refused code text"
#include "../../cryptonets_amd/csrc/cn_rotation.h"
#include <cstdio>
#include <set>

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char name[64]; unsigned n, count;
    while (fscanf(f, "%63s %u %u", name, &n, &count) == 3) {
        std::set<uint64_t> have;
        for (unsigned i = 0; i < count; i++) { unsigned long long e; if (fscanf(f, "%llu", &e) != 1) return 3; have.insert(e); }
        printf("set %s %u\n", name, n);
        for (int steps = -(int)(n / 2) - 1; steps <= (int)(n / 2) + 1; steps++) {
            const CnRotPlan p = cn_rotation_plan(n, steps, [&](uint64_t e) { return have.count(e) != 0; });
            printf("s %d %llu ", steps, (unsigned long long)cn_elt_of_step(n, steps));
            if (p.rc) { printf("refused %d %s\n", p.rc, p.msg); continue; }
            printf("plan");
            for (uint32_t h = 0; h < p.hops; h++) printf(" %llu", (unsigned long long)p.elt[h]);
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
