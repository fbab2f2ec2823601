// CPU run of the host-only plaintext-product planner (cryptonets_amd/csrc/cn_plain_plan.h) over real context tables (cn_tables.cpp), for tests/test_plain_plan.py.
// Input (argv[1]), one parameter set per line of text (the format of policy_table.cpp):
//     name n t dbc gdbc k q_0 .. q_{k-1}          (hex moduli; k = 0: the default coefficient modulus of n)
// Output, once:
//     i bits : cn_f64_acc_interval          (bits 30 .. 61)
//     l name : slot .. | src .. | first,len ..          (plain_sum_slots of the four lists)
// and per set:
//     set name n logn k f64ok bits qmax
//     m f64 mp_fused mp_bcast rr ntt a_bcast pstride alias chain polys count : form policy launches fwd_limbs inv_limbs ptn_bcast refused id=bytes ..
//     s f64 mp_fused rr ptn_order ntt G E : kernel policy accmax order src_bytes grp_bytes slot_bytes
//     e length : the elements of sum_slots_elts
//     c ks_chain keys count length : the elements of sum_slots_plan          (keys: 0 all FP64-form, 1 the second link's missing, 2 the second link's integer-form)
//     w f64 mp_bcast ks_chain ntt rows length : links pp_bytes ctn_bytes chain_off          (rowdot_plan; every key FP64-form where the moduli allow)
// The key-switch switches are a context's defaults: "ks_wide" -1, thresholds 10 and 160, the half-size tables at N = 16384 with every modulus below 2^49.
#include "../../cryptonets_amd/csrc/cn_plain_plan.h"
#include <cstdio>
#include <cstring>

static const char *FORM[] = {"BCAST", "PTN_FUSED", "LIFT_FUSED", "LEGACY"};
static const char *ARRAY[] = {"ctn", "keep", "lift"};
static const char *POLICY[] = {"U64", "F64", "F64L"};

static void print_elts(const std::vector<uint64_t> &e) { for (uint64_t x : e) printf(" %llu", (unsigned long long)x); printf("\n"); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    for (int bits = 30; bits <= 61; bits++) printf("i %d : %u\n", bits, cn_f64_acc_interval(bits));
    const struct { const char *name; std::vector<uint32_t> idx; } lists[] = {
        {"equal", {7, 7, 7, 7}}, {"increasing", {2, 3, 4, 5, 6}}, {"interleaved", {0, 1, 0, 2, 3, 1, 9, 5, 6, 9, 4}}, {"single", {11}}};
    for (const auto &L : lists) {
        const PlainSumSlots s = plain_sum_slots(L.idx.data(), (uint32_t)L.idx.size());
        printf("l %s :", L.name);
        for (uint32_t x : s.slot) printf(" %u", x);
        printf(" |");
        for (uint32_t x : s.src) printf(" %u", x);
        printf(" |");
        for (const auto &r : s.runs) printf(" %u,%u", r.first, r.len);
        printf("\n");
    }
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
        const CnModRange qr = cn_mod_range(hc, 0, hc.k);
        printf("set %s %u %u %u %d %d %llx\n", name, hc.n, hc.logn, hc.k, (int)qr.f64ok, qr.bits, (unsigned long long)qr.qmax);
        auto switches = [&](int f64, int mp_fused, int mp_bcast, int ks_chain, int order, int rr) {
            const KsSwitches ks{-1, 1, 1, 0, 1, rr != 0, hc.logn == 14 && qr.f64ok, 10, 160, (size_t)24 << 30};
            return PlainSwitches{f64, mp_fused, mp_bcast, ks_chain, order, rr != 0, ks};
        };
        const uint32_t counts[] = {1, 3, 4, 5, 845, 5488};
        for (int f64 = 0; f64 < 2; f64++) for (int fused = 0; fused < 2; fused++) for (int bcast = 0; bcast < 2; bcast++) for (int rr = 0; rr < 2; rr++)
        for (int ntt = 0; ntt < 2; ntt++) for (int ab = 0; ab < 2; ab++) for (uint32_t ps = 0; ps < 2; ps++) for (int alias = 0; alias < 2; alias++) for (int chain = 0; chain < 2; chain++)
        for (uint32_t polys = 2; polys <= 3; polys++) for (uint32_t cnt : counts) {
            const PlainPlan p = cn_plain_plan(hc, switches(f64, fused, bcast, 1, 0, rr), {cnt, polys, ps, ntt != 0, ab != 0, chain != 0, alias != 0});
            printf("m %d %d %d %d %d %d %u %d %d %u %u : %s %s %u %llu %llu %u %d", f64, fused, bcast, rr, ntt, ab, ps, alias, chain, polys, cnt, FORM[p.form], POLICY[p.policy], p.launches,
                   (unsigned long long)p.fwd_limbs, (unsigned long long)p.inv_limbs, p.ptn_bcast, p.refusal ? 1 : 0);
            if (p.refusal && strcmp(p.refusal, "internal: chained row-dot batch outside the broadcast product")) return 5;
            for (uint32_t i = 0; i < p.arrays; i++) printf(" %s=%zu", ARRAY[p.scratch[i].id], p.scratch[i].bytes);
            printf("\n");
        }
        for (int f64 = 0; f64 < 2; f64++) for (int fused = 0; fused < 2; fused++) for (int rr = 0; rr < 2; rr++) for (int order = 0; order < 2; order++) for (int ntt = 0; ntt < 2; ntt++)
        for (uint32_t G : {1u, 2u, 100u}) for (uint32_t E : {G, 3 * G}) {
            const PlainSumPlan p = plain_sum_plan(hc, switches(f64, fused, 1, 1, order, rr), ntt != 0, G, E);
            printf("s %d %d %d %d %d %u %u : %d %s %u %u %zu %zu %zu\n", f64, fused, rr, order, ntt, G, E, (int)p.kernel, POLICY[p.policy], p.accmax, p.order, p.src_bytes, p.grp_bytes, p.slot_bytes);
        }
        const uint32_t lengths[] = {0, 1, 2, 8, hc.n / 2 - 1, hc.n / 2, hc.n};
        for (uint32_t len : lengths) { printf("e %u :", len); print_elts(sum_slots_elts(hc.n, len)); }
        for (int chain = 0; chain < 2; chain++) for (int keys = 0; keys < 3; keys++) for (uint32_t cnt : {0u, 2u, 21u, 5488u}) for (uint32_t len : lengths) {
            const std::vector<uint64_t> all = sum_slots_elts(hc.n, len);
            auto key_form = [&](uint64_t e) { return all.size() > 1 && e == all[1] ? (keys == 1 ? -1 : (keys == 2 ? 0 : 1)) : 1; };
            printf("c %d %d %u %u :", chain, keys, cnt, len);
            print_elts(sum_slots_plan(hc, switches(1, 1, 1, chain, 0, 1), cnt, len, key_form));
        }
        for (int f64 = 0; f64 < 2; f64++) for (int bcast = 0; bcast < 2; bcast++) for (int chain = 0; chain < 2; chain++) for (int ntt = 0; ntt < 2; ntt++)
        for (uint32_t rows : {3u, 4u, 21u, 5488u}) for (uint32_t len : {1u, 8u, 0u}) {
            const RowdotPlan r = rowdot_plan(hc, switches(f64, 1, bcast, chain, 0, 1), rows, len, ntt != 0, [&](uint64_t) { return qr.f64ok ? 1 : 0; });
            printf("w %d %d %d %d %u %u : %zu %zu %zu %zu\n", f64, bcast, chain, ntt, rows, len, r.chain.size(), r.pp_bytes, r.ctn_bytes, (size_t)r.chain_off);
        }
    }
    fclose(f);
    return 0;
}
