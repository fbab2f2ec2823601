// CPU run of the host-only multiply planner (cryptonets_amd/csrc/cn_mul_plan.h) over real context tables (cn_tables.cpp), for tests/test_mul_plan.py.
// Input (argv[1]), one parameter set per line of text:
//     name n t dbc gdbc k q_0 .. q_{k-1} nK K_0 .. K_{nK-1}          (hex moduli; k = 0: the default coefficient modulus of n; K: term counts for the product-sum lines)
// Output per set (smax index s: 0 = 24 GiB, 1 = 40 MiB, 2 = 0.00224 GiB, 3 = the bytes of one size-3 product - 1):
//     set name n logn k kb rl_tot dbc behz_f64 f64ok_q f64ok_bsk max_dig m_0 .. m_{k-1} | b_0 .. b_{kb-1}
//     p square cnt f64 sq_fused sq_pipe sq_lds rr cus : form lazy behz_f64 q.policy q.sq q.per_limb bsk.policy bsk.sq bsk.per_limb id:bytes ..
//     b site square count s outputs s32 : per fixed chunk fits ensure(chunk) ensure(1)
//     u K count s digit_i32 : s32 group
//     c f64 rr13 ks_xi rlk_f64 : square_gemm_ctx_ok fused_ok(dig) fused_ok(!dig) defers(switch on, key) defers(switch off) defers(no key)
//     k K mul_sum : mul_sum_fused_ok          (a context that passes square_gemm_ctx_ok where the set can)
//     h sq_halves capturing min c ks_wide s : parts first_0 .. first_parts
//     g O G Kp M dig_i32 : mul_sg_scratch
//     x c : pipeline_cuts parts first_0 ..
#include "../../cryptonets_amd/csrc/cn_mul_plan.h"
#include <cstdio>
#include <vector>

static const char *FORM[] = {"SQUARE_FUSED", "INTT_TENSOR", "ELEMENTWISE"};
static const char *POLICY[] = {"U64", "F64", "F64L"};
static const char *SQ[] = {"PLAIN", "LDS", "PIPE"};
static const char *ARR[] = {"aq", "ab", "bq", "bb", "dq", "db"};
static const uint32_t COUNTS[] = {1, 3, 4, 127, 128, 255, 256, 511, 512, 513, 700, 845};

static MulSwitches switches(const DevConsts &hc, size_t smax) {
    const bool f64ok = cn_mod_range(hc, 0, hc.k).f64ok;
    return {1, 1, 1, 1, 1, true, true, true, cn_rr_size(hc.logn), cn_rr_size(hc.logn, 13), 256, false, smax, true, f64ok,
            KsSwitches{-1, 1, 1, 0, 1, cn_rr_size(hc.logn), false, 10, 160, smax}};
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
        unsigned nK;
        if (fscanf(f, "%u", &nK) != 1) return 3;
        std::vector<uint32_t> Ks(nK);
        for (unsigned i = 0; i < nK; i++) if (fscanf(f, "%u", &Ks[i]) != 1) return 3;
        if (!k) { const int cnt = cn_default_coeff_modulus_impl(n, q); if (cnt <= 0) return 3; k = (unsigned)cnt; }
        static DevConsts hc;
        std::vector<uint64_t> tw((size_t)(2 * k + 3) * 4 * n);
        std::vector<double> twd((size_t)(2 * k + 3) * 2 * n);
        std::vector<uint32_t> index_map(n);
        char err[256];
        if (cn_build_consts(&hc, n, q, k, t, dbc, gdbc, tw.data(), index_map.data(), err, sizeof err)) { fprintf(stderr, "%s: %s\n", name, err); return 4; }
        cn_build_f64_tables(&hc, tw.data(), twd.data());
        const size_t smaxs[4] = {(size_t)24 << 30, (size_t)40 << 20, (size_t)(0.00224 * (double)(1ull << 30)), (size_t)3 * hc.k * hc.n * 8 - 1};
        uint32_t max_dig = 0;
        for (uint32_t j = 0; j < hc.k; j++) max_dig = std::max(max_dig, hc.rl_dig[j]);
        printf("set %s %u %u %u %u %u %d %u %d %d %u", name, hc.n, hc.logn, hc.k, hc.kb, hc.rl_tot, hc.dbc, hc.behz_f64, (int)cn_mod_range(hc, 0, hc.k).f64ok,
               (int)cn_mod_range(hc, hc.k, hc.kb).f64ok, max_dig);
        for (uint32_t j = 0; j < hc.k; j++) printf(" %llx", (unsigned long long)hc.q[j].q);
        printf(" |");
        for (uint32_t j = 0; j < hc.kb; j++) printf(" %llx", (unsigned long long)hc.bsk[j].q);
        printf("\n");
        for (int square = 0; square < 2; square++) for (uint32_t cnt : COUNTS) for (int f64 = 0; f64 < 2; f64++) for (int fused = 0; fused < 2; fused++) for (int pipe = 0; pipe < 3; pipe++)
        for (int lds = 0; lds < 2; lds++) for (int rr = 0; rr < 2; rr++) for (int cus : {1, 64, 256}) {
            MulSwitches sw = switches(hc, smaxs[0]);
            sw.f64 = f64; sw.sq_fused = fused; sw.sq_pipe = pipe; sw.sq_lds = lds; sw.rr = rr != 0; sw.cus = cus;
            const MulPlan p = cn_mul_plan(hc, sw, square != 0, cnt);
            printf("p %d %u %d %d %d %d %d %d : %s %d %d %s %s %u %s %s %u", square, cnt, f64, fused, pipe, lds, rr, cus, FORM[p.form], (int)p.lazy, (int)p.behz_f64, POLICY[p.q.policy], SQ[p.q.sq],
                   p.q.sq == SQ_PIPE ? p.q.per_limb : 0, POLICY[p.bsk.policy], SQ[p.bsk.sq], p.bsk.sq == SQ_PIPE ? p.bsk.per_limb : 0);      // (per_limb: the pipe kernel's alone)
            for (uint32_t i = 0; i < p.arrays; i++) printf(" %s:%zu", ARR[p.scratch[i].id], p.scratch[i].bytes);
            printf("\n");
        }
        for (int site = MUL_AT_MULTIPLY; site <= MUL_AT_SUM_GROUP; site++) for (int square = 0; square < 2; square++) for (uint32_t cnt : COUNTS) for (int s = 0; s < 4; s++)
        for (uint32_t outputs : {0u, 1u, 10u, 100u}) for (int s32 = 0; s32 < 2; s32++) {
            if (site < MUL_AT_SQUARE_GEMM && (outputs || s32)) continue;
            const MulBatch b = mul_batch(hc, switches(hc, smaxs[s]), (MulSite)site, cnt, square != 0, outputs, s32 != 0);
            printf("b %d %d %u %d %u %d : %zu %zu %u %d %zu %zu\n", site, square, cnt, s, outputs, s32, b.per, b.fixed, b.chunk, (int)b.fits, b.ensure(b.chunk), b.ensure(1));
        }
        for (uint32_t K : Ks) for (uint32_t count : {1u, 6u, 100u}) for (int s = 0; s < 4; s++) for (int i32 = 0; i32 < 2; i32++) {
            MulSwitches sw = switches(hc, smaxs[s]);
            sw.digit_i32 = i32 != 0;
            const MulSumBatch b = mul_sum_batch(hc, sw, K, count);
            printf("u %u %u %d %d : %d %u\n", K, count, s, i32, (int)b.s32, b.group);
        }
        for (int f64 = 0; f64 < 2; f64++) for (int rr13 = 0; rr13 < 2; rr13++) for (uint32_t xi = 0; xi < 2; xi++) for (int kf = 0; kf < 2; kf++) {
            MulSwitches sw = switches(hc, smaxs[0]);
            sw.f64 = f64; sw.rr13 = rr13 != 0; sw.rlk_f64 = kf != 0; hc.ks_xi = xi;
            GemmLayout dig, nodig; dig.dig = true;
            MulSwitches off = sw, nokey = sw; off.defer_square_gemm = false; nokey.rlk = false;
            printf("c %d %d %u %d : %d %d %d %d %d %d\n", f64, rr13, xi, kf, (int)square_gemm_ctx_ok(hc, sw), (int)square_gemm_fused_ok(hc, sw, dig), (int)square_gemm_fused_ok(hc, sw, nodig),
                   (int)mul_defers_square_gemm(hc, sw), (int)mul_defers_square_gemm(hc, off), (int)mul_defers_square_gemm(hc, nokey));
        }
        hc.ks_xi = 0;
        for (uint32_t K : Ks) for (int ms = 0; ms < 2; ms++) {
            MulSwitches sw = switches(hc, smaxs[0]);
            sw.mul_sum = ms != 0;
            printf("k %u %d : %d\n", K, ms, (int)mul_sum_fused_ok(hc, sw, K));
        }
        for (int halves = 0; halves < 3; halves++) for (int cap = 0; cap < 2; cap++) for (int min = 1; min <= 2; min++) for (uint32_t c : COUNTS) for (int wide = -1; wide <= 2; wide++)
        for (int s = 0; s < 4; s++) {
            MulSwitches sw = switches(hc, smaxs[s]);
            sw.sq_halves = halves; sw.capturing = cap != 0; sw.ks.ks_wide = wide;
            uint32_t first[4] = {0, 0, 0, 0};
            const uint32_t P = mul_pipeline_parts(hc, sw, c, min, first);
            printf("h %d %d %d %u %d %d : %u", halves, cap, min, c, wide, s, P);
            for (uint32_t i = 0; P && i <= P; i++) printf(" %u", first[i]);
            printf("\n");
        }
        for (uint32_t O : {1u, 10u, 100u}) for (uint32_t G : {1u, 3u}) for (uint32_t Kp : {8u, 848u}) for (uint32_t M : {2u, 32u}) for (int i32 = 0; i32 < 2; i32++) {
            GemmLayout L; L.G = G; L.Kp = Kp; L.M = M; L.dig_i32 = i32 != 0;
            printf("g %u %u %u %u %d : %zu\n", O, G, Kp, M, i32, mul_sg_scratch(hc, L, O));
        }
    }
    fclose(f);
    for (uint32_t c : {1u, 127u, 128u, 200u, 255u, 256u, 383u, 384u, 512u, 513u, 700u, 845u, 5488u}) {
        uint32_t first[4];
        const uint32_t P = pipeline_cuts(c, first);
        printf("x %u : %u", c, P);
        for (uint32_t i = 0; i <= P; i++) printf(" %u", first[i]);
        printf("\n");
    }
    printf("const %u %u %u\n", MUL_SUM_MIN_K, SQ_HALVES_MIN, PRODUCT_SUM_MAX_DIGITS);
    return 0;
}
