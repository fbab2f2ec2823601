// CPU run of the clipped + residual weight form of the scalar GEMM planner (gemm_residual_form, cryptonets_amd/csrc/cn_gemm_plan.h), for
// tests/test_gemm_residual_plan.py.  Input (argv[1]) as tests/cpp/gemm_plan.cpp reads it, one case after the other:
//   case NAME t n dbc k q_0 .. q_(k-1) f64 gemm_mfma gemm_pair digit_mfma digit_i32
//   index O K has_idx   [idx O x K]   W O x K
//   addr O K   A O x K   W O x K   out O
// Output per case: "case NAME", then "refused rc text" or
//   layout K Kp G M mfma P res mtiles ksteps dig dig_mfma off_oidx off_bidx off_w off_dw sum_abs_w entry_bytes
//   image BYTES hex                                     (the whole image)
#include "../../cryptonets_amd/csrc/cn_gemm_plan.h"
#include <cinttypes>
#include <string>

static FILE *f;
static unsigned long long num() { unsigned long long v = 0; if (fscanf(f, "%llu", &v) != 1) exit(3); return v; }
static long long snum() { long long v = 0; if (fscanf(f, "%lld", &v) != 1) exit(3); return v; }

static void print_plan(const GemmLayout &L, const std::vector<char> &image, unsigned entry) {
    printf("layout %u %u %u %u %d %u %d %u %u %d %d %zu %zu %zu %zu %" PRIu64 " %u\n", L.K, L.Kp, L.G, L.M, L.mfma, L.P, L.res, L.mtiles, L.ksteps, L.dig, L.dig_mfma,
           L.off_oidx, L.off_bidx, L.off_w, L.off_dw, L.sum_abs_w, entry);
    printf("image %zu ", image.size());
    for (char c : image) printf("%02x", (unsigned)(unsigned char)c);
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 2 || !(f = fopen(argv[1], "r"))) return 2;
    char word[64], name[64];
    while (fscanf(f, "%63s", word) == 1) {
        if (std::string(word) != "case" || fscanf(f, "%63s", name) != 1) return 3;
        DevConsts hc;
        memset(&hc, 0, sizeof hc);
        hc.t.q = num(); hc.t_half = (hc.t.q + 1) >> 1;
        hc.n = (uint32_t)num(); hc.dbc = (int32_t)num(); hc.k = (uint32_t)num();
        for (uint32_t j = 0; j < hc.k; j++) { hc.q[j].q = num(); hc.lift_inc[j] = hc.q[j].q - hc.t.q; }
        GemmSwitches sw;
        sw.f64 = num() != 0; sw.gemm_mfma = num() != 0; sw.gemm_pair = num() != 0; sw.digit_mfma = num() != 0; sw.digit_i32 = num() != 0;
        if (fscanf(f, "%63s", word) != 1) return 3;
        const uint32_t O = (uint32_t)num(), K = (uint32_t)num();
        printf("case %s\n", name);
        if (std::string(word) == "index") {
            const bool has_idx = num() != 0;
            std::vector<int32_t> idx((size_t)O * K);
            std::vector<uint64_t> W((size_t)O * K);
            if (has_idx) for (int32_t &x : idx) x = (int32_t)snum();
            for (uint64_t &w : W) w = num();
            GemmLayout L; std::vector<char> image; uint32_t max_in = 0; uint64_t nnz = 0;
            const GemmRefusal no = gemm_plan_indices(hc, sw, has_idx ? idx.data() : nullptr, W.data(), O, K, nullptr, 0, L, image, max_in, nnz);
            if (no) { printf("refused %d %s\n", no.rc, no.msg); continue; }
            print_plan(L, image, 4);
        } else {
            std::vector<uint64_t> A((size_t)O * K), W((size_t)O * K), out(O), bias(O, 0);
            for (uint64_t &a : A) a = num();
            for (uint64_t &w : W) w = num();
            for (uint64_t &a : out) a = num();
            GemmAddressPlan R;
            gemm_plan_addresses(hc, sw, A.data(), W.data(), out.data(), bias.data(), O, K, false, R);      // (address tables: the entries are the addresses given)
            print_plan(R.L, R.image, 8);
        }
    }
    fclose(f);
    return 0;
}
