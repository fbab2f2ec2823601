// CPU run of the host-only scalar GEMM planner (cryptonets_amd/csrc/cn_gemm_plan.h), for tests/test_gemm_plan.py.
// Input (argv[1]), one case after the other as whitespace-separated numbers:
//   case NAME t n dbc k q_0 .. q_(k-1) f64 gemm_mfma gemm_pair digit_mfma digit_i32
//   index O K has_idx has_bias bias_count   [idx O x K]   W O x K   [bias_idx O]
//   addr O K rel_on   A O x K   W O x K   out O   bias O
// Output per case: "case NAME", then "refused rc text" or
//   layout K Kp G M MT lazy small two one mfma P mtiles ksteps dig dig_mfma dig_i32 dMT dKw off_oidx off_bidx off_w off_dw
//   plan max_in nnz                                     (index cases)
//   form abs any_bias ibase obase bbase some_input      (address cases)
//   image BYTES hex                                     (the whole image)
#include "../../cryptonets_amd/csrc/cn_gemm_plan.h"
#include <cinttypes>
#include <string>

static FILE *f;
static unsigned long long num() { unsigned long long v = 0; if (fscanf(f, "%llu", &v) != 1) exit(3); return v; }
static long long snum() { long long v = 0; if (fscanf(f, "%lld", &v) != 1) exit(3); return v; }

static void print_layout(const GemmLayout &L) {
    printf("layout %u %u %u %u %u %u %d %d %d %d %u %u %u %d %d %d %u %u %zu %zu %zu %zu\n", L.K, L.Kp, L.G, L.M, L.MT, L.lazy, L.small, L.two, L.one, L.mfma, L.P, L.mtiles,
           L.ksteps, L.dig, L.dig_mfma, L.dig_i32, L.dMT, L.dKw, L.off_oidx, L.off_bidx, L.off_w, L.off_dw);
}
static void print_image(const std::vector<char> &image) {
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
            const bool has_idx = num() != 0, has_bias = num() != 0;
            const uint32_t bias_count = (uint32_t)num();
            std::vector<int32_t> idx((size_t)O * K), bidx(O);
            std::vector<uint64_t> W((size_t)O * K);
            if (has_idx) for (int32_t &x : idx) x = (int32_t)snum();
            for (uint64_t &w : W) w = num();
            if (has_bias) for (int32_t &x : bidx) x = (int32_t)snum();
            GemmLayout L; std::vector<char> image; uint32_t max_in = 0; uint64_t nnz = 0;
            const GemmRefusal no = gemm_plan_indices(hc, sw, has_idx ? idx.data() : nullptr, W.data(), O, K, has_bias ? bidx.data() : nullptr, bias_count, L, image, max_in, nnz);
            if (no) { printf("refused %d %s\n", no.rc, no.msg); continue; }
            print_layout(L);
            printf("plan %u %" PRIu64 "\n", max_in, nnz);
            print_image(image);
        } else {
            const bool rel_on = num() != 0;
            std::vector<uint64_t> A((size_t)O * K), W((size_t)O * K), out(O), bias(O);
            for (uint64_t &a : A) a = num();
            for (uint64_t &w : W) w = num();
            for (uint64_t &a : out) a = num();
            for (uint64_t &a : bias) a = num();
            GemmAddressPlan R;
            gemm_plan_addresses(hc, sw, A.data(), W.data(), out.data(), bias.data(), O, K, rel_on, R);
            print_layout(R.L);
            printf("form %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", R.abs, R.any_bias, R.ibase, R.obase, R.bbase, R.some_input);
            print_image(R.image);
        }
    }
    fclose(f);
    return 0;
}
