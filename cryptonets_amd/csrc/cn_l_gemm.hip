// Launchers of the scalar GEMM kernels (HOT LOOP A).  One translation unit per kernel family: hipcc compiles them in parallel.
#include "cn_runtime.h"
#include <algorithm>
#include "cn_k_gemm.hip.h"

// order 1 (slice-major) needs the slices in multiples of 8 and is launched as a 2-D grid: x = (XCD, output tile, group), y = slice / 8 (gemm_block_coords)
struct GemmGrid { dim3 grid; uint32_t order; };
static GemmGrid gemm_grid(cn_ctx *c, const GemmLaunch &g, uint32_t mtiles) {
    const uint32_t slices = c->chunks * g.polys * c->hc.k;
    if (g.order == 1 && (slices & 7) == 0 && (c->chunks & (c->chunks - 1)) == 0 && (uint64_t)8 * mtiles * g.G < (1ull << 31) && slices / 8 < 65536)
        return {dim3(8 * mtiles * g.G, slices / 8), 1u};
    return {dim3((uint32_t)((size_t)slices * mtiles * g.G)), 0u};
}
template <int MT, bool ABS> static void launch_int(cn_ctx *c, const GemmLaunch &g) {
    const uint32_t mtiles = (g.M + MT - 1) / MT;
    const GemmGrid gg = gemm_grid(c, g, mtiles);
    hipLaunchKernelGGL((k_scalar_gemm<MT, ABS>), gg.grid, dim3(c->bs), 0, c->stream, g.in, g.idx, (const uint64_t *)g.W, g.oidx, g.bias, g.bidx, g.out, c->dc,
                       c->chunks, g.G, g.M, g.K, mtiles, g.lazy, g.Kp, g.obase, g.polys, gg.order, GemmUnits{g.in_unit, g.out_unit, g.bias_unit});
}
template <int MT, bool ABS> static void launch_f64(cn_ctx *c, const GemmLaunch &g) {
    const uint32_t mtiles = (g.M + MT - 1) / MT;
    const GemmGrid gg = gemm_grid(c, g, mtiles);
    if (g.one) hipLaunchKernelGGL((k_scalar_gemm_f64<MT, 1, 0, ABS>), gg.grid, dim3(c->bs), 0, c->stream, g.in, g.idx, (const double *)g.W, g.oidx, g.bias,
                                  g.bidx, g.out, c->dc, c->chunks, g.G, g.M, g.K, mtiles, g.lazy, g.Kp, g.obase, g.polys, gg.order, gemm_f64_rows(g.K), GemmUnits{g.in_unit, g.out_unit, g.bias_unit});
    else if (g.two) hipLaunchKernelGGL((k_scalar_gemm_f64<MT, 2, 22, ABS>), gg.grid, dim3(c->bs), 0, c->stream, g.in, g.idx, (const double *)g.W, g.oidx, g.bias,
                                  g.bidx, g.out, c->dc, c->chunks, g.G, g.M, g.K, mtiles, g.lazy, g.Kp, g.obase, g.polys, gg.order, gemm_f64_rows(g.K), GemmUnits{g.in_unit, g.out_unit, g.bias_unit});
    else hipLaunchKernelGGL((k_scalar_gemm_f64<MT, 3, 17, ABS>), gg.grid, dim3(c->bs), 0, c->stream, g.in, g.idx, (const double *)g.W, g.oidx, g.bias,
                            g.bidx, g.out, c->dc, c->chunks, g.G, g.M, g.K, mtiles, g.lazy, g.Kp, g.obase, g.polys, gg.order, gemm_f64_rows(g.K), GemmUnits{g.in_unit, g.out_unit, g.bias_unit});
}
template <bool ABS> static int launch(cn_ctx *c, const GemmLaunch &g) {
    if (g.small) {
        switch (g.MT) {
            case 20: launch_f64<20, ABS>(c, g); break;
            case 10: launch_f64<10, ABS>(c, g); break;
            case 5: launch_f64<5, ABS>(c, g); break;
            case 1: launch_f64<1, ABS>(c, g); break;
            default: return cn_fail(CN_ERR_ARG, "internal: scalar GEMM tile %u", g.MT);
        }
    } else {
        switch (g.MT) {
            case 10: launch_int<10, ABS>(c, g); break;
            case 5: launch_int<5, ABS>(c, g); break;
            case 1: launch_int<1, ABS>(c, g); break;
            default: return cn_fail(CN_ERR_ARG, "internal: scalar GEMM tile %u", g.MT);
        }
    }
    HIPCHK(hipGetLastError());
    cn_launch_count(c);
    return 0;
}
int cn_l_gemm(cn_ctx *c, const GemmLaunch &g) { return g.abs ? launch<true>(c, g) : launch<false>(c, g); }

// RES...: GemmResidual for a plan in the clipped + residual form (GemmLaunch::res, P = 1), else nothing
template <int P, bool ABS, class... RES> static void launch_mfma(cn_ctx *c, const GemmLaunch &g) {
    const uint32_t mgroups = (g.mtiles + 3) / 4;
    if constexpr (!ABS && P <= 2) {                            // the pre-floor forms of cn_square_gemm (GemmLaunch::form): Bsk limbs / exact integer sums of canonical y
        if (g.form) {                                          // (one or two weight planes: with three the y form spills - square_gemm_prefloor_ok, cn_mul_plan.h)
            const size_t pblocks = (size_t)g.G * mgroups * g.polys * (g.form == GEMM_BSK ? c->hc.kb : c->hc.k) * (c->hc.n / 32);
            if (g.form == GEMM_BSK) hipLaunchKernelGGL((k_scalar_gemm_mfma<P, false, GemmBskForm, RES...>), dim3((uint32_t)pblocks), dim3(256), 0, c->stream, g.in, g.idx, (const int8_t *)g.W, g.oidx,
                                                       nullptr, nullptr, g.out, c->dc, g.G, g.M, g.mtiles, g.ksteps, g.obase, g.polys, GemmUnits{g.in_unit, g.out_unit, 0u});
            else hipLaunchKernelGGL((k_scalar_gemm_mfma<P, false, GemmYForm, RES...>), dim3((uint32_t)pblocks), dim3(256), 0, c->stream, g.in, g.idx, (const int8_t *)g.W, g.oidx,
                                    nullptr, nullptr, g.out, c->dc, g.G, g.M, g.mtiles, g.ksteps, g.obase, g.polys, GemmUnits{g.in_unit, g.out_unit, 0u});
            return;
        }
    }
    const size_t blocks = (size_t)g.G * mgroups * g.polys * c->hc.k * (c->hc.n / 32);
    hipLaunchKernelGGL((k_scalar_gemm_mfma<P, ABS, RES...>), dim3((uint32_t)blocks), dim3(256), 0, c->stream, g.in, g.idx, (const int8_t *)g.W, g.oidx, g.bias, g.bidx, g.out,
                       c->dc, g.G, g.M, g.mtiles, g.ksteps, g.obase, g.polys, GemmUnits{g.in_unit, g.out_unit, g.bias_unit});
}
template <bool ABS> static int launch_mfma_p(cn_ctx *c, const GemmLaunch &g) {
    if (g.form && (ABS || g.P > 2 || g.form > GEMM_Y || !g.in_unit || !g.out_unit)) return cn_fail(CN_ERR_ARG, "internal: pre-floor GEMM form %u", g.form);
    if (g.res && g.P != 1) return cn_fail(CN_ERR_ARG, "internal: residual weights with %u planes", g.P);
    switch (g.P) {
        case 1: if (g.res) launch_mfma<1, ABS, GemmResidual>(c, g); else launch_mfma<1, ABS>(c, g); break;
        case 2: launch_mfma<2, ABS>(c, g); break;
        case 3: launch_mfma<3, ABS>(c, g); break;
        default: return cn_fail(CN_ERR_ARG, "internal: %u weight digit planes", g.P);
    }
    HIPCHK(hipGetLastError());
    cn_launch_count(c);
    return 0;
}
int cn_l_gemm_mfma(cn_ctx *c, const GemmLaunch &g) { return g.abs ? launch_mfma_p<true>(c, g) : launch_mfma_p<false>(c, g); }

// digit GEMM (cn_square_gemm): DG = 5 digits of a source limb per workgroup (a 50-bit limb at dbc 10), more digits per limb in further groups
// (g.i32: S as int32 words - the <.., int32_t> instantiations of the three producers)
template <int MT> static void launch_digit(cn_ctx *c, const DigitGemmLaunch &g, uint32_t ndg, uint32_t mtiles) {
    const size_t blocks = (size_t)(c->hc.n >> 8) * c->hc.k * ndg * mtiles * g.G;
    if (g.i32) hipLaunchKernelGGL((k_digit_gemm<MT, 5, int32_t>), dim3((uint32_t)blocks), dim3(256), 0, c->stream, g.in, g.in_unit, (const int32_t *)g.idx, (const double *)g.W,
                                  (const int32_t *)g.oidx, (int32_t *)g.S, c->dc, g.G, g.M, g.K, mtiles, g.Kp, g.Kw, ndg);
    else hipLaunchKernelGGL((k_digit_gemm<MT, 5>), dim3((uint32_t)blocks), dim3(256), 0, c->stream, g.in, g.in_unit, (const int32_t *)g.idx, (const double *)g.W,
                            (const int32_t *)g.oidx, (double *)g.S, c->dc, g.G, g.M, g.K, mtiles, g.Kp, g.Kw, ndg);
}
// matrix-core form: DG = digit_gemm_mfma_group(P) digits per workgroup (DIGIT_GEMM_RES_GROUP for a plan in the clipped + residual form, g.res); the digit groups of a (column tile, limb) take block ids 8 apart (k_digit_gemm_mfma)
template <int P, int DG, class... RES> static void launch_digit_mfma(cn_ctx *c, const DigitGemmLaunch &g, uint32_t ndg, size_t blocks) {
    if (g.i32) hipLaunchKernelGGL((k_digit_gemm_mfma<P, DG, int32_t, RES...>), dim3((uint32_t)blocks), dim3(256), 0, c->stream, g.in, g.in_unit, (const int32_t *)g.idx, (const int8_t *)g.W,
                                  (const int32_t *)g.oidx, (int32_t *)g.S, c->dc, g.G, g.M, g.mtiles, g.ksteps, ndg);
    else hipLaunchKernelGGL((k_digit_gemm_mfma<P, DG, RES...>), dim3((uint32_t)blocks), dim3(256), 0, c->stream, g.in, g.in_unit, (const int32_t *)g.idx, (const int8_t *)g.W,
                            (const int32_t *)g.oidx, (double *)g.S, c->dc, g.G, g.M, g.mtiles, g.ksteps, ndg);
}
static int digit_gemm_mfma(cn_ctx *c, const DigitGemmLaunch &g, uint32_t ndmax) {
    if (g.res && g.P != 1) return cn_fail(CN_ERR_ARG, "internal: residual weights with %u planes", g.P);
    const uint32_t DG = g.res ? DIGIT_GEMM_RES_GROUP : digit_gemm_mfma_group(g.P), ndg = (ndmax + DG - 1) / DG, mgroups = (g.mtiles + 3) / 4;
    const uint64_t blocks = (uint64_t)g.G * mgroups * c->hc.k * (c->hc.n / 32) * ndg;
    if ((c->hc.n & 255) || !g.ksteps || blocks >= (1ull << 31)) return cn_fail(CN_ERR_ARG, "internal: digit GEMM grid");
    switch (g.P) {
        case 1: if (g.res) launch_digit_mfma<1, DIGIT_GEMM_RES_GROUP, GemmResidual>(c, g, ndg, blocks); else launch_digit_mfma<1, 3>(c, g, ndg, blocks); break;
        case 2: launch_digit_mfma<2, 3>(c, g, ndg, blocks); break;
        case 3: launch_digit_mfma<3, 2>(c, g, ndg, blocks); break;
        default: return cn_fail(CN_ERR_ARG, "internal: %u weight digit planes", g.P);
    }
    HIPCHK(hipGetLastError());
    cn_launch_count(c);
    c->cnt.dg_mfma++;
    return 0;
}
int cn_l_digit_gemm(cn_ctx *c, const DigitGemmLaunch &g) {
    uint32_t ndmax = 0; for (uint32_t l = 0; l < c->hc.k; l++) ndmax = std::max(ndmax, c->hc.rl_dig[l]);
    if (g.mfma) return digit_gemm_mfma(c, g, ndmax);
    const uint32_t ndg = (ndmax + 4) / 5, mtiles = (g.M + g.MT - 1) / g.MT;
    if ((c->hc.n & 255) || (uint64_t)(c->hc.n >> 8) * c->hc.k * ndg * mtiles * g.G >= (1ull << 31)) return cn_fail(CN_ERR_ARG, "internal: digit GEMM grid");
    switch (g.MT) {
        case 10: launch_digit<10>(c, g, ndg, mtiles); break;
        case 2: launch_digit<2>(c, g, ndg, mtiles); break;
        default: return cn_fail(CN_ERR_ARG, "internal: digit GEMM tile %u", g.MT);
    }
    HIPCHK(hipGetLastError());
    cn_launch_count(c);
    return 0;
}

// sum of the K products of every output (cn_mul_relin_sum): ND = the smallest instantiation that holds all digits of every source limb
template <int ND> static void launch_product_sum(cn_ctx *c, const ProductSumLaunch &g, uint32_t blocks) {
    if (g.i32) hipLaunchKernelGGL((k_product_sum<ND, int32_t>), dim3(blocks), dim3(256), 0, c->stream, g.prod, g.K, g.out, (int32_t *)g.S, c->dc);
    else hipLaunchKernelGGL((k_product_sum<ND>), dim3(blocks), dim3(256), 0, c->stream, g.prod, g.K, g.out, (double *)g.S, c->dc);
}
int cn_l_product_sum(cn_ctx *c, const ProductSumLaunch &g) {
    uint32_t ndmax = 0; for (uint32_t l = 0; l < c->hc.k; l++) ndmax = std::max(ndmax, c->hc.rl_dig[l]);
    const uint64_t blocks = (uint64_t)(c->hc.n >> 9) * c->hc.k * g.outputs;
    if ((c->hc.n & 511) || !g.K || !g.outputs || ndmax > PRODUCT_SUM_MAX_DIGITS || c->hc.dbc > 31 || blocks >= (1ull << 31)) return cn_fail(CN_ERR_ARG, "internal: product sum grid");
    if (ndmax <= 2) launch_product_sum<2>(c, g, (uint32_t)blocks);
    else if (ndmax <= 4) launch_product_sum<4>(c, g, (uint32_t)blocks);
    else if (ndmax <= 5) launch_product_sum<5>(c, g, (uint32_t)blocks);
    else launch_product_sum<8>(c, g, (uint32_t)blocks);
    HIPCHK(hipGetLastError());
    cn_launch_count(c);
    return 0;
}
