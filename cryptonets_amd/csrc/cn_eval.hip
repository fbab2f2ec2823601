// libcnhip.so host runtime (2/5): the evaluator - linear operations, scalar GEMM planning, BEHZ multiply, key switching, rotations (launch logic behind the C ABI).
#include "cn_api_shared.h"
#include "cn_gemm_plan.h"

// ---------------------------------------------------------------- linear ops
int addsub(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count, int op) {
    GETCT(A, a, 0); GETCT(O, out, A->size);
    Buffer *B = A;
    if (op != 2) { B = getbuf(ctx, b, 0); if (!B || B->size != A->size) return fail(CN_ERR_ARG, "operand sizes do not match"); }
    if (!range_ok(A, ai, count) || !range_ok(O, oi, count) || (op != 2 && !range_ok(B, bi, count))) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    uint32_t limbs = count * A->size * ctx->hc.k;
    hipLaunchKernelGGL(k_addsub, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, A->d + ai * A->item_words,
                       B->d + (op != 2 ? bi : ai) * B->item_words, O->d + oi * O->item_words, ctx->dc, ctx->chunks, op);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    return 0;
}
int addsub_body(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count, int op) {
    if (deferring(ctx)) { int rc = defer_addsub(ctx, a, ai, b, bi, out, oi, count, op); if (rc <= 0) return rc; }      // > 0: not deferrable (size-3 operands)
    CHECK(cn_defer_flush(ctx)); CHECK(addsub(ctx, a, ai, b, bi, out, oi, count, op));
    if (op) ctx->st.Subtraction += count; else ctx->st.Addition += count;
    return 0;
}
extern "C" int cn_add(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count) {
    if (submit_async(ctx) && count <= DEFER_STAGED_MAX) return ring_push(ctx, SUB_ADD, count, a, ai, b, bi, out, oi, 0, 0);
    API_BODY LOCK_ONLY; return addsub_body(ctx, a, ai, b, bi, out, oi, count, 0); API_END
}
extern "C" int cn_sub(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count) {
    if (submit_async(ctx) && count <= DEFER_STAGED_MAX) return ring_push(ctx, SUB_SUB, count, a, ai, b, bi, out, oi, 0, 0);
    API_BODY LOCK_ONLY; return addsub_body(ctx, a, ai, b, bi, out, oi, count, 1); API_END
}
extern "C" int cn_negate(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle out, uint32_t oi, uint32_t count) { API_BODY
    LOCK; return addsub(ctx, a, ai, a, ai, out, oi, count, 2);
API_END }
extern "C" int cn_add_many(cn_ctx *ctx, cn_handle in, const uint32_t *idx, uint32_t n_idx, cn_handle out, uint32_t oi) { API_BODY
    LOCK; GETCT(I, in, 0); GETCT(O, out, I->size);
    if (!n_idx || !idx) return fail(CN_ERR_ARG, "AddMany of an empty list");
    for (uint32_t i = 0; i < n_idx; i++) if (idx[i] >= I->count) return fail(CN_ERR_ARG, "index out of range");
    if (oi >= O->count) return fail(CN_ERR_ARG, "index out of range");
    CHECK(ensure_scratch(ctx, al(n_idx * 4)));
    uint32_t *didx; CHECK(upload_tmp(ctx, idx, n_idx, &didx));
    uint32_t limbs = I->size * ctx->hc.k;
    hipLaunchKernelGGL(k_add_many, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, I->d, didx, n_idx, I->item_words,
                       O->d + oi * O->item_words, ctx->dc, ctx->chunks);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    ctx->st.AddMany += 1; ctx->st.AddManyItemCount += n_idx;
    return 0;
API_END }
extern "C" int cn_add_plain(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, int subtract, cn_handle out, uint32_t oi, uint32_t count) {
    if (submit_async(ctx) && count <= DEFER_STAGED_MAX) return ring_push(ctx, SUB_ADD_PLAIN, count, a, ai, pt, pi, out, oi, subtract ? 1u : 0u, 0);
    API_BODY LOCK_ONLY; return add_plain_body(ctx, a, ai, pt, pi, subtract, out, oi, count); API_END
}
int add_plain_body(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, int subtract, cn_handle out, uint32_t oi, uint32_t count) {
    if (deferring(ctx)) { int rc = defer_add_plain(ctx, a, ai, pt, pi, subtract, out, oi, count); if (rc <= 0) return rc; }
    CHECK(cn_defer_flush(ctx));
    GETCT(A, a, 0); GETCT(O, out, A->size); GETPT(P, pt);
    if (!range_ok(A, ai, count) || !range_ok(O, oi, count) || !range_ok(P, pi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    uint32_t limbs = count * A->size * ctx->hc.k;
    hipLaunchKernelGGL(k_add_plain, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, A->d + ai * A->item_words,
                       P->d + (size_t)pi * ctx->hc.n, ctx->hc.n, O->d + oi * O->item_words, ctx->dc, ctx->chunks, A->size, subtract);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    if (subtract) ctx->st.PlainSubtraction += count; else ctx->st.PlainAddition += count;
    return 0;
}
// the switches of this context that the plaintext planner reads (cn_plain_plan.h): the only place that copies them out of a context for the plaintext family
PlainSwitches plain_switches(const cn_ctx *ctx) { return {ctx->opt.f64, ctx->opt.mp_fused, ctx->opt.mp_bcast, ctx->opt.ks_chain, ctx->opt.ptn_order, rr_kernels(ctx), ks_switches(ctx)}; }
// neither the same range nor disjoint: `words` words at a and at o overlap with a shift (a null operand overlaps nothing)
bool shifted_overlap(const uint64_t *a, const uint64_t *o, size_t words) { return a && a != o && a < o + words && o < a + words; }
static int mul_plain_overlap(const CtSpan &A, const CtSpan &O, size_t item_words) {      // block c writes out[c] while another block still reads in[c']
    if (!shifted_overlap(A.d, O.d, O.count * item_words)) return 0;
    return fail(CN_ERR_ARG, "multiply_plain: input and output ranges overlap partially (use the same range or disjoint ranges)");
}
static int plain_not_zero(const PtSpan &P, uint32_t count) {
    for (uint32_t c = 0; P.zero && c < (P.stride ? count : 1u); c++) if (P.zero[c * P.stride]) return fail(CN_ERR_ZERO, "plain cannot be zero");
    return 0;
}
// MultiplyPlain as planned (PlainPlan, cn_plain_plan.h): checks, the plan, its scratch arrays, the launches of its form
int mul_plain_impl(cn_ctx *ctx, CtSpan A, bool a_bcast, PtSpan P, CtSpan O, uint32_t polys, const BcastNext *nx) {
    const uint32_t n = ctx->hc.n, k = ctx->hc.k, count = O.count, pstride = P.stride, npt = pstride ? count : 1;
    const size_t item_words = (size_t)polys * k * n;
    if (!count) return 0;
    if (!a_bcast) CHECK(mul_plain_overlap(A, O, item_words));
    CHECK(plain_not_zero(P, count));
    uint64_t *o = O.d;
    const uint64_t *src = A.d;
    const bool alias = a_bcast && src >= o && src < o + (size_t)count * item_words;
    const PlainPlan p = cn_plain_plan(ctx->hc, plain_switches(ctx), {count, polys, pstride, P.ntt, a_bcast, nx != nullptr, alias});
    if (p.refusal) return fail(CN_ERR_ARG, "%s", p.refusal);
    uint64_t *arr[PLAIN_ARRAYS] = {nx ? nx->ctn : nullptr, nullptr, nullptr};      // (a chained batch brings its `ctn`: no ensure_scratch, the caller's arena must not move)
    size_t bytes = 0;
    for (uint32_t i = 0; i < p.arrays; i++) bytes += al(p.scratch[i].bytes);
    if (p.arrays) CHECK(ensure_scratch(ctx, bytes));
    for (uint32_t i = 0; i < p.arrays; i++)
        if (!(arr[p.scratch[i].id] = salloc<uint64_t>(ctx, p.scratch[i].bytes / 8))) return fail(CN_ERR_HIP, "internal: scratch exhausted in multiply_plain");
    if (arr[PLAIN_KEEP]) {                                         // one input ciphertext broadcast over the outputs: it must survive until the last block has read it
        HIPCHK(hipMemcpyAsync(arr[PLAIN_KEEP], src, item_words * 8, hipMemcpyDeviceToDevice, ctx->stream));
        src = arr[PLAIN_KEEP];
    }
    const RrOps *rr = rr_ops[p.policy];
    switch (p.form) {
    case PLAIN_BCAST:                                              // transform the ciphertext once, the plaintexts inside the product kernel
        HIPCHK(hipMemcpyAsync(arr[PLAIN_CTN], src, item_words * 8, hipMemcpyDeviceToDevice, ctx->stream));
        CHECK(cn_run_ntt(ctx, arr[PLAIN_CTN], polys * k, 0, k, 0));
        rr->mul_plain_bcast(ctx, P.d, pstride, arr[PLAIN_CTN], o, count, polys, nx ? (uint32_t)nx->elt : 0u, nx ? nx->out : nullptr, P.ntt);
        break;
    case PLAIN_PTN_FUSED:                                          // pstride as given
        rr->mul_plain_fused(ctx, nullptr, 0, 0, const_cast<uint64_t *>(P.d), src, a_bcast ? 0 : item_words, pstride, o, count, polys);
        break;
    case PLAIN_LIFT_FUSED:
        rr->mul_plain_fused(ctx, P.d, pstride ? pstride : 1u, npt, arr[PLAIN_LIFT], src, a_bcast ? 0 : item_words, pstride ? 1u : 0u, o, count, polys);
        break;
    case PLAIN_LEGACY: {
        const uint64_t *lift = P.d;                                // NTT-form plaintexts are multiplied where they lie: no lift, no transform of theirs
        if (!P.ntt) {                                              // lift every referenced plaintext into the k limbs (one launch), NTT them
            hipLaunchKernelGGL(k_lift_plain, dim3(npt * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, P.d, arr[PLAIN_LIFT], ctx->dc, ctx->chunks, pstride ? pstride : 1u);
            HIPCHK(hipGetLastError());
            CHECK(cn_run_ntt(ctx, arr[PLAIN_LIFT], npt * k, 0, k, 0));
            lift = arr[PLAIN_LIFT];
        }
        if (a_bcast) {
            for (uint32_t c = 0; c < count; c++)
                if (o + c * item_words != src) HIPCHK(hipMemcpyAsync(o + c * item_words, src, item_words * 8, hipMemcpyDeviceToDevice, ctx->stream));
        } else if (o != src) HIPCHK(hipMemcpyAsync(o, src, count * item_words * 8, hipMemcpyDeviceToDevice, ctx->stream));
        const uint32_t limbs = count * polys * k;
        CHECK(cn_run_ntt(ctx, o, limbs, 0, k, 0));
        hipLaunchKernelGGL(k_dyadic_pt, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, o, lift, P.ntt ? pstride : (pstride ? 1u : 0u), ctx->dc, ctx->chunks, polys);
        HIPCHK(hipGetLastError());
        CHECK(cn_run_ntt(ctx, o, limbs, 0, k, 1));
        break;
    }
    }
    HIPCHK(hipGetLastError()); launch_count(ctx, p.launches);
    ctx->cnt.ptn_bcast += p.ptn_bcast; ctx->st.ntt_forward_limbs += p.fwd_limbs; ctx->st.ntt_inverse_limbs += p.inv_limbs;
    ctx->st.PlainMultiplication += count;
    return 0;
}
extern "C" int cn_mul_plain(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, uint32_t pstride, cn_handle out, uint32_t oi, uint32_t count) { API_BODY
    LOCK_ONLY; GETCT(A, a, 0); GETCT(O, out, A->size); GETPT_OR_PTN(P, pt);
    SPAN(sa, A, ai, count); SPAN(so, O, oi, count); PTSPAN(sp, P, pi, count, pstride);
    if (queues(ctx, count) && A->size == 2 && !sp.ntt) {       // (an NTT-form operand is never queued: the queue is flushed and the call runs at once)                 // the per-row MultiplyPlain of an unchanged caller: queued, rows merged at flush
        CHECK(plain_not_zero(sp, count)); CHECK(mul_plain_overlap(sa, so, A->item_words));
        return defer_staged(ctx, DOP_MULPLAIN, sa, CtSpan{}, so, 0, sp.d, pstride * ctx->hc.n);
    }
    CHECK(cn_defer_flush(ctx));
    return mul_plain_impl(ctx, sa, false, sp, so, A->size);
API_END }
// ptn[oi + i] = NTT-form of pt[pi + i], i < count: Evaluator.TransformToNtt(plain, parms_id) of SEAL (evaluator.cpp; the reference never calls it - its plaintext
// products transform their operand on every call, EncryptedSealBfvMatrix.cs:79-120).  The words the product kernels read: limb j = NTT_j(lift_j(m)), canonical.
// Only kernel launches: allowed while a graph is recorded; the zero flags travel at call time.
// pt_to_ntt: register-radix sizes ONE launch of k_lift_ntt into the array; other sizes and "legacy_ntt": k_lift_plain + the generic transform (cn_diag_encode writes its
// NTT-form output through it, too)
int pt_to_ntt(cn_ctx *ctx, const uint64_t *src, uint32_t count, uint64_t *dst) {
    const uint32_t k = ctx->hc.k;
    const PlainSwitches sw = plain_switches(ctx);
    if (sw.rr) {
        rr_ops[plain_policy(ctx->hc, sw)]->mul_plain_fused(ctx, src, 1, count, dst, nullptr, 0, 0, nullptr, 0, 0);
        HIPCHK(hipGetLastError()); launch_count(ctx);
        ctx->st.ntt_forward_limbs += (uint64_t)count * k;
        return 0;
    }
    hipLaunchKernelGGL(k_lift_plain, dim3(count * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, src, dst, ctx->dc, ctx->chunks, 1u);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    return cn_run_ntt(ctx, dst, count * k, 0, k, 0);
}
extern "C" int cn_pt_transform(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t count, cn_handle ptn, uint32_t oi) { API_BODY
    LOCK; GETPT(P, pt); GETPTN(O, ptn);
    if (!range_ok(P, pi, count) || !range_ok(O, oi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    CHECK(pt_to_ntt(ctx, P->d + (size_t)pi * ctx->hc.n, count, O->d + (size_t)oi * O->item_words));
    for (uint32_t c = 0; c < count; c++) O->pt_zero[oi + c] = P->pt_zero[pi + c];
    return 0;
API_END }
extern "C" int cn_mul_scalar(cn_ctx *ctx, cn_handle a, uint32_t ai, const uint64_t *scalars, uint32_t sstride, cn_handle out, uint32_t oi, uint32_t count) { API_BODY
    LOCK; GETCT(A, a, 0); GETCT(O, out, A->size);
    if (!range_ok(A, ai, count) || !range_ok(O, oi, count) || !scalars) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    const uint32_t k = ctx->hc.k, ns = sstride ? count : 1;
    std::vector<uint64_t> sc((size_t)ns * k);
    for (uint32_t c = 0; c < ns; c++) {
        uint64_t w = scalars[(size_t)c * sstride];
        if (w >= ctx->hc.t.q) return fail(CN_ERR_ARG, "scalar >= plain modulus");
        if (!w) return fail(CN_ERR_ZERO, "plain cannot be zero");
        for (uint32_t j = 0; j < k; j++) sc[(size_t)c * k + j] = lift_scalar(ctx->hc, w, j);
    }
    CHECK(ensure_scratch(ctx, al(sc.size() * 8)));
    uint64_t *dsc; CHECK(upload_tmp(ctx, sc.data(), sc.size(), &dsc));
    uint32_t limbs = count * A->size * k;
    hipLaunchKernelGGL(k_mul_scalar, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, A->d + ai * A->item_words, dsc, sstride ? 1u : 0u,
                       O->d + oi * O->item_words, ctx->dc, ctx->chunks, A->size);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    ctx->st.PlainMultiplication += count;
    return 0;
API_END }
// ---------------------------------------------------------------- scalar GEMM (planned in cn_gemm_plan.h)
static_assert(GEMM_ERR_ARG == CN_ERR_ARG, "the planner's refusals are argument errors");
// the switches of this context that the planner reads; a change of one drops the cached plans (defer_square_drop_plans)
GemmSwitches gemm_switches(const cn_ctx *ctx) { return {ctx->opt.f64 != 0, ctx->opt.gemm_mfma != 0, ctx->opt.gemm_pair != 0, ctx->opt.digit_mfma != 0, ctx->opt.digit_i32 != 0}; }
int free_gemm_plan(cn_ctx *ctx, Buffer &b) {
    if (b.plan && b.plan->dev) { HIPCHK(hipStreamSynchronize(ctx->stream)); HIPCHK(hipFree(b.plan->dev)); b.plan->dev = nullptr; }
    return 0;
}
int build_gemm_plan(cn_ctx *ctx, const int32_t *idx, const uint64_t *W, uint32_t O, uint32_t K, Buffer *BP, cn_handle bias_pt, const int32_t *bias_idx,
                           GemmPlan &P) {
    if (O && K && W && bias_pt && (!BP || !bias_idx)) return fail(CN_ERR_ARG, "invalid bias plaintext handle");
    const GemmRefusal no = gemm_plan_indices(ctx->hc, gemm_switches(ctx), idx, W, O, K, BP ? bias_idx : nullptr, BP ? BP->count : 0, P, P.host, P.max_in, P.nnz);
    if (no) return fail(no.rc, "%s", no.msg);
    P.O = O; P.has_bias = BP != nullptr; P.bias_pt = bias_pt; P.bias_count = BP ? BP->count : 0;
    return 0;
}
// tables: device image of P.host (scratch or the plan's own allocation)
// in3 (cn_square_gemm): the inputs are the first TWO components of the size-3 products at in3 (P.max_in of them, checked by the caller) instead of the ciphertexts of I
int run_gemm_plan(cn_ctx *ctx, const GemmPlan &P, const char *tables, Buffer *I, Buffer *OB, uint32_t oi, const uint64_t *in3) {
    if (!range_ok(OB, oi, P.O)) return fail(CN_ERR_ARG, "output index out of range");
    if (!in3) {
    if (I == OB) return fail(CN_ERR_ARG, "scalar GEMM cannot run in place");
    if (P.max_in > I->count) return fail(CN_ERR_ARG, "input index out of range");
    // Evaluator::multiply_plain / add take ciphertexts of any size: size 3 = products that have not been relinearized yet (the sum of weighted
    // products is then relinearized once per OUTPUT instead of once per input)
    if (I->size != OB->size || I->size < 2 || I->size > 3) return fail(CN_ERR_ARG, "scalar GEMM: input and output ciphertext sizes must match (2 or 3)");
    } else if (OB->size != 2) return fail(CN_ERR_ARG, "scalar GEMM: output ciphertext size must be 2");
    const uint64_t *bias = nullptr;
    if (P.has_bias) {
        Buffer *BP = getbuf(ctx, P.bias_pt, 1);
        if (!BP || BP->count < P.bias_count) return fail(CN_ERR_ARG, "invalid bias plaintext handle");
        bias = BP->d;
    }
    // the size-3 products of cn_square_gemm: 3 k N words apart, their first two components; else the ciphertexts of I, one after the other
    GemmLaunch gl = gemm_launch(ctx, P, tables).bias_at(bias, tables + P.off_bidx, 0).outputs(OB->d, oi, 0);
    if (in3) gl.inputs(in3, (uint32_t)(3 * ctx->hc.k * ctx->hc.n), 2); else gl.inputs(I->d, 0, I->size);
    CHECK(run_gemm_launch(ctx, P, gl));
    ctx->st.PlainMultiplication += P.nnz; ctx->st.Addition += P.nnz - P.O;
    if (P.has_bias) ctx->st.PlainAddition += P.O;
    return 0;
}
extern "C" int cn_scalar_gemm(cn_ctx *ctx, cn_handle in, const int32_t *idx, const uint64_t *W, uint32_t O, uint32_t K, cn_handle bias_pt,
                              const int32_t *bias_idx, cn_handle out, uint32_t oi) { API_BODY
    LOCK; GETCT(I, in, 0); GETCT(OB, out, 0);
    Buffer *BP = bias_pt ? getbuf(ctx, bias_pt, 1) : nullptr;
    GemmPlan P;
    CHECK(build_gemm_plan(ctx, idx, W, O, K, BP, bias_pt, bias_idx, P));
    CHECK(ensure_scratch(ctx, al(P.host.size())));
    char *tables; CHECK(upload_tmp(ctx, P.host.data(), P.host.size(), &tables));
    return run_gemm_plan(ctx, P, tables, I, OB, oi);
API_END }
// Plan once, apply per inference: the weight tiles and gather tables stay in HBM (cn_free releases the plan).
extern "C" int cn_gemm_plan_create(cn_ctx *ctx, const int32_t *idx, const uint64_t *W, uint32_t O, uint32_t K, cn_handle bias_pt, const int32_t *bias_idx,
                                   cn_handle *plan) { API_BODY
    LOCK; NOT_CAPTURING("cn_gemm_plan_create");
    if (!plan) return fail(CN_ERR_ARG, "null argument");
    Buffer *BP = bias_pt ? getbuf(ctx, bias_pt, 1) : nullptr;
    std::shared_ptr<GemmPlan> P = std::make_shared<GemmPlan>();
    CHECK(build_gemm_plan(ctx, idx, W, O, K, BP, bias_pt, bias_idx, *P));
    HIPCHK(hipMalloc((void **)&P->dev, P->host.size()));
    HIPCHK(hipMemcpy(P->dev, P->host.data(), P->host.size(), hipMemcpyHostToDevice));
    P->host.clear(); P->host.shrink_to_fit();
    Buffer b; b.kind = 2; b.count = O; b.size = 0; b.d = nullptr; b.item_words = 0; b.plan = P;
    *plan = ctx->bufs.insert(std::move(b));
    return 0;
API_END }
extern "C" int cn_gemm_plan_apply(cn_ctx *ctx, cn_handle plan, cn_handle in, cn_handle out, uint32_t oi) { API_BODY
    LOCK; GETCT(I, in, 0); GETCT(OB, out, 0);
    Buffer *PB = getbuf(ctx, plan, 2);
    if (!PB || !PB->plan) return fail(CN_ERR_ARG, "invalid scalar GEMM plan handle");
    return run_gemm_plan(ctx, *PB->plan, PB->plan->dev, I, OB, oi);
API_END }

// ---------------------------------------------------------------- BEHZ multiply / key switching
// the switches of this context that the multiply planner reads (cn_mul_plan.h): the only place that copies them out of a context for the multiply family
MulSwitches mul_switches(const cn_ctx *ctx) {
    return {ctx->opt.f64, ctx->opt.sq_fused, ctx->opt.sq_pipe, ctx->opt.sq_lds, ctx->opt.sq_halves, ctx->opt.mul_sum != 0, ctx->opt.digit_i32 != 0, ctx->opt.defer_square_gemm != 0, rr_kernels(ctx), rr_kernels(ctx, 13),
            ctx->cus, ctx->capturing.load(), ctx->smax, ctx->rlk.d != nullptr, ctx->rlk.f64, ks_switches(ctx), ctx->opt.sg_prefloor};
}
// the context's second stream (squaring overlap): created on first use, kept only if it runs beside the context's own stream (a hardware queue of its own)
bool aux_stream_ready(cn_ctx *ctx) {
    if (ctx->stream2) return true;
    if (ctx->stream2_failed) return false;
    hipStream_t cand[4] = {nullptr, nullptr, nullptr, nullptr};
    int got = -1;
    for (int i = 0; i < 4 && got < 0; i++) {
        if (hipStreamCreateWithFlags(&cand[i], hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); cand[i] = nullptr; break; }
        if (!streams_share_a_queue(cand[i], ctx->stream)) got = i;
    }
    for (int i = 0; i < 4; i++) if (cand[i] && i != got) (void)hipStreamDestroy(cand[i]);
    if (got < 0 || hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (got >= 0) (void)hipStreamDestroy(cand[got]);
        ctx->stream2_failed = true;
        return false;
    }
    ctx->stream2 = cand[got];
    return true;
}
// a, b: pointers to first operand ciphertext (size 2); out3: [cnt][3][k][N]; scratch must be ensured by caller.  atab / btab: one
// operand address per ciphertext instead of a + ct*astride*ctw (deferred per-ciphertext calls; atab == btab: squarings).  What is launched: MulPlan (cn_mul_plan.h)
int do_multiply(cn_ctx *ctx, const uint64_t *a, uint32_t astride, const uint64_t *b, uint32_t bstride, uint64_t *out3, uint32_t cnt,
                       const uint64_t *const *atab, const uint64_t *const *btab, const MulKeep *keep) {
    const uint32_t n = ctx->hc.n, k = ctx->hc.k, kb = ctx->hc.kb;
    const bool square = atab ? atab == btab : (a == b && astride == bstride);
    MulPlan p = cn_mul_plan(ctx->hc, mul_switches(ctx), square, cnt);
    if (keep && (p.form != MUL_SQUARE_FUSED || !p.lazy || p.bsk.sq == SQ_PLAIN)) return fail(CN_ERR_ARG, "internal: kept tensor words without the fused squaring kernels");
    if (keep) p.bsk.ntt01 = true;
    uint64_t *arr[MUL_ARRAYS] = {};
    for (uint32_t i = 0; i < p.arrays; i++) {
        if (keep && (p.scratch[i].id == MUL_DQ || p.scratch[i].id == MUL_DB)) { arr[p.scratch[i].id] = p.scratch[i].id == MUL_DQ ? keep->dq : keep->db; continue; }
        if (!(arr[p.scratch[i].id] = (uint64_t *)salloc<char>(ctx, p.scratch[i].bytes))) return fail(CN_ERR_HIP, "internal: scratch exhausted in multiply");
    }
    uint64_t *const aq = arr[MUL_AQ], *const ab = arr[MUL_AB], *const bq = square ? aq : arr[MUL_BQ], *const bb = square ? ab : arr[MUL_BB], *const dq = arr[MUL_DQ], *const db = arr[MUL_DB];
    CHECK(cn_l_behz_extend(ctx, a, astride, atab, aq, ab, cnt, p.behz_f64));
    if (!square) CHECK(cn_l_behz_extend(ctx, b, bstride, btab, bq, bb, cnt, p.behz_f64));
    const char *const no_kernel = "internal: tensor form without a kernel of its policy";
    if (p.form == MUL_SQUARE_FUSED) {
        if (!rr_ops[p.q.policy]->square_fused(ctx, a, (size_t)astride * 2 * k * n, atab, dq, cnt, 0, k, p.q)) return fail(CN_ERR_ARG, no_kernel);
        if (!rr_ops[p.bsk.policy]->square_fused(ctx, ab, (size_t)2 * kb * n, nullptr, db, cnt, k, kb, p.bsk)) return fail(CN_ERR_ARG, no_kernel);
        launch_count(ctx, 2);
        ctx->st.ntt_forward_limbs += (uint64_t)cnt * 2 * (k + kb); ctx->st.ntt_inverse_limbs += (uint64_t)cnt * (3 * k + (keep ? 1 : 3) * kb);
    } else {
        CHECK(cn_run_ntt(ctx, aq, cnt * 2 * k, 0, k, 0)); CHECK(cn_run_ntt(ctx, ab, cnt * 2 * kb, k, kb, 0));
        if (!square) { CHECK(cn_run_ntt(ctx, bq, cnt * 2 * k, 0, k, 0)); CHECK(cn_run_ntt(ctx, bb, cnt * 2 * kb, k, kb, 0)); }
        if (p.form == MUL_INTT_TENSOR) {
            if (!rr_ops[p.q.policy]->intt_tensor(ctx, aq, bq, dq, cnt, 0, k, p.lazy)) return fail(CN_ERR_ARG, no_kernel);
            if (!rr_ops[p.bsk.policy]->intt_tensor(ctx, ab, bb, db, cnt, k, kb, p.lazy)) return fail(CN_ERR_ARG, no_kernel);
            launch_count(ctx, 2);
            ctx->st.ntt_inverse_limbs += (uint64_t)cnt * 3 * (k + kb);
        } else {
            hipLaunchKernelGGL(k_tensor, dim3(cnt * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, aq, bq, dq, ctx->dc, ctx->chunks, k, 0u);
            hipLaunchKernelGGL(k_tensor, dim3(cnt * kb * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, ab, bb, db, ctx->dc, ctx->chunks, kb, k);
            HIPCHK(hipGetLastError()); launch_count(ctx, 2);
            CHECK(cn_run_ntt(ctx, dq, cnt * 3 * k, 0, k, 1)); CHECK(cn_run_ntt(ctx, db, cnt * 3 * kb, k, kb, 1));
        }
    }
    HIPCHK(hipGetLastError());
    if (keep) CHECK(cn_l_behz_floor_c2(ctx, dq, db, out3, cnt)); else CHECK(cn_l_behz_floor(ctx, dq, db, out3, cnt, p.behz_f64, p.lazy));
    ctx->st.Multiplication += cnt;
    return 0;
}
template <int EPT> static void launch_ks_legacy(cn_ctx *c, uint32_t nt, const KsArgs &a) {
    hipLaunchKernelGGL(k_keyswitch<EPT>, dim3(a.cnt * c->hc.k), dim3(nt), (size_t)c->hc.n * 8, c->stream, a.target, a.tstride, a.add0, a.add1, a.astride, a.key,
                       a.out, c->dc, a.galois, a.out_tab);
}
int ensure_ks_part(cn_ctx *ctx, size_t need) {
    if (need <= ctx->ks_part_cap) return 0;
    if (ctx->capturing || ctx->graphs_alive) return fail(CN_ERR_ARG, "the key-switch arena would have to grow while a graph is recorded / alive: run the sequence once before cn_graph_begin");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->ks_part) HIPCHK(hipFree(ctx->ks_part));
    ctx->ks_part = nullptr; ctx->ks_part_cap = 0;
    HIPCHK(hipMalloc(&ctx->ks_part, need));
    ctx->ks_part_cap = need;
    return 0;
}
// the switches of this context that the key-switch planner reads (cn_ks_plan.h); CN_KS_DIGIT_MAX / CN_KS_WIDE_MAX override the two block thresholds (A/B), read once
KsSwitches ks_switches(const cn_ctx *ctx) {
    static const uint32_t digit_max = getenv("CN_KS_DIGIT_MAX") ? (uint32_t)atoi(getenv("CN_KS_DIGIT_MAX")) : 10u;
    static const uint32_t wide_max = getenv("CN_KS_WIDE_MAX") ? (uint32_t)atoi(getenv("CN_KS_WIDE_MAX")) : 160u;
    return {ctx->opt.ks_wide, ctx->opt.ks_split14, ctx->opt.ks_pair14, ctx->opt.ks_xcd, ctx->opt.ks_perm_fused, rr_kernels(ctx), ctx->hc.twdh != nullptr, digit_max, wide_max, ctx->smax};
}
KsPlan ks_plan(const cn_ctx *ctx, const KsKey &key, uint32_t cnt, int galois) { return cn_ks_plan(ctx->hc, ks_switches(ctx), key.f64, cnt, galois); }
// One key switch.  call: the operands by name (KsCall, cn_runtime.h); the key words and the plan (cn_ks_plan.h: form, accmax, xcd_cts, arena bytes) are added here.
// perm_elt != 0 (two-launch forms only - the caller asks ks_perm_on_load first): target / add0 are the c1 / c0 of the ciphertext a rotation
// READS and the kernels apply the automorphism x -> x^perm_elt while loading them
// KS_PAIR14 (N = 16384): one launch per key switch.  A rotation then hands in target = sigma(c1) (permuted ahead of time: k_galois_limbs, or the
// previous link of a rotate-and-add chain), add0 = the unpermuted c0 and perm_elt; next_elt / next_out ask for sigma_next of the new c1 on the side.
int do_keyswitch(cn_ctx *ctx, const KsKey &key, const KsCall &call) {
    const uint32_t n = ctx->hc.n, k = ctx->hc.k, cnt = call.cnt, tot_dig = call.galois ? ctx->hc.gk_tot : ctx->hc.rl_tot;
    KsArgs a{call, key.d, ks_plan(ctx, key, cnt, call.galois)};
    const KsRefusal no = ks_refusal(ctx->hc, a.plan, key.f64, a.galois, {a.dig != nullptr, a.perm_elt != 0, a.items != nullptr, a.next_elt != 0});
    if (no) return fail(no.rc, "%s", no.msg);
    CHECK(ensure_ks_part(ctx, a.plan.arena_bytes));
    switch (a.plan.form) {
        case KS_LEGACY: {                   // radix-2 LDS (N < 1024, legacy_ntt): no fused accumulator -> one element-wise add behind it
            // The accumulator may be the result's own array (SumAllSlots adds in place): the key switch then writes into the key-switch arena
            // (unused by this path) and the add reads it beside the untouched accumulator.  (Writing `out` first doubled the key switch there.)
            uint64_t *const out = a.out;
            if (a.extra) {
                if (a.xstride != ctx->ctw2 || a.out_tab) return fail(CN_ERR_ARG, "internal: accumulator stride");
                CHECK(ensure_ks_part(ctx, (size_t)cnt * ctx->ctw2 * 8));
                a.out = (uint64_t *)ctx->ks_part;
            }
            const uint32_t nt = std::min<uint32_t>(1024, n);
            switch (n / nt) {
                case 1: launch_ks_legacy<1>(ctx, nt, a); break;
                case 2: launch_ks_legacy<2>(ctx, nt, a); break;
                case 4: launch_ks_legacy<4>(ctx, nt, a); break;
                case 8: launch_ks_legacy<8>(ctx, nt, a); break;
                case 16: launch_ks_legacy<16>(ctx, nt, a); break;
                default: return fail(CN_ERR_ARG, "unsupported poly modulus degree for key switching");
            }
            if (a.extra) {
                hipLaunchKernelGGL(k_addsub, dim3(cnt * 2 * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, (const uint64_t *)ctx->ks_part, a.extra, out, ctx->dc,
                                   ctx->chunks, 0);
                launch_count(ctx);
            }
            break;
        }
        default:
            if (!ks_ops[a.plan.policy]->launch(ctx, a)) return fail(CN_ERR_ARG, "internal: key-switch form without a kernel of its policy");
            if (a.plan.form == KS_SPLIT14) {        // the halves of k_keyswitch_split14 lie in ks_part: the combining pass (rounds 1-4; A/B)
                hipLaunchKernelGGL(k_ks_combine14, dim3(cnt * 2 * k * (n / 512)), dim3(256), 0, ctx->stream, (const uint64_t *)ctx->ks_part, a.add0, a.add1, a.astride, a.out, ctx->dc,
                                   a.extra, a.xstride, a.out_tab);
                launch_count(ctx);
            }
    }
    HIPCHK(hipGetLastError()); launch_count(ctx);
    if (a.dig && a.dig_i32) ctx->cnt.ks_dig_i32++;
    ctx->st.ntt_forward_limbs += (uint64_t)cnt * tot_dig * k; ctx->st.ntt_inverse_limbs += (uint64_t)cnt * 2 * k;
    return 0;
}
// Multiply + Relinearize of `count` products in the chunks of mul_batch: per chunk the address tables (if any), the size-3 products, the multiply and ONE key switch -
// or the same in parts over the two streams (mul_pipeline_parts, pipelined_halves).  Chunks and parts write results while later ones still read operands
int run_mul_relin(cn_ctx *ctx, const MulRelinCall &m, uint32_t count, MulSite site, int sq_halves_min) {
    const size_t kn = (size_t)ctx->hc.k * ctx->hc.n, ctw = ctx->ctw2;
    const bool square = m.ha ? m.ha == m.hb : (m.a == m.b && m.astride == m.bstride);
    const MulSwitches sw = mul_switches(ctx);
    return mul_chunks(ctx, mul_batch(ctx->hc, sw, site, count, square), count, true, [&](uint32_t s, uint32_t c) -> int {
        const uint64_t **da = nullptr, **db = nullptr; uint64_t **dout = nullptr;
        if (m.ha) {
            CHECK(upload_tmp(ctx, m.ha + s, c, &da));
            db = da;
            if (!square) CHECK(upload_tmp(ctx, m.hb + s, c, &db));
        }
        if (m.ho) CHECK(upload_tmp(ctx, m.ho + s, c, &dout));
        uint64_t *t3 = salloc<uint64_t>(ctx, (size_t)c * 3 * kn);
        if (!t3) return fail(CN_ERR_HIP, "internal: scratch exhausted in multiply + relinearize");
        auto mul = [&](uint32_t f, uint32_t n_) {
            if (m.ha) return do_multiply(ctx, nullptr, 1, nullptr, 1, t3 + (size_t)f * 3 * kn, n_, da + f, db + f);
            return do_multiply(ctx, m.a + (size_t)(s + f) * m.astride * ctw, m.astride, m.b + (size_t)(s + f) * m.bstride * ctw, m.bstride, t3 + (size_t)f * 3 * kn, n_);
        };
        auto ksw = [&](uint32_t f, uint32_t n_) {
            KsCall ks = KsCall::relin(t3 + (size_t)f * 3 * kn, kn, n_);
            return do_keyswitch(ctx, ctx->rlk, m.ho ? ks.to_table(dout + f) : ks.to(m.out + (size_t)(s + f) * ctw));
        };
        uint32_t first[4];
        if (mul_pipeline_parts(ctx->hc, sw, c, sq_halves_min, first) && aux_stream_ready(ctx)) return pipelined_halves(ctx, c, mul, ksw);
        CHECK(mul(0, c));
        return ksw(0, c);
    });
}

extern "C" int cn_multiply(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out3, uint32_t oi, uint32_t count) { API_BODY TWO_LIMBS("cn_multiply");
    LOCK; GETCT(A, a, 2); GETCT(B, b, 2); GETCT(O, out3, 3);
    if (!range_ok(A, ai, count) || !range_ok(B, bi, count) || !range_ok(O, oi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    const uint64_t *pa = A->d + ai * A->item_words, *pb = B->d + bi * B->item_words;
    return mul_chunks(ctx, mul_batch(ctx->hc, mul_switches(ctx), MUL_AT_MULTIPLY, count, pa == pb), count, true, [&](uint32_t s, uint32_t c) {
        return do_multiply(ctx, pa + s * A->item_words, 1, pb + s * B->item_words, 1, O->d + (oi + s) * O->item_words, c);
    });
API_END }
extern "C" int cn_relinearize(cn_ctx *ctx, cn_handle in3, uint32_t ii, cn_handle out, uint32_t oi, uint32_t count) { API_BODY TWO_LIMBS("cn_relinearize");
    LOCK; GETCT(I, in3, 3); GETCT(O, out, 2);
    if (!range_ok(I, ii, count) || !range_ok(O, oi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!ctx->rlk.d) return fail(CN_ERR_NOKEY, "relinearization keys not set");
    if (!count) return 0;
    const size_t kn = (size_t)ctx->hc.k * ctx->hc.n;
    const uint64_t *p = I->d + ii * I->item_words;
    CHECK(do_keyswitch(ctx, ctx->rlk, KsCall::relin(p, kn, count).to(O->d + oi * O->item_words)));
    ctx->st.Relinarization += count;
    return 0;
API_END }
// cn_mul_relin: does [oi, oi + count) of `out` intersect the span operand x reads - [xi, xi + (count - 1) xstride] - in the same handle, other than as exactly the same
// range (in place)?  Chunks and pipelined parts write results while later ones still read operands: such calls are refused.  Handles and indices only (no lookup):
// also checked before a call is published without the lock (defer = 2)
static int mul_relin_overlap(cn_handle x, uint32_t xi, uint32_t xstride, cn_handle out, uint32_t oi, uint32_t count) {
    if (x != out || !count) return 0;
    const uint64_t lo = xi, hi = (uint64_t)xi + (uint64_t)(count - 1) * xstride + 1, olo = oi, ohi = (uint64_t)oi + count;
    if ((lo == olo && hi == ohi) || hi <= olo || ohi <= lo) return 0;
    return fail(CN_ERR_ARG, "mul_relin: an operand range and the result range overlap partially (use the same range or disjoint ranges)");
}
extern "C" int cn_mul_relin(cn_ctx *ctx, cn_handle a, uint32_t ai, uint32_t astride, cn_handle b, uint32_t bi, uint32_t bstride, cn_handle out,
                            uint32_t oi, uint32_t count) {
    TWO_LIMBS("cn_mul_relin");
    CHECK(mul_relin_overlap(a, ai, astride, out, oi, count)); CHECK(mul_relin_overlap(b, bi, bstride, out, oi, count));
    if (submit_async(ctx) && count <= DEFER_STAGED_MAX) return ring_push(ctx, SUB_MUL_RELIN, count, a, ai, b, bi, out, oi, astride, bstride);      // PointwiseMultiply of one column
    API_BODY LOCK_ONLY; return mul_relin_body(ctx, a, ai, astride, b, bi, bstride, out, oi, count); API_END
}
int mul_relin_body(cn_ctx *ctx, cn_handle a, uint32_t ai, uint32_t astride, cn_handle b, uint32_t bi, uint32_t bstride, cn_handle out, uint32_t oi, uint32_t count) {
    CHECK(mul_relin_overlap(a, ai, astride, out, oi, count)); CHECK(mul_relin_overlap(b, bi, bstride, out, oi, count));
    if (deferring(ctx)) return defer_mul_relin(ctx, a, ai, astride, b, bi, bstride, out, oi, count);
    CHECK(cn_defer_flush(ctx));
    GETCT(A, a, 2); GETCT(B, b, 2); GETCT(O, out, 2);
    if (!range_ok(A, ai, astride ? count : 1, astride ? astride : 1) || !range_ok(B, bi, bstride ? count : 1, bstride ? bstride : 1) || !range_ok(O, oi, count))
        return fail(CN_ERR_ARG, "index out of range");
    if (!ctx->rlk.d) return fail(CN_ERR_NOKEY, "relinearization keys not set");
    if (!count) return 0;
    MulRelinCall m;
    m.a = A->d + ai * A->item_words; m.astride = astride; m.b = B->d + bi * B->item_words; m.bstride = bstride; m.out = O->d + oi * O->item_words;
    CHECK(run_mul_relin(ctx, m, count, MUL_AT_MUL_RELIN, 1));
    ctx->st.Relinarization += count;
    return 0;
}

// ---------------------------------------------------------------- squaring layer + dense layer in one call
// SquareActivation relinearizes every product, ct_k = (d0_k + KS0(d2_k), d1_k + KS1(d2_k)), and the PoolLayer behind it forms out_o = sum_k w_ok ct_k.  A key switch is
// linear over Z_{q_j} in the DIGITS of its operand - digit extraction is its only non-linear step and comes first - and so is the scalar GEMM, hence word for word
//   sum_k w_ok KSc(d2_k)[j] = INTT_j( sum_{l,d} NTT_j(S_{o,l,d}) K^c_{l,d,j} ),   S_{o,l,d} = sum_k w_ok dig_{k,l,d}   (a plain integer, the same for every j).
// The pair therefore needs one key switch per dense OUTPUT, fed with the weight-combined digit polynomials S (k_digit_gemm), not one per input: 100 + 10 instead of
// 845 + 100 for CryptoNets, the same ciphertext words.  (Not forward_relinearize_late's "relinearize the sum": there the digits are those of the sum.)
// Runs when the plan allows it (GemmPlan::dig: small weights, |S| below every q_j / 2 and 2^52), every modulus and the key are on an FP64 policy, the ring has the
// register-radix kernels up to N = 8192 and the decomposition is the plain one; anything else takes the two separate steps inside the same call.
// (square_gemm_fused_ok and square_gemm_ctx_ok, cn_mul_plan.h; the product loop in the chunks of mul_batch)
// The pre-floor form (square_gemm_prefloor_ok, "sg_prefloor"): the fast floor is linear too, in the Bsk residues of the tensor and in the canonical y of its q
// residues - so components 0 and 1 are not floored per input either: the Bsk words of d0, d1 stay in NTT form, the plan's weights sum them mod b and their y as exact
// integers, and ONE floor tail per output (+ bias) writes what the GEMM over the floored words wrote.  Component 2 keeps its floor: its digits are cut per product.
extern "C" int cn_square_gemm(cn_ctx *ctx, cn_handle plan, cn_handle in, uint32_t ii, cn_handle out, uint32_t oi) { TWO_LIMBS("cn_square_gemm"); API_BODY
    LOCK; GETCT(I, in, 2); GETCT(OB, out, 2);
    Buffer *PB = getbuf(ctx, plan, 2);
    if (!PB || !PB->plan) return fail(CN_ERR_ARG, "invalid scalar GEMM plan handle");
    const GemmPlan &P = *PB->plan;
    const uint32_t cnt = P.max_in;
    if (!range_ok(I, ii, cnt)) return fail(CN_ERR_ARG, "input index out of range");
    if (!range_ok(OB, oi, P.O)) return fail(CN_ERR_ARG, "output index out of range");
    if (I == OB) return fail(CN_ERR_ARG, "cn_square_gemm cannot run in place");
    if (!ctx->rlk.d) return fail(CN_ERR_NOKEY, "relinearization keys not set");
    const uint32_t n = ctx->hc.n, k = ctx->hc.k, tot = ctx->hc.rl_tot;
    const size_t kn = (size_t)k * n;
    const MulSwitches sw = mul_switches(ctx);
    MulBatch B = mul_batch(ctx->hc, sw, MUL_AT_SQUARE_GEMM, cnt, true, P.O, P.dig_i32);
    // the pre-floor form (square_gemm_prefloor_ok, cn_mul_plan.h) where its arrays fit beside the old form's; else the old form with the old chunks
    bool pre = B.fits && square_gemm_prefloor_ok(ctx->hc, sw, P);
    const SgPrefloorScratch PS = square_gemm_prefloor_scratch(ctx->hc, cnt, P.O);
    if (pre) {
        if (B.fixed + PS.total + B.per > sw.smax) pre = false;
        else { B.fixed += PS.total; B.chunk = (uint32_t)std::min<size_t>(cnt, (sw.smax - B.fixed) / B.per); }
    }
    if (!square_gemm_fused_ok(ctx->hc, sw, P) || !B.fits) {                       // the two steps as they are: square + relinearize into a temporary, the GEMM from it
        cn_handle tmp = 0;
        CHECK(alloc_buf(ctx, 0, cnt, 2, &tmp));
        int rc = mul_relin_body(ctx, in, ii, 1, in, ii, 1, tmp, 0, cnt);
        if (!rc) rc = cn_defer_flush(ctx);                                        // (a context that queues its calls has queued this one)
        OB = getbuf(ctx, out, 0);                                                 // the handle table may have moved
        if (!rc) rc = run_gemm_plan(ctx, P, P.dev, getbuf(ctx, tmp, 0), OB, oi);
        const int rf = free_body(ctx, tmp);
        return rc ? rc : rf;
    }
    CHECK(ensure_scratch(ctx, B.ensure(B.chunk)));
    uint64_t *t3 = salloc<uint64_t>(ctx, (size_t)cnt * 3 * kn);
    void *S = salloc<char>(ctx, (size_t)P.O * tot * n * (P.dig_i32 ? 4 : 8));     // int32 words where the plan's digit bound allows (GemmPlan::dig_i32)
    if (!t3 || !S) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_square_gemm");
    const uint64_t *pa = I->d + ii * I->item_words;
    uint64_t *sg[SG_ARRAYS] = {};
    if (pre) for (const auto &a : PS.scratch) if (!(sg[a.id] = (uint64_t *)salloc<char>(ctx, a.bytes))) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_square_gemm");
    const size_t kbn = (size_t)ctx->hc.kb * n;
    CHECK(mul_chunks(ctx, B, cnt, false, [&](uint32_t s, uint32_t c) {           // the products, all of them, before the first sum
        const MulKeep keep{sg[SG_DQ] + (size_t)s * 3 * kn, sg[SG_DB] + (size_t)s * 3 * kbn};
        return do_multiply(ctx, pa + (size_t)s * I->item_words, 1, pa + (size_t)s * I->item_words, 1, t3 + (size_t)s * 3 * kn, c, nullptr, nullptr, pre ? &keep : nullptr);
    }));
    if (pre) {
        // components 0 and 1: X = the weighted sums of the NTT-form Bsk words, back to coefficients once per output; Y = the exact sums of the canonical y; one floor
        // tail per output (+ bias) straight into the outputs.  The plan's own tables and weight fragments
        const uint64_t *bias = nullptr;
        if (P.has_bias) {
            Buffer *BP = getbuf(ctx, P.bias_pt, 1);
            if (!BP || BP->count < P.bias_count) return fail(CN_ERR_ARG, "invalid bias plaintext handle");
            bias = BP->d;
        }
        CHECK(cn_l_gemm_mfma(ctx, gemm_launch(ctx, P, P.dev).inputs(sg[SG_DB], (uint32_t)(3 * kbn), 2).outputs(sg[SG_X], 0, (uint32_t)(2 * kbn)).prefloor(1)));
        CHECK(cn_l_gemm_mfma(ctx, gemm_launch(ctx, P, P.dev).inputs(sg[SG_DQ], (uint32_t)(3 * kn), 2).outputs(sg[SG_Y], 0, (uint32_t)(2 * kn)).prefloor(2)));
        CHECK(cn_run_ntt(ctx, sg[SG_X], P.O * 2 * ctx->hc.kb, k, ctx->hc.kb, 1));
        CHECK(cn_l_behz_floor_out(ctx, {sg[SG_X], sg[SG_Y], (const int32_t *)(P.dev + P.off_oidx), bias, (const int32_t *)(P.dev + P.off_bidx), OB->d, oi, P.G * P.M}));
        ctx->st.PlainMultiplication += P.nnz; ctx->st.Addition += P.nnz - P.O;
        if (P.has_bias) ctx->st.PlainAddition += P.O;
        ctx->cnt.sg_prefloor++;
    } else
    CHECK(run_gemm_plan(ctx, P, P.dev, nullptr, OB, oi, t3));                     // components 0 and 1 (+ bias) straight into the outputs
    CHECK(cn_l_digit_gemm(ctx, DigitGemmLaunch::of(P, P.dev, t3 + 2 * kn, 3 * kn, P.dev, S)));
    uint64_t *o = OB->d + oi * OB->item_words;
    CHECK(do_keyswitch(ctx, ctx->rlk, KsCall::relin_digits(S, P.dig_i32, o, kn, P.O).to(o)));
    ctx->st.Relinarization += cnt; ctx->cnt.sg_fused++;
    return 0;
API_END }

// ---------------------------------------------------------------- sum of encrypted x encrypted products in one call
// DenseMatrixBySparseVectorMultiply with both operands encrypted (AtomicSealBfvVector.cs:459-465,502) and DotProduct of two encrypted dense vectors (:839-840,
// 888-900) form out = sum_k Relinearize(Multiply(a_k, b_k)).  With ct_k = (d0_k + KS0(d2_k), d1_k + KS1(d2_k)) this is the identity above with unit weights:
//   out = (sum_k d0_k, sum_k d1_k) + KS(S),   S_(l,d) = sum_k digit_(l,d)(d2_k)   - the digits cut per product, before the sum: the reference's words,
// K multiplies and ONE key switch per output instead of K.  k_product_sum forms the three sums in one pass over the products.
// The fused form runs when mul_sum_fused_ok holds (cn_mul_plan.h: the switches, K and the kernel's numeric bounds) and the scratch limit leaves room for the products
// of one output (mul_sum_batch); anything else takes the literal sequence - cn_mul_relin per term into a temporary, AddMany per output - inside the same call.
// AddMany of the K terms of every output out of the temporary of the literal sequence (term k of output i at k * count + i): one table, one launch per output
static int add_many_terms(cn_ctx *ctx, Buffer *T, uint32_t K, Buffer *O, uint32_t oi, uint32_t count) {
    std::vector<uint32_t> idx((size_t)count * K);
    for (uint32_t i = 0; i < count; i++) for (uint32_t kk = 0; kk < K; kk++) idx[(size_t)i * K + kk] = kk * count + i;
    CHECK(ensure_scratch(ctx, al(idx.size() * 4) + 4096));
    uint32_t *didx; CHECK(upload_tmp(ctx, idx.data(), idx.size(), &didx));
    const uint32_t limbs = T->size * ctx->hc.k;
    for (uint32_t i = 0; i < count; i++) {
        hipLaunchKernelGGL(k_add_many, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, T->d, didx + (size_t)i * K, K, T->item_words,
                           O->d + (oi + i) * O->item_words, ctx->dc, ctx->chunks);
        HIPCHK(hipGetLastError()); launch_count(ctx);
    }
    return 0;
}
extern "C" int cn_mul_relin_sum(cn_ctx *ctx, const cn_handle *a, const uint32_t *a_idx, const cn_handle *b, const uint32_t *b_idx, uint32_t K, uint32_t b_stride,
                                cn_handle out, uint32_t oi, uint32_t count) { TWO_LIMBS("cn_mul_relin_sum"); API_BODY
    LOCK;
    if (!a || !b) return fail(CN_ERR_ARG, "null argument");
    if (!K || !count) return fail(CN_ERR_ARG, "cn_mul_relin_sum of an empty list");
    if (b_stride > 1) return fail(CN_ERR_ARG, "cn_mul_relin_sum: b_stride is 0 (one ciphertext for every output) or 1");
    if ((uint64_t)K * count > 0x7fffffffull) return fail(CN_ERR_ARG, "cn_mul_relin_sum: too many products");
    GETCT(O, out, 2);
    if (!range_ok(O, oi, count)) return fail(CN_ERR_ARG, "output index out of range");
    auto ai = [&](uint32_t kk) { return a_idx ? a_idx[kk] : 0u; };
    auto bi = [&](uint32_t kk) { return b_idx ? b_idx[kk] : 0u; };
    for (uint32_t kk = 0; kk < K; kk++) {
        if (a[kk] == out || b[kk] == out) return fail(CN_ERR_ARG, "cn_mul_relin_sum cannot run in place (out is an operand handle)");
        Buffer *A = getbuf(ctx, a[kk], 0), *B = getbuf(ctx, b[kk], 0);
        if (!A || !B) return fail(CN_ERR_ARG, "invalid ciphertext handle in term %u", kk);
        if (A->size != 2 || B->size != 2) return fail(CN_ERR_ARG, "ciphertext size mismatch in term %u", kk);
        if (!range_ok(A, ai(kk), count) || !range_ok(B, bi(kk), b_stride ? count : 1)) return fail(CN_ERR_ARG, "index out of range in term %u", kk);
    }
    if (!ctx->rlk.d) return fail(CN_ERR_NOKEY, "relinearization keys not set");
    ctx->ms_groups = 0;
    const uint32_t n = ctx->hc.n, k = ctx->hc.k, tot = ctx->hc.rl_tot;
    const size_t kn = (size_t)k * n;
    if (K == 1) {                                                                 // one term per output: Multiply + Relinearize straight into the outputs
        int rc = mul_relin_body(ctx, a[0], ai(0), 1, b[0], bi(0), b_stride, out, oi, count);
        if (!rc) rc = cn_defer_flush(ctx);                                        // (a context that queues its calls has queued this one)
        if (!rc) { ctx->st.AddMany += count; ctx->st.AddManyItemCount += count; }
        return rc;
    }
    const MulSwitches sw = mul_switches(ctx);
    const MulSumBatch G = mul_sum_batch(ctx->hc, sw, K, count);                   // outputs per group, S as int32 words
    const bool s32 = G.s32;
    const uint32_t g = G.group;
    if (!mul_sum_fused_ok(ctx->hc, sw, K) || !g) {                                    // the literal sequence: Multiply + Relinearize per term into a temporary, AddMany per output
        cn_handle tmp = 0;
        CHECK(alloc_buf(ctx, 0, K * count, 2, &tmp));
        int rc = 0;
        for (uint32_t kk = 0; kk < K && !rc; kk++) rc = mul_relin_body(ctx, a[kk], ai(kk), 1, b[kk], bi(kk), b_stride, tmp, kk * count, count);
        if (!rc) rc = cn_defer_flush(ctx);
        if (!rc) rc = add_many_terms(ctx, getbuf(ctx, tmp, 0), K, getbuf(ctx, out, 0), oi, count);      // (the handle table may have moved)
        if (!rc) { ctx->st.AddMany += count; ctx->st.AddManyItemCount += (uint64_t)count * K; }
        const int rf = free_body(ctx, tmp);
        return rc ? rc : rf;
    }
    std::vector<const uint64_t *> ha((size_t)g * K), hb((size_t)g * K);
    for (uint32_t o0 = 0; o0 < count; o0 += g) {                                  // the groups, one after the other
        const uint32_t go = std::min(g, count - o0), np = go * K;
        const MulBatch B = mul_batch(ctx->hc, sw, MUL_AT_SUM_GROUP, np, false, go, s32);
        CHECK(ensure_scratch(ctx, B.ensure(B.chunk)));
        uint64_t *t3 = salloc<uint64_t>(ctx, (size_t)np * 3 * kn);
        void *S = salloc<char>(ctx, (size_t)go * tot * n * (s32 ? 4 : 8));
        if (!t3 || !S) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_mul_relin_sum");
        for (uint32_t i = 0; i < go; i++) for (uint32_t kk = 0; kk < K; kk++) {
            const Buffer *A = getbuf(ctx, a[kk], 0), *B = getbuf(ctx, b[kk], 0);
            ha[(size_t)i * K + kk] = A->d + (size_t)(ai(kk) + o0 + i) * A->item_words;
            hb[(size_t)i * K + kk] = B->d + (size_t)(bi(kk) + (o0 + i) * b_stride) * B->item_words;
        }
        const uint64_t **da, **db;
        CHECK(upload_tmp(ctx, ha.data(), np, &da)); CHECK(upload_tmp(ctx, hb.data(), np, &db));
        CHECK(mul_chunks(ctx, B, np, false, [&](uint32_t s, uint32_t c) {        // the products, all of them, before the sum
            return do_multiply(ctx, nullptr, 1, nullptr, 1, t3 + (size_t)s * 3 * kn, c, da + s, db + s);
        }));
        uint64_t *o = O->d + (size_t)(oi + o0) * O->item_words;
        CHECK(cn_l_product_sum(ctx, ProductSumLaunch{t3, K, o, S, go, s32}));     // (sum d0, sum d1) straight into the outputs, the digit sums into S
        CHECK(do_keyswitch(ctx, ctx->rlk, KsCall::relin_digits(S, s32, o, kn, go).to(o)));
        ctx->ms_groups++;
    }
    ctx->st.Relinarization += (uint64_t)K * count; ctx->st.AddMany += count; ctx->st.AddManyItemCount += (uint64_t)count * K;
    ctx->cnt.ms_fused++;
    return 0;
API_END }

// ---------------------------------------------------------------- rotations
const KsKey *galois_key(cn_ctx *ctx, uint64_t elt) { auto it = ctx->gk.find(elt); return it != ctx->gk.end() && it->second.d ? &it->second : nullptr; }
static int columns_key(cn_ctx *ctx) { return galois_key(ctx, 2ull * ctx->hc.n - 1) ? 0 : fail(CN_ERR_NOKEY, "Galois key not present"); }
// The rotate-and-ADD forms refuse an operand or accumulator that overlaps the result with a shift: the fused accumulator is read where the result is stored, no path
// reads it ahead of the stores
static int add_overlap(cn_ctx *ctx, const uint64_t *in, const uint64_t *acc, const uint64_t *out, uint32_t count) {
    if (!shifted_overlap(in, out, count * ctx->ctw2) && !shifted_overlap(acc, out, count * ctx->ctw2)) return 0;
    return fail(CN_ERR_ARG, "rotate-and-add: operand / accumulator and result ranges overlap partially (use the same range or disjoint ranges)");
}
// in / out: `count` size-2 ciphertexts each, tmp holds as many; acc: out = acc + galois(in) in the same launches (acc may alias out and/or in)
// pre: sigma_elt(c1) of `in` if somebody has produced it already ([ct][k][N]); next_elt / next_out: see KsCall (both only on the one-launch N = 16384 path)
int do_galois(cn_ctx *ctx, const GaloisCall &g) {
    const KsKey *key = galois_key(ctx, g.elt);
    if (!key) return fail(CN_ERR_NOKEY, "Galois key not present");
    const size_t kn = (size_t)ctx->hc.k * ctx->hc.n;
    const uint32_t count = g.count, limbs = count * 2 * ctx->hc.k, elt = (uint32_t)g.elt;
    // A result range that overlaps the operand range with a SHIFT (the same handle, different first indices): the kernels that apply the automorphism while they
    // load (one-launch N = 16384 kernel, two-launch small-batch kernels) would read ciphertext c after another workgroup has written c' over it - safe when the two
    // arrays are the same or disjoint, a workgroup only touches its own (ciphertext, limb).  Shifted calls keep the permutation pass, which has read all of `in`
    // before anything is written (they used to be refused on every path).
    const bool shifted = shifted_overlap(g.in, g.out, count * ctx->ctw2);
    CHECK(add_overlap(ctx, nullptr, g.acc, g.out, count));
    // how the automorphism reaches the key switch, decided once: c1 permuted ahead and c0 inside KS_PAIR14 (N = 16384, batch); applied by the two-launch kernels
    // while they load c1 and c0 (small batches: no permutation pass); or a permutation pass over the whole ciphertext
    enum { PERM_AHEAD, PERM_ON_LOAD, PERM_PASS } via = PERM_PASS;
    if (!shifted && ks_plan(ctx, *key, count, 1).form == KS_PAIR14) via = PERM_AHEAD;
    else if (!shifted && ks_perm_on_load(ctx->hc, ks_switches(ctx), count)) via = PERM_ON_LOAD;
    if (via != PERM_AHEAD && (g.pre || g.next_elt)) return fail(CN_ERR_ARG, "internal: rotation chain outside the one-launch key switch");
    KsCall ks;
    switch (via) {
        case PERM_AHEAD:                                                 // c1 is permuted once (here unless the caller brings it)
            if (!g.pre) {
                hipLaunchKernelGGL(k_galois_limbs, dim3(count * ctx->hc.k), dim3(1024), (size_t)ctx->hc.n * 8, ctx->stream, g.in + kn, 2 * kn, g.tmp, kn, ctx->dc, g.elt);
                HIPCHK(hipGetLastError()); launch_count(ctx);
            }
            ks = KsCall::galois_of(g.pre ? g.pre : g.tmp, kn, g.in, kn, count).perm(elt).next((uint32_t)g.next_elt, g.next_out);
            break;
        case PERM_ON_LOAD: ks = KsCall::galois_of(g.in + kn, 2 * kn, g.in, kn, count).perm(elt); break;
        case PERM_PASS:
            if (ctx->hc.n >= 1024) hipLaunchKernelGGL(k_galois_lds, dim3(limbs), dim3(std::min<uint32_t>(1024, ctx->hc.n / 4)), (size_t)ctx->hc.n * 8, ctx->stream, g.in, g.tmp, ctx->dc, g.elt);
            else hipLaunchKernelGGL(k_galois, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, g.in, g.tmp, ctx->dc, ctx->chunks, g.elt);
            HIPCHK(hipGetLastError()); launch_count(ctx);
            ks = KsCall::galois_of(g.tmp + kn, 2 * kn, g.tmp, kn, count);
    }
    CHECK(do_keyswitch(ctx, *key, ks.to(g.out).plus(g.acc, ctx->ctw2)));
    ctx->st.Rotation += count;
    if (g.acc) ctx->st.Addition += count;
    return 0;
}
// scratch for `arrays` arrays of `count` size-2 ciphertexts; returns the first
static int ct_scratch(cn_ctx *ctx, uint32_t count, uint32_t arrays, uint64_t **first) {
    CHECK(ensure_scratch(ctx, al(count * ctx->ctw2 * 8) * arrays));
    *first = salloc<uint64_t>(ctx, count * ctx->ctw2);
    return 0;
}
int galois_impl(cn_ctx *ctx, CtSpan in, uint64_t elt, CtSpan acc, CtSpan out) {      // acc.d: out = acc + galois(in)
    if (acc.d) CHECK(add_overlap(ctx, in.d, acc.d, out.d, out.count));
    if (!out.count) return 0;
    uint64_t *tmp; CHECK(ct_scratch(ctx, out.count, 1, &tmp));
    return do_galois(ctx, {.in = in.d, .elt = elt, .out = out.d, .tmp = tmp, .count = out.count, .acc = acc.d});
}
extern "C" int cn_apply_galois(cn_ctx *ctx, cn_handle in, uint32_t ii, uint64_t elt, cn_handle out, uint32_t oi, uint32_t count) { API_BODY TWO_LIMBS("cn_apply_galois");
    LOCK; GETCT(I, in, 2); GETCT(O, out, 2); SPAN(si, I, ii, count); SPAN(so, O, oi, count);
    CHECK(galois_impl(ctx, si, elt, CtSpan{}, so));
    rec_galois(ctx, elt);
    return 0;
API_END }
// Evaluator::rotate_internal with the keys this context holds (cn_rotation.h): the hops of RotateRows(steps), or the refusal.  Queued rotations are checked with it
// when they are queued, like every other argument
int plan_rotation(cn_ctx *ctx, int steps, CnRotPlan *plan) {
    const CnRotPlan p = cn_rotation_plan(ctx->hc.n, steps, [ctx](uint64_t e) { return galois_key(ctx, e) != nullptr; });
    if (plan) *plan = p;
    return p.rc ? fail(p.rc, "%s", p.msg) : 0;
}
// the hops of a plan one after the other, in place
static int rotate_hops(cn_ctx *ctx, const CnRotPlan &p, uint64_t *cur, uint64_t *tmp, uint32_t count) {
    for (uint32_t h = 0; h < p.hops; h++) CHECK(do_galois(ctx, {.in = cur, .elt = p.elt[h], .out = cur, .tmp = tmp, .count = count}));
    return 0;
}
int rotate_rows_impl(cn_ctx *ctx, CtSpan in, int steps, CtSpan out) {
    const uint32_t count = out.count;
    if (!count) return 0;
    CnRotPlan p; CHECK(plan_rotation(ctx, steps, &p));                   // (a refused rotation enqueues nothing and leaves `out` as it is)
    const bool shifted = shifted_overlap(in.d, out.d, count * ctx->ctw2);
    uint64_t *tmp; CHECK(ct_scratch(ctx, count, shifted ? 2 : 1, &tmp));
    if (p.hops == 1) return do_galois(ctx, {.in = in.d, .elt = p.elt[0], .out = out.d, .tmp = tmp, .count = count});   // one hop: no staging copy
    if (shifted) {                                    // overlapping ranges: through a staging array (a device-to-device copy between overlapping ranges is undefined)
        uint64_t *stage = salloc<uint64_t>(ctx, count * ctx->ctw2);
        HIPCHK(hipMemcpyAsync(stage, in.d, count * ctx->ctw2 * 8, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(out.d, stage, count * ctx->ctw2 * 8, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (out.d != in.d) HIPCHK(hipMemcpyAsync(out.d, in.d, count * ctx->ctw2 * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return rotate_hops(ctx, p, out.d, tmp, count);
}
static int rotate_planned(cn_ctx *ctx, std::vector<RotJob> &jobs);
int rotate_jobs(cn_ctx *ctx, std::vector<RotJob> &jobs) {
    for (RotJob &j : jobs) CHECK(plan_rotation(ctx, j.steps, &j.plan));
    return rotate_planned(ctx, jobs);
}
// ... with the hops of every job planned already (RotJob::plan; cn_rotate_rows_sum runs all but the last hop of its terms through here)
static int rotate_planned(cn_ctx *ctx, std::vector<RotJob> &jobs) {
    const uint32_t n = (uint32_t)jobs.size();
    if (!n) return 0;
    uint32_t rounds = 0;
    for (RotJob &j : jobs) rounds = std::max(rounds, j.plan.hops);
    bool aliased = false;
    for (uint32_t a = 0; a < n && !aliased; a++) for (uint32_t b = 0; b < n; b++) if (a != b && (jobs[a].dst == jobs[b].src || jobs[a].dst == jobs[b].dst)) { aliased = true; break; }
    const KsSwitches sw = ks_switches(ctx);
    const bool tables_ok = !aliased && ks_perm_on_load(ctx->hc, sw, n);
    if (!tables_ok && !aliased && n > 1) {
        // More rotations than ONE table-driven two-launch key switch takes (LoLa-CIFAR's ConvertToColumnVector: 83 maps at N = 16384 - 664 (ciphertext, limb)
        // blocks against the 160 up to which a key switch runs as two launches): pieces of the largest size that does, each a launch chain of its own, instead
        // of 83 x ~4 single-ciphertext rotations of two launches each (round 5: 632 -> ~40 launches per plaintext prime and image).  Independent jobs: any order.
        const uint32_t piece = ks_largest_perm_on_load(ctx->hc, sw, std::min<uint32_t>(n - 1, 64));
        if (piece) {
            for (uint32_t s0 = 0; s0 < n; s0 += piece) {
                std::vector<RotJob> part(jobs.begin() + s0, jobs.begin() + std::min<uint32_t>(n, s0 + piece));
                CHECK(rotate_planned(ctx, part));
            }
            return 0;
        }
    }
    if (!tables_ok) {                                      // large batches (fused kernel), aliased operands: one after the other
        CHECK(ensure_scratch(ctx, al(ctx->ctw2 * 8)));
        for (RotJob &j : jobs) {
            ctx->soff = 0;
            uint64_t *tmp = salloc<uint64_t>(ctx, ctx->ctw2);
            if (j.plan.hops == 1) { CHECK(do_galois(ctx, {.in = j.src, .elt = j.plan.elt[0], .out = j.dst, .tmp = tmp, .count = 1})); continue; }
            if (j.dst != j.src) HIPCHK(hipMemcpyAsync(j.dst, j.src, ctx->ctw2 * 8, hipMemcpyDeviceToDevice, ctx->stream));
            CHECK(rotate_hops(ctx, j.plan, j.dst, tmp, 1));
        }
        return 0;
    }
    {   // rotations by 0 steps: copies
        std::vector<Tab2> cp;
        for (RotJob &j : jobs) if (!j.plan.hops && j.dst != j.src) cp.push_back({(const NTT_GLOBAL uint64_t *)j.src, (NTT_GLOBAL uint64_t *)j.dst});
        if (!cp.empty()) { CHECK(ensure_stage(ctx, al(cp.size() * sizeof(Tab2)))); CHECK(copy_by_table(ctx, cp, (Tab2 *)ctx->stage, (uint32_t)ctx->ctw2)); }
    }
    for (uint32_t r = 0; r < rounds; r++) {
        std::vector<KsItem> items; std::vector<uint64_t *> outs;
        const KsKey *any = nullptr;
        for (RotJob &j : jobs) {
            if (j.plan.hops <= r) continue;
            const KsKey &key = *galois_key(ctx, j.plan.elt[r]);
            any = &key;
            items.push_back({r == 0 ? j.src : j.dst, key.d, (uint32_t)j.plan.elt[r], 0u});
            outs.push_back(j.dst);
        }
        const uint32_t cnt = (uint32_t)items.size();
        ctx->soff = 0;
        CHECK(ensure_scratch(ctx, al(cnt * sizeof(KsItem)) + al(cnt * sizeof(uint64_t *))));
        KsItem *d_items = salloc<KsItem>(ctx, cnt);
        uint64_t **d_outs = salloc<uint64_t *>(ctx, cnt);
        const void *p_items, *p_outs;
        CHECK(place_table(ctx, items.data(), cnt * sizeof(KsItem), d_items, &p_items));
        CHECK(place_table(ctx, outs.data(), cnt * sizeof(uint64_t *), d_outs, &p_outs));
        CHECK(do_keyswitch(ctx, *any, KsCall::galois_items((const KsItem *)p_items, cnt).to_table((uint64_t *const *)p_outs)));
        ctx->st.Rotation += cnt;
    }
    return 0;
}

// RotateRows of n ciphertexts by n different step counts, one launch chain (see include/cnhip.h)
extern "C" int cn_rotate_rows_many(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const int *steps, uint32_t n, cn_handle out, const uint32_t *oi) { API_BODY TWO_LIMBS("cn_rotate_rows_many");
    LOCK_ONLY; GETCT(I, in, 2); GETCT(O, out, 2);
    if (!n) return 0;
    if (!ii || !steps || !oi) return fail(CN_ERR_ARG, "null argument");
    std::vector<RotJob> jobs(n);
    for (uint32_t i = 0; i < n; i++) {
        SPAN(si, I, ii[i], 1); SPAN(so, O, oi[i], 1);
        CHECK(plan_rotation(ctx, steps[i]));
        for (uint32_t j = 0; j < i; j++) if (O == I ? (oi[i] == oi[j] || oi[i] == ii[j] || ii[i] == oi[j]) : oi[i] == oi[j])
            return fail(CN_ERR_ARG, "rotate_rows_many: a result would overwrite another rotation's operand or result");
        jobs[i] = {si.d, so.d, steps[i]};
    }
    for (uint32_t i = 0; i < n; i++) rec_rows(ctx, steps[i]);               // (every argument has been checked)
    if (deferring(ctx)) {                                   // queued like n cn_rotate_rows calls
        for (const RotJob &j : jobs) CHECK(defer_staged(ctx, DOP_ROT, CtSpan{const_cast<uint64_t *>(j.src), 1}, CtSpan{}, CtSpan{j.dst, 1}, j.steps));
        return 0;
    }
    CHECK(cn_defer_flush(ctx));
    return rotate_jobs(ctx, jobs);
API_END }
// n rotations of ONE ciphertext that share its digit transforms (include/cnhip.h; the plan: cn_ks_hoist_plan, the kernels: k_ks_digit_ntt + k_ks_hoist_mac).  steps != null:
// RotateRows step counts (0: a copy), else Galois elements (1: a copy).  Every check comes before the first launch: a refused call leaves `out` as it is
static int hoisted_rotations(cn_ctx *ctx, cn_handle in, uint32_t ii, const uint64_t *elts, const int *steps, uint32_t n, cn_handle out, const uint32_t *oi) {
    GETCT(I, in, 0); GETCT(O, out, 0);
    if (I->size != 2 || O->size != 2) return fail(CN_ERR_ARG, "hoisted rotations: operands must be size-2 ciphertexts");
    if (!n) return fail(CN_ERR_ARG, "hoisted rotations: an empty list");
    if (!oi || (!elts && !steps)) return fail(CN_ERR_ARG, "null argument");
    SPAN(si, I, ii, 1);
    const uint64_t N = ctx->hc.n;
    std::vector<uint64_t> e(n);
    const KsKey *first = nullptr;
    uint32_t nrot = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!range_ok(O, oi[i], 1)) return fail(CN_ERR_ARG, "index out of range");
        if (O == I && oi[i] == ii) return fail(CN_ERR_ARG, "hoisted rotations: an output is the input ciphertext");
        for (uint32_t j = 0; j < i; j++) if (oi[i] == oi[j]) return fail(CN_ERR_ARG, "hoisted rotations: an output index is listed twice");
        e[i] = steps ? (steps[i] ? cn_elt_of_step(N, steps[i]) : 1) : elts[i];
        if (steps && !e[i]) return fail(CN_ERR_ARG, "step count too large");
        if (!(e[i] & 1) || e[i] >= 2 * N) return fail(CN_ERR_ARG, "invalid Galois element");
    }
    for (uint32_t i = 0; i < n; i++) {                     // every element needs its OWN key: a chain of non-adjacent-form hops is sequential, nothing to hoist
        if (e[i] == 1) continue;
        const KsKey *key = galois_key(ctx, e[i]);
        if (!key) return fail(CN_ERR_NOKEY, "Galois key not present");
        if (first && key->f64 != first->f64) return fail(CN_ERR_ARG, "hoisted rotations: the Galois keys were loaded in different forms (\"f64\" changed between the uploads)");
        if (!first) first = key;
        nrot++;
    }
    KsHoistPlan plan{};
    if (nrot) {
        plan = cn_ks_hoist_plan(ctx->hc, ks_switches(ctx), first->f64, nrot);
        if (plan.rc) return fail(plan.rc, "%s", plan.msg);
        CHECK(ensure_ks_part(ctx, plan.arena_bytes));
        CHECK(ensure_scratch(ctx, al(nrot * sizeof(KsHoistItem))));
    }
    if (nrot) {                                            // the rotations first: nothing has been written when the launcher still refuses
        std::vector<KsHoistItem> items;
        for (uint32_t i = 0; i < n; i++) if (e[i] != 1) items.push_back({galois_key(ctx, e[i])->d, O->d + (size_t)oi[i] * O->item_words, (uint32_t)e[i], 0u});
        KsHoistItem *d_items; CHECK(upload_tmp(ctx, items.data(), items.size(), &d_items));      // (by value: a recorded call replays this list)
        if (!ks_ops[plan.policy]->hoist(ctx, {si.d, d_items, plan})) return fail(CN_ERR_ARG, "internal: hoisted rotations without a kernel of their policy");
        HIPCHK(hipGetLastError());
        ctx->st.ntt_forward_limbs += plan.fwd_limbs; ctx->st.ntt_inverse_limbs += plan.inv_limbs;
        ctx->st.Rotation += nrot;
        ctx->ks_hoisted++;
    }
    for (uint32_t i = 0; i < n; i++)                       // step 0 / element 1: copies
        if (e[i] == 1) HIPCHK(hipMemcpyAsync(O->d + (size_t)oi[i] * O->item_words, si.d, ctx->ctw2 * 8, hipMemcpyDeviceToDevice, ctx->stream));
    for (uint32_t i = 0; i < n; i++) { if (steps) rec_rows(ctx, steps[i]); else if (e[i] != 1) rec_galois(ctx, e[i]); }
    return 0;
}
extern "C" int cn_apply_galois_hoisted(cn_ctx *ctx, cn_handle in, uint32_t ii, const uint64_t *elts, uint32_t n, cn_handle out, const uint32_t *oi) { API_BODY TWO_LIMBS("cn_apply_galois_hoisted");
    LOCK; if (n && !elts) return fail(CN_ERR_ARG, "null argument");
    return hoisted_rotations(ctx, in, ii, elts, nullptr, n, out, oi);
API_END }
extern "C" int cn_rotate_rows_hoisted(cn_ctx *ctx, cn_handle in, uint32_t ii, const int *steps, uint32_t n, cn_handle out, const uint32_t *oi) { API_BODY TWO_LIMBS("cn_rotate_rows_hoisted");
    LOCK; if (n && !steps) return fail(CN_ERR_ARG, "null argument");
    return hoisted_rotations(ctx, in, ii, nullptr, steps, n, out, oi);
API_END }
// Summed rotations (include/cnhip.h; the plan: cn_ks_sum_plan, the kernels: the term MAC of the two-launch key switch + k_ks_sum_terms): out[oi + g] = the sum over
// the terms e of group g of the rotation of in[ii[e]].  steps != null: RotateRows step counts (0: a plain addend) with the hops of cn_rotation.h, else Galois elements
// (1: a plain addend), each with its own key.  Every check and every hop is planned before anything is copied or launched: a refused call leaves `out` as it is.
// Where the plan says "compose" the literal sequence runs through a temporary - the rotations as cn_rotate_rows_many's rounds, k_add_many per group: the same words.
static int rotation_sum(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const uint64_t *elts, const int *steps, const uint32_t *grp_off, uint32_t G, cn_handle out, uint32_t oi) {
    GETCT(I, in, 0); GETCT(O, out, 0);
    if (I->size != 2 || O->size != 2) return fail(CN_ERR_ARG, "summed rotations: operands must be size-2 ciphertexts");
    if (!ii || !grp_off || (!elts && !steps)) return fail(CN_ERR_ARG, "null argument");
    if (!G) return fail(CN_ERR_ARG, "summed rotations: no output group");
    if (grp_off[0] != 0) return fail(CN_ERR_ARG, "summed rotations: grp_off must start at 0");
    for (uint32_t g = 0; g < G; g++) if (grp_off[g + 1] <= grp_off[g]) return fail(CN_ERR_ARG, "summed rotations: an empty group (grp_off must increase strictly)");
    const uint32_t E = grp_off[G];
    if (E > 0x00ffffffu) return fail(CN_ERR_ARG, "summed rotations: too many terms");
    if (!range_ok(O, oi, G)) return fail(CN_ERR_ARG, "output index out of range");
    const uint64_t N = ctx->hc.n;
    std::vector<CnRotPlan> hops(E);
    const KsKey *first = nullptr;
    uint32_t rotated = 0, multi = 0;
    for (uint32_t e = 0; e < E; e++) {
        if (!range_ok(I, ii[e], 1)) return fail(CN_ERR_ARG, "index out of range");
        if (O == I && ii[e] >= oi && ii[e] - oi < G) return fail(CN_ERR_ARG, "summed rotations: the output range contains a ciphertext the call reads");
        if (!steps && (!(elts[e] & 1) || elts[e] >= 2 * N)) return fail(CN_ERR_ARG, "invalid Galois element");
    }
    for (uint32_t e = 0; e < E; e++) {
        if (steps) CHECK(plan_rotation(ctx, steps[e], &hops[e]));
        else if (elts[e] != 1) {                           // every element needs its OWN key
            if (!galois_key(ctx, elts[e])) return fail(CN_ERR_NOKEY, "Galois key not present");
            hops[e].hops = 1; hops[e].elt[0] = elts[e];
        }
        for (uint32_t h = 0; h < hops[e].hops; h++) {
            const KsKey *key = galois_key(ctx, hops[e].elt[h]);
            if (first && key->f64 != first->f64) return fail(CN_ERR_ARG, "summed rotations: the Galois keys were loaded in different forms (\"f64\" changed between the uploads)");
            if (!first) first = key;
        }
        rotated += hops[e].hops != 0; multi += hops[e].hops > 1;
    }
    uint32_t outputs = 0;                                  // groups with a rotated term: the fused form's; the others are plain AddMany of their operands
    std::vector<uint8_t> has_rot(G, 0);
    for (uint32_t g = 0; g < G; g++) { for (uint32_t e = grp_off[g]; e < grp_off[g + 1]; e++) if (hops[e].hops) has_rot[g] = 1; outputs += has_rot[g]; }
    const KsSumPlan plan = cn_ks_sum_plan(ctx->hc, ks_switches(ctx), first && first->f64, E, rotated, outputs);
    const bool fused = plan.form != KS_SUM_COMPOSE;
    if (fused) CHECK(ensure_ks_part(ctx, plan.arena_bytes));          // (the arena cannot grow while a graph records or lives: refused here, before the first launch)
    const uint32_t tmp_cts = !rotated ? 0 : (fused ? multi : E);      // fused: the terms with earlier hops; composed: every term
    cn_handle tmp = 0;
    if (tmp_cts) CHECK(alloc_buf(ctx, 0, tmp_cts, 2, &tmp));
    int rc = [&]() -> int {
        Buffer *T = tmp ? getbuf(ctx, tmp, 0) : nullptr;
        I = getbuf(ctx, in, 0); O = getbuf(ctx, out, 0);              // (the handle table may have moved)
        auto src_of = [&](uint32_t e) { return I->d + (size_t)ii[e] * I->item_words; };
        std::vector<uint32_t> slot(E, 0);                  // of a term in the temporary
        std::vector<RotJob> jobs;
        for (uint32_t e = 0, m = 0; e < E; e++) {
            if (!T || (fused && hops[e].hops < 2)) continue;
            slot[e] = m++;
            RotJob j{src_of(e), T->d + (size_t)slot[e] * T->item_words, steps ? steps[e] : 0, hops[e]};
            if (fused) j.plan.hops--;                      // the last hop belongs to the two launches below
            jobs.push_back(j);
        }
        CHECK(rotate_planned(ctx, jobs));
        const uint32_t limbs = 2 * ctx->hc.k;
        if (!fused) {                                      // AddMany per group: out of the temporary, or - nothing rotated at all - out of the operands
            std::vector<uint32_t> idx(E);
            for (uint32_t e = 0; e < E; e++) idx[e] = rotated ? slot[e] : ii[e];
            CHECK(ensure_scratch(ctx, al((size_t)E * 4)));
            uint32_t *didx; CHECK(upload_tmp(ctx, idx.data(), idx.size(), &didx));
            const Buffer *S = rotated ? T : I;
            for (uint32_t g = 0; g < G; g++) {
                hipLaunchKernelGGL(k_add_many, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, S->d, didx + grp_off[g], grp_off[g + 1] - grp_off[g], S->item_words,
                                   O->d + (size_t)(oi + g) * O->item_words, ctx->dc, ctx->chunks);
                HIPCHK(hipGetLastError()); launch_count(ctx);
            }
            return 0;
        }
        std::vector<KsItem> items; std::vector<KsSumOut> outs; std::vector<KsSumTerm> terms; std::vector<uint32_t> idx;
        std::vector<uint32_t> plain_groups;
        for (uint32_t g = 0; g < G; g++) {
            if (!has_rot[g]) { plain_groups.push_back(g); continue; }
            KsSumOut og{O->d + (size_t)(oi + g) * O->item_words, (uint32_t)terms.size(), grp_off[g + 1] - grp_off[g], 0u, 0u};
            for (uint32_t e = grp_off[g]; e < grp_off[g + 1]; e++) {          // the rotated terms first
                if (!hops[e].hops) continue;
                const uint64_t *src = hops[e].hops > 1 ? T->d + (size_t)slot[e] * T->item_words : src_of(e);
                const uint32_t elt = (uint32_t)hops[e].elt[hops[e].hops - 1];
                terms.push_back({src, elt, (uint32_t)items.size()});
                items.push_back({src, galois_key(ctx, elt)->d, elt, 0u});
                og.rotated++;
            }
            for (uint32_t e = grp_off[g]; e < grp_off[g + 1]; e++) if (!hops[e].hops) terms.push_back({src_of(e), 1u, 0u});
            outs.push_back(og);
        }
        for (uint32_t g : plain_groups) for (uint32_t e = grp_off[g]; e < grp_off[g + 1]; e++) idx.push_back(ii[e]);
        CHECK(ensure_scratch(ctx, al(items.size() * sizeof(KsItem)) + al(outs.size() * sizeof(KsSumOut)) + al(terms.size() * sizeof(KsSumTerm)) + al(idx.size() * 4 + 4)));
        KsItem *d_items; KsSumOut *d_outs; KsSumTerm *d_terms; uint32_t *didx = nullptr;      // (by value: a recorded call replays these tables)
        CHECK(upload_tmp(ctx, items.data(), items.size(), &d_items)); CHECK(upload_tmp(ctx, outs.data(), outs.size(), &d_outs));
        CHECK(upload_tmp(ctx, terms.data(), terms.size(), &d_terms));
        if (!idx.empty()) CHECK(upload_tmp(ctx, idx.data(), idx.size(), &didx));
        if (!ks_ops[plan.policy]->sum(ctx, {d_items, d_outs, d_terms, plan})) return fail(CN_ERR_ARG, "internal: summed rotations without a kernel of their policy");
        HIPCHK(hipGetLastError());
        ctx->st.ntt_forward_limbs += plan.fwd_limbs; ctx->st.ntt_inverse_limbs += plan.inv_limbs;
        ctx->st.Rotation += rotated;
        ctx->ks_summed++;
        size_t at = 0;
        for (uint32_t g : plain_groups) {
            const uint32_t cnt = grp_off[g + 1] - grp_off[g];
            hipLaunchKernelGGL(k_add_many, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, I->d, didx + at, cnt, I->item_words, O->d + (size_t)(oi + g) * O->item_words,
                               ctx->dc, ctx->chunks);
            HIPCHK(hipGetLastError()); launch_count(ctx);
            at += cnt;
        }
        return 0;
    }();
    if (!rc) {
        ctx->st.AddMany += G; ctx->st.AddManyItemCount += E;
        for (uint32_t e = 0; e < E; e++) { if (steps) rec_rows(ctx, steps[e]); else if (elts[e] != 1) rec_galois(ctx, elts[e]); }
    }
    const int rf = tmp ? free_body(ctx, tmp) : 0;
    return rc ? rc : rf;
}
extern "C" int cn_apply_galois_sum(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const uint64_t *elts, const uint32_t *grp_off, uint32_t G, cn_handle out, uint32_t oi) { API_BODY TWO_LIMBS("cn_apply_galois_sum");
    LOCK; if (!elts) return fail(CN_ERR_ARG, "null argument");
    return rotation_sum(ctx, in, ii, elts, nullptr, grp_off, G, out, oi);
API_END }
extern "C" int cn_rotate_rows_sum(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const int *steps, const uint32_t *grp_off, uint32_t G, cn_handle out, uint32_t oi) { API_BODY TWO_LIMBS("cn_rotate_rows_sum");
    LOCK; if (!steps) return fail(CN_ERR_ARG, "null argument");
    return rotation_sum(ctx, in, ii, nullptr, steps, grp_off, G, out, oi);
API_END }
static int add_kernel(cn_ctx *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, uint32_t count) {
    hipLaunchKernelGGL(k_addsub, dim3(count * 2 * ctx->hc.k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, a, b, out, ctx->dc, ctx->chunks, 0);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    ctx->st.Addition += count;
    return 0;
}
// out = acc + RotateRows(in, steps): the rotate-and-add step of SumAllSlots (AtomicSealBfvVector.cs:862-868) with the addition
// fused into the last kernel of the key switch.  Same words as cn_rotate_rows followed by cn_add.
int rotate_rows_add_impl(cn_ctx *ctx, CtSpan in, int steps, CtSpan acc, CtSpan out) {
    const uint32_t count = out.count;
    CHECK(add_overlap(ctx, in.d, acc.d, out.d, count));
    if (!count) return 0;
    CnRotPlan p; CHECK(plan_rotation(ctx, steps, &p));                   // (a refused rotation enqueues nothing)
    if (!p.hops) return add_kernel(ctx, in.d, acc.d, out.d, count);
    uint64_t *tmp; CHECK(ct_scratch(ctx, count, p.hops > 1 ? 2 : 1, &tmp));
    if (p.hops == 1) return do_galois(ctx, {.in = in.d, .elt = p.elt[0], .out = out.d, .tmp = tmp, .count = count, .acc = acc.d});
    // multi-hop (NAF) rotation: rotate into a staging array, then one element-wise add
    uint64_t *stage = salloc<uint64_t>(ctx, count * ctx->ctw2);
    HIPCHK(hipMemcpyAsync(stage, in.d, count * ctx->ctw2 * 8, hipMemcpyDeviceToDevice, ctx->stream));
    CHECK(rotate_hops(ctx, p, stage, tmp, count));
    return add_kernel(ctx, acc.d, stage, out.d, count);
}
// cn_rotate_rows and cn_rotate_rows_add (acc.d null: no accumulator) behind their range checks.  Queued (defer = 1, up to DEFER_STAGED_MAX ciphertexts): the keys are
// asked through the planner now, like every other argument; else everything pending is flushed and the call runs at once.  A refused call records no step.
static int rotate_rows_call(cn_ctx *ctx, CtSpan in, int steps, CtSpan acc, CtSpan out) {
    if (queues(ctx, out.count)) { CHECK(plan_rotation(ctx, steps)); rec_rows(ctx, steps); return defer_staged(ctx, acc.d ? DOP_ROTADD : DOP_ROT, in, acc, out, steps); }
    CHECK(cn_defer_flush(ctx));
    CHECK(acc.d ? rotate_rows_add_impl(ctx, in, steps, acc, out) : rotate_rows_impl(ctx, in, steps, out));
    rec_rows(ctx, steps);
    return 0;
}
// ... and the column swap the same way; it is recorded only when its key is present (an empty call asks for no key)
static int rotate_columns_call(cn_ctx *ctx, CtSpan in, CtSpan acc, CtSpan out) {
    const uint64_t elt = 2ull * ctx->hc.n - 1;
    if (queues(ctx, out.count)) { CHECK(columns_key(ctx)); rec_columns(ctx); return defer_staged(ctx, acc.d ? DOP_COLSADD : DOP_COLS, in, acc, out, 0); }
    CHECK(cn_defer_flush(ctx));
    CHECK(galois_impl(ctx, in, elt, acc, out));
    if (galois_key(ctx, elt)) rec_columns(ctx);
    return 0;
}
extern "C" int cn_rotate_rows(cn_ctx *ctx, cn_handle in, uint32_t ii, int steps, cn_handle out, uint32_t oi, uint32_t count) { API_BODY TWO_LIMBS("cn_rotate_rows");
    LOCK_ONLY; GETCT(I, in, 2); GETCT(O, out, 2); SPAN(si, I, ii, count); SPAN(so, O, oi, count);
    return rotate_rows_call(ctx, si, steps, CtSpan{}, so);
API_END }
extern "C" int cn_rotate_rows_add(cn_ctx *ctx, cn_handle in, uint32_t ii, int steps, cn_handle acc, uint32_t ai, cn_handle out, uint32_t oi, uint32_t count) { API_BODY TWO_LIMBS("cn_rotate_rows_add");
    LOCK_ONLY; GETCT(I, in, 2); GETCT(A, acc, 2); GETCT(O, out, 2); SPAN(si, I, ii, count); SPAN(sa, A, ai, count); SPAN(so, O, oi, count);
    return rotate_rows_call(ctx, si, steps, sa, so);
API_END }
extern "C" int cn_rotate_columns_add(cn_ctx *ctx, cn_handle in, uint32_t ii, cn_handle acc, uint32_t ai, cn_handle out, uint32_t oi, uint32_t count) { API_BODY TWO_LIMBS("cn_rotate_columns_add");
    LOCK_ONLY; GETCT(I, in, 2); GETCT(A, acc, 2); GETCT(O, out, 2); SPAN(si, I, ii, count); SPAN(sa, A, ai, count); SPAN(so, O, oi, count);
    return rotate_columns_call(ctx, si, sa, so);
API_END }
// SumAllSlots(length) of AtomicSealBfvVector.cs:888-935 on `count` single-block ciphertexts at once, in place: the column swap when
// length >= N/2, then log2 rotate-and-add steps (RotateRows(-2^s) + AddInplace).  length 0 = all N slots.
// (the sequence and whether it runs as the one-launch chain: sum_slots_seq / sum_slots_plan, cn_plain_plan.h)
static int galois_key_form(cn_ctx *ctx, uint64_t elt) { const KsKey *key = galois_key(ctx, elt); return key ? (int)key->f64 : -1; }
// ready: the chained row-dot batch's plan - its arena already holds sigma_(chain[0])(c1) of every ciphertext at chain_off (written by the producer of h: k_mul_plain_bcast)
int sum_slots_impl(cn_ctx *ctx, CtSpan h, uint32_t length, const RowdotPlan *ready) {
    const uint32_t n = ctx->hc.n, count = h.count;
    // N = 16384, batch: the links of the chain as ONE launch each - link s leaves sigma_(s+1) of its new c1 beside its result (k_keyswitch_pair14), so only the
    // first link needs a permutation pass (none when the producer has left it).  Same words as the loop below (the same key switches on the same operands).
    const std::vector<uint64_t> elts = ready ? ready->chain : sum_slots_plan(ctx->hc, plain_switches(ctx), count, length, [&](uint64_t e) { return galois_key_form(ctx, e); });
    if (elts.empty() && ready) return fail(CN_ERR_ARG, "internal: chained row-dot batch without a chain");
    if (!elts.empty()) {
        const size_t kn = (size_t)ctx->hc.k * n;
        if (ready) ctx->soff = ready->chain_off; else CHECK(ensure_scratch(ctx, al(count * ctx->ctw2 * 8)));
        uint64_t *pp[2]; pp[0] = salloc<uint64_t>(ctx, count * ctx->ctw2); pp[1] = pp[0] + (size_t)count * kn;
        for (size_t s = 0; s < elts.size(); s++) {
            const bool last = s + 1 == elts.size();
            CHECK(do_galois(ctx, {.in = h.d, .elt = elts[s], .out = h.d, .tmp = pp[s & 1], .count = count, .acc = h.d, .pre = (s || ready) ? pp[s & 1] : nullptr,
                                  .next_elt = last ? 0 : elts[s + 1], .next_out = pp[(s + 1) & 1]}));
        }
        return 0;
    }
    const SumSlotsSeq seq = sum_slots_seq(n, length);
    if (seq.columns) CHECK(galois_impl(ctx, h, 2ull * n - 1, h, h));
    for (uint32_t i = 0; i < seq.rows; i++) CHECK(rotate_rows_add_impl(ctx, h, -(int)(1u << i), h, h));
    return 0;
}
extern "C" int cn_sum_slots(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint32_t length) { API_BODY TWO_LIMBS("cn_sum_slots");
    LOCK_ONLY; GETCT(H, h, 2); SPAN(sh, H, first, count);
    if (!count) return 0;
    if (queues(ctx, count)) {
        const SumSlotsSeq seq = sum_slots_seq(ctx->hc.n, length);
        if (seq.columns) CHECK(columns_key(ctx));
        for (uint32_t i = 0; i < seq.rows; i++) CHECK(plan_rotation(ctx, -(int)(1u << i)));
        rec_sum_slots(ctx, length);
        return defer_staged(ctx, DOP_SUMSLOTS, sh, CtSpan{}, sh, length);
    }
    CHECK(cn_defer_flush(ctx));
    CHECK(sum_slots_impl(ctx, sh, length));
    rec_sum_slots(ctx, length);
    return 0;
API_END }
// out[r] = SumAllSlots(v * pt[r], length) for r < rows: every row of a plaintext matrix against ONE packed ciphertext
// (EncryptedSealBfvMatrix.Mul row-major, EncryptedSealBfvMatrix.cs:79-120 -> DotProduct, AtomicSealBfvVector.cs:963-977).
extern "C" int cn_rowdot_batch(cn_ctx *ctx, cn_handle v, uint32_t vi, cn_handle pt, uint32_t pi, uint32_t rows, uint32_t length, cn_handle out, uint32_t oi) { API_BODY TWO_LIMBS("cn_rowdot_batch");
    LOCK; GETCT(V, v, 2); GETCT(O, out, 2); GETPT_OR_PTN(P, pt);
    if (!rows) return 0;
    if (V == O && vi >= oi && vi < oi + rows) return fail(CN_ERR_ARG, "row-dot batch cannot overwrite its input");
    SPAN(sv, V, vi, 1); SPAN(so, O, oi, rows); PTSPAN(sp, P, pi, rows, 1u);
    if (length != 1) rec_sum_slots(ctx, length);
    const RowdotPlan rd = rowdot_plan(ctx->hc, plain_switches(ctx), rows, length, sp.ntt, [&](uint64_t e) { return galois_key_form(ctx, e); });
    if (!rd.chain.empty()) {                                       // one arena for the chain's two scratch arrays and the transformed ciphertext (RowdotPlan)
        CHECK(ensure_scratch(ctx, al(rd.pp_bytes) + al(rd.ctn_bytes)));
        uint64_t *p0 = salloc<uint64_t>(ctx, rd.pp_bytes / 8), *ctn = salloc<uint64_t>(ctx, rd.ctn_bytes / 8);
        if (!p0 || !ctn) return fail(CN_ERR_HIP, "internal: scratch exhausted in the row-dot batch");
        const BcastNext nx{rd.chain[0], p0, ctn};
        CHECK(mul_plain_impl(ctx, sv, true, sp, so, 2, &nx));
        return sum_slots_impl(ctx, so, length, &rd);
    }
    CHECK(mul_plain_impl(ctx, sv, true, sp, so, 2));
    if (length == 1) return 0;
    return sum_slots_impl(ctx, so, length);
API_END }
// out[oi + g] = sum over the terms e of group g of MultiplyPlain(ct[ci + ct_idx[e]], pt[pi + e]) (include/cnhip.h).  Register-radix sizes: the distinct
// ciphertexts transformed once into scratch (like `ctn` of the row-dot batch), then ONE launch of k_mul_plain_sum; other sizes: cn_mul_plain per term into a temporary
// and AddMany per group.
extern "C" int cn_mul_plain_sum(cn_ctx *ctx, cn_handle ct, uint32_t ci, cn_handle pt, uint32_t pi, const uint32_t *grp_off, const uint32_t *ct_idx, uint32_t G,
                                cn_handle out, uint32_t oi) { API_BODY
    LOCK; GETCT(A, ct, 2); GETCT(O, out, 2); GETPT_OR_PTN(P, pt);
    const bool ptn = P->kind == 4;                                   // NTT-form plaintexts (cn_pt_transform): k_mul_ptn_sum, no transform of theirs
    if (!grp_off || !ct_idx) return fail(CN_ERR_ARG, "null argument");
    if (!G) return fail(CN_ERR_ARG, "cn_mul_plain_sum of an empty list");
    if (grp_off[0]) return fail(CN_ERR_ARG, "cn_mul_plain_sum: grp_off[0] must be 0");
    uint32_t maxlen = 0;
    for (uint32_t g = 0; g < G; g++) {
        if (grp_off[g + 1] <= grp_off[g]) return fail(CN_ERR_ARG, "cn_mul_plain_sum: group %u is empty", g);
        maxlen = std::max(maxlen, grp_off[g + 1] - grp_off[g]);
    }
    const uint32_t E = grp_off[G];
    if (!range_ok(O, oi, G) || !range_ok(P, pi, E) || ci >= A->count) return fail(CN_ERR_ARG, "index out of range");
    for (uint32_t e = 0; e < E; e++) {
        if (ct_idx[e] >= A->count - ci) return fail(CN_ERR_ARG, "ciphertext index out of range in term %u", e);
        if (A == O && ci + ct_idx[e] >= oi && ci + ct_idx[e] < oi + G) return fail(CN_ERR_ARG, "cn_mul_plain_sum cannot overwrite a ciphertext it reads");
    }
    for (uint32_t e = 0; e < E; e++) if (P->pt_zero[pi + e]) return fail(CN_ERR_ZERO, "plain cannot be zero");
    const uint32_t k = ctx->hc.k;
    const PlainSumPlan sp = plain_sum_plan(ctx->hc, plain_switches(ctx), ptn, G, E);
    if (!sp.kernel) {                                                // compose the existing calls
        cn_handle tmp = 0;
        CHECK(alloc_buf(ctx, 0, maxlen, 2, &tmp));
        int rc = 0;
        std::vector<uint32_t> ident(maxlen);
        for (uint32_t i = 0; i < maxlen; i++) ident[i] = i;
        for (uint32_t g = 0; g < G && !rc; g++) {
            const uint32_t len = grp_off[g + 1] - grp_off[g];
            Buffer *T = getbuf(ctx, tmp, 0);                                      // (the handle table may have moved)
            A = getbuf(ctx, ct, 0); O = getbuf(ctx, out, 0); P = getbuf(ctx, pt, ptn ? 4 : 1);
            for (uint32_t i = 0, e = grp_off[g]; i < len && !rc; i++, e++)      // (ranges and zero plaintexts were checked above)
                rc = mul_plain_impl(ctx, CtSpan{A->d + (ci + ct_idx[e]) * ctx->ctw2, 1}, false, PtSpan{P->d + (size_t)(pi + e) * P->item_words, 1, nullptr, ptn}, CtSpan{T->d + i * ctx->ctw2, 1}, 2);
            if (rc) break;
            if ((rc = ensure_scratch(ctx, al((size_t)len * 4)))) break;
            uint32_t *didx;
            if ((rc = upload_tmp(ctx, ident.data(), len, &didx))) break;
            hipLaunchKernelGGL(k_add_many, dim3(2 * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, T->d, didx, len, T->item_words, O->d + (size_t)(oi + g) * O->item_words, ctx->dc,
                               ctx->chunks);
            if (hipGetLastError() != hipSuccess) rc = fail(CN_ERR_HIP, "launch of k_add_many failed");
            launch_count(ctx);
        }
        if (!rc) { ctx->st.AddMany += G; ctx->st.AddManyItemCount += E; }
        const int rf = free_body(ctx, tmp);
        return rc ? rc : rf;
    }
    const PlainSumSlots ss = plain_sum_slots(ct_idx, E);             // the distinct ciphertexts -> slots of the NTT-form scratch copy
    const uint32_t D = (uint32_t)ss.src.size();
    CHECK(ensure_scratch(ctx, al(D * sp.src_bytes) + al(sp.grp_bytes) + al(sp.slot_bytes)));
    uint64_t *ctn = salloc<uint64_t>(ctx, (size_t)D * A->item_words);
    if (!ctn) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_mul_plain_sum");
    uint32_t *dgo, *dslot;
    CHECK(upload_tmp(ctx, grp_off, (size_t)G + 1, &dgo)); CHECK(upload_tmp(ctx, ss.slot.data(), E, &dslot));
    for (const PlainSumSlots::Run &r : ss.runs)                      // runs of neighbouring ciphertexts travel in one copy
        HIPCHK(hipMemcpyAsync(ctn + (size_t)r.first * A->item_words, A->d + (size_t)(ci + ss.src[r.first]) * A->item_words, (size_t)r.len * A->item_words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    CHECK(cn_run_ntt(ctx, ctn, D * 2 * k, 0, k, 0));
    const MulPlainSumLaunch launch{P->d + (size_t)pi * P->item_words, ctn, dgo, dslot, O->d + (size_t)oi * O->item_words, G, sp.accmax, sp.order};
    CHECK(ptn ? cn_l_mul_ptn_sum(ctx, sp.policy, launch) : cn_l_mul_plain_sum(ctx, sp.policy, launch));
    if (!ptn) ctx->st.ntt_forward_limbs += (uint64_t)E * 2 * k;      // the plaintexts, beside the D 2k limbs cn_run_ntt counted (NTT-form plaintexts: those are all that ran)
    ctx->st.ntt_inverse_limbs += (uint64_t)G * 2 * k;
    ctx->st.PlainMultiplication += E; ctx->st.AddMany += G; ctx->st.AddManyItemCount += E;
    return 0;
API_END }
extern "C" int cn_rotate_columns(cn_ctx *ctx, cn_handle in, uint32_t ii, cn_handle out, uint32_t oi, uint32_t count) { API_BODY TWO_LIMBS("cn_rotate_columns");
    LOCK_ONLY; GETCT(I, in, 2); GETCT(O, out, 2); SPAN(si, I, ii, count); SPAN(so, O, oi, count);
    return rotate_columns_call(ctx, si, CtSpan{}, so);
API_END }
