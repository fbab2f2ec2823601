// libcnhip.so host runtime: modulus switching (SEAL 3.2 Evaluator.ModSwitchToNext / ModSwitchTo) - level contexts and cn_mod_switch.
//
// A level context is an ordinary context over the prefix q[0..limbs) of its parent's coefficient modulus (its own transform, BEHZ and
// decryption tables - SEAL 3.2 builds a base converter per level) that takes the parent's settled options and a slice of every key the parent
// holds.  Under "ks_xi" = 1 its key-switch digits use the chain's top modulus (DevConsts::ks_inv_qhat_q), because the sliced keys carry it.
#include "cn_api_shared.h"

// every (l, d) entry with l < limbs is a prefix of the entries in (l, d) order: entries x 2 polynomials, each the first `limbs` limbs of the parent's k
static int slice_polys(cn_ctx *child, uint64_t *dst, const uint64_t *src, size_t rows, uint32_t k_src, uint32_t k_dst) {
    const size_t n = child->hc.n;
    HIPCHK(hipMemcpy2DAsync(dst, k_dst * n * 8, src, k_src * n * 8, k_dst * n * 8, rows, hipMemcpyDeviceToDevice, child->stream));
    return 0;
}
static int slice_ks_key(cn_ctx *child, const cn_ctx *parent, const KsKey &from, KsKey &to, int which) {
    const size_t words = cn_key_words(child, which);
    HIPCHK(hipMalloc((void **)&to.d, words * 8));
    to.owned = true; to.f64 = from.f64;
    CHECK(slice_polys(child, to.d, from.d, words / ((size_t)child->hc.k * child->hc.n), parent->hc.k, child->hc.k));
    // the child keeps its keys in the form its key-switch kernels read (a dropped prime of 49 bits or more can put the child on the FP64 path)
    const bool want = keys_as_f64(child);
    if (want != to.f64) {
        if (want) hipLaunchKernelGGL(k_u64_to_f64, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, child->stream, to.d, words);
        else hipLaunchKernelGGL(k_f64_to_u64, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, child->stream, to.d, words);
        HIPCHK(hipGetLastError());
        to.f64 = want;
    }
    return 0;
}
static int adopt_from_parent(cn_ctx *c, cn_ctx *parent) {
    const uint32_t k = c->hc.k;
    c->opt = parent->opt;
    memcpy(c->rng_key, parent->rng_key, sizeof c->rng_key);
    c->hc.ks_xi = parent->hc.ks_xi;
    for (uint32_t l = 0; l < k; l++) c->hc.ks_inv_qhat_q[l] = parent->hc.ks_inv_qhat_q[l];
    HIPCHK(hipMemcpy(c->dc, &c->hc, sizeof(DevConsts), hipMemcpyHostToDevice));
    HIPCHK(hipStreamSynchronize(parent->stream));                  // the parent's keys are complete (uploads and conversions run on its stream)
    const size_t kn = (size_t)k * c->hc.n;
    if (parent->rlk.d) CHECK(slice_ks_key(c, parent, parent->rlk, c->rlk, 0));
    for (auto &kv : parent->gk) if (kv.second.d) CHECK(slice_ks_key(c, parent, kv.second, c->gk[kv.first], 1));
    if (parent->pk) { HIPCHK(hipMalloc((void **)&c->pk, 2 * kn * 8)); CHECK(slice_polys(c, c->pk, parent->pk, 2, parent->hc.k, k)); }
    if (parent->sk) { HIPCHK(hipMalloc((void **)&c->sk, kn * 8)); HIPCHK(hipMemcpyAsync(c->sk, parent->sk, kn * 8, hipMemcpyDeviceToDevice, c->stream)); }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->level = true;
    return 0;
}
extern "C" int cn_ctx_create_level(cn_ctx *parent, uint32_t limbs, cn_ctx **out) {
    if (!parent || !out) return fail(CN_ERR_ARG, "null argument");
    if (limbs == 0 || limbs >= parent->hc.k) return fail(CN_ERR_ARG, "a level keeps 1 .. %u of the %u coefficient moduli (got %u)", parent->hc.k - 1, parent->hc.k, limbs);
    uint64_t q[CN_MAXK];
    for (uint32_t j = 0; j < limbs; j++) q[j] = parent->hc.q[j].q;        // (n, q, t, dbc, gdbc, device never change after creation)
    cn_ctx *c = nullptr;
    CHECK(cn_ctx_create(parent->hc.n, q, limbs, parent->hc.t.q, parent->hc.dbc, parent->hc.gdbc, parent->device, &c));
    const int rc = [&]() -> int {
        cn_ctx *ctx = parent;                                              // (the macros name the context `ctx`)
        return ctx->mu.run([&]() -> int { LOCK; NOT_CAPTURING("cn_ctx_create_level"); return adopt_from_parent(c, parent); });
    }();
    if (rc) {
        char msg[256]; snprintf(msg, sizeof msg, "%s", cn_last_error());
        (void)cn_ctx_destroy(c);
        return fail(rc, "%s", msg);
    }
    *out = c;
    return 0;
}

// ---------------------------------------------------------------- cn_mod_switch
static int flush_all(cn_ctx *ctx) { CHECK(use(ctx)); CHECK(ring_sync(ctx, true)); return cn_defer_flush(ctx); }
static int mod_switch_locked(cn_ctx *src, cn_handle in, uint32_t ii, uint32_t count, cn_ctx *dst, cn_handle out, uint32_t oi) {
    {   cn_ctx *ctx = src; NOT_CAPTURING("cn_mod_switch"); }
    {   cn_ctx *ctx = dst; NOT_CAPTURING("cn_mod_switch"); }
    const DevConsts &a = src->hc, &b = dst->hc;
    if (src->device != dst->device) return fail(CN_ERR_ARG, "cn_mod_switch: the target context is on another device");
    if (a.n != b.n || a.t.q != b.t.q) return fail(CN_ERR_ARG, "cn_mod_switch: the target context has another N or t");
    if (b.k >= a.k) return fail(CN_ERR_ARG, "cn_mod_switch: the target keeps %u of the source's %u coefficient moduli (must be fewer)", b.k, a.k);
    for (uint32_t j = 0; j < b.k; j++) if (a.q[j].q != b.q[j].q) return fail(CN_ERR_ARG, "cn_mod_switch: the target's coefficient modulus is not a prefix of the source's");
    if (a.ks_xi != b.ks_xi) return fail(CN_ERR_ARG, "cn_mod_switch: the contexts use different key-switch conventions (ks_xi)");
    if (a.ks_xi) for (uint32_t j = 0; j < b.k; j++) if (a.ks_inv_qhat_q[j] != b.ks_inv_qhat_q[j])
        return fail(CN_ERR_ARG, "cn_mod_switch: under ks_xi = 1 the target must be a level of the source's chain (cn_ctx_create_level)");
    // not deferrable: both contexts' queued calls and published records are submitted first (a handle may come from the lock-free ring)
    {   cn_ctx *ctx = src; CHECK(flush_all(ctx)); }
    {   cn_ctx *ctx = dst; CHECK(flush_all(ctx)); }
    Buffer *I = nullptr, *O = nullptr;
    { cn_ctx *ctx = src; GETCT(I_, in, 0); I = I_; }
    { cn_ctx *ctx = dst; GETCT(O_, out, 0); O = O_; }
    if (I->size != O->size || (I->size != 2 && I->size != 3)) return fail(CN_ERR_ARG, "cn_mod_switch: ciphertext sizes %u and %u (both 2 or both 3)", I->size, O->size);
    if (!range_ok(I, ii, count) || !range_ok(O, oi, count)) return fail(CN_ERR_ARG, "index out of range");
    // the FP64 form needs the "f64" option and every modulus of the source chain below 2^49 (the target's are a prefix)
    bool f64 = src->opt.f64 && dst->opt.f64, ran_f64 = false;
    for (uint32_t j = 0; j < a.k; j++) f64 = f64 && a.f64ok[j];
    if (!count) return 0;
    // ordering without a host wait: dst's stream waits for everything submitted to src (the writers of `in`), runs the switch behind its own earlier
    // work (the readers and writers of `out`), and src's stream waits for the switch (later writers of `in`)
    if (!src->ev_ms) HIPCHK(hipEventCreateWithFlags(&src->ev_ms, hipEventDisableTiming));
    if (!dst->ev_ms) HIPCHK(hipEventCreateWithFlags(&dst->ev_ms, hipEventDisableTiming));
    HIPCHK(hipEventRecord(src->ev_ms, src->stream));
    HIPCHK(hipStreamWaitEvent(dst->stream, src->ev_ms, 0));
    CHECK(cn_l_mod_switch(dst, I->d + (size_t)ii * I->item_words, O->d + (size_t)oi * O->item_words, src->dc, a.k, b.k, count * I->size, a.logn,
                          f64, &ran_f64));
    src->ms_f64 = dst->ms_f64 = ran_f64;
    HIPCHK(hipEventRecord(dst->ev_ms, dst->stream));
    HIPCHK(hipStreamWaitEvent(src->stream, dst->ev_ms, 0));
    return 0;
}
extern "C" int cn_mod_switch(cn_ctx *src, cn_handle in, uint32_t ii, uint32_t count, cn_ctx *dst, cn_handle out, uint32_t oi) {
    if (!src || !dst) return fail(CN_ERR_ARG, "null argument");
    if (src == dst) return fail(CN_ERR_ARG, "cn_mod_switch: source and target are the same context");
    // both locks, in chain order (more limbs first): two switches along one chain cannot deadlock
    cn_ctx *first = src->hc.k >= dst->hc.k ? src : dst, *second = first == src ? dst : src;
    if (first->hc.k == second->hc.k && first > second) std::swap(first, second);
    CnGuard g1(first->mu);
    CnGuard g2(second->mu);
    return mod_switch_locked(src, in, ii, count, dst, out, oi);
}
