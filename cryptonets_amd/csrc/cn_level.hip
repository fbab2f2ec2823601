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
int flush_all(cn_ctx *ctx) { CHECK(use(ctx)); CHECK(ring_sync(ctx, true)); return cn_defer_flush(ctx); }
// may a ciphertext of src be switched down to dst?  (cn_mod_switch; the members of a recording across levels, cn_graph_begin_levels)
static int chain_check(const cn_ctx *src, const cn_ctx *dst, const char *what) {
    const DevConsts &a = src->hc, &b = dst->hc;
    if (src->device != dst->device) return fail(CN_ERR_ARG, "%s: the target context is on another device", what);
    if (a.n != b.n || a.t.q != b.t.q) return fail(CN_ERR_ARG, "%s: the target context has another N or t", what);
    if (b.k >= a.k) return fail(CN_ERR_ARG, "%s: the target keeps %u of the source's %u coefficient moduli (must be fewer)", what, b.k, a.k);
    for (uint32_t j = 0; j < b.k; j++) if (a.q[j].q != b.q[j].q) return fail(CN_ERR_ARG, "%s: the target's coefficient modulus is not a prefix of the source's", what);
    if (a.ks_xi != b.ks_xi) return fail(CN_ERR_ARG, "%s: the contexts use different key-switch conventions (ks_xi)", what);
    if (a.ks_xi) for (uint32_t j = 0; j < b.k; j++) if (a.ks_inv_qhat_q[j] != b.ks_inv_qhat_q[j])
        return fail(CN_ERR_ARG, "%s: under ks_xi = 1 the target must be a level of the source's chain (cn_ctx_create_level)", what);
    return 0;
}
static int mod_switch_locked(cn_ctx *src, cn_handle in, uint32_t ii, uint32_t count, cn_ctx *dst, cn_handle out, uint32_t oi) {
    // while a graph is recorded, only a switch between two contexts of one recording across levels is possible (it is recorded like any call)
    if ((src->capturing || dst->capturing) && !(src->cap_root && src->cap_root == dst->cap_root)) {
        cn_ctx *ctx = src->capturing ? src : dst; NOT_CAPTURING("cn_mod_switch (other than between the contexts of one cn_graph_begin_levels)");
    }
    CHECK(chain_check(src, dst, "cn_mod_switch"));
    const DevConsts &a = src->hc, &b = dst->hc;
    // not deferrable: both contexts' queued calls and published records are submitted first (a handle may come from the lock-free ring)
    {   cn_ctx *ctx = src; CHECK(flush_all(ctx)); }
    {   cn_ctx *ctx = dst; CHECK(flush_all(ctx)); }
    Buffer *I = nullptr, *O = nullptr;
    { cn_ctx *ctx = src; GETCT(I_, in, 0); I = I_; }
    { cn_ctx *ctx = dst; GETCT(O_, out, 0); O = O_; }
    if (I->size != O->size || (I->size != 2 && I->size != 3)) return fail(CN_ERR_ARG, "cn_mod_switch: ciphertext sizes %u and %u (both 2 or both 3)", I->size, O->size);
    if (!range_ok(I, ii, count) || !range_ok(O, oi, count)) return fail(CN_ERR_ARG, "index out of range");
    // the FP64 form needs the "f64" option and every modulus of the source chain below 2^49 (the target's are a prefix)
    bool f64 = src->opt.f64 && dst->opt.f64 && cn_mod_range(a, 0, a.k).f64ok, ran_f64 = false;
    if (!count) return 0;
    // ordering without a host wait: dst's stream waits for everything submitted to src (the writers of `in`), runs the switch behind its own earlier
    // work (the readers and writers of `out`), and src's stream waits for the switch (later writers of `in`)
    // (two contexts of one recording share the root's stream: stream order is enough, and the recorded graph stays one chain)
    const bool one_stream = src->stream == dst->stream;
    if (!one_stream) {
        if (!src->ev_ms) HIPCHK(hipEventCreateWithFlags(&src->ev_ms, hipEventDisableTiming));
        if (!dst->ev_ms) HIPCHK(hipEventCreateWithFlags(&dst->ev_ms, hipEventDisableTiming));
        HIPCHK(hipEventRecord(src->ev_ms, src->stream));
        HIPCHK(hipStreamWaitEvent(dst->stream, src->ev_ms, 0));
    }
    CHECK(cn_l_mod_switch(dst, I->d + (size_t)ii * I->item_words, O->d + (size_t)oi * O->item_words, src->dc, a.k, b.k, count * I->size, a.logn,
                          f64, &ran_f64));
    src->ms_f64 = dst->ms_f64 = ran_f64;
    if (!one_stream) {
        HIPCHK(hipEventRecord(dst->ev_ms, dst->stream));
        HIPCHK(hipStreamWaitEvent(src->stream, dst->ev_ms, 0));
    }
    return 0;
}
extern "C" int cn_mod_switch(cn_ctx *src, cn_handle in, uint32_t ii, uint32_t count, cn_ctx *dst, cn_handle out, uint32_t oi) {
    if (!src || !dst) return fail(CN_ERR_ARG, "null argument");
    if (src == dst) return fail(CN_ERR_ARG, "cn_mod_switch: source and target are the same context");
    // both locks, in chain order (more limbs first): two switches along one chain cannot deadlock
    cn_ctx *first = src->hc.k >= dst->hc.k ? src : dst, *second = first == src ? dst : src;
    if (first->hc.k == second->hc.k && first > second) std::swap(first, second);
    HeldLocks locks({first, second});
    return mod_switch_locked(src, in, ii, count, dst, out, oi);
}

// ---------------------------------------------------------------- recording across levels
// the contexts of a recording group in lock order: more limbs first, as cn_mod_switch takes two of them (equal limbs: lower address first)
static bool lock_order(const cn_ctx *x, const cn_ctx *y) { return x->hc.k != y->hc.k ? x->hc.k > y->hc.k : x < y; }
static int graph_begin_levels_locked(cn_ctx *root, const std::vector<cn_ctx *> &members) {
    {   cn_ctx *ctx = root; NOT_CAPTURING("cn_graph_begin_levels"); }
    for (cn_ctx *m : members) {
        if (m->capturing) return fail(CN_ERR_ARG, "cn_graph_begin_levels: a member context is already recording or a member of another recording");
        CHECK(chain_check(root, m, "cn_graph_begin_levels"));
    }
    // queued calls and published records of every context are submitted first (on their own streams)
    {   cn_ctx *ctx = root; CHECK(flush_all(ctx)); }
    for (cn_ctx *m : members) { cn_ctx *ctx = m; CHECK(flush_all(ctx)); }
    CHECK(use(root));
    for (cn_ctx *c : members) { c->cap_staged.clear(); c->cap_allocs.clear(); }
    root->cap_staged.clear(); root->cap_allocs.clear();
    HIPCHK(hipStreamBeginCapture(root->stream, hipStreamCaptureModeRelaxed));
    // every member launches on the root's capture stream until cn_graph_end (its own stream does not join the capture: one linear chain)
    for (cn_ctx *m : members) { m->own_stream = m->stream; m->stream = root->stream; m->cap_root = root; m->capturing = true; }
    root->cap_members = members; root->cap_root = root; root->capturing = true;
    return 0;
}
extern "C" int cn_graph_begin_levels(cn_ctx *root, cn_ctx *const *levels, uint32_t n) {
    if (!root || (n && !levels)) return fail(CN_ERR_ARG, "null argument");
    if (!n) return cn_graph_begin(root);
    std::vector<cn_ctx *> members(levels, levels + n);
    for (uint32_t i = 0; i < n; i++) {
        if (!members[i]) return fail(CN_ERR_ARG, "cn_graph_begin_levels: null level context at position %u", i);
        if (members[i] == root) return fail(CN_ERR_ARG, "cn_graph_begin_levels: the root is listed as a member");
    }
    std::sort(members.begin(), members.end(), lock_order);
    if (std::adjacent_find(members.begin(), members.end()) != members.end()) return fail(CN_ERR_ARG, "cn_graph_begin_levels: a level context is listed twice");
    for (cn_ctx *m : members) if (m->hc.k >= root->hc.k) return fail(CN_ERR_ARG, "cn_graph_begin_levels: a member keeps %u of the root's %u coefficient moduli (must be fewer)", m->hc.k, root->hc.k);
    // the root has the most limbs: root first, then the members in lock order
    std::vector<cn_ctx *> order(1, root);
    order.insert(order.end(), members.begin(), members.end());
    HeldLocks locks(order);
    return graph_begin_levels_locked(root, members);
}
