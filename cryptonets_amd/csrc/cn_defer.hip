// libcnhip.so host runtime (4/5): deferred submission of per-ciphertext calls (queue, hazard levels, flush as batched launches) and the consumer side of the
// lock-free submission ring (cn_submit.h).
#include "cn_api_shared.h"
#include "cn_gemm_plan.h"


// ---------------------------------------------------------------- deferred submission of per-ciphertext calls
// The reference's layers call the evaluator one ciphertext at a time from Defaults.ThreadCount threads: PoolLayer.Apply issues one
// DenseMatrixBySparseVectorMultiply + Add per (map, corner) (NeuralNetworks/PoolLayer.cs:113-121,182,214), ElementWiseMultiply one
// Multiply + Relinearize per column (HE Wrapper/EncryptedSealBfvMatrix.cs:140-154), each through Utils.ParallelProcessInEnv
// (HE Wrapper/Utils.cs:46-88).  With cn_set_option("defer", 1) such calls are not launched one by one: they are QUEUED with the device
// addresses of their operands, ordered by a dependency level (read-after-write, write-after-read and write-after-write hazards on whole
// ciphertexts), and flushed as a handful of batched launches - all pending calls of one level and one kind become ONE launch of the
// same kernels the batched entry points use, reading their operands through address tables.  A flush happens when a call arrives
// whose level is deeper than anything queued (the previous layer is then complete: its callers had to wait for it), when the queue is
// full, and before every entry point that is not deferrable (cn_sync, downloads, rotations, key changes ...).  Results are the same
// words as the immediate calls - every operation is exact modular arithmetic, batching changes no value.  Errors of a flush (HIP
// failures) surface at the call that triggered it; argument errors are still reported by the call that made them.
// What a flush launches is decided in cn_defer_plan.h (host-only: admission and the layer-boundary rule, the three queue rewrites, pending squarings, parking, staging
// layout, the ordered steps); this unit keeps the queue's plumbing and the device work.
DeferQueue *cn_defer_new() { DeferQueue *q = new DeferQueue(); q->sq = new DeferSquare(); return q; }
void cn_defer_delete(DeferQueue *q) { if (q) delete q->sq; delete q; }
// (products whose relinearisation is held back count as pending work: an array released meanwhile waits in DeferQueue::frees for the flush that settles them)
bool cn_defer_pending(cn_ctx *ctx) { return ctx->dq && (!ctx->dq->ops.empty() || !ctx->dq->sq->out.empty()); }

// what the planner reads of the environment and of a context; null: the switches alone, all that admission reads.  The only reader of the three variables:
// CN_DEFER_TRACE=1 one line per (flush, level), 2 also the host time of every flush; CN_DEFER_MERGE_GEMM=0, CN_DEFER_REL=0 (A/B)
DeferSwitches defer_switches(cn_ctx *ctx) {
    static const DeferSwitches env = [] {
        auto num = [](const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; };
        DeferSwitches s;
        s.trace = num("CN_DEFER_TRACE", 0); s.merge_gemm = num("CN_DEFER_MERGE_GEMM", 1) != 0; s.rel = num("CN_DEFER_REL", 1) != 0;
        return s; }();
    DeferSwitches s = env;
    if (!ctx) return s;
    s.fold_zero = ctx->opt.fold_zero && zero_fold_ok(ctx); s.t_half = ctx->hc.t_half;
    s.square_gemm = mul_defers_square_gemm(ctx->hc, mul_switches(ctx));
    s.ctw2 = ctx->ctw2; s.n = ctx->hc.n; s.park_max = ctx->smax / 4;
    return s;
}
// queue one operation (what it reads: defer_reads)
int defer_push(cn_ctx *ctx, DOp op) {
    DeferQueue *q = ctx->dq;
    const DeferAdmit ad = defer_admit(*q, op, defer_switches(nullptr));
    if (ad.flush) {
        // a layer boundary (or a full queue): launch what is queued, the callers go on queueing the next layer behind it
        std::vector<uint64_t> ta, tw;
        if (op.type == DOP_GEMM1) {                     // the terms of this call sit at the end of the term arrays: keep them over the flush
            ta.assign(q->addr.begin() + op.terms, q->addr.end()); tw.assign(q->wt.begin() + op.terms, q->wt.end());
            q->addr.resize(op.terms); q->wt.resize(op.terms);
        }
        CHECK(cn_defer_flush(ctx, ad.flush == DEFER_FLUSH_BOUNDARY));
        if (op.type == DOP_GEMM1) { op.terms = 0; q->addr = ta; q->wt = tw; }
    }
    defer_record(*q, op, ad);
    return 0;
}

// element-wise kernels over address tables: entry c = {a, b, out} (b: second ciphertext or plaintext polynomial)
struct Tab3 { const NTT_GLOBAL uint64_t *a, *b; NTT_GLOBAL uint64_t *out; };          // global addresses (global_load / global_store, not flat)
__global__ void k_addsub_tab(const Tab3 *__restrict__ tab, const DevConsts *__restrict__ C, uint32_t chunks, int op) {
    uint32_t limb, i; decode(chunks, limb, i);
    const uint32_t per = 2 * C->k, ct = limb / per, l = limb % per;
    const Tab3 t = tab[ct];
    const uint64_t q = C->q[l % C->k].q; const size_t o = (size_t)l * C->n + i;
    const uint64_t x = t.a[o];
    t.out[o] = op == 0 ? addmod(x, t.b[o], q) : submod(x, t.b[o], q);
}
__global__ void k_add_plain_tab(const Tab3 *__restrict__ tab, const DevConsts *__restrict__ C, uint32_t chunks, int subtract) {
    uint32_t limb, i; decode(chunks, limb, i);
    const uint32_t k = C->k, per = 2 * k, ct = limb / per, l = limb % per, j = l % k;
    const Tab3 t = tab[ct];
    const size_t o = (size_t)l * C->n + i;
    uint64_t x = t.a[o];
    if (l < k) {
        const uint64_t s = scale_plain(C, t.b[i], j), q = C->q[j].q;
        x = subtract ? submod(x, s, q) : addmod(x, s, q);
    }
    t.out[o] = x;
}

// all queued DenseMatrixBySparseVectorMultiply calls of one level with K terms each: ONE scalar GEMM over address tables
int flush_gemm_group(cn_ctx *ctx, DeferQueue *q, const std::vector<const DOp *> &ops, uint32_t K, const DeferSwitches &sw) {
    const uint32_t O = (uint32_t)ops.size();
    // the calls' lists, contiguous: A[o][kk] = address of term kk of output o (0 = padded tap), Wt[o][kk] its weight
    std::vector<uint64_t> A((size_t)O * K), Wt((size_t)O * K), out(O), bias(O);
    for (uint32_t o = 0; o < O; o++) {
        memcpy(&A[(size_t)o * K], &q->addr[ops[o]->terms], (size_t)K * 8);
        memcpy(&Wt[(size_t)o * K], &q->wt[ops[o]->terms], (size_t)K * 8);
        out[o] = (uint64_t)ops[o]->out; bias[o] = (uint64_t)ops[o]->bias;
    }
    // (the gather lists are not paired here as cn_gemm_plan_create pairs them: end to end neutral, the pairing's host time at the head of a batch - profiles/r06_defer_pair_ab.txt)
    GemmAddressPlan R;
    gemm_plan_addresses(ctx->hc, gemm_switches(ctx), A.data(), Wt.data(), out.data(), bias.data(), O, K, sw.rel, R);      // (CN_DEFER_REL=0 keeps the address tables, A/B)
    CHECK(ensure_scratch(ctx, al(R.image.size())));
    char *tables; CHECK(upload_tmp(ctx, R.image.data(), R.image.size(), &tables));
    GemmLaunch gl = gemm_launch(ctx, R.L, tables);
    if (R.abs) gl.addresses((const uint64_t *)R.some_input, R.any_bias);
    else gl.inputs((const uint64_t *)R.ibase, 32, 2).bias_at(R.any_bias ? (const uint64_t *)R.bbase : nullptr, tables + R.L.off_bidx, 32).outputs((uint64_t *)R.obase, 0, 32);
    return run_gemm_launch(ctx, R.L, gl);
}
int flush_elementwise_group(cn_ctx *ctx, const std::vector<const DOp *> &ops, int type) {
    std::vector<Tab3> tab(ops.size());
    for (size_t i = 0; i < ops.size(); i++) tab[i] = {(const NTT_GLOBAL uint64_t *)ops[i]->a, (const NTT_GLOBAL uint64_t *)ops[i]->b, (NTT_GLOBAL uint64_t *)ops[i]->out};
    CHECK(ensure_scratch(ctx, al(tab.size() * sizeof(Tab3))));
    Tab3 *dt; CHECK(upload_tmp(ctx, tab.data(), tab.size(), &dt));
    const uint32_t limbs = (uint32_t)ops.size() * 2 * ctx->hc.k;
    if (type == DOP_ADD || type == DOP_SUB) hipLaunchKernelGGL(k_addsub_tab, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, dt, ctx->dc, ctx->chunks, type == DOP_SUB);
    else hipLaunchKernelGGL(k_add_plain_tab, dim3(limbs * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, dt, ctx->dc, ctx->chunks, type == DOP_SUBPLAIN);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    return 0;
}
// ---- deferred squarings that feed the next dense layer (DeferSquare, cn_api_shared.h)
static bool defer_trace() { static const bool on = defer_switches(nullptr).trace != 0; return on; }
void defer_square_drop_plans(cn_ctx *ctx) {
    if (!ctx->dq || ctx->dq->sq->plans.empty()) return;
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto &p : ctx->dq->sq->plans) if (p->P.dev) (void)hipFree(p->P.dev);
    ctx->dq->sq->plans.clear();
}
void defer_square_release(cn_ctx *ctx) {
    if (!ctx->dq) return;
    defer_square_drop_plans(ctx);
    DeferSquare &sq = *ctx->dq->sq;
    if (sq.arr) (void)hipFree(sq.arr);
    sq.arr = nullptr; sq.cap = 0; sq.out.clear(); sq.slot.clear();
}
// The squarings of one level at a layer-boundary flush that may keep their relinearisation back (defer_can_park) do so if the products fit the context's product array
// (the array is not grown while a graph is alive).  Only the Multiply half runs: products into slots 0 .. n - 1, output array -> slot noted.  False: the caller
// relinearises them at once.
static bool park_squarings(cn_ctx *ctx, DeferQueue *q, const std::vector<const DOp *> &ops, const DeferReleased &released, const DeferSwitches &sw, int32_t level, int *rc) {
    DeferSquare &sq = *q->sq;
    if (!defer_can_park(*q, ops, released, sw, !sq.out.empty())) return false;
    const size_t kn = (size_t)ctx->hc.k * ctx->hc.n, need = ops.size() * sw.product_bytes();
    if (need > sq.cap) {
        if (ctx->capturing || ctx->graphs_alive) return false;
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { *rc = fail(CN_ERR_HIP, "hipStreamSynchronize failed"); return true; }
        if (sq.arr) (void)hipFree(sq.arr);
        sq.arr = nullptr; sq.cap = 0;
        const size_t want = need + (need >> 3);
        if (hipMalloc((void **)&sq.arr, want) != hipSuccess) { (void)hipGetLastError(); sq.arr = nullptr; return false; }
        sq.cap = want;
    }
    const uint32_t n = (uint32_t)ops.size();
    std::vector<const uint64_t *> ha(n);
    for (uint32_t i = 0; i < n; i++) ha[i] = ops[i]->a;
    *rc = mul_chunks(ctx, mul_batch(ctx->hc, mul_switches(ctx), MUL_AT_PARK, n, true), n, true, [&](uint32_t s0, uint32_t c) -> int {
        const uint64_t **da;
        CHECK(upload_tmp(ctx, ha.data() + s0, c, &da));
        return do_multiply(ctx, nullptr, 1, nullptr, 1, sq.arr + (size_t)s0 * 3 * kn, c, da, da);
    });
    if (*rc) return true;
    sq.out.resize(n);
    for (uint32_t i = 0; i < n; i++) { sq.out[i] = ops[i]->out; sq.slot[ops[i]->out] = i; }
    if (defer_trace()) fprintf(stderr, "defer %p level %d: parks %u squarings (Multiply only, %zu MB of products)\n", (void *)ctx, level, n, need >> 20);
    return true;
}
// every product with need[slot] set is relinearised into its own output array (do_keyswitch from its slot, as flush_mulrelin_group would have), runs of slots per launch
static int pending_materialise(cn_ctx *ctx, DeferSquare &sq, const std::vector<uint8_t> &need) {
    const uint32_t n = (uint32_t)sq.out.size();
    const size_t kn = (size_t)ctx->hc.k * ctx->hc.n;
    CHECK(ensure_scratch(ctx, al((size_t)n * 8) + 4096));
    uint64_t **dout; CHECK(upload_tmp(ctx, sq.out.data(), n, &dout));
    uint32_t done = 0;
    for (uint32_t s = 0; s < n;) {
        if (!need[s]) { s++; continue; }
        uint32_t e = s; while (e < n && need[e]) e++;
        CHECK(do_keyswitch(ctx, ctx->rlk, KsCall::relin(sq.arr + (size_t)s * 3 * kn, kn, e - s).to_table(dout + s)));
        done += e - s; s = e;
    }
    if (defer_trace()) fprintf(stderr, "defer %p: materialises %u of %u pending products (one key switch each)\n", (void *)ctx, done, n);
    return 0;
}
// the plan of a dense layer on deferred squarings: found by (O, K, weights, renumbered slot pattern) or built (build_gemm_plan: validation, grouping, weight tiles,
// GemmPlan::dig) and kept, its weights on the device.  `keep`: entries used since this tick belong to the flush at hand and are not evicted
static SgPlan *sg_plan(cn_ctx *ctx, DeferSquare &sq, uint32_t O, uint32_t K, std::vector<uint64_t> &W, std::vector<int32_t> &cidx, uint64_t keep) {
    for (auto &p : sq.plans)
        if (p->O == O && p->K == K && !memcmp(p->W.data(), W.data(), W.size() * 8) && !memcmp(p->cidx.data(), cidx.data(), cidx.size() * 4)) { p->used = ++sq.tick; return p.get(); }
    if (sq.plans.size() >= DEFER_SQ_PLANS) {
        size_t v = sq.plans.size();
        for (size_t i = 0; i < sq.plans.size(); i++) if (sq.plans[i]->used <= keep && (v == sq.plans.size() || sq.plans[i]->used < sq.plans[v]->used)) v = i;
        if (v < sq.plans.size()) {
            if (sq.plans[v]->P.dev) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(sq.plans[v]->P.dev); }
            sq.plans.erase(sq.plans.begin() + v);
        }
    }
    std::unique_ptr<SgPlan> p(new SgPlan());
    p->O = O; p->K = K; p->W.swap(W); p->cidx.swap(cidx); p->used = ++sq.tick;
    GemmPlan &P = p->P;
    if (build_gemm_plan(ctx, p->cidx.data(), p->W.data(), O, K, nullptr, 0, nullptr, P)) return nullptr;     // (unreachable for queued calls: their weights and rows were checked when they were queued)
    p->ok = P.dig;                                                // (a layer outside the digit bound stays cached as such: it is not planned again every batch)
    if (p->ok) {
        p->idx.assign(P.gather<int32_t>(P.host.data()), P.gather<int32_t>(P.host.data()) + (size_t)P.G * P.Kp);
        p->oidx.assign(P.members<int32_t>(P.host.data()), P.members<int32_t>(P.host.data()) + (size_t)P.G * P.M);
        if (hipMalloc((void **)&P.dev, P.host.size()) != hipSuccess || hipMemcpy(P.dev, P.host.data(), P.host.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            if (P.dev) (void)hipFree(P.dev);
            P.dev = nullptr; p->ok = false;
        }
    }
    P.host.clear(); P.host.shrink_to_fit();
    sq.plans.push_back(std::move(p));
    return sq.plans.back().get();
}
// The device half of the decision about pending products (defer_pending_decide has rules (a)-(d) and the candidate groups): the plan of every group is found or built,
// passes square_gemm_fused_ok and fits the scratch limits, and the group's biases are addressable - or the answer is no for all.  plans[g]: the plan of groups[g]
static bool sg_prepare(cn_ctx *ctx, DeferQueue *q, const std::vector<uint8_t> &dead, const DeferReleased &released, const DeferSwitches &sw, std::vector<DeferSgGroup> &groups,
                       std::vector<SgPlan *> &plans, std::vector<uint8_t> &need) {
    DeferSquare &sq = *q->sq;
    if (!defer_pending_decide(*q, dead, released, sq.out, sq.slot, sw, need, groups)) return false;
    const uint64_t keep = sq.tick;
    for (DeferSgGroup &g : groups) {
        SgPlan *plan = sg_plan(ctx, sq, (uint32_t)g.rows.size(), g.K, g.W, g.cidx, keep);
        if (!plan || !plan->ok || !square_gemm_fused_ok(ctx->hc, mul_switches(ctx), plan->P) || mul_sg_scratch(ctx->hc, plan->P, plan->P.O) > ctx->smax) return false;
        if (mul_sg_scratch(ctx->hc, plan->P, plan->P.O) > ctx->scap && ctx->graphs_alive) return false;       // (the scratch arena does not grow while a graph is alive)
        if (!g.bias_ok) return false;
        plans.push_back(plan);
    }
    return true;
}
// one group in cn_square_gemm's second half: the GEMM over components 0 and 1 of the products (+ the folded bias) into a contiguous temporary, the digit GEMM into S,
// one KsDigits key switch per output that adds the temporary and writes the callers' arrays through its output table (no scatter copy)
static int sg_run(cn_ctx *ctx, DeferQueue *q, const DeferSgGroup &g, const SgPlan &sp) {
    const GemmPlan &P = sp.P;
    const uint32_t n = ctx->hc.n, k = ctx->hc.k, tot = ctx->hc.rl_tot;
    const size_t kn = (size_t)k * n;
    std::vector<int32_t> pidx(sp.idx.size()), bidx(sp.oidx.size(), 0);
    std::vector<uint64_t *> outs(P.O);
    for (size_t x = 0; x < pidx.size(); x++) pidx[x] = sp.idx[x] >= 0 ? g.slot_of[sp.idx[x]] : -1;
    const bool bias = g.rows[0]->bias != nullptr;
    uint64_t bbase = ~0ull;
    if (bias) {
        for (const DOp *r : g.rows) bbase = std::min(bbase, (uint64_t)r->bias);
        for (size_t x = 0; x < bidx.size(); x++) if (sp.oidx[x] >= 0) bidx[x] = (int32_t)(((uint64_t)g.rows[sp.oidx[x]]->bias - bbase) >> 8);
    }
    for (uint32_t o = 0; o < P.O; o++) outs[o] = g.rows[o]->out;
    CHECK(ensure_scratch(ctx, mul_sg_scratch(ctx->hc, P, P.O)));
    uint64_t *T = salloc<uint64_t>(ctx, (size_t)P.O * 2 * kn);
    void *S = salloc<char>(ctx, (size_t)P.O * tot * n * (P.dig_i32 ? 4 : 8));       // int32 words where the plan's digit bound allows (GemmPlan::dig_i32)
    if (!T || !S) return fail(CN_ERR_HIP, "internal: scratch exhausted in the deferred square + dense form");
    int32_t *dpidx, *dbidx; uint64_t **douts;
    CHECK(upload_tmp(ctx, pidx.data(), pidx.size(), &dpidx)); CHECK(upload_tmp(ctx, bidx.data(), bidx.size(), &dbidx)); CHECK(upload_tmp(ctx, outs.data(), outs.size(), &douts));
    const uint64_t *arr = q->sq->arr;
    // two components of every product, three apart; bias polynomials as 256-byte offsets from the lowest one (as flush_gemm_group)
    CHECK(run_gemm_launch(ctx, P, gemm_launch(ctx, P, P.dev).gather(dpidx).inputs(arr, (uint32_t)(3 * kn), 2).bias_at(bias ? (const uint64_t *)bbase : nullptr, dbidx, 32).outputs(T, 0, 0)));
    CHECK(cn_l_digit_gemm(ctx, DigitGemmLaunch::of(P, P.dev, arr + 2 * kn, 3 * kn, dpidx, S)));
    CHECK(do_keyswitch(ctx, ctx->rlk, KsCall::relin_digits(S, P.dig_i32, T, kn, P.O).to_table(douts)));
    ctx->cnt.dsg_fused++;
    if (defer_trace()) fprintf(stderr, "defer %p level %d: fuses %u scalar products over %zu pending products (GEMM, digit GEMM%s, %u key switches)\n", (void *)ctx, g.level, P.O,
                               g.slot_of.size(), P.dig_mfma ? " on the matrix cores" : "", P.O);
    return 0;
}

// the queued squarings (SquareActivation: the fused kernel) or the queued general products (separate launches) of one level, as the schedule splits them: the batched
// BEHZ pipeline + ONE key switch, operands and results through tables
int flush_mulrelin_group(cn_ctx *ctx, const std::vector<const DOp *> &ops, bool sq) {
    std::vector<const uint64_t *> ha(ops.size()), hb(sq ? 0 : ops.size()); std::vector<uint64_t *> ho(ops.size());
    for (size_t i = 0; i < ops.size(); i++) { ha[i] = ops[i]->a; ho[i] = ops[i]->out; if (!sq) hb[i] = ops[i]->b; }
    MulRelinCall m;
    m.ha = ha.data(); m.hb = sq ? ha.data() : hb.data(); m.ho = ho.data();
    return run_mul_relin(ctx, m, (uint32_t)ops.size(), MUL_AT_DEFERRED, 2);
}

// ---- staged kinds (DOP_COPY .. DOP_SUMSLOTS): the per-ciphertext calls of an unchanged LoLa-style caller - one MultiplyPlain, SumAllSlots,
// RotateRows(AndAdd) per matrix row (EncryptedSealBfvMatrix.cs:79-120: `leVectors[row].DotProduct(v)` in a loop over the rows, LLInterleaveLayer:
// one PointwiseMultiply per column).  The rows are independent, so the queue puts row r's k-th call and row r''s k-th call on the same
// level; at flush all calls of one level, kind and parameter (rotation steps / slot count) are executed as ONE batched call of the same
// implementation the batched entry points use: their operand ciphertexts are gathered into a contiguous staging array (one table-driven
// copy launch), the batched implementation runs on it, the results are scattered to the callers' arrays (one more copy launch).  The
// copies move 2 x 640 KiB per ciphertext and call - microseconds against the key switches they let merge (13 rows of LoLa's dense
// layer: 13 x 10 single-ciphertext key switches become 10 key switches of 13 ciphertexts).  Same words: the batched implementations
// are bit-identical to their count-1 selves (tests/test_deferred.py, tests/test_lola.py).

__global__ void k_copy_tab(const Tab2 *__restrict__ tab, uint32_t pairs_per_item) {          // grid (chunks, items); 16 B per thread
    const Tab2 t = tab[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    typedef unsigned long long v2u64 __attribute__((ext_vector_type(2)));          // (a plain vector type: assignable through a global-address-space pointer)
    if (i < pairs_per_item) reinterpret_cast<NTT_GLOBAL v2u64 *>(t.dst)[i] = reinterpret_cast<const NTT_GLOBAL v2u64 *>(t.src)[i];
}
int ensure_stage(cn_ctx *ctx, size_t bytes) {
    if (bytes <= ctx->stage_cap) return 0;
    if (ctx->capturing || ctx->graphs_alive) return fail(CN_ERR_ARG, "the staging arena would have to grow while a graph is recorded / alive");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->stage) HIPCHK(hipFree(ctx->stage));
    ctx->stage = nullptr; ctx->stage_cap = 0;
    const size_t want = bytes + (bytes >> 2) + (1 << 20);
    HIPCHK(hipMalloc((void **)&ctx->stage, want));
    ctx->stage_cap = want;
    return 0;
}
// host table -> device (a block the context keeps alive until the stream has drained, like upload_tmp), then one copy launch
int copy_by_table(cn_ctx *ctx, const std::vector<Tab2> &tab, Tab2 *dtab, uint32_t words_per_item) {
    if (tab.empty()) return 0;
    const void *ptab;
    CHECK(place_table(ctx, tab.data(), tab.size() * sizeof(Tab2), dtab, &ptab));
    const uint32_t pairs = words_per_item / 2;
    hipLaunchKernelGGL(k_copy_tab, dim3((pairs + 255) / 256, (unsigned)tab.size()), dim3(256), 0, ctx->stream, (const Tab2 *)ptab, pairs);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    return 0;
}
static_assert(sizeof(Tab2) == DEFER_TAB2_BYTES, "defer_staged_layout sizes the copy tables");
// one step of a staged kind, as the schedule cuts them: all copies of a level, few rotations by any step counts, or the calls of one kind and one argument
int flush_staged_group(cn_ctx *ctx, const DeferStep &step, const DeferSwitches &sw) {
    const std::vector<const DOp *> &ops = step.ops;
    const int type = step.type;
    if (step.kind == DSTEP_COPY) {                           // Ciphertext copies: the table copy is the operation
        CHECK(ensure_stage(ctx, al(ops.size() * sizeof(Tab2))));
        std::vector<Tab2> tab(ops.size());
        for (size_t i = 0; i < ops.size(); i++) tab[i] = {(const NTT_GLOBAL uint64_t *)ops[i]->a, (NTT_GLOBAL uint64_t *)ops[i]->out};
        return copy_by_table(ctx, tab, (Tab2 *)ctx->stage, (uint32_t)ctx->ctw2);
    }
    if (step.kind == DSTEP_ROT_JOBS) {                       // few rotations, any step counts: one launch chain per hop round
        std::vector<RotJob> jobs(ops.size());
        for (size_t i = 0; i < ops.size(); i++) jobs[i] = {ops[i]->a, ops[i]->out, (int)ops[i]->arg};
        return rotate_jobs(ctx, jobs);
    }
    // one batched call: operands the callers hold equally spaced are used in place, the others gathered into the staging arena (defer_staged_layout)
    const uint32_t n = ctx->hc.n, cnt = (uint32_t)ops.size(); const size_t ctw = ctx->ctw2;
    const DeferStaged L = defer_staged_layout(type, ops, sw);
    if (!L.consistent) return fail(CN_ERR_ARG, "internal: in-place staged call with different operand and result addresses");
    CHECK(ensure_stage(ctx, L.total));
    char *base = ctx->stage;
    Tab2 *t_in = (Tab2 *)(base + L.off_tin), *t_pt = (Tab2 *)(base + L.off_tpt), *t_out = (Tab2 *)(base + L.off_tout);
    uint64_t *A = L.a_direct ? const_cast<uint64_t *>(ops[0]->a) : (uint64_t *)(base + L.off_a);
    uint64_t *B = !L.has_b ? nullptr : L.b_direct ? const_cast<uint64_t *>(ops[0]->b) : (uint64_t *)(base + L.off_b);
    uint64_t *P = !L.has_p ? nullptr : L.p_direct ? const_cast<uint64_t *>(ops[0]->b) : (uint64_t *)(base + L.off_p);
    uint64_t *O = L.out_direct ? ops[0]->out : (uint64_t *)(base + L.off_o);
    std::vector<Tab2> gin, gpt, gout;
    for (uint32_t i = 0; i < cnt; i++) {
        if (!L.a_direct) gin.push_back({(const NTT_GLOBAL uint64_t *)ops[i]->a, (NTT_GLOBAL uint64_t *)(A + (size_t)i * ctw)});
        if (L.has_b && !L.b_direct) gin.push_back({(const NTT_GLOBAL uint64_t *)ops[i]->b, (NTT_GLOBAL uint64_t *)(B + (size_t)i * ctw)});
        if (L.has_p && !L.p_direct) gpt.push_back({(const NTT_GLOBAL uint64_t *)ops[i]->b, (NTT_GLOBAL uint64_t *)(P + (size_t)i * n)});
        if (!L.out_direct) gout.push_back({(const NTT_GLOBAL uint64_t *)(O + (size_t)i * ctw), (NTT_GLOBAL uint64_t *)ops[i]->out});
    }
    if (!gin.empty()) CHECK(copy_by_table(ctx, gin, t_in, (uint32_t)ctw));
    if (!gpt.empty()) CHECK(copy_by_table(ctx, gpt, t_pt, n));
    const CtSpan sa{A, L.same_a ? 1u : cnt}, sb{B, cnt}, so{O, cnt};
    int rc = 0;
    switch (type) {
    case DOP_MULPLAIN: rc = mul_plain_impl(ctx, sa, L.same_a, PtSpan{P, 1, nullptr}, so, 2); break;      // (zero plaintexts were refused when the calls were queued)
    case DOP_ROT: rc = rotate_rows_impl(ctx, sa, (int)step.key, so); break;
    case DOP_ROTADD: rc = rotate_rows_add_impl(ctx, sa, (int)step.key, sb, so); break;
    case DOP_COLS: case DOP_COLSADD: rc = galois_impl(ctx, sa, 2ull * n - 1, sb, so); break;
    case DOP_SUMSLOTS: rc = sum_slots_impl(ctx, sa, (uint32_t)step.key); break;
    default: rc = fail(CN_ERR_ARG, "internal: staged kind %d", type);
    }
    CHECK(rc);
    if (!gout.empty()) CHECK(copy_by_table(ctx, gout, t_out, (uint32_t)ctw));
    return 0;
}
// queue `count` per-ciphertext operations of a staged kind (arguments were checked by the caller)
int defer_staged(cn_ctx *ctx, int type, CtSpan a, CtSpan b, CtSpan o, int64_t arg, const uint64_t *plain, uint32_t pstride_words) {
    for (uint32_t c = 0; c < o.count; c++) {
        const uint64_t *pa = a.d + c * ctx->ctw2, *pb = b.d ? b.d + c * ctx->ctw2 : nullptr;
        DOp op{type, 0, o.d + c * ctx->ctw2, pa, plain ? plain + (size_t)c * pstride_words : pb, 0, 0, nullptr};
        op.arg = arg;
        CHECK(defer_push(ctx, op));
    }
    return 0;
}

// n single ciphertexts (or dense plaintexts) that live in n arrays into consecutive places of one array, ONE launch (see include/cnhip.h)
extern "C" int cn_copy_many(cn_ctx *ctx, const cn_handle *src, const uint32_t *sfirst, uint32_t n, cn_handle dst, uint32_t dfirst) { API_BODY
    LOCK_ONLY;
    if (!n) return 0;
    if (!src) return fail(CN_ERR_ARG, "null argument");
    Buffer *d = ctx->bufs.find(dst);
    if (!d || d->kind > 1) return fail(CN_ERR_ARG, "invalid handle");
    if (!range_ok(d, dfirst, n)) return fail(CN_ERR_ARG, "index out of range");
    std::vector<Buffer *> sb(n);
    for (uint32_t i = 0; i < n; i++) {
        Buffer *b = ctx->bufs.find(src[i]);
        const uint32_t f = sfirst ? sfirst[i] : 0;
        if (!b) return fail(CN_ERR_ARG, "invalid handle");
        if (b->kind != d->kind || b->item_words != d->item_words) return fail(CN_ERR_ARG, "copy between different buffer shapes");
        if (!range_ok(b, f, 1)) return fail(CN_ERR_ARG, "index out of range");
        if (b == d && f >= dfirst && f < dfirst + n && f != dfirst + i) return fail(CN_ERR_ARG, "copy_many: a source lies inside the destination range");
        sb[i] = b;
    }
    if (deferring(ctx) && d->kind == 0 && d->size == 2) {          // queued like n cn_copy calls
        for (uint32_t i = 0; i < n; i++)
            CHECK(defer_staged(ctx, DOP_COPY, CtSpan{sb[i]->d + (sfirst ? sfirst[i] : 0) * ctx->ctw2, 1}, CtSpan{}, CtSpan{d->d + (dfirst + i) * ctx->ctw2, 1}, 0));
        return 0;
    }
    CHECK(cn_defer_flush(ctx));
    CHECK(ensure_stage(ctx, al(n * sizeof(Tab2))));
    std::vector<Tab2> tab(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t f = sfirst ? sfirst[i] : 0;
        tab[i] = {(const NTT_GLOBAL uint64_t *)(sb[i]->d + (size_t)f * d->item_words), (NTT_GLOBAL uint64_t *)(d->d + (size_t)(dfirst + i) * d->item_words)};
        if (d->kind == 1) d->pt_zero[dfirst + i] = sb[i]->pt_zero[f];
    }
    return copy_by_table(ctx, tab, (Tab2 *)ctx->stage, (uint32_t)d->item_words);
API_END }

// all queued Encryptor.Encrypt calls of one level: one sampling / transform / tail launch chain over a table
int flush_encrypt_group(cn_ctx *ctx, const std::vector<const DOp *> &ops) {
    std::vector<EncTab> tab(ops.size());
    for (size_t i = 0; i < ops.size(); i++) tab[i] = {(NTT_GLOBAL uint64_t *)ops[i]->out, (const NTT_GLOBAL uint64_t *)ops[i]->a, ops[i]->nonce, ops[i]->item};
    const size_t per = (size_t)ctx->hc.k * ctx->hc.n * 8 + 3 * (size_t)ctx->hc.n + sizeof(EncTab) + 64;
    const uint32_t ch = cn_chunk_of(ctx->smax, per, (uint32_t)ops.size());
    for (uint32_t s0 = 0; s0 < ops.size(); s0 += ch) {
        const uint32_t c = std::min<uint32_t>(ch, (uint32_t)ops.size() - s0);
        CHECK(encrypt_chain(ctx, c, nullptr, 0, nullptr, 0, tab.data() + s0));
    }
    return 0;
}
// the weighted sums of folded zero encryptions (cn_defer_flush), added onto the outputs of the scalar products `gemms` (launched just before): the samplers draw
// u, e1, e2 of every folded encryption exactly as flush_encrypt_group would have (its nonce, its item), k_encrypt_fold does the rest
bool zero_fold_ok(cn_ctx *ctx) {
    return ctx->pk && ctx->opt.enc_fused && rr_kernels(ctx, 13) && ctx->opt.f64 && cn_mod_range(ctx->hc, 0, ctx->hc.k).f64ok;
}
int flush_zero_folds(cn_ctx *ctx, DeferQueue *q, const std::vector<const DOp *> &gemms) {
    const uint32_t n = ctx->hc.n;
    std::vector<EncTab> tab; std::vector<FoldOut> fo; std::vector<FoldTerm> ft;
    const uint64_t t = ctx->hc.t.q, t_half = ctx->hc.t_half;
    for (const DOp *G : gemms) {
        fo.push_back({G->out, (uint32_t)ft.size(), G->fold_count});
        for (uint32_t f = 0; f < G->fold_count; f++) {
            const DeferQueue::Fold &fd = q->folds[(size_t)G->fold_first + f];
            const DOp &E = q->ops[fd.enc];
            tab.push_back({nullptr, nullptr, E.nonce, E.item});
            ft.push_back({fd.w >= t_half ? -(double)(t - fd.w) : (double)fd.w, (uint32_t)tab.size() - 1, 0});
        }
    }
    const uint32_t cnt = (uint32_t)tab.size();
    CHECK(ensure_scratch(ctx, al((size_t)cnt * n) + al((size_t)cnt * 2 * n) + al(cnt * sizeof(EncTab)) + al(fo.size() * sizeof(FoldOut)) + al(ft.size() * sizeof(FoldTerm)) + 1024));
    int8_t *us = salloc<int8_t>(ctx, (size_t)cnt * n), *es = salloc<int8_t>(ctx, (size_t)cnt * 2 * n);
    if (!us || !es) return fail(CN_ERR_HIP, "internal: scratch exhausted in the zero-encryption fold");
    EncTab *dtab; FoldOut *dfo; FoldTerm *dft;
    CHECK(upload_tmp(ctx, tab.data(), tab.size(), &dtab)); CHECK(upload_tmp(ctx, fo.data(), fo.size(), &dfo)); CHECK(upload_tmp(ctx, ft.data(), ft.size(), &dft));
    const RngKey key = rng_key_of(ctx);
    hipLaunchKernelGGL(k_sample_small, dim3((unsigned)(((uint64_t)cnt * (n / 16) + 255) / 256)), dim3(256), 0, ctx->stream, us, n, 0, 1u, cnt, key, 0ull, 0u, 0ull, (const EncTab *)dtab, cn_noise_table());
    hipLaunchKernelGGL(k_sample_small, dim3((unsigned)(((uint64_t)cnt * 2 * (n / 8) + 255) / 256)), dim3(256), 0, ctx->stream, es, n, 1, 2u, cnt, key, 0ull, 1u, 0ull, (const EncTab *)dtab, cn_noise_table());
    const int pol = cn_policy(cn_mod_range(ctx->hc, 0, ctx->hc.k), true);       // zero_fold_ok held when the folds were queued: the pick is between the two FP64 policies
    if (!rr_ops[pol]->enc_fold(ctx, us, es, dfo, dft, (uint32_t)fo.size())) return fail(CN_ERR_ARG, "internal: zero-encryption fold without a kernel");
    HIPCHK(hipGetLastError()); launch_count(ctx, 3);
    ctx->st.ntt_forward_limbs += (uint64_t)fo.size() * ctx->hc.k; ctx->st.ntt_inverse_limbs += (uint64_t)fo.size() * 2 * ctx->hc.k;
    return 0;
}
int defer_encrypt(cn_ctx *ctx, const uint64_t *ptd, uint32_t pt_stride_words, Buffer *O, uint32_t oi, uint32_t count, uint64_t seed) {
    for (uint32_t c = 0; c < count; c++) {
        DOp op{DOP_ENCRYPT, 0, O->d + (size_t)(oi + c) * O->item_words, ptd ? ptd + (size_t)c * pt_stride_words : nullptr, nullptr, 0, 0, nullptr};
        op.nonce = seed; op.item = ctx->rng_item++;
        CHECK(defer_push(ctx, op));
    }
    return 0;
}

// CN_DEFER_TRACE: one line per (flush, level) - calls per kind with the number of their arguments, launches (the steps of the level begin at steps[first])
static void defer_trace_level(cn_ctx *ctx, int32_t lv, const std::vector<DeferStep> &steps, size_t first, uint64_t l0) {
    size_t calls[DOP_TYPES] = {}; std::map<int64_t, int> args[DOP_TYPES];
    for (size_t i = first; i < steps.size() && steps[i].level == lv; i++) {
        if (steps[i].kind == DSTEP_ZERO_FOLD) continue;      // (its scalar products are counted with their own step)
        for (const DOp *op : steps[i].ops) { calls[op->type]++; args[op->type][op->arg]++; }
    }
    char line[512]; int o = snprintf(line, sizeof line, "defer %p level %d:", (void *)ctx, lv);
    for (int t = 0; t < DOP_TYPES; t++) if (calls[t]) o += snprintf(line + o, sizeof line - o, " kind%d x%zu (%zu args)", t, calls[t], args[t].size());
    fprintf(stderr, "%s -> %llu launches\n", line, (unsigned long long)(ctx->st.kernel_launches - l0));
}
// the flush: the planner's rewrites and steps (cn_defer_plan.h), one batched launch chain per step
int cn_defer_flush(cn_ctx *ctx, bool boundary) {
    DeferQueue *q = ctx->dq;
    if (!q) return 0;
    int rc = 0;
    DeferSquare &sqs = *q->sq;
    const bool work = !q->ops.empty() || !sqs.out.empty();
    const DeferSwitches sw = defer_switches(work ? ctx : nullptr);      // (every locked entry point comes through here: an empty queue reads nothing of the context)
    // CN_DEFER_TRACE=2: host time of every flush (the flush runs on the thread of the call that triggered it, under the context lock: every other caller of the
    // context waits for it, and so does the device if it has run dry)
    struct FlushTimer { bool on; size_t nops; cn_ctx *c; std::chrono::steady_clock::time_point t0; ~FlushTimer() {
        if (on && nops) fprintf(stderr, "defer %p flush of %zu calls: %.0f us of host time\n", (void *)c, nops,
                                1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); } }
        ft{sw.trace >= 2, q->ops.size(), ctx, std::chrono::steady_clock::now()};
    if (work) {
        const DeferReleased released(q->frees);
        std::vector<uint8_t> dead(q->ops.size(), 0);
        defer_fold_bias(*q, dead, released);
        ctx->cnt.folded_zero += defer_fold_zero(*q, dead, released, sw);
        defer_merge_gemm(*q, dead, sw);
        // products whose relinearisation an earlier layer-boundary flush held back: the scalar products that read them run in cn_square_gemm's second half (at their
        // level, below), or every product is relinearised into its own array first and the flush proceeds as ever
        std::vector<DeferSgGroup> sgs; std::vector<SgPlan *> plans;
        if (!sqs.out.empty()) {
            std::vector<uint8_t> need;
            if (!sg_prepare(ctx, q, dead, released, sw, sgs, plans, need)) { sgs.clear(); rc = pending_materialise(ctx, sqs, need); }
            sqs.out.clear(); sqs.slot.clear();              // (the groups carry the slots they read; released arrays without a reader just give their slots back)
        }
        const std::vector<DeferStep> steps = defer_schedule(*q, dead, sgs, boundary, sw, [&](size_t count) { return ks_few_rotations(ctx->hc, ks_switches(ctx), count); });
        size_t at = 0;
        for (int32_t lv = 0; lv <= q->maxlevel && !rc; lv++) {
            const uint64_t l0 = ctx->st.kernel_launches;
            const size_t first = at;
            for (; at < steps.size() && steps[at].level == lv && !rc; at++) {
                const DeferStep &s = steps[at];
                switch (s.kind) {
                case DSTEP_GEMM: rc = flush_gemm_group(ctx, q, s.ops, (uint32_t)s.key, sw); break;
                case DSTEP_FUSED: rc = sg_run(ctx, q, sgs[s.key], *plans[s.key]); break;
                case DSTEP_ZERO_FOLD: rc = flush_zero_folds(ctx, q, s.ops); break;
                case DSTEP_ELEMENTWISE: rc = flush_elementwise_group(ctx, s.ops, s.type); break;
                case DSTEP_ENCRYPT: rc = flush_encrypt_group(ctx, s.ops); break;
                case DSTEP_COPY: case DSTEP_ROT_JOBS: case DSTEP_STAGED: rc = flush_staged_group(ctx, s, sw); break;
                case DSTEP_MULRELIN: if (!(s.park && park_squarings(ctx, q, s.ops, released, sw, lv, &rc))) rc = flush_mulrelin_group(ctx, s.ops, s.key == 1); break;
                }
            }
            if (sw.trace) defer_trace_level(ctx, lv, steps, first, l0);
        }
    }
    if (rc) { sqs.out.clear(); sqs.slot.clear(); }          // an error drops the pending state with the queue
    q->ops.clear(); q->addr.clear(); q->wt.clear(); q->haz.clear(); q->maxlevel = -1; q->folds.clear();
    for (auto &f : q->frees) { int r2 = dev_release(ctx, f.first, f.second); if (!rc) rc = r2; }
    q->frees.clear();
    return rc;
}
// true when the call is to be queued rather than launched (the caller holds the lock)
bool deferring(cn_ctx *ctx) { return ctx->defer && !ctx->capturing; }

/* DenseMatrixBySparseVectorMultiply for ONE output block whose K input ciphertexts are separate objects (see include/cnhip.h) */
extern "C" int cn_scalar_dot(cn_ctx *ctx, const cn_handle *in, const uint32_t *in_idx, const uint64_t *w, uint32_t K, cn_handle out, uint32_t oi) {
    if (submit_async(ctx) && K && in && w) {            // the call's lists travel in one block: K handles, K weights, K indices (if any)
        char *blk = (char *)malloc((size_t)K * (in_idx ? 20 : 16));
        if (!blk) return fail(CN_ERR_ARG, "out of host memory");
        memcpy(blk, in, (size_t)K * 8); memcpy(blk + (size_t)K * 8, w, (size_t)K * 8);
        if (in_idx) memcpy(blk + (size_t)K * 16, in_idx, (size_t)K * 4);
        return ring_push(ctx, SUB_SCALAR_DOT, 1, 0, in_idx ? 1u : 0u, 0, 0, out, oi, K, (uint64_t)(uintptr_t)blk);
    }
    API_BODY LOCK_ONLY; return scalar_dot_body(ctx, in, in_idx, w, K, out, oi); API_END
}
int scalar_dot_body(cn_ctx *ctx, const cn_handle *in, const uint32_t *in_idx, const uint64_t *w, uint32_t K, cn_handle out, uint32_t oi) {
    GETCT(O, out, 2);
    if (!K || !in || !w) return fail(CN_ERR_ARG, "empty scalar product");
    if (oi >= O->count) return fail(CN_ERR_ARG, "index out of range");
    DeferQueue *q = ctx->dq;
    const size_t t0 = q->addr.size();
    bool any = false;
    uint64_t *o = O->d + (size_t)oi * O->item_words;
    uint64_t nnz = 0;
    for (uint32_t kk = 0; kk < K; kk++) {
        const uint64_t wk = w[kk];
        if (wk >= ctx->hc.t.q) { q->addr.resize(t0); q->wt.resize(t0); return fail(CN_ERR_ARG, "weight >= plain modulus"); }
        uint64_t a = 0;
        if (in[kk]) {                                        // handle 0: padded tap (PoolLayer.cs:68-80), skipped
            Buffer *I = getbuf(ctx, in[kk], 0);
            const uint32_t ii = in_idx ? in_idx[kk] : 0;
            if (!I || I->size != 2 || ii >= I->count) { q->addr.resize(t0); q->wt.resize(t0); return fail(CN_ERR_ARG, "invalid input ciphertext %u", kk); }
            const uint64_t *p = I->d + (size_t)ii * I->item_words;
            if (p == o) { q->addr.resize(t0); q->wt.resize(t0); return fail(CN_ERR_ARG, "scalar product cannot run in place"); }
            a = (uint64_t)p;                  // (a zero weight keeps its address: outputs that share a patch still share a gather list)
            if (wk) { any = true; nnz++; }                   // zero weights contribute nothing (AtomicSealBfvVector.cs:468 skips them)
        }
        q->addr.push_back(a); q->wt.push_back(a ? wk : 0);
    }
    if (!any) { q->addr.resize(t0); q->wt.resize(t0); return fail(CN_ERR_ARG, "output has no non-zero term (AddMany of nothing)"); }
    DOp op{DOP_GEMM1, 0, o, nullptr, nullptr, K, t0, nullptr};
    CHECK(defer_push(ctx, op));
    ctx->st.PlainMultiplication += nnz; ctx->st.Addition += nnz - 1;
    if (!deferring(ctx)) return cn_defer_flush(ctx);
    return 0;
}

// ---- the deferrable forms of the per-ciphertext entry points (arguments are checked now, the work is queued)
int defer_addsub(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count, int op) {
    GETCT(A, a, 0); GETCT(O, out, A->size);
    Buffer *B = getbuf(ctx, b, 0);
    if (!B || B->size != A->size) return fail(CN_ERR_ARG, "operand sizes do not match");
    if (!range_ok(A, ai, count) || !range_ok(O, oi, count) || !range_ok(B, bi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (A->size != 2) return 1;
    for (uint32_t c = 0; c < count; c++) {
        const uint64_t *pa = A->d + (size_t)(ai + c) * A->item_words, *pb = B->d + (size_t)(bi + c) * B->item_words;
        CHECK(defer_push(ctx, DOp{op ? DOP_SUB : DOP_ADD, 0, O->d + (size_t)(oi + c) * O->item_words, pa, pb, 0, 0, nullptr}));
    }
    if (op) ctx->st.Subtraction += count; else ctx->st.Addition += count;
    return 0;
}
int defer_add_plain(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, int subtract, cn_handle out, uint32_t oi, uint32_t count) {
    GETCT(A, a, 0); GETCT(O, out, A->size); GETPT(P, pt);
    if (!range_ok(A, ai, count) || !range_ok(O, oi, count) || !range_ok(P, pi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (A->size != 2) return 1;
    for (uint32_t c = 0; c < count; c++) {
        const uint64_t *pa = A->d + (size_t)(ai + c) * A->item_words;
        CHECK(defer_push(ctx, DOp{subtract ? DOP_SUBPLAIN : DOP_ADDPLAIN, 0, O->d + (size_t)(oi + c) * O->item_words, pa, P->d + (size_t)(pi + c) * ctx->hc.n, 0, 0, nullptr}));
    }
    if (subtract) ctx->st.PlainSubtraction += count; else ctx->st.PlainAddition += count;
    return 0;
}
int defer_mul_relin(cn_ctx *ctx, cn_handle a, uint32_t ai, uint32_t astride, cn_handle b, uint32_t bi, uint32_t bstride, cn_handle out, uint32_t oi, uint32_t count) {
    GETCT(A, a, 2); GETCT(B, b, 2); GETCT(O, out, 2);
    if (!range_ok(A, ai, astride ? count : 1, astride ? astride : 1) || !range_ok(B, bi, bstride ? count : 1, bstride ? bstride : 1) || !range_ok(O, oi, count))
        return fail(CN_ERR_ARG, "index out of range");
    if (!ctx->rlk.d) return fail(CN_ERR_NOKEY, "relinearization keys not set");
    for (uint32_t c = 0; c < count; c++) {
        const uint64_t *pa = A->d + ((size_t)ai + (size_t)c * astride) * A->item_words, *pb = B->d + ((size_t)bi + (size_t)c * bstride) * B->item_words;
        CHECK(defer_push(ctx, DOp{DOP_MULRELIN, 0, O->d + (size_t)(oi + c) * O->item_words, pa, pb, 0, 0, nullptr}));
    }
    ctx->st.Relinarization += count;          // (Multiplication is counted by the batched multiply at flush time)
    return 0;
}

// ---------------------------------------------------------------- lock-free submission ("defer" = 2, cn_submit.h): the consumer side
// ready_refill (lock held): single-ciphertext arrays for the lock-free cn_ct_alloc / cn_encrypt_zero_new.  The target starts small and doubles whenever
// a caller found the ring empty since the last refill (a flush that holds the lock for a millisecond is outrun by ~1 000 allocations).
void ready_refill(cn_ctx *ctx) {
    ReadyRing &r = *ctx->ready;
    if (ctx->capturing) return;
    if (r.misses.exchange(0, std::memory_order_relaxed)) r.target = std::min<uint32_t>(r.target * 2, (uint32_t)ReadyRing::CAP / 2);
    while (r.size() < r.target) {
        cn_handle h = 0;
        if (alloc_buf(ctx, 0, 1, 2, &h)) return;                 // out of memory: the callers fall back to the locked path and see the error there
        if (!r.push(h)) { Buffer *b = ctx->bufs.find(h); (void)dev_release(ctx, b->d, b->item_words * 8); ctx->bufs.erase(h); return; }
    }
}
int ring_exec(cn_ctx *ctx, const SubRec &r) {
    switch (r.type) {
    case SUB_FREE: return free_body(ctx, r.a);
    case SUB_FREE_MANY: { cn_handle *blk = (cn_handle *)(uintptr_t)r.arg; const int rc = free_many_body(ctx, blk, r.x); free(blk); return rc; }
    case SUB_SCALAR_DOT: {
        char *blk = (char *)(uintptr_t)r.arg; const uint32_t K = r.x;
        const int rc = scalar_dot_body(ctx, (const cn_handle *)blk, r.ai ? (const uint32_t *)(blk + (size_t)K * 16) : nullptr, (const uint64_t *)(blk + (size_t)K * 8), K, r.out, r.oi);
        free(blk);
        return rc;
    }
    case SUB_ADD: return addsub_body(ctx, r.a, r.ai, r.b, r.bi, r.out, r.oi, r.count, 0);
    case SUB_SUB: return addsub_body(ctx, r.a, r.ai, r.b, r.bi, r.out, r.oi, r.count, 1);
    case SUB_ADD_PLAIN: return add_plain_body(ctx, r.a, r.ai, r.b, r.bi, (int)r.x, r.out, r.oi, r.count);
    case SUB_MUL_RELIN: return mul_relin_body(ctx, r.a, r.ai, r.x, r.b, r.bi, (uint32_t)r.arg, r.out, r.oi, r.count);
    case SUB_ENCRYPT: return encrypt_body(ctx, r.b, r.bi, r.x, r.out, r.oi, r.count, r.arg);
    case SUB_ENCRYPT_ZERO: {
        Buffer *O = ctx->bufs.find(r.out);
        if (!O || O->kind != 0 || O->size != 2) return fail(CN_ERR_ARG, "invalid ciphertext handle");
        if (!ctx->pk) return fail(CN_ERR_NOKEY, "public key not set");
        if (!cn_rr_size(ctx->hc.logn)) return fail(CN_ERR_ARG, "device encryption needs 1024 <= N <= 16384");
        return defer_encrypt(ctx, nullptr, 0, O, 0, 1, r.arg);
    }
    default: return fail(CN_ERR_ARG, "internal: submission record of type %u", r.type);
    }
}
// lock held.  Executes published records in claim order; upto = ~0: as far as they are published (an opportunistic drain stops at a slot that is claimed
// but not written yet), else every record claimed before position `upto` (waiting for a writer that was descheduled between its claim and its publication).
void ring_drain(cn_ctx *ctx, uint64_t upto) {
    SubmitRing &q = *ctx->ring;
    (void)hipSetDevice(ctx->device);
    uint64_t done = 0;
    for (;;) {
        SubRec *r = q.peek();
        if (!r) {
            if (upto == ~0ull || q.head.load(std::memory_order_relaxed) >= upto) break;
            for (int spins = 0; !(r = q.peek()); spins++) { if (spins < 256) __builtin_ia32_pause(); else sched_yield(); }
        }
        const int rc = ring_exec(ctx, *r);
        if (rc && !ctx->async_rc) { ctx->async_rc = rc; ctx->async_msg = cn_last_error(); }
        q.pop();
        done++;
    }
    if (done && ctx->defer.load(std::memory_order_relaxed) == 2) ready_refill(ctx);
}
int ring_sync(cn_ctx *ctx, bool report) {
    SubmitRing &q = *ctx->ring;
    const uint64_t t = q.tail.load(std::memory_order_acquire);
    if (q.head.load(std::memory_order_relaxed) != t) ring_drain(ctx, t);
    if (report && ctx->async_rc) {
        const int rc = ctx->async_rc; ctx->async_rc = 0;
        return fail(rc, "a call submitted without the lock (defer = 2) failed when it was executed: %s", ctx->async_msg.c_str());
    }
    return 0;
}
// producer: claim, write, publish; then drain if nobody else is (nobody waits for the lock here)
int ring_push(cn_ctx *ctx, uint32_t type, uint32_t count, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t x, uint64_t arg) {
    SubmitRing &q = *ctx->ring;
    const uint64_t pos = q.claim();
    for (int spins = 0; !q.writable(pos); spins++) {           // a full lap ahead of the consumer: help
        if (ctx->mu.try_lock()) { ring_drain(ctx, ~0ull); ctx->mu.unlock_now(); }
        else if (spins < 64) __builtin_ia32_pause(); else sched_yield();
    }
    SubRec &r = q.slot(pos);
    r.type = type; r.count = count; r.a = a; r.b = b; r.out = out; r.ai = ai; r.bi = bi; r.oi = oi; r.x = x; r.arg = arg;
    q.publish(pos);
    while (q.peek_published() && ctx->mu.try_lock()) { ring_drain(ctx, ~0ull); ctx->mu.unlock_now(); }
    return 0;
}
