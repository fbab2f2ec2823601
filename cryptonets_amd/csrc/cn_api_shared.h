// Shared internals of the translation units the host runtime of libcnhip.so is built from (round 6: cn_api.hip was one 3 200-line unit):
//   cn_api.hip     contexts, streams, options, buffers, graphs, uploads / downloads, encoder, raw transforms, timing, statistics
//   cn_eval.hip    the evaluator: linear operations, scalar GEMM plans and their launches, BEHZ multiply, key switching, rotations
//   cn_client.hip  the data owner's side on the device: keys, sampler, keygen, encrypt, decrypt, noise
//   cn_defer.hip   deferred submission of per-ciphertext calls (queue, hazards, flush) and the consumer side of the lock-free submission ring
//   cn_multi.hip   the key broadcast between contexts (RCCL)
// How a scalar GEMM is planned - weight class, kernel form, pairing and grouping of gather lists, weight tiles, the device image - is decided in cn_gemm_plan.h
// (host-only; included by the two units that plan: cn_eval.hip, and cn_defer.hip for the flush of queued scalar products).
// What a flush of the deferred queue launches - the arrays a queued call reads, admission and the layer-boundary rule, the three queue rewrites, pending squarings,
// parking, staging layout, the ordered steps - is decided in cn_defer_plan.h (host-only; the queue's types DOp and DeferQueue live there; cn_defer.hip does the device work).
// What a ciphertext product launches - tensor form, FP64 / lazy choice, squaring kernels, scratch list -, how its batches are cut into chunks under the scratch limit and
// the gates of the one-key-switch-per-output forms are decided in cn_mul_plan.h (host-only; mul_switches in cn_eval.hip builds what it reads of a context).
// What a plaintext product launches - broadcast, NTT-form, lift + product or the separate launches -, its scratch list, the SumAllSlots sequence and its one-launch chain,
// the arena of a chained row-dot batch and the kernel / composition of cn_mul_plain_sum are decided in cn_plain_plan.h (host-only; plain_switches in cn_eval.hip).
// Which arithmetic policy a modulus range takes and which ring sizes have the register-radix kernels is decided in cn_policy.h (cn_mod_range, cn_policy, cn_rr_size).
// Everything here is internal: the C ABI is include/cnhip.h.  The element-wise kernels (cn_k_elem.hip.h) have internal linkage - every unit that launches one
// carries its own copy.
#pragma once
#include "cn_runtime.h"
#include "cn_rotation.h"
#include "cn_defer_plan.h"
#include "cn_plain_plan.h"
#include <thread>
#include "cn_k_elem.hip.h"
#include <algorithm>
#include <chrono>
#include <mutex>
#include <map>
#include <unordered_map>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define fail cn_fail
struct GemmPlan; struct GemmSwitches; struct Tab2; struct RotJob; struct BcastNext; struct Slab;

static const RrOps *const rr_ops[3] = {&cn_rr_u64, &cn_rr_f64, &cn_rr_f64l};
static const KsOps *const ks_ops[3] = {&cn_ks_u64, &cn_ks_f64, &cn_ks_f64l};
inline bool rr_kernels(const cn_ctx *c, uint32_t max_logn = 14) { return !c->opt.legacy_ntt && cn_rr_size(c->hc.logn, max_logn); }   // the context runs register-radix kernels
// Small arrays (a per-ciphertext caller allocates every Ciphertext on its own: thousands of 640 KiB arrays per layer) are carved out of
// slabs - one hipMalloc per SLAB_PIECES arrays, neighbours in the address space - and only ever travel between the handles and the pool;
// the slabs themselves are released with the context.
static const size_t SLAB_MAX_ITEM = 8u << 20, SLAB_BYTES = 64u << 20;
struct Slab { char *base; size_t bytes; };
static const uint32_t DEFER_STAGED_MAX = 4;       // per-ciphertext callers: calls on up to this many ciphertexts are queued, larger ones run at once
// What the batched implementations (*_impl) work on: the entry points check handles and ranges and hand over spans, the deferred flush builds them from its staging
// pointers.  CtSpan: `count` ciphertexts from d on, one after the other (size 2 - ctx->ctw2 words each - wherever no `polys` says otherwise).  PtSpan: plaintexts of N
// coefficients from d on, `stride` plaintexts apart (0: one for every ciphertext); zero: their all-zero flags, or null when the caller has refused zero plaintexts already
struct CtSpan { uint64_t *d; uint32_t count; };
struct PtSpan { const uint64_t *d; uint32_t stride; const uint8_t *zero; bool ntt; };   // ntt: the plaintexts of an NTT-form array (Buffer::kind 4: k N words each, stride in plaintexts)
// do_galois: in / out / tmp hold `count` size-2 ciphertexts; acc, pre, next_elt / next_out: see cn_eval.hip
struct GaloisCall {
    const uint64_t *in; uint64_t elt; uint64_t *out, *tmp; uint32_t count;
    const uint64_t *acc = nullptr, *pre = nullptr; uint64_t next_elt = 0; uint64_t *next_out = nullptr;
};
// out[c] = a[c * (a_bcast ? 0 : 1)] * pt[c * stride]; a_bcast: ONE ciphertext against `count` plaintexts (row-dot batches)
// Dense MultiplyPlain in two launches (k_lift_ntt, k_mul_plain_fused); ranges were checked by the caller
// A row-dot batch whose SumAllSlots chain follows: the product kernel leaves sigma_elt(c1) of every product in `out` ([row][k][N], the chain's first scratch array) and takes
// its transformed ciphertext from `ctn` - both inside the scratch arena the caller has sized for the whole call (no ensure_scratch in between: the arena must not move)
struct BcastNext { uint64_t elt; uint64_t *out, *ctn; };
// A scalar GEMM is planned once per (gather table, weight matrix): validation, grouping of the outputs that share a gather list,
// weight tiles in the kernel's layout.  A plan can live in HBM (cn_gemm_plan_create: the weights of a layer are uploaded once, every
// inference only launches) or in the per-call scratch (cn_scalar_gemm).
struct GemmPlan : GemmLayout {               // the layout of its image (cn_policy.h), filled by gemm_plan_indices (cn_gemm_plan.h)
    uint32_t O = 0, max_in = 0;
    bool has_bias = false;
    cn_handle bias_pt = 0; uint32_t bias_count = 0;
    uint64_t nnz = 0;                        // non-zero, non-padded terms (statistics)
    std::vector<char> host;                  // the image until it is uploaded
    char *dev = nullptr;                     // persistent plans: device copy of `host`
};
// ---- deferred squarings that feed the next dense layer (cn_set_option "defer_square_gemm", cn_defer.hip).  A layer-boundary flush runs only the Multiply half of the
// squarings it launches: the size-3 products stay in `arr` ([slot][3][k][N], owned by the context, grown on demand and never while a graph is alive), the callers'
// output arrays are not written, `slot` remembers output array -> slot.  The next flush either runs the scalar products that read them in cn_square_gemm's second half
// (GEMM over components 0 and 1, digit GEMM, one KsDigits key switch per OUTPUT) or relinearises every product into its own array first and goes on as ever.
// SgPlan: the plan of one such dense layer, built once and found again by memcmp - the rows sorted by their weights and the slots renumbered in order of first
// appearance, so that the order in which the caller's threads issued the calls does not change the key; the tables that hold slots, biases and output addresses
// are made per flush (idx / oidx: the plan's gather rows and output members on the host).
struct SgPlan {
    bool ok = false, bias = false; uint32_t O = 0, K = 0;
    std::vector<uint64_t> W; std::vector<int32_t> cidx;      // the key: weights [O][K], renumbered slots [O][K] (-1: padded tap)
    GemmPlan P; std::vector<int32_t> idx, oidx;              // P.dev: weights on the device; idx [G][Kp], oidx [G][M]
    uint64_t used = 0;
};
struct DeferSquare {
    uint64_t *arr = nullptr; size_t cap = 0;                 // bytes
    std::vector<uint64_t *> out;                             // slot -> the output array its product is relinearised into
    std::unordered_map<const uint64_t *, uint32_t> slot;
    std::vector<std::unique_ptr<SgPlan>> plans; uint64_t tick = 0;
};
static const size_t DEFER_SQ_PLANS = 8;
// ---- rotations of n ciphertexts by n DIFFERENT step counts as one launch chain (cn_rotate_rows_many; the queued RotateRows calls of one level).
// A single-image network rotates the 13 masked vectors of an Interleave by 13 different amounts, the 5 maps of a Vectorize by 5: one rotation
// is 2 dependent dispatches per hop, and dependent dispatches are what the latency of such a chain is made of.  The hops of a
// rotation (the element of its step count if the key exists, else its NAF terms - the plan of cn_rotation.h that every rotation walks, so the words are the
// same) are taken in rounds: round r is ONE two-launch key switch over every ciphertext that has an r-th hop, each with its own key and element
// from a table (KsItem); round 0 reads the source and writes the destination, later rounds work on the destination in place.
struct Tab2 { const NTT_GLOBAL uint64_t *src; NTT_GLOBAL uint64_t *dst; };          // one (source, destination) pair of k_copy_tab
struct RotJob { const uint64_t *src; uint64_t *dst; int steps; CnRotPlan plan; };

// ---- functions defined in one unit and used by the others
int cn_run_ntt(cn_ctx *c, uint64_t *data, uint32_t limbs, uint32_t base_off, uint32_t nmod, int inverse);
const NoiseTab &cn_noise_table();          // thresholds of the noise sampler (cn_client.hip)
std::vector<Slab> &slabs_of(cn_ctx *ctx);
bool in_slab(cn_ctx *ctx, const void *p);
int use(cn_ctx *c);
int ensure_scratch(cn_ctx *c, size_t bytes);
size_t al(size_t b);
char *pin_block(cn_ctx *c, size_t bytes);
int upload_bytes(cn_ctx *c, const void *host, size_t bytes, void *dev);
int place_table(cn_ctx *c, const void *host, size_t bytes, void *fallback, const void **dev);
Buffer *getbuf(cn_ctx *c, cn_handle h, int kind);
int range_ok(const Buffer *b, uint32_t first, uint32_t count, uint32_t stride = 1);
bool streams_share_a_queue(hipStream_t a, hipStream_t b);
int pick_stream(cn_ctx *c);
int ctx_init(cn_ctx *c, uint32_t n, uint32_t k, int device, std::vector<uint64_t> &tw);
void ctx_teardown(cn_ctx *ctx);
bool keys_as_f64(const cn_ctx *ctx);
int set_key(cn_ctx *ctx, KsKey &slot, const uint64_t *words, size_t count, size_t expect, int is_dev, bool coeff_form = false);
void pool_flush(cn_ctx *ctx);
int dev_alloc(cn_ctx *ctx, size_t bytes, uint64_t **out);
int dev_release(cn_ctx *ctx, uint64_t *p, size_t bytes);
int alloc_buf(cn_ctx *ctx, int kind, uint32_t count, uint32_t size, cn_handle *out);
bool submit_async(const cn_ctx *ctx);
int free_body(cn_ctx *ctx, cn_handle h);
int free_many_body(cn_ctx *ctx, const cn_handle *h, uint32_t n);
int free_graph(cn_ctx *ctx, Buffer &b);
void end_recording(cn_ctx *root);
int ensure_index_map(cn_ctx *ctx);
int addsub(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count, int op);
int addsub_body(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count, int op);
int add_plain_body(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, int subtract, cn_handle out, uint32_t oi, uint32_t count);
bool shifted_overlap(const uint64_t *a, const uint64_t *o, size_t words);
PlainSwitches plain_switches(const cn_ctx *ctx);           // (cn_plain_plan.h)
int pt_to_ntt(cn_ctx *ctx, const uint64_t *src, uint32_t count, uint64_t *dst);      // dst[i] = NTT form ([k][N]) of the coefficient-form plaintext src + i N
int mul_plain_impl(cn_ctx *ctx, CtSpan A, bool a_bcast, PtSpan P, CtSpan O, uint32_t polys, const BcastNext *nx = nullptr);
GemmSwitches gemm_switches(const cn_ctx *ctx);           // (cn_gemm_plan.h)
int free_gemm_plan(cn_ctx *ctx, Buffer &b);
int build_gemm_plan(cn_ctx *ctx, const int32_t *idx, const uint64_t *W, uint32_t O, uint32_t K, Buffer *BP, cn_handle bias_pt, const int32_t *bias_idx, GemmPlan &P);
int run_gemm_plan(cn_ctx *ctx, const GemmPlan &P, const char *tables, Buffer *I, Buffer *OB, uint32_t oi, const uint64_t *in3 = nullptr);
// the launch of a planned layout whose image is at `tables` (operands by name: GemmLaunch, cn_runtime.h) and the kernel family it goes to
inline GemmLaunch gemm_launch(const cn_ctx *ctx, const GemmLayout &L, const char *tables) { return GemmLaunch::of(L, tables, (uint32_t)ctx->opt.gemm_order); }
inline int run_gemm_launch(cn_ctx *ctx, const GemmLayout &L, const GemmLaunch &gl) { return L.mfma ? cn_l_gemm_mfma(ctx, gl) : cn_l_gemm(ctx, gl); }
MulSwitches mul_switches(const cn_ctx *ctx);               // (cn_mul_plan.h)
bool aux_stream_ready(cn_ctx *ctx);
// "sq_halves": Multiply + Relinearize of a batch software-pipelined in parts over the context's two streams (round 6): part i on stream i % 2, its Multiply behind the Multiply
// of the part before it (event), its key switch behind its own Multiply (stream order) - [mul 0][ks 0 | mul 1][ks 1 | mul 2][ks 2]: the HBM-bound base extension / floor and
// the transform kernels of a Multiply fill what the FP64-bound key switch of the part before leaves.  The context's stream continues behind the last part of either stream.
// Three parts of 30 / 40 / 30 % measured best for the CryptoNets batch (profiles/r06_mulrelin_parts.txt: plain loop of the two primes 12.6 -> 12.0-12.2 ms, the half-batch
// stagger of the primes 12.2-12.6; two parts 12.4-12.5, four 12.7, five 12.4).
// mul(first, count), ks(first, count) launch on ctx->stream.  When a batch takes it, and its cuts: mul_pipeline_parts, pipeline_cuts (cn_mul_plan.h)
template <class FM, class FK> static int pipelined_halves(cn_ctx *ctx, uint32_t c, FM mul, FK ks) {
    uint32_t first[4];
    const uint32_t P = pipeline_cuts(c, first);
    if (P < 2) { CHECK(mul(0u, c)); return ks(0u, c); }
    ctx->cnt.mr_pipelined++;
    int rc = 0;
    for (uint32_t i = 0; i < P && !rc; i++) {
        const bool aux = (i & 1) != 0;
        if (i) {                                                      // this part's Multiply behind the previous part's (recorded on the other stream)
            if (hipStreamWaitEvent(aux ? ctx->stream2 : ctx->stream, ctx->ev_fork, 0) != hipSuccess) { rc = fail(CN_ERR_HIP, "hipStreamWaitEvent failed"); break; }
        }
        if (aux) std::swap(ctx->stream, ctx->stream2);
        rc = mul(first[i], first[i + 1] - first[i]);
        if (!rc && i + 1 < P && hipEventRecord(ctx->ev_fork, ctx->stream) != hipSuccess) rc = fail(CN_ERR_HIP, "hipEventRecord failed");
        if (!rc) rc = ks(first[i], first[i + 1] - first[i]);
        if (!rc && aux && i + 2 >= P && hipEventRecord(ctx->ev_join, ctx->stream) != hipSuccess) rc = fail(CN_ERR_HIP, "hipEventRecord failed");      // the last part on the second stream
        if (aux) std::swap(ctx->stream, ctx->stream2);
    }
    if (rc) {                                                         // work may be queued on the second stream: the context's stream still waits for it, so that
        if (hipEventRecord(ctx->ev_join, ctx->stream2) == hipSuccess) (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);   // the next call cannot reuse scratch under it
        return rc;
    }
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    return 0;
}
// keep (cn_square_gemm's pre-floor form, squarings on the fused kernels): the tensor words stay in the caller's arrays dq / db [cnt][3][k | kb][N] - components 0 and 1
// of db in NTT form (MulBase::ntt01) - and only component 2 is floored into out3
struct MulKeep { uint64_t *dq, *db; };
int do_multiply(cn_ctx *ctx, const uint64_t *a, uint32_t astride, const uint64_t *b, uint32_t bstride, uint64_t *out3, uint32_t cnt, const uint64_t *const *atab = nullptr, const uint64_t *const *btab = nullptr,
                const MulKeep *keep = nullptr);
int ensure_ks_part(cn_ctx *ctx, size_t need);
KsSwitches ks_switches(const cn_ctx *ctx);
KsPlan ks_plan(const cn_ctx *ctx, const KsKey &key, uint32_t cnt, int galois);
int do_keyswitch(cn_ctx *ctx, const KsKey &key, const KsCall &call);
// Multiply + Relinearize of a batch (run_mul_relin, cn_eval.hip).  Operand i: a + i * astride ciphertexts (stride 0: one for all), or the i-th address of a host list
// (hb == ha: squarings); result i: out + i ciphertexts, or the i-th address of a host list.  The lists reach the device per chunk
struct MulRelinCall {
    const uint64_t *a = nullptr, *b = nullptr; uint32_t astride = 0, bstride = 0;
    const uint64_t *const *ha = nullptr, *const *hb = nullptr;
    uint64_t *out = nullptr; uint64_t *const *ho = nullptr;
};
int run_mul_relin(cn_ctx *ctx, const MulRelinCall &m, uint32_t count, MulSite site, int sq_halves_min);
int mul_relin_body(cn_ctx *ctx, cn_handle a, uint32_t ai, uint32_t astride, cn_handle b, uint32_t bi, uint32_t bstride, cn_handle out, uint32_t oi, uint32_t count);
const KsKey *galois_key(cn_ctx *ctx, uint64_t elt);          // null: not present
int do_galois(cn_ctx *ctx, const GaloisCall &g);
int galois_impl(cn_ctx *ctx, CtSpan in, uint64_t elt, CtSpan acc, CtSpan out);
int plan_rotation(cn_ctx *ctx, int steps, CnRotPlan *plan = nullptr);      // null: the check alone
int rotate_rows_impl(cn_ctx *ctx, CtSpan in, int steps, CtSpan out);
int rotate_jobs(cn_ctx *ctx, std::vector<RotJob> &jobs);
int rotate_rows_add_impl(cn_ctx *ctx, CtSpan in, int steps, CtSpan acc, CtSpan out);
int sum_slots_impl(cn_ctx *ctx, CtSpan h, uint32_t length, const RowdotPlan *ready = nullptr);
int set_plain_key(cn_ctx *ctx, uint64_t **slot, const uint64_t *words, size_t count, size_t expect, bool is_dev = false, bool coeff_form = false);
RngKey rng_key_of(const cn_ctx *ctx);
int sample_poly(cn_ctx *ctx, uint64_t *dst, uint32_t polys, int kind, uint64_t seed, uint64_t stream);
int gen_ksk(cn_ctx *ctx, const uint64_t *snew, int dbc, const uint32_t *dig, uint32_t tot, uint64_t seed, uint64_t *key, uint64_t *e);
int adopt_ksk(cn_ctx *ctx, KsKey &slot, uint64_t *dev, size_t words);
int encrypt_chain(cn_ctx *ctx, uint32_t cnt, const uint64_t *ptd, uint32_t pt_stride_words, uint64_t *out, uint64_t seed, const EncTab *htab, bool in_arena = false);
size_t encrypt_scratch_bytes(const cn_ctx *ctx, uint32_t cnt, bool tab);
int encrypt_body(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t pt_stride, cn_handle out, uint32_t oi, uint32_t count, uint64_t seed);
int decrypt_phase(cn_ctx *ctx, Buffer *I, uint32_t ci, uint32_t count, uint64_t *&acc, size_t extra = 0);
DeferQueue *cn_defer_new();
void cn_defer_delete(DeferQueue *q);
bool cn_defer_pending(cn_ctx *ctx);
DeferSwitches defer_switches(cn_ctx *ctx);                   // (cn_defer_plan.h; null: the environment switches alone)
int defer_push(cn_ctx *ctx, DOp op);
int flush_gemm_group(cn_ctx *ctx, DeferQueue *q, const std::vector<const DOp *> &ops, uint32_t K, const DeferSwitches &sw);
int flush_elementwise_group(cn_ctx *ctx, const std::vector<const DOp *> &ops, int type);
int flush_mulrelin_group(cn_ctx *ctx, const std::vector<const DOp *> &ops, bool sq);
int ensure_stage(cn_ctx *ctx, size_t bytes);
int copy_by_table(cn_ctx *ctx, const std::vector<Tab2> &tab, Tab2 *dtab, uint32_t words_per_item);
int flush_staged_group(cn_ctx *ctx, const DeferStep &step, const DeferSwitches &sw);
int defer_staged(cn_ctx *ctx, int type, CtSpan a, CtSpan b, CtSpan o, int64_t arg, const uint64_t *plain = nullptr, uint32_t pstride_words = 0);
int flush_encrypt_group(cn_ctx *ctx, const std::vector<const DOp *> &ops);
bool zero_fold_ok(cn_ctx *ctx);
int flush_zero_folds(cn_ctx *ctx, DeferQueue *q, const std::vector<const DOp *> &gemms);
int defer_encrypt(cn_ctx *ctx, const uint64_t *ptd, uint32_t pt_stride_words, Buffer *O, uint32_t oi, uint32_t count, uint64_t seed);
int cn_defer_flush(cn_ctx *ctx, bool boundary = false);      // boundary: the layer-boundary trigger of defer_push; every other flush is a demand flush
void defer_square_drop_plans(cn_ctx *ctx);                   // the cached plans of deferred square + dense layers (changes of the switches build_gemm_plan reads)
void defer_square_release(cn_ctx *ctx);                      // ... and the product array (ctx_teardown)
bool deferring(cn_ctx *ctx);
// per-ciphertext callers: does a staged call (cn_mul_plain, the rotations) on `count` ciphertexts join the queue?  Larger ones run at once
static inline bool queues(cn_ctx *ctx, uint32_t count) { return deferring(ctx) && count && count <= DEFER_STAGED_MAX; }
int scalar_dot_body(cn_ctx *ctx, const cn_handle *in, const uint32_t *in_idx, const uint64_t *w, uint32_t K, cn_handle out, uint32_t oi);
int defer_addsub(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count, int op);
int defer_add_plain(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, int subtract, cn_handle out, uint32_t oi, uint32_t count);
int defer_mul_relin(cn_ctx *ctx, cn_handle a, uint32_t ai, uint32_t astride, cn_handle b, uint32_t bi, uint32_t bstride, cn_handle out, uint32_t oi, uint32_t count);
void ready_refill(cn_ctx *ctx);
int ring_exec(cn_ctx *ctx, const SubRec &r);
void ring_drain(cn_ctx *ctx, uint64_t upto);
int ring_sync(cn_ctx *ctx, bool report);
int ring_push(cn_ctx *ctx, uint32_t type, uint32_t count, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t x, uint64_t arg);
int raw_ntt(cn_ctx *ctx, void *p, uint32_t limbs, int base, int inverse);

// cn_set_option("record_steps", 1): the steps / column rotations a caller asks for, noted by the entry points before any NAF split (cn_rotation_steps)
static inline void rec_rows(cn_ctx *ctx, int steps) { if (ctx->rec_steps && steps) ctx->rec_set.insert(steps); }
static inline void rec_columns(cn_ctx *ctx) { if (ctx->rec_steps) ctx->rec_cols = true; }
static inline void rec_sum_slots(cn_ctx *ctx, uint32_t length) {          // the chain of sum_slots_impl
    if (!ctx->rec_steps) return;
    const SumSlotsSeq seq = sum_slots_seq(ctx->hc.n, length);
    if (seq.columns) ctx->rec_cols = true;
    for (uint32_t i = 0; i < seq.rows; i++) ctx->rec_set.insert(-(int)(1u << i));
}
static inline void rec_galois(cn_ctx *ctx, uint64_t elt) {                // cn_apply_galois: 2N - 1 = the column swap, 3^s = RotateRows(s)
    if (!ctx->rec_steps) return;
    const uint64_t n = ctx->hc.n, m = 2 * n;
    if (elt == m - 1) { ctx->rec_cols = true; return; }
    uint64_t e = 1;
    for (uint64_t s2 = 1; s2 < n / 2; s2++) { e = (e * 3) & (m - 1); if (e == elt) { ctx->rec_set.insert(s2 <= n / 4 ? (int)s2 : (int)s2 - (int)(n / 2)); return; } }
}

// the chunks of a planned batch (mul_batch, cn_mul_plan.h), body(first, c) for each.  own_arena: every chunk sizes the scratch arena for itself (ensure_scratch rewinds
// it); else the caller has sized it and every chunk's scratch starts where the caller's ends
template <class F> static int mul_chunks(cn_ctx *ctx, const MulBatch &B, uint32_t count, bool own_arena, F body) {
    const size_t mark = ctx->soff;
    for (uint32_t s = 0; s < count; s += B.chunk) {
        const uint32_t c = std::min(B.chunk, count - s);
        if (own_arena) CHECK(ensure_scratch(ctx, B.ensure(c))); else ctx->soff = mark;
        CHECK(body(s, c));
    }
    return 0;
}

#define GETCT(var, h, sz) Buffer *var = getbuf(ctx, h, 0); if (!var) return fail(CN_ERR_ARG, "invalid ciphertext handle " #h); \
    if ((sz) && var->size != (uint32_t)(sz)) return fail(CN_ERR_ARG, "ciphertext size mismatch for " #h)
#define GETPT(var, h) Buffer *var = getbuf(ctx, h, 1); if (!var) return fail(CN_ERR_ARG, "invalid plaintext handle " #h)
// the operand of a plaintext product (cn_mul_plain, cn_rowdot_batch, cn_mul_plain_sum): a coefficient-form array or an NTT-form one (cn_pt_transform)
#define GETPT_OR_PTN(var, h) Buffer *var = getbuf(ctx, h, 1); if (!var) var = getbuf(ctx, h, 4); if (!var) return fail(CN_ERR_ARG, "invalid plaintext handle " #h)
#define GETPTN(var, h) Buffer *var = getbuf(ctx, h, 4); if (!var) return fail(CN_ERR_ARG, "invalid NTT-form plaintext handle " #h)
#define SPAN(var, b, first, count) if (!range_ok(b, first, count)) return fail(CN_ERR_ARG, "index out of range"); \
    const CtSpan var{b->d + (size_t)(first) * b->item_words, count}
#define PTSPAN(var, b, first, count, stride) if (!range_ok(b, first, (stride) ? count : 1, (stride) ? (stride) : 1)) return fail(CN_ERR_ARG, "index out of range"); \
    const PtSpan var{b->d + (size_t)(first) * b->item_words, stride, b->pt_zero.data() + (first), b->kind == 4}
#define LOCK_ONLY CHECK(use(ctx)); CHECK(ring_sync(ctx, false))
#define API_BODY return ctx->mu.run([&]() -> int {
#define API_END });
#define LOCK CHECK(use(ctx)); CHECK(ring_sync(ctx, true)); CHECK(cn_defer_flush(ctx))

#define launch_count cn_launch_count
#define NOT_CAPTURING(what) do { if (ctx->capturing) return fail(CN_ERR_ARG, what " is not possible while a graph is recorded (cn_graph_begin .. cn_graph_end)"); } while (0)
// a level context (cn_ctx_create_level) gets its keys from its parent only (SEAL 3.2 generates keys at the first level only)
#define NOT_LEVEL(what) do { if (ctx->level) return fail(CN_ERR_ARG, what " is not possible on a level context (its keys are its parent's, sliced)"); } while (0)
// the BEHZ multiply and the key switch are not run on one coefficient modulus (include/cnhip.h: cn_ctx_create_level)
#define TWO_LIMBS(what) do { if (ctx->hc.k < 2) return fail(CN_ERR_ARG, what " needs at least 2 coefficient moduli (a 1-limb context runs the linear operations, encryption and decryption)"); } while (0)
#define DISPATCH_K2(fn, ...) switch (ctx->hc.k) { \
    case 1: fn<1>(__VA_ARGS__); break; case 2: fn<2>(__VA_ARGS__); break; case 3: fn<3>(__VA_ARGS__); break; case 4: fn<4>(__VA_ARGS__); break; \
    case 5: fn<5>(__VA_ARGS__); break; case 6: fn<6>(__VA_ARGS__); break; case 7: fn<7>(__VA_ARGS__); break; case 8: fn<8>(__VA_ARGS__); break; \
    case 9: fn<9>(__VA_ARGS__); break; default: return fail(CN_ERR_ARG, "at most 9 coefficient moduli"); }

// The context locks one call holds besides its own (cn_mod_switch, the recordings across levels): taken in the given order and noted per thread, so that
// a graph released from inside such a call (a release executed from the lock-free ring) hands its members' arrays back without taking a lock twice.
struct HeldLocks {
    explicit HeldLocks(const std::vector<cn_ctx *> &ctxs);
    ~HeldLocks();
    static bool here(const cn_ctx *c);         // does this thread hold c's lock through a HeldLocks?
    HeldLocks(const HeldLocks &) = delete;
    HeldLocks &operator=(const HeldLocks &) = delete;
private:
    std::vector<std::unique_ptr<CnGuard>> g;
};
int flush_all(cn_ctx *ctx);

template <class T> static T *salloc(cn_ctx *c, size_t count) {
    size_t b = al(count * sizeof(T));
    if (c->soff + b > c->scap) return nullptr;
    T *p = (T *)(c->scratch + c->soff); c->soff += b; return p;
}
template <class T> static int upload_tmp(cn_ctx *c, const T *host, size_t count, T **dev) {
    *dev = salloc<T>(c, count);
    if (!*dev) return fail(CN_ERR_HIP, "internal: scratch exhausted");
    return upload_bytes(c, host, count * sizeof(T), *dev);
}

template <class K> static int big_lds(K kern, size_t bytes) {
    HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
template <int EPT> static int set_ks_attr(size_t bytes) {
    HIPCHK(hipFuncSetAttribute((const void *)k_keyswitch<EPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}
