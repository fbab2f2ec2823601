// Host-side structures of libcnhip.so shared by the runtime units (cn_api.hip, cn_eval.hip, cn_client.hip, cn_defer.hip, cn_multi.hip: cn_api_shared.h) and the kernel-launch translation units
// (cn_l_*.hip).  The library is built from several translation units so that hipcc compiles the kernel families in parallel: the
// register-radix kernels alone are ~180 instantiations (5 transform sizes x 3 arithmetic policies x 12 kernels).
#pragma once
#include "../../include/cnhip.h"
#include "cn_policy.h"
#include "cn_options.h"
#include "cn_ks_plan.h"
#include "cn_mul_plan.h"
#include "cn_submit.h"
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

int cn_fail(int code, const char *fmt, ...);       // sets the thread-local message of cn_last_error(), returns `code`
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return cn_fail(CN_ERR_HIP, "%s failed: %s", #x, hipGetErrorString(e_)); } while (0)
#define CHECK(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)

struct GemmPlan;
// A captured operation sequence (cn_graph_begin / cn_graph_end): the instantiated HIP graph, the host blocks its upload nodes read at
// every launch, and the device arrays that were handed out while it was recorded and are not owned by a live handle - they stay
// reserved for the graph (its kernels carry their addresses), out of the pool, until the graph is freed.
// A graph recorded across levels (cn_graph_begin_levels) also carries, per member context, the arrays reserved out of that member's pool.
struct cn_ctx;
struct CapturedGraph {
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    std::vector<std::unique_ptr<char[]>> staged;
    std::vector<std::pair<uint64_t *, size_t>> reserved;
    struct Member { cn_ctx *ctx; std::vector<std::pair<uint64_t *, size_t>> reserved; };
    std::vector<Member> members;           // in lock order (more limbs first); empty for cn_graph_begin
};
struct Buffer {
    int kind;                 // 0 = ciphertext array, 1 = dense plaintext array, 2 = scalar GEMM plan, 3 = captured graph, 4 = NTT-form plaintext array [pt][k][N]
    std::shared_ptr<GemmPlan> plan;
    std::shared_ptr<CapturedGraph> cg;
    uint32_t count, size;     // size = polys per ciphertext
    uint64_t *d;
    size_t item_words;
    std::vector<uint8_t> pt_zero;   // per plaintext: all coefficients zero?
};
// Handle table: a handle is (generation << 32) | (slot + 1) - looked up by indexing, not hashing (a dense-layer call of the unchanged
// caller names 845 input handles), stale handles are recognised by their generation.
class HandleTable {
    struct Slot { Buffer b; uint32_t gen = 0; bool live = false; };
    std::vector<Slot> slots;
    std::vector<uint32_t> free_;
    size_t live_ = 0;
public:
    Buffer *find(cn_handle h) {
        const uint32_t s = (uint32_t)h - 1u;
        if ((uint32_t)h == 0 || s >= slots.size() || !slots[s].live || slots[s].gen != (uint32_t)(h >> 32)) return nullptr;
        return &slots[s].b;
    }
    cn_handle insert(Buffer &&b) {
        uint32_t s;
        if (!free_.empty()) { s = free_.back(); free_.pop_back(); } else { s = (uint32_t)slots.size(); slots.emplace_back(); }
        slots[s].b = std::move(b); slots[s].live = true; slots[s].gen = (slots[s].gen + 1) & 0x7fffffffu;
        live_++;
        return ((cn_handle)slots[s].gen << 32) | (cn_handle)(s + 1);
    }
    void erase(cn_handle h) {
        const uint32_t s = (uint32_t)h - 1u;
        slots[s].live = false; slots[s].b = Buffer(); free_.push_back(s); live_--;
    }
    size_t size() const { return live_; }
    template <class F> void for_each(F f) { for (Slot &s : slots) if (s.live) f(s.b); }
};
struct KsKey { uint64_t *d; bool owned; bool f64; };   // f64: words converted to doubles for the FP64 key-switch kernel

// The contexts are called from Defaults.ThreadCount threads at once (HE Wrapper/Utils.cs:46-88) and the critical sections are a few
// hundred nanoseconds of bookkeeping (handle table, deferred-operation queue): a futex mutex hands every contended acquisition through
// the kernel, so waiters spin (and yield when the wait gets long).
// Spin lock (cn_host.cpp): the critical sections are short, waiters spin briefly and then yield.
// A request published by a thread that found the lock held: the holder executes it (combining) and reports back through it.
struct CnReq {
    int (*fn)(void *) = nullptr; void *arg = nullptr; int rc = 0;
    std::atomic<int> done{0}, asleep{0};
    CnReq *next = nullptr;
    char err[256];
};
class CnMutex {
public:
    struct Node {};           // (per-acquisition state of a queue lock; the current lock needs none)
    void lock(Node &n);
    void unlock(Node &n);
    // Run f() under the lock.  Default: plain acquisition.  With CN_LOCK_COMBINE=1 (an experiment that is kept switchable, measured slower -
    // cn_host.cpp): on this thread when the lock is free - and then ALSO every request other threads published meanwhile - or, when it is
    // held, on the holder's thread (the request is published, this thread waits for its completion), so that the few cache lines every call
    // works on (queue tails, hazard table, handle table, counters) stay in one core's cache.  f must not call into the same context again.
    template <class F> int run(F &&f) {
        if (!combining()) { Node n; lock(n); const int rc = f(); unlock(n); return rc; }
        if (try_take_me()) { const int rc = f(); serve(); release(); return rc; }
        typedef typename std::remove_reference<F>::type Fn;
        CnReq r;
        r.fn = [](void *p) -> int { return (*static_cast<Fn *>(p))(); };
        r.arg = (void *)&f; r.err[0] = 0;
        return submit(r);
    }
    // the lock-free submission path (cn_submit.h): whoever finds the lock free drains the ring; nobody waits
    bool try_lock() { return try_take_me(); }
    void unlock_now() { release(); }
    bool is_held() const { return held.load(std::memory_order_relaxed) != 0; }
private:
    std::atomic<int> held{0};
    std::atomic<int> spinners{0};      // waiters that spin; the others sleep on wake_seq (cn_host.cpp)
    std::atomic<int> sleepers{0}, wake_seq{0};
    std::atomic<uint32_t> last_owner{0}, burst{0};   // owner bias (cn_host.cpp): who released last, how many times in a row it re-acquired
    std::atomic<uint64_t> released_at{0};            // TSC of the last release
    std::atomic<CnReq *> pending{nullptr};           // published requests (a stack; served oldest first)
    bool try_take(uint32_t me);
    bool try_take_me();
    static bool combining();
    void release();
    void serve();
    int submit(CnReq &r);
};
struct CnGuard {
    CnMutex &m; CnMutex::Node n;
    explicit CnGuard(CnMutex &m_) : m(m_) { m.lock(n); }
    ~CnGuard() { m.unlock(n); }
    CnGuard(const CnGuard &) = delete;
    CnGuard &operator=(const CnGuard &) = delete;
};

struct DeferQueue;            // cn_api_shared.h / cn_defer.hip
struct cn_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    CnTunables opt;           // every switch of cn_set_option's table (cn_options.h)
    DevConsts hc;             // host copy
    DevConsts *dc = nullptr;  // device copy
    uint64_t *tw = nullptr;
    CnMutex mu;
    HandleTable bufs;
    KsKey rlk{nullptr, false, false};
    double *twd = nullptr, *twdh = nullptr;
    std::map<uint64_t, KsKey> gk;
    uint64_t *sk = nullptr, *pk = nullptr;   // client-side keys (NTT form) when the data owner's GPU runs keygen/encrypt/decrypt
    uint64_t rng_item = 0;                    // running polynomial counter of the sampler (part of the ChaCha20 block counter)
    uint32_t rng_key[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // 256-bit ChaCha20 key of the sampler (cn_set_rng_key; cn_set_rng_salt sets the first 64 bits)
    char *scratch = nullptr; size_t scap = 0, soff = 0, smax;
    std::vector<std::unique_ptr<char[]>> staged;   // host blocks of in-flight upload_tmp copies
    cn_stats st{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_order = nullptr;     // cn_ctx_wait_for: marks a point of this context's stream another context waits for
    uint32_t bs, chunks;      // element-wise geometry
    std::vector<uint32_t> index_map;   // BatchEncoder slot -> coefficient position
    uint32_t *d_index_map = nullptr;   // the same table in HBM (cn_encode_batch / cn_decode_batch)
    size_t ctw2;              // words of a size-2 ciphertext
    // freed ciphertext / plaintext arrays are kept per size and handed out again: every op of a context is ordered on its
    // stream, so reuse needs no synchronisation, while hipFree / hipMalloc cost ~60 / ~25 us and a device-wide sync each
    // (a LoLa inference allocates and frees ~300 temporaries per plaintext prime)
    std::unordered_map<size_t, std::vector<uint64_t *>> pool;
    size_t pool_bytes = 0, pool_max;
    void *slabs = nullptr;                // std::vector<Slab>*: small arrays are carved out of slabs (one hipMalloc per <= 64 arrays), cn_api.hip
    void *ks_part = nullptr; size_t ks_part_cap = 0;   // partial products of the two-launch key switch [ct][digit][2][k][N]
    char *pin = nullptr, *pin_dev = nullptr; size_t pin_off = 0; uint32_t pin_laps = 0;           // ring of pinned host memory for the small table uploads (cn_api.hip: pin_block)
    char *stage = nullptr; size_t stage_cap = 0;       // staging arena of the deferred per-ciphertext rotations / plaintext products (gather, batched call, scatter)
    int stream_tries = 0;                        // streams created until one had a hardware queue of its own (cn_api.hip: pick_stream)
    std::atomic<int> probe_pins{0};              // > 0: a cn_ctx_create on this device is measuring this context's stream; cn_ctx_destroy waits
    std::atomic<bool> capturing{false};   // between cn_graph_begin and cn_graph_end: work is recorded on the stream, nothing that synchronises or allocates may run
    std::vector<std::unique_ptr<char[]>> cap_staged;                 // host blocks of the upload nodes recorded so far
    std::vector<std::pair<uint64_t *, size_t>> cap_allocs;           // arrays handed out while recording
    int graphs_alive = 0;     // graphs carry the addresses of the scratch arenas: those must not move while one exists (also the graphs of a root this context is a member of)
    // recording across levels (cn_graph_begin_levels): the root records on its stream and every member's work goes onto it.  cap_root: the root of
    // the recording this context takes part in (the root itself included), null otherwise; cap_members: the root's members, in lock order;
    // own_stream: a member's stream, put back at cn_graph_end; member_graphs: live graphs of other contexts that hold this one (cn_ctx_destroy refuses);
    // ev_graph: marks a point of this context's stream a replay (or the members behind it) waits for
    cn_ctx *cap_root = nullptr;
    std::vector<cn_ctx *> cap_members;
    hipStream_t own_stream = nullptr;
    int member_graphs = 0;
    hipEvent_t ev_graph = nullptr;
    int cus = 0;              // compute units of the device
    CnCounters cnt;           // what cn_get_option reads back by the names of kCounters (cn_options.h)
    std::atomic<uint64_t> packed_bad{0};       // packed uploads whose rows held a residue >= its modulus (counted where the flag is read)
    uint64_t ks_hoisted = 0;   // calls of cn_rotate_rows_hoisted / cn_apply_galois_hoisted that launched ("ks_hoisted")
    uint64_t ks_summed = 0;    // calls of cn_rotate_rows_sum / cn_apply_galois_sum that launched the fused form ("ks_summed")
    uint32_t ms_groups = 0;    // output groups of the last cn_mul_relin_sum call ("mul_sum_groups"; 0: it took the literal sequence)
    uint64_t uid = 0;         // creation order within the process (cn_ctx_create)
    hipStream_t stream2 = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; bool stream2_failed = false;   // second stream of pipelined_halves (aux_stream_ready)
    // deferred submission (cn_set_option("defer", 1)): per-ciphertext calls are queued and flushed as batched launches; 2: ... and submitted without the
    // context lock through `ring` (cn_submit.h), executed by whoever drains it
    std::atomic<int> defer{0};
    DeferQueue *dq = nullptr;
    SubmitRing *ring = nullptr;
    ReadyRing *ready = nullptr;
    int async_rc = 0; std::string async_msg;        // first error of a record executed from the ring: reported by the next synchronising call
    // modulus switching (cn_level.hip): a level context (cn_ctx_create_level) holds keys sliced from its parent's and refuses key generation and key
    // uploads; ev_ms marks the point of this context's stream the other context of a cn_mod_switch waits for; ms_f64: the last cn_mod_switch
    // this context took part in ran the exact-FP64 kernel (cn_get_option "mod_switch_f64")
    bool level = false;
    // cn_set_option("record_steps", 1): the RotateRows steps the caller asked for (before the NAF split) and whether a column rotation was asked for (cn_rotation_steps)
    bool rec_steps = false, rec_cols = false;
    std::set<int> rec_set;
    hipEvent_t ev_ms = nullptr;
    bool ms_f64 = false;
};

// ---------------------------------------------------------------- kernel launchers (cn_l_*.hip); the tables of RrOps / KsOps are indexed by cn_policy (cn_policy.h)
// One key switch of `cnt` ciphertexts: out[ct] = (add0[ct], add1[ct]) + KeySwitch(target[ct]) (+ extra[ct] - the fused accumulator of
// the cn_*_add entry points).  target / add0 / add1 / extra are strided per ciphertext (in words); out is dense size-2, or - out_tab -
// one address per ciphertext (deferred per-ciphertext calls whose results live in separate arrays).
// per-ciphertext operands of a two-launch key switch that rotates every ciphertext by its own step count (cn_rotate_rows_many): the ciphertext it reads
// (c0 at in, c1 behind it), the Galois key of its element, the element
struct KsItem { const uint64_t *in; const void *key; uint32_t elt, pad; };
// KsCall: the operands a caller of do_keyswitch names - by designated initialisers or through the constructors of the three shapes that occur; do_keyswitch
// adds the rest of KsArgs (key words, the plan of cn_ks_plan.h) and the launchers read both parts
struct KsCall {
    const uint64_t *target = nullptr; size_t tstride = 0;
    const uint64_t *add0 = nullptr, *add1 = nullptr; size_t astride = 0;
    uint64_t *out = nullptr; uint32_t cnt = 0; int galois = 0;
    const uint64_t *extra = nullptr; size_t xstride = 0;
    uint64_t *const *out_tab = nullptr;
    const KsItem *items = nullptr;   // two-launch variants: per-ciphertext (operand, key, element) table instead of target / add0 / key / perm_elt
    uint32_t perm_elt = 0;    // two-launch variants: Galois element of a rotation whose automorphism the kernels apply while loading (target / add0 = the UNPERMUTED c1 / c0)
                              // k_keyswitch_pair14: target = sigma(c1) already, add0 = the UNPERMUTED c0 (permuted through LDS by the workgroup that owns the limb)
    uint32_t next_elt = 0; uint64_t *next_out = nullptr;   // k_keyswitch_pair14: the new c1 leaves a second time as sigma_next(c1) -> next_out[ct][k][N] (rotate-and-add chains)
    const void *dig = nullptr;       // register-radix kernels, FP64 policies, relinearisation: ready-made digit polynomials [cnt][rl_tot][N] (exact signed integers, |S| < q_j / 2)
                                     // instead of `target` (cn_square_gemm: the weight-combined digits of a dense layer's inputs)
    bool dig_i32 = false;            // ... stored as int32 words (|S| <= 2^31 - 1: GemmPlan::dig_i32) instead of doubles
    // The shapes (kn = k N words per polynomial): relinearise the products prod [cnt][3][kn]; relinearise from the digit polynomials S on top of the size-2
    // ciphertexts base [cnt][2][kn]; Galois switch of c1 (c1_stride apart) with c0 [cnt][2][kn] added, or of every ciphertext with its own operand, key and element
    static KsCall relin(const uint64_t *prod, size_t kn, uint32_t cnt) {
        return {.target = prod + 2 * kn, .tstride = 3 * kn, .add0 = prod, .add1 = prod + kn, .astride = 3 * kn, .cnt = cnt};
    }
    static KsCall relin_digits(const void *S, bool i32, const uint64_t *base, size_t kn, uint32_t cnt) {
        return {.add0 = base, .add1 = base + kn, .astride = 2 * kn, .cnt = cnt, .dig = S, .dig_i32 = i32};
    }
    static KsCall galois_of(const uint64_t *c1, size_t c1_stride, const uint64_t *c0, size_t kn, uint32_t cnt) {
        return {.target = c1, .tstride = c1_stride, .add0 = c0, .astride = 2 * kn, .cnt = cnt, .galois = 1};
    }
    static KsCall galois_items(const KsItem *items, uint32_t cnt) { return {.cnt = cnt, .galois = 1, .items = items}; }
    KsCall &to(uint64_t *dense) { out = dense; return *this; }                       // results: a dense size-2 array, or one address per ciphertext
    KsCall &to_table(uint64_t *const *tab) { out_tab = tab; return *this; }
    KsCall &plus(const uint64_t *acc, size_t stride) { extra = acc; xstride = stride; return *this; }      // the fused accumulator (may be null)
    KsCall &perm(uint32_t elt) { perm_elt = elt; return *this; }
    KsCall &next(uint32_t elt, uint64_t *nout) { next_elt = elt; next_out = nout; return *this; }
};
struct KsArgs : KsCall {
    const uint64_t *key;
    KsPlan plan;              // form, accmax, xcd_cts, twl, whole (cn_ks_plan.h)
};
// k_encrypt_fold (cn_k_rr.hip.h): a scalar-product output that receives the weighted sum of `count` folded zero encryptions, and the terms of all outputs
struct FoldOut { uint64_t *out; uint32_t first, count; };               // terms [first, first + count) of the term table
struct FoldTerm { double w; uint32_t enc, pad; };                       // centred weight (|w| <= t/2), index of the encryption in the samplers' int8 arrays
struct RrOps {                // register-radix kernels of one arithmetic policy; every launcher returns false when the size has no kernel
    int (*set_attrs)(uint32_t logn, size_t lds);
    bool (*ntt)(cn_ctx *c, uint64_t *data, uint32_t limbs, uint32_t base_off, uint32_t nmod, int inverse);
    bool (*intt_tensor)(cn_ctx *c, const uint64_t *A, const uint64_t *B, uint64_t *D, uint32_t cnt, uint32_t base_off, uint32_t Lm, bool lazy);   // lazy (FP64 policies): D as lazy-FP64 hand-off words
    // FP64 policies; D: lazy-FP64 hand-off words; b: the planned kernel of the base (MulBase, cn_mul_plan.h)
    bool (*square_fused)(cn_ctx *c, const uint64_t *A, size_t astride, const uint64_t *const *atab, uint64_t *D, uint32_t cnt, uint32_t base_off, uint32_t Lm, const MulBase &b);
    bool (*mul_plain_fused)(cn_ctx *c, const uint64_t *pt, uint32_t pitch, uint32_t npt, uint64_t *lift, const uint64_t *src, size_t sstride, uint32_t pstride,
                            uint64_t *out, uint32_t count, uint32_t polys);            // pt null: `lift` is the NTT form already; src null: the lift alone
    bool (*enc_tail)(cn_ctx *c, const uint64_t *u, const uint64_t *pt, uint32_t pts, uint64_t *out, uint32_t cnt, const int8_t *noise, const void *tab);   // U64, F64; tab: EncTab[cnt] or null
    bool (*enc_fused)(cn_ctx *c, const int8_t *us, const uint64_t *pt, uint32_t pts, uint64_t *out, uint32_t cnt, const int8_t *noise, const void *tab);  // all policies, N <= 8192: u (int8) -> transform -> both components in one kernel
    bool (*mul_plain_bcast)(cn_ctx *c, const uint64_t *pt, uint32_t pitch, const uint64_t *ctn, uint64_t *out, uint32_t count, uint32_t polys, uint32_t next_elt,
                            uint64_t *next_out, bool ptn);                             // ONE ciphertext (NTT form) x count plaintexts (+ sigma_next(c1) of every product on the side); ptn: NTT-form plaintexts
    bool (*enc_fold)(cn_ctx *c, const int8_t *us, const int8_t *noise, const void *fout, const void *terms, uint32_t outputs);   // FP64 policies, N <= 8192: k_encrypt_fold
};
// hoisted rotations (cn_ks_plan.h: KsHoistPlan): per rotation its Galois key, its output ciphertext and its element (the table k_ks_hoist_mac reads); the call:
// the ONE input ciphertext (c0, c1 behind it), the table on the device (the plan's blocks_mac says how many rotations it holds)
struct KsHoistItem { const void *key; uint64_t *out; uint32_t elt, pad; };
struct KsHoistArgs { const uint64_t *in; const KsHoistItem *items; KsHoistPlan plan; };
// summed rotations (cn_ks_plan.h: KsSumPlan).  Per output its ciphertext and its slice [first, first + count) of the term table, whose first `rotated` entries
// are the rotated terms; per term the ciphertext it reads (c0 at in, c1 behind it), its element (1: a plain addend) and - rotated terms - the index of its
// partial products in the arena, which is its index in the KsItem table of the term MAC
struct KsSumOut { uint64_t *out; uint32_t first, count, rotated, pad; };
struct KsSumTerm { const uint64_t *in; uint32_t elt, part; };
struct KsSumArgs { const KsItem *items; const KsSumOut *outs; const KsSumTerm *terms; KsSumPlan plan; };
struct KsOps {
    int (*set_attrs)(uint32_t logn, size_t lds);
    bool (*launch)(cn_ctx *c, const KsArgs &a);                        // the kernels of a.plan.form; false: this policy (or ring size) has no instantiation of it
    bool (*hoist)(cn_ctx *c, const KsHoistArgs &a);                    // k_ks_digit_ntt + k_ks_hoist_mac of this policy; false: no instantiation at this ring size
    bool (*sum)(cn_ctx *c, const KsSumArgs &a);                        // the term MAC of a.plan.form + k_ks_sum_terms; false: no instantiation at this ring size
};
extern const RrOps cn_rr_u64, cn_rr_f64, cn_rr_f64l;
extern const KsOps cn_ks_u64, cn_ks_f64, cn_ks_f64l;

// BEHZ element-wise steps (cn_l_behz.hip); src_tab: one source address per ciphertext instead of src + ct*stride*2kN
// f64, lazy: MulPlan::behz_f64 and MulPlan::lazy of the chain (cn_mul_plan.h) - the FP64 kernels; dq / db hold the lazy-FP64 hand-off words of an FP64 tensor kernel
int cn_l_behz_extend(cn_ctx *c, const uint64_t *src, uint32_t stride, const uint64_t *const *src_tab, uint64_t *aq, uint64_t *ab, uint32_t cnt, bool f64);
int cn_l_behz_floor(cn_ctx *c, const uint64_t *dq, const uint64_t *db, uint64_t *out, uint32_t cnt, bool f64, bool lazy);
// cn_square_gemm's pre-floor form (FP64 floor, lazy words): the floor of component 2 alone; the floor tail once per dense output (k_behz_floor_out, cn_k_behz.hip.h) -
// X [output][2][kb][N] canonical coefficients, Y [output][2][k][N] exact 64-bit sums, oidx / bidx the plan's member and bias tables of `slots` entries, bias null: none
int cn_l_behz_floor_c2(cn_ctx *c, const uint64_t *dq, const uint64_t *db, uint64_t *out, uint32_t cnt);
struct FloorOutLaunch { const uint64_t *X, *Y; const int32_t *oidx; const uint64_t *bias; const int32_t *bidx; uint64_t *out; uint32_t obase, slots; };
int cn_l_behz_floor_out(cn_ctx *c, const FloorOutLaunch &g);

// scalar GEMM (cn_l_gemm.hip).  Relative addressing: input / output ciphertext = base + index * ctw; absolute (ABS): the tables hold
// device addresses (deferred per-ciphertext calls: every ciphertext is its own array), 0 = padded tap / no output.
struct GemmLaunch {
    bool small, two, abs; uint32_t MT;
    const uint64_t *in; const void *idx; const void *W; const void *oidx; const uint64_t *bias; const void *bidx; uint64_t *out;
    uint32_t G, M, K, lazy, Kp, obase;
    uint32_t P = 0, mtiles = 0, ksteps = 0;          // matrix-core kernel: weight digit planes, 32-row output tiles, 32-term K steps
    uint32_t polys = 2;                              // ciphertext size of inputs and outputs (3: unrelinearized products)
    uint32_t order = 0;                              // workgroup order of the VALU kernels: 0 group-major, 1 slice-major (gemm_block_coords)
    bool one = false;                                // k_scalar_gemm_f64<MT, 1, 0>: the words are not split (gemm_one_limb)
    bool res = false;                                // matrix-core kernel, P = 1: the clipped + residual form (GemmLayout::res) - the <.., GemmResidual> instantiations
    uint32_t in_unit = 0, out_unit = 0, bias_unit = 0;   // words per index unit of the table-driven kernels; 0 = one ciphertext / one plaintext (plans).  Deferred calls: 32 (256 B offsets from the lowest address)
    uint32_t form = 0;                               // matrix-core kernel, the pre-floor form of cn_square_gemm: 1 = Bsk limbs (7 digits, mod b), 2 = lazy q words -> canonical y -> exact int64 sums (cn_k_gemm.hip.h)
    // the launch of a planned layout (GemmLayout, cn_policy.h) whose image is at `tables`: weights, output members and - until inputs() / bias_at() name others -
    // gather rows and bias entries at their offsets; order: the "gemm_order" option.  Then the operands by name, `unit` as in_unit / bias_unit / out_unit above
    static GemmLaunch of(const GemmLayout &L, const char *tables, uint32_t order) {
        return {.small = L.small, .two = L.two, .abs = false, .MT = L.MT, .in = nullptr, .idx = tables, .W = tables + L.off_w, .oidx = tables + L.off_oidx, .bias = nullptr,
                .bidx = tables + L.off_bidx, .out = nullptr, .G = L.G, .M = L.M, .K = L.K, .lazy = L.lazy, .Kp = L.Kp, .obase = 0, .P = L.P, .mtiles = L.mtiles, .ksteps = L.ksteps,
                .order = order, .one = L.one, .res = L.res};
    }
    GemmLaunch &inputs(const uint64_t *base, uint32_t unit, uint32_t polys_) { in = base; in_unit = unit; polys = polys_; return *this; }
    GemmLaunch &gather(const void *rows) { idx = rows; return *this; }                             // gather rows made per call (the plan's own: at `tables`)
    GemmLaunch &bias_at(const uint64_t *base, const void *entries, uint32_t unit) { bias = base; bidx = entries; bias_unit = unit; return *this; }      // base null: no bias
    GemmLaunch &outputs(uint64_t *base, uint32_t first, uint32_t unit) { out = base; obase = first; out_unit = unit; return *this; }
    // address-table form: every table entry is a device address; `any`: some input (the kernels read a valid word at padded taps); bias entries only where a call has one
    GemmLaunch &prefloor(uint32_t form_) { form = form_; bias = nullptr; return *this; }
    GemmLaunch &addresses(const uint64_t *any, bool with_bias) { abs = true; in = any; if (!with_bias) bidx = nullptr; return *this; }
};
int cn_l_gemm(cn_ctx *c, const GemmLaunch &g);
int cn_l_gemm_mfma(cn_ctx *c, const GemmLaunch &g);   // k_scalar_gemm_mfma: W = weight digit fragments, idx rows of ksteps * 32 entries
// digit GEMM of cn_square_gemm (k_digit_gemm): in = component 2 of product 0 (products in_unit words apart), S [outputs][rl_tot][N] doubles (i32: int32 words); W = signed doubles
// [G][mtiles][Kw][MT], MT = 10 or 2.  mfma (k_digit_gemm_mfma): W = the plan's weight digit fragments (pack_gemm_mfma), idx rows of ksteps * 32 entries
struct DigitGemmLaunch {
    const uint64_t *in; size_t in_unit; const void *idx; const void *W; const void *oidx; void *S;
    uint32_t G, M, K, Kp, Kw, MT;
    bool mfma = false; uint32_t P = 0, mtiles = 0, ksteps = 0;
    bool i32 = false;
    bool res = false;                                // mfma, P = 1: the clipped + residual form (GemmLayout::res)
    // the digit GEMM of a plan that has one (GemmLayout::dig): component 2 of the products at `in`, in_unit words apart, gathered through idx
    static DigitGemmLaunch of(const GemmLayout &L, const char *tables, const uint64_t *in, size_t in_unit, const void *idx, void *S) {
        return {.in = in, .in_unit = in_unit, .idx = idx, .W = tables + (L.dig_mfma ? L.off_w : L.off_dw), .oidx = tables + L.off_oidx, .S = S, .G = L.G, .M = L.M, .K = L.K,
                .Kp = L.Kp, .Kw = L.dKw, .MT = L.dMT, .mfma = L.dig_mfma, .P = L.dig_mfma ? L.P : 0, .mtiles = L.dig_mfma ? L.mtiles : 0, .ksteps = L.dig_mfma ? L.ksteps : 0,
                .i32 = L.dig_i32, .res = L.dig_mfma && L.res};
    }
};
inline uint32_t digit_gemm_mfma_group(uint32_t P) { return P <= 2 ? 3u : 2u; }     // digits per workgroup: 16 (P + 1) DG accumulator registers per wave
int cn_l_digit_gemm(cn_ctx *c, const DigitGemmLaunch &g);
// sum of unrelinearized products (cn_mul_relin_sum, k_product_sum): prod [outputs][K][3][k][N] -> components 0 and 1 summed mod q_l into out [outputs][2][k][N],
// the digit sums of component 2 into S [outputs][rl_tot][N] doubles (i32: int32 words).  Every source limb has at most PRODUCT_SUM_MAX_DIGITS digits of at most 31 bits
struct ProductSumLaunch { const uint64_t *prod; uint32_t K; uint64_t *out; void *S; uint32_t outputs; bool i32 = false; };      // (PRODUCT_SUM_MAX_DIGITS: cn_mul_plan.h)
int cn_l_product_sum(cn_ctx *c, const ProductSumLaunch &g);
// sums of plaintext x ciphertext products (cn_mul_plain_sum; cn_l_diag.hip, k_mul_plain_sum): group g < groups = terms [grp_off[g], grp_off[g + 1]), term e = plaintext
// pt + e N (coefficients mod t) times the NTT-form ciphertext ctn + slot[e] 2kN; out [groups][2][k][N].  grp_off / slot: device memory.  policy: cn_policy of the q limbs
// Both launchers have a kernel where cn_plain_wide (cn_policy.h) holds; accmax and order come from the plan (PlainSumPlan, cn_plain_plan.h)
struct MulPlainSumLaunch { const uint64_t *pt, *ctn; const uint32_t *grp_off, *slot; uint64_t *out; uint32_t groups, accmax, order; };      // order: k_mul_ptn_sum only ("ptn_order")
int cn_l_mul_plain_sum(cn_ctx *c, int policy, const MulPlainSumLaunch &a);
int cn_l_diag_set_attrs(uint32_t logn, size_t lds);
// the same sums over an NTT-form plaintext array (cn_l_ptn.hip, k_mul_ptn_sum): a.pt = the NTT-form words of term 0 ([term][k][N], cn_pt_transform), a.accmax = the
// recentring interval of the lazy FP64 accumulators (cn_ptn_sum_interval, cn_policy.h)
int cn_l_mul_ptn_sum(cn_ctx *c, int policy, const MulPlainSumLaunch &a);
int cn_l_ptn_set_attrs(uint32_t logn, size_t lds);
// a diagonal plan built on the device (cn_diag_scan, cn_diag_encode; cn_l_diagplan.hip, cn_k_diagplan.hip.h): S = the slot-order weight matrix [R][N] decoded from the row
// plaintexts, of which rows below R and columns below dim are read.  A run = up to CN_DIAG_RUN terms (c, J, b0 + db) that are neighbours in the term list; `first` counts
// from the `out` / `nz` of the launch.  The scan ORs into flags [2][N / 2], the gather into nz [terms] (bytes, zeroed by the caller) and writes every word of its terms
struct DiagRunHost { uint32_t c, J, b0, len, first; };
static const uint32_t CN_DIAG_RUN = 32, CN_DIAG_MAX_RUNS = 65535;
int cn_l_diag_scan(cn_ctx *c, const uint64_t *S, uint32_t R, uint32_t dim, uint8_t *flags);
int cn_l_diag_gather(cn_ctx *c, const uint64_t *S, uint32_t R, uint32_t dim, const DiagRunHost *runs, uint32_t nruns, const uint32_t *index_map, uint64_t *out, uint8_t *nz);
// modulus switching (cn_l_modswitch.hip): `items` (ciphertext, poly) pairs [items][ks][N] -> [items][kd][N] on c's stream with the constants of the source context
int cn_l_mod_switch(cn_ctx *c, const uint64_t *src, uint64_t *dst, const DevConsts *src_consts, uint32_t ks, uint32_t kd, uint32_t items, uint32_t logn,
                    bool f64, bool *ran_f64);
// invariant noise norm (cn_l_noise.hip): `count` ciphertexts (c0 of ciphertext i at c0 + i * ct_stride, acc [count][k][N] from decrypt_phase) ->
// out [count][k] words on c's stream
int cn_l_noise_norm(cn_ctx *c, const uint64_t *c0, size_t ct_stride, const uint64_t *acc, uint64_t *out, uint32_t count);
// reply path (cn_l_join.hip, cn_k_join.hip.h): the CRT join of `count` x `nslots` values out of the transformed plaintexts plain [P][count][N] on c's stream (tab: the call's
// JoinTab on the device; values [count][nslots] doubles and words [count][nslots][W] may be null), and the arg max per slot over the ciphertexts from those words
int cn_l_crt_join(cn_ctx *c, const uint64_t *plain, const uint32_t *index_map, const void *tab, uint32_t P, uint32_t W, double *values, uint64_t *words, uint32_t count, uint32_t nslots);
int cn_l_join_argmax(cn_ctx *c, const uint64_t *words, uint32_t W, int32_t *argmax, uint32_t count, uint32_t nslots);
// request path (cn_l_split.hip, cn_k_split.hip.h): `count` plaintexts of `nvalues` values each, split modulo t[0 .. P) on c's stream - element (ct, s) at
// values[ct stride_ct + s stride_slot] (device memory, 8 bytes each: doubles, or int64 under CN_SPLIT_I64), row ct of prime i at dst[i] + ct N in the slot order of
// index_map (position 0 under CN_SPLIT_COEFF0), zero beyond nvalues.  nz [P][nz_stride] and bad [1]: device words zeroed by the caller, OR-ed with 1 for a plaintext with
// a non-zero coefficient / when a value does not fit.  At most 65535 x 16 plaintexts per launch.
int cn_l_crt_split(cn_ctx *c, const void *values, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues, uint32_t flags, double scale,
                   const uint64_t *t, uint64_t *const *dst, uint32_t P, const uint32_t *index_map, uint32_t *nz, uint32_t nz_stride, uint32_t *bad);
// seeded ciphertexts (cn_l_seeded.hip, k_seeded): `cnt` ciphertexts, poly 0 of ciphertext i at out + i * ct_stride.  expand_only: poly 1 = INTT(a) alone (cn_ct_expand);
// else both components of a secret-key encryption - noise: the int8 polynomials [cnt][N] of k_sample_small, pt: plaintexts (null = zero) pt_stride_words apart
struct SeededArgs {
    uint64_t *out; size_t ct_stride; uint32_t cnt; bool expand_only;
    const uint8_t *a_seed32; uint64_t a_nonce, a_item0;
    const int8_t *noise; const uint64_t *pt; uint32_t pt_stride_words;
};
int cn_l_seeded(cn_ctx *c, const SeededArgs &a);
// packed rows (cn_l_packed.hip, cn_k_packed.hip.h): `cnt` ciphertexts of `polys` polynomials, packed [cnt][polys][limb] rows <-> poly 0 .. polys - 1 of the items at
// arr + i * item_words; flag: one device word the unpack ORs 1 into when it saw a residue >= q_j (stored reduced).  stream null: the context's
size_t cn_packed_row_words(const cn_ctx *c);
int cn_l_unpack_rows(cn_ctx *c, const uint64_t *packed, uint64_t *arr, size_t item_words, uint32_t cnt, uint32_t polys, uint32_t *flag, hipStream_t stream = nullptr);
int cn_l_pack_rows(cn_ctx *c, const uint64_t *arr, size_t item_words, uint64_t *packed, uint32_t cnt, uint32_t polys, hipStream_t stream = nullptr);
// Galois keys for `elts` elements in one launch (cn_l_keygen.hip, k_ksk_gen): outs = one key address per element, fac = [tot] x CN_MAXK message factors (gen_ksk's
// KeyFactors per entry), perm = [elts][N] NTT-domain automorphism indices, noise = the int8 polynomials [elts * tot][N] of k_sample_small; entry e of element g draws
// its `a` at sampler item item0 + 2 (g tot + e)
struct KskGenArgs {
    const void *outs, *fac; const uint16_t *perm; const int8_t *noise;
    uint64_t seed, item0; uint32_t elts, tot; bool f64out;
};
int cn_l_ksk_gen(cn_ctx *c, const KskGenArgs &a);

inline void cn_launch_count(cn_ctx *c, int n = 1) { c->st.kernel_launches += n; }
