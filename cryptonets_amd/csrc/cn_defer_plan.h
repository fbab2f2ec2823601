// What a flush of the deferred queue launches, decided here and nowhere else: which arrays a queued call reads, the level a call is admitted on and whether it
// triggers a flush, the three rewrites of the queue (bias fold, zero fold, merge of scalar products across levels), the fate of products whose relinearisation is held
// back, what may be parked, the staging-arena layout of a staged group and the ordered list of steps.  cn_defer.hip asks this header for every decision and keeps the
// device work.  Host-only and free of HIP and of cn_ctx: a plain C++ compiler builds it (tests/cpp/defer_plan.cpp).
#pragma once
#include "cn_internal.h"
#include <algorithm>
#include <cstring>
#include <map>
#include <unordered_map>
#include <utility>
#include <vector>

enum { DOP_GEMM1 = 0, DOP_ADD, DOP_SUB, DOP_ADDPLAIN, DOP_SUBPLAIN, DOP_MULRELIN, DOP_ENCRYPT,
       DOP_COPY, DOP_MULPLAIN, DOP_ROT, DOP_ROTADD, DOP_COLS, DOP_COLSADD, DOP_SUMSLOTS, DOP_TYPES };      // DOP_COPY .. : staged (gather / batched call / scatter) at flush time
struct DOp {
    int type; int32_t level;
    uint64_t *out;                 // output ciphertext (size 2)
    const uint64_t *a, *b;         // operands (ADD/SUB/MULRELIN: ciphertexts; ADDPLAIN/SUBPLAIN: b = plaintext polynomial)
    uint32_t K; size_t terms;      // GEMM1: K (address, weight) pairs from DeferQueue::addr / ::wt [terms ..)
    const uint64_t *bias;          // GEMM1: plaintext polynomial added to the result (an AddPlain folded in at flush time), or null
    uint64_t nonce = 0, item = 0;  // ENCRYPT: the call's seed and the sampler item of this ciphertext (a = plaintext polynomial or null)
    int64_t arg = 0;               // staged kinds: rotation steps (ROT, ROTADD) / slot count (SUMSLOTS); MULPLAIN: b = plaintext polynomial; ROTADD / COLSADD: b = accumulator
    int32_t fold_first = -1; uint32_t fold_count = 0;   // GEMM1: terms [fold_first, +fold_count) of DeferQueue::folds - zero encryptions folded onto this output (defer_fold_zero)
};
struct DeferSquare;
struct DeferQueue {
    std::vector<DOp> ops;
    std::vector<uint64_t> addr, wt;
    struct Haz { int32_t w = -1, r = -1, wop = -1; uint32_t readers = 0; int32_t hd = 0; };   // level of the last writer / deepest reader since / index of the writing op / readers since / heavy depth of the value (defer_admit)
    // address -> hazard record: open addressing, cleared by bumping the epoch (a dense-layer call touches 845 records)
    struct HazMap {
        struct E { const uint64_t *key = nullptr; uint32_t epoch = 0; Haz v; };
        std::vector<E> tab = std::vector<E>(1 << 12);
        uint32_t epoch = 1; size_t used = 0;
        static size_t hash(const uint64_t *p) { uint64_t x = (uint64_t)p >> 8; x *= 0x9E3779B97F4A7C15ull; return (size_t)(x >> 20); }
        const Haz *find(const uint64_t *p) const {
            for (size_t i = hash(p) & (tab.size() - 1);; i = (i + 1) & (tab.size() - 1)) {
                if (tab[i].epoch != epoch) return nullptr;
                if (tab[i].key == p) return &tab[i].v;
            }
        }
        Haz &operator[](const uint64_t *p) {
            if (2 * (used + 1) > tab.size()) grow();
            for (size_t i = hash(p) & (tab.size() - 1);; i = (i + 1) & (tab.size() - 1)) {
                if (tab[i].epoch != epoch) { tab[i].key = p; tab[i].epoch = epoch; tab[i].v = Haz(); used++; return tab[i].v; }
                if (tab[i].key == p) return tab[i].v;
            }
        }
        void grow() {
            std::vector<E> old; old.swap(tab);
            tab.assign(old.size() * 2, E()); used = 0;
            for (const E &e : old) if (e.epoch == epoch) (*this)[e.key] = e.v;
        }
        void clear() { used = 0; if (++epoch == 0) { for (E &e : tab) e.epoch = 0; epoch = 1; } }
    } haz;
    int32_t maxlevel = -1;
    std::vector<std::pair<uint64_t *, size_t>> frees;      // arrays released by the caller while calls were pending: back to the pool after the flush
    struct Fold { int32_t enc; uint64_t w; };               // a zero encryption (index of its DOp) folded into a scalar product with weight w (residue mod t)
    std::vector<Fold> folds;
    DeferSquare *sq = nullptr;                              // squarings whose relinearisation is held back for the next dense layer (cn_api_shared.h, cn_defer.hip)
};

static const size_t DEFER_FLUSH_MIN = 64, DEFER_MAX_OPS = 32768;
// what the rules read of the environment and of a context, by value (defer_switches in cn_defer.hip builds it and is the only reader of the three variables)
struct DeferSwitches {
    int trace = 0;                 // CN_DEFER_TRACE: 1 one line per (flush, level) and per parked / fused / materialised group, 2 also the host time of every flush
    bool merge_gemm = true;        // CN_DEFER_MERGE_GEMM=0 keeps the scalar products on their levels (A/B)
    bool rel = true;               // CN_DEFER_REL=0 keeps the address tables of flush_gemm_group (A/B)
    size_t flush_min = DEFER_FLUSH_MIN, max_ops = DEFER_MAX_OPS;      // a layer boundary launches what is queued if at least flush_min calls wait; a queue of max_ops is full
    // of the context (left as they stand where no context was given: admission reads none of them)
    bool fold_zero = false;        // "fold_zero" is on and the context has the kernels of the fold (zero_fold_ok)
    uint64_t t_half = 0;           // DevConsts::t_half
    bool square_gemm = false;      // "defer_square_gemm" is on, the context takes cn_square_gemm's second half (square_gemm_ctx_ok) and has relinearisation keys: mul_defers_square_gemm, cn_mul_plan.h
    size_t ctw2 = 0; uint32_t n = 0;      // words of a size-2 ciphertext, ring size
    size_t park_max = 0;           // bytes of products a flush may park: a quarter of the scratch limit
    size_t product_bytes() const { return ctw2 / 2 * 3 * 8; }      // one size-3 product
};

// ---- the arrays a queued call reads, by kind: fn(address, i) - i the term of a scalar product, 0 / 1 for operands a / b.  Null taps are skipped; the plaintext operand
// of ADDPLAIN / SUBPLAIN / MULPLAIN and of an encryption is no read (a plaintext is never the output of a queued call)
template <class F> inline void defer_reads(const DeferQueue &q, const DOp &op, F fn) {
    if (op.type == DOP_GEMM1) {
        for (uint32_t kk = 0; kk < op.K; kk++) { const uint64_t *p = (const uint64_t *)q.addr[op.terms + kk]; if (p) fn(p, kk); }
        return;
    }
    if (op.type == DOP_ENCRYPT) return;
    if (op.a) fn(op.a, 0u);
    const bool b_plain = op.type == DOP_ADDPLAIN || op.type == DOP_SUBPLAIN || op.type == DOP_MULPLAIN;
    if (!b_plain && op.b) fn(op.b, 1u);
}

// ---- admission.  The level of a call: behind the last writer of everything it reads, behind the last writer and the deepest reader of what it writes.
// A flush is triggered by demand (any entry point that needs results), by a full queue, and at LAYER BOUNDARIES, so that the device works on
// one layer while the callers queue the next.  A boundary is recognised by the "heavy depth" of a value: 0 for anything that was not
// produced by a queued call, and for fresh encryptions; a scalar product (DenseMatrixBySparseVectorMultiply) or a Multiply + Relinearize
// produces depth 1 + the deepest of its inputs; additions, plaintext products, rotations and copies pass the depth of their inputs on.  A heavy call that would reach depth 2 reads
// the result of another queued heavy call: the layer that produced it is complete (its callers have returned) - everything queued is
// launched, if at least flush_min calls wait.  (Round 2 used the plain dependency level for this; with the literal padded taps -
// encryption -> scalar product -> plain addition inside ONE layer - several caller threads interleave those levels and the layer was cut
// into dozens of small launches: 0.47 of the batched rate at 4-32 threads against 0.84 at one.  Flushing whenever the stream had run dry
// instead cut the first layers into 256-call pieces and lost the bias folding: 0.85 against 0.93.)
enum { DEFER_FLUSH_NONE = 0, DEFER_FLUSH_BOUNDARY, DEFER_FLUSH_FULL };
struct DeferAdmit { int32_t level, hd; int flush; };      // flush: what has to be launched BEFORE the call is queued (level and hd are then those of an empty queue)
inline DeferAdmit defer_admit(const DeferQueue &q, const DOp &op, const DeferSwitches &sw) {
    int32_t lv = 0, hd = 0;
    defer_reads(q, op, [&](const uint64_t *p, uint32_t) {
        const DeferQueue::Haz *h = q.haz.find(p);
        if (h) { lv = std::max(lv, h->w + 1); hd = std::max(hd, h->hd); }
    });
    const DeferQueue::Haz *ho = q.haz.find(op.out);
    if (ho) lv = std::max(lv, std::max(ho->w, ho->r) + 1);
    const bool heavy = op.type == DOP_GEMM1 || op.type == DOP_MULRELIN;      // (rotations counted as heavy too was measured: the LoLa rows were cut into more, smaller
                                                                               // launches - 388 instead of 309 per prime, 14.3 instead of 12.1 ms per image)
    hd += heavy ? 1 : 0;
    const bool full = q.ops.size() >= sw.max_ops;
    if (full || (heavy && hd >= 2 && q.ops.size() >= sw.flush_min)) return {0, heavy ? 1 : 0, full ? DEFER_FLUSH_FULL : DEFER_FLUSH_BOUNDARY};
    return {lv, hd, DEFER_FLUSH_NONE};
}
// the call joins the queue on the level it was admitted on: its reads and its write go into the hazard records
inline void defer_record(DeferQueue &q, DOp op, const DeferAdmit &ad) {
    op.level = ad.level;
    const int32_t me = (int32_t)q.ops.size();
    defer_reads(q, op, [&](const uint64_t *p, uint32_t) { DeferQueue::Haz &h = q.haz[p]; h.r = std::max(h.r, ad.level); h.readers++; });
    DeferQueue::Haz &ho = q.haz[op.out];
    ho.w = ad.level; ho.r = -1; ho.wop = me; ho.readers = 0; ho.hd = ad.hd;
    q.maxlevel = std::max(q.maxlevel, ad.level);
    q.ops.push_back(op);
}

// ---- the arrays the caller has released while calls were pending (DeferQueue::frees lists whole buffers), built once per flush
struct DeferReleased {
    std::map<const uint64_t *, size_t> rng;      // base address -> bytes
    explicit DeferReleased(const std::vector<std::pair<uint64_t *, size_t>> &frees) { for (auto &f : frees) rng[f.first] = f.second; }
    bool base(const uint64_t *p) const { return rng.count(p) != 0; }      // p is the base address of a released buffer
    bool holds(const uint64_t *p) const {                                  // p lies inside a released buffer (an output may be an element of a handle of several ciphertexts)
        auto it = rng.upper_bound(p);
        if (it == rng.begin()) return false;
        --it;
        return (const char *)p < (const char *)it->first + it->second;
    }
};

// ---- rewrite 1: an AddPlain that only adds the bias to a DenseMatrixBySparseVectorMultiply result the caller has already released
// (PoolLayer.cs:184-186: `using (conv = ConvolveOnce(..)) res[k] = conv.Add(bias)`) is folded into the GEMM's epilogue - the GEMM
// then runs at the AddPlain's level and writes its output: safe when nothing else reads the intermediate and no later call
// overwrites the GEMM's inputs
inline void defer_fold_bias(DeferQueue &q, std::vector<uint8_t> &dead, const DeferReleased &released) {
    std::vector<DOp> &ops = q.ops;
    for (size_t x = 0; x < ops.size(); x++) {
        DOp &X = ops[x];
        if (X.type != DOP_ADDPLAIN || X.a == X.out) continue;
        const DeferQueue::Haz *hi = q.haz.find(X.a);
        // the recorded writer must be the op that PRODUCED X's operand: a handle reused as the output of a later call has its last
        // writer BEHIND X (GEMM1 -> tmp, AddPlain(tmp) -> r1, GEMM2 -> tmp ...: folding GEMM2 into the first AddPlain would be wrong)
        if (!hi || hi->wop < 0 || hi->wop >= (int32_t)x || hi->readers != 1 || !released.base(X.a)) continue;
        if (ops[hi->wop].level >= X.level) continue;
        DOp &Gm = ops[hi->wop];
        if (Gm.type != DOP_GEMM1 || Gm.bias || Gm.out != X.a || dead[hi->wop]) continue;
        bool ok = true;
        defer_reads(q, Gm, [&](const uint64_t *in, uint32_t) { const DeferQueue::Haz *h2 = q.haz.find(in); if (h2 && h2->wop > hi->wop) ok = false; });
        if (!ok) continue;
        Gm.out = X.out; Gm.bias = X.b; Gm.level = X.level;
        dead[x] = 1;
    }
}
// ---- rewrite 2: fresh encryptions of ZERO that only feed one queued scalar product and have been released (PoolLayer.ElementAt / ReleaseTemp, PoolLayer.cs:67-90) are
// not materialised: their weighted sum is folded onto the scalar product's output by linearity (k_encrypt_fold: same words, a fifth of the transforms, the
// scalar product reads no extra ciphertexts and the outputs of a border patch share their gather list again).  Conditions, all on whole arrays: the
// encryption is the last writer of its array, exactly one queued call reads it - a scalar product on a deeper level - and the caller has released it.
// Returns the number of encryptions folded (dead = 2).
inline uint64_t defer_fold_zero(DeferQueue &q, std::vector<uint8_t> &dead, const DeferReleased &released, const DeferSwitches &sw) {
    if (!sw.fold_zero) return 0;
    std::vector<DOp> &ops = q.ops;
    std::unordered_map<const uint64_t *, int32_t> cand;
    size_t zero_encs = 0;
    for (size_t x = 0; x < ops.size(); x++) {
        const DOp &E = ops[x];
        if (dead[x] || E.type != DOP_ENCRYPT || E.a) continue;
        zero_encs++;
        const DeferQueue::Haz *h = q.haz.find(E.out);
        if (h && h->wop == (int32_t)x && h->readers == 1 && released.base(E.out)) cand[E.out] = (int32_t)x;
    }
    // all or nothing: a caller that parks its releases (cn_free_many of 32 at a time, the locked twin of rounds 3-5) leaves some of a layer's zero vectors alive at
    // the flush - folding the rest would run BOTH chains (samplers + k_encrypt_fused for the live ones, samplers + k_encrypt_fold for the others) and cut the scalar
    // products of a layer into more gather groups: 17.4 against 15.8 ms per batch (profiles/r06_bench_default_flags.json, `locked`)
    if (cand.size() != zero_encs) cand.clear();
    if (cand.empty()) return 0;
    const uint64_t max_terms = (1ull << 52) / std::max<uint64_t>(1, sw.t_half * 20);
    uint64_t folded = 0;
    for (size_t x = 0; x < ops.size(); x++) {
        DOp &G = ops[x];
        if (dead[x] || G.type != DOP_GEMM1 || G.level == 0) continue;
        auto folds_in = [&](const uint64_t *a) { auto it = cand.find(a); return it != cand.end() && ops[it->second].level < G.level ? it : cand.end(); };
        uint32_t nf = 0, left = 0;
        defer_reads(q, G, [&](const uint64_t *a, uint32_t kk) { if (folds_in(a) != cand.end()) nf++; else if (q.wt[G.terms + kk]) left++; });
        if (!nf || !left || nf > max_terms) continue;              // (a scalar product keeps at least one real term: its launch writes the output the fold adds onto)
        G.fold_first = (int32_t)q.folds.size();
        defer_reads(q, G, [&](const uint64_t *a, uint32_t kk) {
            auto it = folds_in(a);
            if (it == cand.end()) return;
            if (q.wt[G.terms + kk]) { q.folds.push_back({it->second, q.wt[G.terms + kk]}); G.fold_count++; }      // (weight 0: the term contributes nothing, AtomicSealBfvVector.cs:468)
            q.addr[G.terms + kk] = 0; q.wt[G.terms + kk] = 0;
            dead[it->second] = 2;
            cand.erase(it);
        });
        folded += nf;
    }
    return folded;
}
// ---- rewrite 3: scalar products of one term count on different levels of the same flush become ONE launch where nothing stands in the way (round 5).  The
// literal PoolLayer pattern puts the outputs that read a fresh encryption of zero (a padded tap) one level behind the others: two GEMM launches per
// convolution, the second one a fifth the size and barely half as efficient (k_scalar_gemm<1>: 0.30 ms for 125 outputs against 0.50 ms for 720).
// A scalar product may wait for the deepest level that holds others of its kind if, behind its own level, nobody reads or writes its output and
// nobody writes its inputs (checked against every queued call, conservatively: any later level counts).
inline void defer_merge_gemm(DeferQueue &q, const std::vector<uint8_t> &dead, const DeferSwitches &sw) {
    if (!sw.merge_gemm) return;
    std::vector<DOp> &ops = q.ops;
    std::map<uint32_t, std::pair<int32_t, int32_t>> span;          // term count -> (shallowest, deepest) level of its live scalar products
    for (size_t x = 0; x < ops.size(); x++) if (!dead[x] && ops[x].type == DOP_GEMM1) {
        auto it = span.find(ops[x].K);
        if (it == span.end()) span[ops[x].K] = {ops[x].level, ops[x].level};
        else { it->second.first = std::min(it->second.first, ops[x].level); it->second.second = std::max(it->second.second, ops[x].level); }
    }
    bool any = false;
    for (auto &kv : span) any = any || kv.second.first != kv.second.second;
    if (!any) return;
    struct RW { int32_t r = -1, w = -1; };                      // deepest level at which a queued call reads / writes the array
    std::unordered_map<const uint64_t *, RW> touch;
    touch.reserve(ops.size() * 2);
    for (size_t x = 0; x < ops.size(); x++) {
        if (dead[x]) continue;
        const DOp &X = ops[x];
        defer_reads(q, X, [&](const uint64_t *p, uint32_t) { RW &t = touch[p]; t.r = std::max(t.r, X.level); });
        RW &t = touch[X.out]; t.w = std::max(t.w, X.level);
    }
    for (size_t x = 0; x < ops.size(); x++) {
        DOp &X = ops[x];
        if (dead[x] || X.type != DOP_GEMM1) continue;
        const int32_t deep = span[X.K].second;
        if (X.level >= deep) continue;
        const RW &to = touch[X.out];
        bool ok = to.r <= X.level && to.w <= X.level;
        defer_reads(q, X, [&](const uint64_t *in, uint32_t) { auto it = touch.find(in); ok = ok && (it == touch.end() || it->second.w <= X.level); });
        if (ok) X.level = deep;
    }
}

// ---- products whose relinearisation an earlier layer-boundary flush held back (pending[slot] = the output array of the product in that slot, slot_of the inverse).
// The decision of a flush that finds products pending (once, all or nothing): may every queued reader of a pending array run in cn_square_gemm's second half?
//   (a) the caller has released every pending output array, (b) only scalar products read pending arrays - and those form groups (one level, one term count)
//   whose plan passes square_gemm_fused_ok (cn_mul_plan.h), with a bias on every output or on none, (c) every gathered term of such a scalar product is a pending array (and no zero
//   encryption was folded onto it), (d) no queued call writes a pending array.
// need[slot]: the product has to be relinearised if the answer is no - somebody reads its array or the caller still holds it.
// This is the pure half: rules (a)-(d) and the candidate groups with the key their plan is found by; the plan itself, square_gemm_fused_ok and the scratch limits (mul_sg_scratch, cn_mul_plan.h) are
// sg_prepare's (cn_defer.hip), which says no for all groups if it says no for one.
struct DeferSgGroup {
    int32_t level; uint32_t K;
    std::vector<size_t> members;             // the scalar products, as indices into DeferQueue::ops
    std::vector<const DOp *> rows;           // ... in the plan's output order: sorted by their weights
    std::vector<int32_t> slot_of;            // renumbered slot -> slot (slots are renumbered by first appearance)
    std::vector<uint64_t> W; std::vector<int32_t> cidx;      // the plan's key: weights [O][K], renumbered slots [O][K] (-1: padded tap)
    bool bias_ok;                            // a bias on all rows or on none, offsets from the lowest one a multiple of 256 bytes and below 2^31 units
};
inline bool defer_pending_decide(const DeferQueue &q, const std::vector<uint8_t> &dead, const DeferReleased &released, const std::vector<uint64_t *> &pending,
                                 const std::unordered_map<const uint64_t *, uint32_t> &slots, const DeferSwitches &sw, std::vector<uint8_t> &need, std::vector<DeferSgGroup> &groups) {
    const std::vector<DOp> &ops = q.ops;
    const uint32_t n = (uint32_t)pending.size();
    need.assign(n, 0);
    groups.clear();
    bool ok = sw.square_gemm;
    auto slot_of = [&](const uint64_t *p) -> int32_t { auto it = slots.find(p); return it == slots.end() ? -1 : (int32_t)it->second; };
    std::map<std::pair<int32_t, uint32_t>, std::vector<size_t>> cand;            // (level, term count) -> scalar products that read pending arrays
    for (size_t x = 0; x < ops.size(); x++) {
        if (dead[x]) continue;
        const DOp &X = ops[x];
        if (slot_of(X.out) >= 0) ok = false;                                         // (d)
        uint32_t np = 0, other = 0;
        defer_reads(q, X, [&](const uint64_t *p, uint32_t) { const int32_t s = slot_of(p); if (s >= 0) { need[s] = 1; np++; } else other++; });
        if (!np) continue;
        if (X.type != DOP_GEMM1) { ok = false; continue; }                           // (b)
        if (other || X.fold_count) ok = false;                                       // (c)
        cand[{X.level, X.K}].push_back(x);
    }
    for (uint32_t s = 0; s < n; s++) if (!released.holds(pending[s])) { need[s] = 1; ok = false; }      // (a)
    if (!ok) return false;
    for (auto &kv : cand) {
        const uint32_t K = kv.first.second, O = (uint32_t)kv.second.size();
        DeferSgGroup g; g.level = kv.first.first; g.K = K; g.members = kv.second;
        for (size_t x : kv.second) g.rows.push_back(&ops[x]);
        // the key must not depend on the order in which the caller's threads issued the calls: rows by their weights, slots by first appearance
        std::stable_sort(g.rows.begin(), g.rows.end(), [&](const DOp *x, const DOp *y) {
            return std::lexicographical_compare(&q.wt[x->terms], &q.wt[x->terms] + K, &q.wt[y->terms], &q.wt[y->terms] + K); });
        g.W.resize((size_t)O * K); g.cidx.assign((size_t)O * K, -1);
        std::vector<int32_t> canon(n, -1);
        for (uint32_t o = 0; o < O; o++) {
            memcpy(&g.W[(size_t)o * K], &q.wt[g.rows[o]->terms], (size_t)K * 8);
            defer_reads(q, *g.rows[o], [&](const uint64_t *p, uint32_t kk) {
                const int32_t s = slot_of(p);          // (rule (c): every gathered term of a member is a pending array)
                if (canon[s] < 0) { canon[s] = (int32_t)g.slot_of.size(); g.slot_of.push_back(s); }
                g.cidx[(size_t)o * K + kk] = canon[s];
            });
        }
        uint64_t bbase = ~0ull;
        g.bias_ok = true;
        for (const DOp *r : g.rows) { if ((r->bias != nullptr) != (g.rows[0]->bias != nullptr)) g.bias_ok = false; if (r->bias) bbase = std::min(bbase, (uint64_t)r->bias); }
        for (const DOp *r : g.rows) if (r->bias && ((((uint64_t)r->bias - bbase) & 255) || (((uint64_t)r->bias - bbase) >> 8) >= 0x7fffffffull)) g.bias_ok = false;
        groups.push_back(std::move(g));
    }
    return true;
}

// ---- parking.  The squarings of one level at a layer-boundary flush keep their relinearisation back if every one of them is the last writer of its output array, nothing
// queued reads that array, the caller has not released it, no two of them write the same array, nothing is pending already and the products fit a quarter of the scratch limit
inline bool defer_can_park(const DeferQueue &q, const std::vector<const DOp *> &ops, const DeferReleased &released, const DeferSwitches &sw, bool pending) {
    if (pending || ops.size() * sw.product_bytes() > sw.park_max) return false;
    std::unordered_map<const uint64_t *, int> seen;
    for (const DOp *op : ops) {
        const DeferQueue::Haz *h = q.haz.find(op->out);
        if (!h || h->wop != (int32_t)(op - q.ops.data()) || h->readers || released.holds(op->out) || seen[op->out]++) return false;
    }
    return true;
}

// ---- the staging arena of one (staged kind, argument) group: [tables of the gather copies (2 cnt entries of ciphertexts, cnt of plaintexts) | table of the scatter copy |
// A | B (ROTADD, COLSADD) | O (not SUMSLOTS: in place) | P (MULPLAIN)], every part on a 256-byte boundary.
// An operand whose addresses are equally spaced already IS the array the batched implementation wants (always so for a single call -
// 12 rotations by 12 different step counts are 12 groups of one): it is used in place; only scattered operands are gathered.
// same_a: MultiplyPlain of ONE ciphertext by the plaintexts of several rows (the per-row DotProduct of a dense layer: every row multiplies the same vector): the broadcast
// form - the ciphertext is transformed once, not once per row, and nothing is gathered (round 6)
struct DeferStaged {
    bool has_b, has_p, in_place, same_a;
    bool a_direct, b_direct, p_direct, out_direct;      // used where the callers have them: no gather (scatter) copy
    bool consistent;                                    // false: an in-place kind whose operands are direct and whose results are not, or the reverse (internal error)
    size_t off_tin, off_tpt, off_tout, off_a, off_b, off_o, off_p, total;      // bytes from the arena's base (off_b / off_p: 0 where the kind has none)
};
inline size_t defer_al(size_t b) { return (b + 255) & ~(size_t)255; }
static const size_t DEFER_TAB2_BYTES = 16;              // one (source, destination) pair of the copy kernel
inline DeferStaged defer_staged_layout(int type, const std::vector<const DOp *> &ops, const DeferSwitches &sw) {
    const uint32_t cnt = (uint32_t)ops.size(), n = sw.n; const size_t ctw = sw.ctw2;
    DeferStaged L{};
    L.has_b = type == DOP_ROTADD || type == DOP_COLSADD; L.has_p = type == DOP_MULPLAIN; L.in_place = type == DOP_SUMSLOTS;
    const size_t tabs = defer_al(3 * cnt * DEFER_TAB2_BYTES) + defer_al(cnt * DEFER_TAB2_BYTES), ctb = defer_al(cnt * ctw * 8);
    L.total = tabs + ctb * (1 + (L.has_b ? 1 : 0) + (L.in_place ? 0 : 1)) + (L.has_p ? defer_al((size_t)cnt * n * 8) : 0);
    L.off_tin = 0; L.off_tpt = 2 * cnt * DEFER_TAB2_BYTES; L.off_tout = defer_al(3 * cnt * DEFER_TAB2_BYTES);
    L.off_a = tabs; L.off_b = L.has_b ? L.off_a + ctb : 0;
    L.off_o = L.in_place ? L.off_a : L.off_a + ctb * (L.has_b ? 2 : 1); L.off_p = L.has_p ? L.off_o + ctb : 0;
    auto spaced = [&](auto get, size_t words) { for (uint32_t i = 1; i < cnt; i++) if (get(ops[i]) != get(ops[0]) + (size_t)i * words) return false; return true; };
    L.same_a = L.has_p && cnt >= 2;
    for (uint32_t i = 1; i < cnt && L.same_a; i++) L.same_a = ops[i]->a == ops[0]->a;
    for (uint32_t i = 0; i < cnt && L.same_a; i++) L.same_a = (const uint64_t *)ops[i]->out != ops[0]->a;      // (the shared operand is nobody's result)
    L.a_direct = L.same_a || spaced([](const DOp *o) { return o->a; }, ctw);
    L.b_direct = L.has_b && spaced([](const DOp *o) { return o->b; }, ctw);
    L.p_direct = L.has_p && spaced([](const DOp *o) { return o->b; }, n);
    L.out_direct = spaced([](const DOp *o) { return (const uint64_t *)o->out; }, ctw);
    L.consistent = !(L.in_place && L.a_direct != L.out_direct);
    return L;
}

// ---- the ordered steps of a flush: level by level, one batched launch chain per step
enum { DSTEP_GEMM,          // scalar products of one term count (key), without those of the fused groups
       DSTEP_FUSED,         // a group of defer_pending_decide in cn_square_gemm's second half (key: its index)
       DSTEP_ZERO_FOLD,     // the zero encryptions folded onto the scalar products of this level (launched just before)
       DSTEP_ELEMENTWISE,   // ADD, SUB, ADDPLAIN, SUBPLAIN (type)
       DSTEP_ENCRYPT,
       DSTEP_COPY,          // Ciphertext copies: the table copy is the operation
       DSTEP_ROT_JOBS,      // few rotations, any step counts: one launch chain per hop round
       DSTEP_STAGED,        // one staged kind (type), one argument (key: rotation steps, slot count)
       DSTEP_MULRELIN };    // key 1: squarings (SquareActivation: the fused kernel; park: they may keep their relinearisation back), then key 0: general products
struct DeferStep { int32_t level; int kind, type; int64_t key; bool park; std::vector<const DOp *> ops; };
// fused: the groups the pending-squarings decision accepted (empty: none).  few_rot(count): queued rotations of this count run as one chain per hop round (ks_few_rotations)
template <class FewRot> inline std::vector<DeferStep> defer_schedule(const DeferQueue &q, const std::vector<uint8_t> &dead, const std::vector<DeferSgGroup> &fused, bool boundary,
                                                                      const DeferSwitches &sw, FewRot few_rot) {
    const std::vector<DOp> &ops = q.ops;
    std::vector<uint8_t> in_fused(ops.size(), 0);
    int32_t sg_deepest = -1;
    for (const DeferSgGroup &g : fused) { for (size_t x : g.members) in_fused[x] = 1; sg_deepest = std::max(sg_deepest, g.level); }
    std::vector<DeferStep> steps;
    auto step = [&](int32_t lv, int kind, int type, int64_t key) -> DeferStep & { steps.push_back({lv, kind, type, key, false, {}}); return steps.back(); };
    for (int32_t lv = 0; lv <= q.maxlevel; lv++) {
        std::vector<const DOp *> by_type[DOP_TYPES];
        for (size_t x = 0; x < ops.size(); x++) if (!dead[x] && ops[x].level == lv) by_type[ops[x].type].push_back(&ops[x]);
        if (!by_type[DOP_GEMM1].empty()) {
            std::map<uint32_t, std::vector<const DOp *>> byK;
            for (const DOp *op : by_type[DOP_GEMM1]) if (!in_fused[op - ops.data()]) byK[op->K].push_back(op);
            for (auto &kv : byK) step(lv, DSTEP_GEMM, DOP_GEMM1, kv.first).ops.swap(kv.second);
            for (size_t g = 0; g < fused.size(); g++) if (fused[g].level == lv) step(lv, DSTEP_FUSED, DOP_GEMM1, (int64_t)g).ops = fused[g].rows;
            std::vector<const DOp *> folded;
            for (const DOp *op : by_type[DOP_GEMM1]) if (op->fold_count) folded.push_back(op);
            if (!folded.empty()) step(lv, DSTEP_ZERO_FOLD, DOP_GEMM1, 0).ops.swap(folded);
        }
        for (int t : {DOP_ADD, DOP_SUB, DOP_ADDPLAIN, DOP_SUBPLAIN}) if (!by_type[t].empty()) step(lv, DSTEP_ELEMENTWISE, t, 0).ops.swap(by_type[t]);
        if (!by_type[DOP_ENCRYPT].empty()) step(lv, DSTEP_ENCRYPT, DOP_ENCRYPT, 0).ops.swap(by_type[DOP_ENCRYPT]);
        for (int t = DOP_COPY; t <= DOP_SUMSLOTS; t++) {
            if (by_type[t].empty()) continue;
            if (t == DOP_COPY) { step(lv, DSTEP_COPY, t, 0).ops.swap(by_type[t]); continue; }
            if (t == DOP_ROT && few_rot(by_type[t].size())) { step(lv, DSTEP_ROT_JOBS, t, 0).ops.swap(by_type[t]); continue; }
            std::map<int64_t, std::vector<const DOp *>> by_arg;      // one batched call per parameter value (rotation steps, slot count)
            for (const DOp *op : by_type[t]) by_arg[op->arg].push_back(op);
            for (auto &kv : by_arg) step(lv, DSTEP_STAGED, t, kv.first).ops.swap(kv.second);
        }
        for (int sq = 1; sq >= 0; sq--) {
            std::vector<const DOp *> part;
            for (const DOp *op : by_type[DOP_MULRELIN]) if ((op->a == op->b) == (sq == 1)) part.push_back(op);
            if (part.empty()) continue;
            DeferStep &s = step(lv, DSTEP_MULRELIN, DOP_MULRELIN, sq);
            s.ops.swap(part);
            // (new products take the slots from 0: only behind the last group that still reads the old ones)
            s.park = sq == 1 && boundary && sw.square_gemm && lv > sg_deepest;
        }
    }
    return steps;
}
