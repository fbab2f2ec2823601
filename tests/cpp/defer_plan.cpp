// CPU run of the host-only flush planner of the deferred queue (cryptonets_amd/csrc/cn_defer_plan.h), for tests/test_defer_plan.py: text programs of queued calls over
// synthetic addresses (never dereferenced) go through defer_admit / defer_record and, at every flush, through the planner exactly as cn_defer_flush drives it; the
// device half of the decision about pending products is a flag of the program.
// Input (argv[1]), hex addresses, one statement per line:
//     program NAME device=0|1 n ctw2 t_half park_max fold_zero merge flush_min max_ops few_rot square_gemm
//     gemm OUT ADDR:W ...            (ADDR 0: padded tap)              enc OUT PT ITEM      (PT 0: an encryption of zero)
//     add|sub|mulrelin OUT A B       addplain|subplain|mulplain OUT A PT                    copy|cols OUT A         rot OUT A ARG
//     rotadd OUT A B ARG             colsadd OUT A B                   sumslots A ARG       free BASE BYTES         flush boundary|demand          end
// Output: `admit` per call (index in the queue, level, heavy depth, flush triggered); per flush the rewritten calls (`op`), `dead`, `fold`, the decision about pending
// products (`pending`, `group`), the `step` list with `park` / `staged` decisions, and `endflush` with what the flush did (counts for the coverage condition).
#include "../../cryptonets_amd/csrc/cn_defer_plan.h"
#include <cstdio>
#include <sstream>
#include <string>
#include <fstream>

static const char *KIND[] = {"gemm", "add", "sub", "addplain", "subplain", "mulrelin", "enc", "copy", "mulplain", "rot", "rotadd", "cols", "colsadd", "sumslots"};
static const char *STEP[] = {"GEMM", "FUSED", "ZERO_FOLD", "ELEMENTWISE", "ENCRYPT", "COPY", "ROT_JOBS", "STAGED", "MULRELIN"};

struct Harness {
    DeferQueue q; DeferSwitches sw; bool device = true; size_t few_rot = 0; int flushes = 0;
    std::vector<uint64_t *> pending; std::unordered_map<const uint64_t *, uint32_t> slots;      // DeferSquare::out / ::slot
    size_t idx(const DOp *op) const { return (size_t)(op - q.ops.data()); }
    void flush(bool boundary) {
        if (q.ops.empty() && pending.empty()) { q.frees.clear(); return; }
        printf("flush %d boundary=%d ops=%zu\n", flushes++, (int)boundary, q.ops.size());
        const DeferReleased released(q.frees);
        std::vector<uint8_t> dead(q.ops.size(), 0);
        defer_fold_bias(q, dead, released);
        const uint64_t folded = defer_fold_zero(q, dead, released, sw);
        std::vector<int32_t> before(q.ops.size());
        for (size_t x = 0; x < q.ops.size(); x++) before[x] = q.ops[x].level;
        defer_merge_gemm(q, dead, sw);
        size_t merged = 0, bias_folds = 0;
        for (size_t x = 0; x < q.ops.size(); x++) { merged += before[x] != q.ops[x].level; bias_folds += dead[x] == 1; }
        for (size_t x = 0; x < q.ops.size(); x++) {
            const DOp &X = q.ops[x];
            printf("op %zu %s level=%d dead=%d out=%llx a=%llx b=%llx bias=%llx arg=%lld item=%llu folds=%d+%u terms", x, KIND[X.type], X.level, (int)dead[x], (unsigned long long)X.out,
                   (unsigned long long)X.a, (unsigned long long)X.b, (unsigned long long)X.bias, (long long)X.arg, (unsigned long long)X.item, X.fold_first, X.fold_count);
            if (X.type == DOP_GEMM1) for (uint32_t kk = 0; kk < X.K; kk++) printf(" %llx:%llu", (unsigned long long)q.addr[X.terms + kk], (unsigned long long)q.wt[X.terms + kk]);
            printf("\n");
        }
        for (size_t f = 0; f < q.folds.size(); f++) printf("fold %zu enc=%d w=%llu\n", f, q.folds[f].enc, (unsigned long long)q.folds[f].w);
        std::vector<DeferSgGroup> sgs;
        int fused = 0, materialised = 0;
        if (!pending.empty()) {
            std::vector<uint8_t> need;
            bool ok = defer_pending_decide(q, dead, released, pending, slots, sw, need, sgs);
            const bool pure = ok;
            for (const DeferSgGroup &g : sgs) ok = ok && g.bias_ok;
            ok = ok && device;
            printf("pending %zu pure=%d fused=%d need", pending.size(), (int)pure, (int)ok);
            for (uint8_t v : need) printf(" %d", (int)v);
            printf("\n");
            if (!ok) { sgs.clear(); for (uint8_t v : need) materialised += v; }
            fused = (int)sgs.size();
            for (size_t g = 0; g < sgs.size(); g++) {
                printf("group %zu level=%d K=%u bias_ok=%d rows", g, sgs[g].level, sgs[g].K, (int)sgs[g].bias_ok);
                for (const DOp *r : sgs[g].rows) printf(" %zu", idx(r));
                printf(" slot_of");
                for (int32_t s : sgs[g].slot_of) printf(" %d", s);
                printf(" cidx");
                for (int32_t c : sgs[g].cidx) printf(" %d", c);
                printf("\n");
            }
            pending.clear(); slots.clear();
        }
        const std::vector<DeferStep> steps = defer_schedule(q, dead, sgs, boundary, sw, [&](size_t count) { return count <= few_rot; });
        int parked = 0;
        for (const DeferStep &s : steps) {
            printf("step level=%d %s %s key=%lld park=%d ops", s.level, STEP[s.kind], KIND[s.type], (long long)s.key, (int)s.park);
            for (const DOp *op : s.ops) printf(" %zu", idx(op));
            printf("\n");
            if (s.kind == DSTEP_MULRELIN && s.park) {
                const bool can = defer_can_park(q, s.ops, released, sw, !pending.empty());
                printf("park level=%d %d\n", s.level, (int)can);
                if (can) { parked++; for (const DOp *op : s.ops) { slots[op->out] = (uint32_t)pending.size(); pending.push_back(op->out); } }
            }
            if (s.kind == DSTEP_STAGED) {
                const DeferStaged L = defer_staged_layout(s.type, s.ops, sw);
                printf("staged level=%d %s key=%lld same_a=%d direct=%d%d%d%d consistent=%d off=%zu,%zu,%zu,%zu,%zu,%zu,%zu total=%zu\n", s.level, KIND[s.type], (long long)s.key, (int)L.same_a,
                       (int)L.a_direct, (int)L.b_direct, (int)L.p_direct, (int)L.out_direct, (int)L.consistent, L.off_tin, L.off_tpt, L.off_tout, L.off_a, L.off_b, L.off_o, L.off_p, L.total);
            }
        }
        printf("endflush bias_folds=%zu zero_folds=%llu merged=%zu parked=%d fused=%d materialised=%d\n", bias_folds, (unsigned long long)folded, merged, parked, fused, materialised);
        q.ops.clear(); q.addr.clear(); q.wt.clear(); q.haz.clear(); q.maxlevel = -1; q.folds.clear(); q.frees.clear();
    }
    void push(DOp op) {                                       // defer_push (cn_defer.hip) without the device
        const DeferAdmit ad = defer_admit(q, op, sw);
        if (ad.flush) {
            std::vector<uint64_t> ta, tw;
            if (op.type == DOP_GEMM1) {
                ta.assign(q.addr.begin() + op.terms, q.addr.end()); tw.assign(q.wt.begin() + op.terms, q.wt.end());
                q.addr.resize(op.terms); q.wt.resize(op.terms);
            }
            flush(ad.flush == DEFER_FLUSH_BOUNDARY);
            if (op.type == DOP_GEMM1) { op.terms = 0; q.addr = ta; q.wt = tw; }
        }
        printf("admit %zu %s level=%d hd=%d flush=%d\n", q.ops.size(), KIND[op.type], ad.level, ad.hd, ad.flush);
        defer_record(q, op, ad);
    }
};

static uint64_t hex(std::istringstream &in) { std::string s; in >> s; return s.empty() ? 0 : std::stoull(s, nullptr, 16); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    std::string line;
    Harness *h = nullptr;
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string w; in >> w;
        if (w.empty()) continue;
        if (w == "program") {
            delete h; h = new Harness();
            std::string name; int device, fold_zero, merge, square; in >> name >> device;
            in >> h->sw.n >> h->sw.ctw2 >> h->sw.t_half >> h->sw.park_max >> fold_zero >> merge >> h->sw.flush_min >> h->sw.max_ops >> h->few_rot >> square;
            h->device = device != 0; h->sw.fold_zero = fold_zero != 0; h->sw.merge_gemm = merge != 0; h->sw.square_gemm = square != 0;
            if (!in) return 3;
            printf("program %s\n", name.c_str());
            continue;
        }
        if (!h) return 3;
        auto ptr = [&]() { return (uint64_t *)(uintptr_t)hex(in); };
        if (w == "end") { h->flush(false); printf("end\n"); continue; }
        if (w == "flush") { std::string how; in >> how; h->flush(how == "boundary"); continue; }
        if (w == "free") {
            uint64_t *base = ptr(); size_t bytes = 0; in >> bytes;
            if (!h->q.ops.empty() || !h->pending.empty()) h->q.frees.emplace_back(base, bytes);      // (cn_defer_pending: else the array goes back at once)
            continue;
        }
        int type = -1;
        for (int t = 0; t < DOP_TYPES; t++) if (w == KIND[t]) type = t;
        if (type < 0) return 3;
        uint64_t *out = ptr();
        DOp op{type, 0, out, nullptr, nullptr, 0, 0, nullptr};
        if (type == DOP_GEMM1) {
            op.terms = h->q.addr.size();
            std::string term;
            while (in >> term) {
                const size_t c = term.find(':');
                if (c == std::string::npos) return 3;
                h->q.addr.push_back(std::stoull(term.substr(0, c), nullptr, 16)); h->q.wt.push_back(std::stoull(term.substr(c + 1)));
                op.K++;
            }
        } else if (type == DOP_ENCRYPT) { op.a = ptr(); in >> op.item; }
        else if (type == DOP_SUMSLOTS) { op.a = out; in >> op.arg; }
        else {
            op.a = ptr();
            if (type != DOP_COPY && type != DOP_COLS && type != DOP_ROT) op.b = ptr();
            if (type == DOP_ROT || type == DOP_ROTADD) in >> op.arg;
        }
        h->push(op);
    }
    delete h;
    return 0;
}
