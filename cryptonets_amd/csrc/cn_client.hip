// libcnhip.so host runtime (3/5): the data owner's side on the device - keys, ChaCha20 sampler, keygen, encrypt, decrypt, noise.
#include "cn_api_shared.h"
#include "cn_k_split.hip.h"          // (includes cn_k_join.hip.h)
#include "cn_noise_table.h"

// ---------------------------------------------------------------- client side on the device
int set_plain_key(cn_ctx *ctx, uint64_t **slot, const uint64_t *words, size_t count, size_t expect, bool is_dev, bool coeff_form) {
    if (!words || count != expect) return fail(CN_ERR_ARG, "key has %zu words, expected %zu", count, expect);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!*slot) HIPCHK(hipMalloc((void **)slot, expect * 8));
    HIPCHK(hipMemcpy(*slot, words, expect * 8, is_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (coeff_form) { CHECK(cn_run_ntt(ctx, *slot, (uint32_t)(expect / ctx->hc.n), 0, ctx->hc.k, 0)); HIPCHK(hipStreamSynchronize(ctx->stream)); }
    return 0;
}
// any key in either representation (include/cnhip.h)
extern "C" int cn_load_key(cn_ctx *ctx, int which, uint64_t elt, const uint64_t *words, size_t count, int is_dev, int form) { API_BODY
    LOCK; NOT_CAPTURING("cn_load_key"); NOT_LEVEL("cn_load_key");
    if (form != 0 && form != 1) return fail(CN_ERR_ARG, "key form must be 0 (NTT) or 1 (coefficients)");
    switch (which) {
        case 0: return set_key(ctx, ctx->rlk, words, count, cn_key_words(ctx, 0), is_dev, form == 1);
        case 1:
            if (!(elt & 1) || elt >= 2ull * ctx->hc.n) return fail(CN_ERR_ARG, "invalid Galois element");
            return set_key(ctx, ctx->gk[elt], words, count, cn_key_words(ctx, 1), is_dev, form == 1);
        case 2: return set_plain_key(ctx, &ctx->pk, words, count, ctx->ctw2, is_dev != 0, form == 1);
        case 3: return set_plain_key(ctx, &ctx->sk, words, count, ctx->ctw2 / 2, is_dev != 0, form == 1);
    }
    return fail(CN_ERR_ARG, "unknown key kind %d", which);
API_END }
extern "C" int cn_set_public_key(cn_ctx *ctx, const uint64_t *words, size_t count) { API_BODY LOCK; NOT_CAPTURING("cn_set_public_key"); NOT_LEVEL("cn_set_public_key"); return set_plain_key(ctx, &ctx->pk, words, count, ctx->ctw2); API_END }
extern "C" int cn_set_secret_key(cn_ctx *ctx, const uint64_t *words, size_t count) { API_BODY LOCK; NOT_CAPTURING("cn_set_secret_key"); NOT_LEVEL("cn_set_secret_key"); return set_plain_key(ctx, &ctx->sk, words, count, ctx->ctw2 / 2); API_END }
// which: 0 relin, 1 galois(elt), 2 public, 3 secret.  Exports u64 residues (FP64-form keys are converted back).
extern "C" int cn_get_key(cn_ctx *ctx, int which, uint64_t elt, uint64_t *host, size_t count) { API_BODY
    LOCK; NOT_CAPTURING("cn_get_key");
    const uint64_t *src = nullptr; size_t words = 0; bool f64 = false;
    if (which == 0) { src = ctx->rlk.d; words = cn_key_words(ctx, 0); f64 = ctx->rlk.f64; }
    else if (which == 1) { auto it = ctx->gk.find(elt); if (it != ctx->gk.end()) { src = it->second.d; f64 = it->second.f64; } words = cn_key_words(ctx, 1); }
    else if (which == 2) { src = ctx->pk; words = ctx->ctw2; }
    else if (which == 3) { src = ctx->sk; words = ctx->ctw2 / 2; }
    if (!src) return fail(CN_ERR_NOKEY, "key not present");
    if (!host || count != words) return fail(CN_ERR_ARG, "key has %zu words", words);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(host, src, words * 8, hipMemcpyDeviceToHost));
    if (f64) for (size_t i = 0; i < words; i++) { double d; memcpy(&d, &host[i], 8); host[i] = (uint64_t)d; }
    return 0;
API_END }
RngKey rng_key_of(const cn_ctx *ctx) { RngKey k; memcpy(k.k, ctx->rng_key, sizeof k.k); return k; }
// thresholds of sample_noise8 (cn_dev_common.hip.h), computed once per process: the formula is in cn_noise_table.h
const NoiseTab &cn_noise_table() {
    static const NoiseTab tab = cn_noise_table_compute();
    return tab;
}
// `polys` polynomials [polys][k][N] of residues: kind 0 ternary, 1 clipped normal (both drawn ONCE per coefficient into an int8 array in
// scratch - the caller's ensure_scratch leaves room for polys * N bytes - and expanded to the k limbs), 2 uniform per limb
int sample_poly(cn_ctx *ctx, uint64_t *dst, uint32_t polys, int kind, uint64_t seed, uint64_t stream) {
    const uint32_t n = ctx->hc.n, k = ctx->hc.k;
    if (n < 16) return fail(CN_ERR_ARG, "device sampling needs N >= 16");
    if (kind == 2) {
        const uint64_t threads = (uint64_t)polys * k * (n / 8);
        hipLaunchKernelGGL(k_sample_uniform, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, dst, ctx->dc, polys, rng_key_of(ctx), seed, (uint32_t)stream, ctx->rng_item);
    } else {
        int8_t *small = salloc<int8_t>(ctx, (size_t)polys * n);
        if (!small) return fail(CN_ERR_HIP, "internal: scratch exhausted in the sampler");
        const uint64_t threads = (uint64_t)polys * (n / (kind == 0 ? 16 : 8));
        hipLaunchKernelGGL(k_sample_small, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, small, n, kind, 1u, polys, rng_key_of(ctx), seed, (uint32_t)stream,
                           ctx->rng_item, (const EncTab *)nullptr, cn_noise_table());
        hipLaunchKernelGGL(k_expand_small, dim3(polys * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, small, dst, ctx->dc, ctx->chunks);
        launch_count(ctx);
    }
    HIPCHK(hipGetLastError()); launch_count(ctx);
    ctx->rng_item += polys;
    return 0;
}
// one key-switch key for the NTT-form target polynomial snew: [(l,d)][2][k][N]
int gen_ksk(cn_ctx *ctx, const uint64_t *snew, int dbc, const uint32_t *dig, uint32_t tot, uint64_t seed, uint64_t *key, uint64_t *e) {
    const uint32_t n = ctx->hc.n, k = ctx->hc.k; const size_t kn = (size_t)k * n;
    uint64_t *p = key;
    for (uint32_t l = 0; l < k; l++) {
        for (uint32_t d = 0; d < dig[l]; d++, p += 2 * kn) {
            CHECK(sample_poly(ctx, p + kn, 1, 2, seed, 3));                 // a: uniform, directly in the NTT domain
            CHECK(sample_poly(ctx, e, 1, 1, seed, 1));
            CHECK(cn_run_ntt(ctx, e, k, 0, k, 0));
            // message term 2^(dbc d) snew in limb l only; "ks_xi": the RNS image of (q/q_l) 2^(dbc d) snew = (q/q_l mod q_l) 2^(dbc d) snew in limb l, zero elsewhere (DevConsts::ks_xi)
            KeyFactors fac{};
            for (uint32_t j = 0; j < k; j++) {
                if (!ctx->hc.ks_xi && j != l) continue;
                const uint64_t qj = ctx->hc.q[j].q; unsigned __int128 f = 1;
                for (uint32_t i = 0; i < d; i++) f = (f << dbc) % qj;
                if (ctx->hc.ks_xi) f = f * ctx->hc.qhat_q[l][j] % qj;
                fac.f[j] = (uint64_t)f;
            }
            hipLaunchKernelGGL(k_key_b, dim3(k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, p + kn, e, ctx->sk, snew, fac, p, ctx->dc, ctx->chunks);
            HIPCHK(hipGetLastError()); launch_count(ctx);
        }
    }
    (void)tot;
    return 0;
}
int adopt_ksk(cn_ctx *ctx, KsKey &slot, uint64_t *dev, size_t words) {          // takes ownership of a device buffer
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (slot.owned && slot.d) HIPCHK(hipFree(slot.d));
    slot = {dev, true, false};
    if (keys_as_f64(ctx)) {
        hipLaunchKernelGGL(k_u64_to_f64, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, ctx->stream, dev, words);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        slot.f64 = true;
    }
    return 0;
}
// sampler key material: the 256-bit ChaCha20 key of every block keygen / encrypt draw from now on (cn_set_rng_salt: its first 64 bits)
extern "C" int cn_set_rng_salt(cn_ctx *ctx, uint64_t salt) { API_BODY LOCK; ctx->rng_key[0] = (uint32_t)salt; ctx->rng_key[1] = (uint32_t)(salt >> 32); return 0; API_END }
// known-answer hook: the generator's block for (key, counter words 12-13, nonce words 14-15) - RFC 7539 section 2.3.2 is reproduced with
// counter = 0x09000000'00000001, nonce = 0x00000000'4a000000 (tests/test_gpu_client.py)
extern "C" int cn_rng_selftest(cn_ctx *ctx, const uint8_t *key32, uint64_t counter, uint64_t nonce, uint32_t *out16) { API_BODY
    LOCK; NOT_CAPTURING("cn_rng_selftest");
    if (!key32 || !out16) return fail(CN_ERR_ARG, "null argument");
    RngKey k; memcpy(k.k, key32, 32);
    CHECK(ensure_scratch(ctx, 256));
    uint32_t *d = salloc<uint32_t>(ctx, 16);
    hipLaunchKernelGGL(k_rng_block, dim3(1), dim3(1), 0, ctx->stream, k, counter, nonce, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out16, d, 64, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
API_END }
extern "C" int cn_set_rng_key(cn_ctx *ctx, const uint8_t *key32) { API_BODY
    LOCK;
    if (!key32) return fail(CN_ERR_ARG, "null argument");
    memcpy(ctx->rng_key, key32, 32);
    return 0;
API_END }
// KeyGenerator (AtomicSealBfvVector.cs:62-74,163-173 runs it inside SEAL): secret, public, relinearisation and the default Galois
// key set (2N-1, 3^(2^i), 3^(-2^i)) generated on the device from the ChaCha20 sampler.
extern "C" int cn_keygen(cn_ctx *ctx, uint64_t seed, int with_galois) { API_BODY
    LOCK; NOT_CAPTURING("cn_keygen"); NOT_LEVEL("cn_keygen");
    const uint32_t n = ctx->hc.n, k = ctx->hc.k; const size_t kn = (size_t)k * n;
    if (!ctx->sk) HIPCHK(hipMalloc((void **)&ctx->sk, kn * 8));
    if (!ctx->pk) HIPCHK(hipMalloc((void **)&ctx->pk, 2 * kn * 8));
    // the sampler carves an N-byte int8 array out of the scratch arena per call and keygen makes ~2 such calls per key digit: room for all of them
    const size_t draws = 4 + 2 * ((size_t)ctx->hc.rl_tot + (with_galois ? (size_t)ctx->hc.gk_tot * (2 * ctx->hc.logn) : 0));
    CHECK(ensure_scratch(ctx, al(kn * 8) * 4 + draws * al(n)));
    uint64_t *e = salloc<uint64_t>(ctx, kn), *snew = salloc<uint64_t>(ctx, kn), *tmp = salloc<uint64_t>(ctx, kn);
    ctx->rng_item = 0;
    CHECK(sample_poly(ctx, ctx->sk, 1, 0, seed, 0));
    CHECK(cn_run_ntt(ctx, ctx->sk, k, 0, k, 0));
    // public key (-(a s + e), a)
    CHECK(sample_poly(ctx, ctx->pk + kn, 1, 2, seed, 3));
    CHECK(sample_poly(ctx, e, 1, 1, seed, 1));
    CHECK(cn_run_ntt(ctx, e, k, 0, k, 0));
    hipLaunchKernelGGL(k_key_b, dim3(k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, ctx->pk + kn, e, ctx->sk, ctx->sk, KeyFactors{}, ctx->pk, ctx->dc, ctx->chunks);
    HIPCHK(hipGetLastError());
    // relinearisation key: target s^2
    hipLaunchKernelGGL(k_mul_limbs, dim3(k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, ctx->sk, ctx->sk, snew, ctx->dc, ctx->chunks);
    HIPCHK(hipGetLastError());
    uint64_t *rl; size_t rlw = cn_key_words(ctx, 0);
    HIPCHK(hipMalloc((void **)&rl, rlw * 8));
    CHECK(gen_ksk(ctx, snew, ctx->hc.dbc, ctx->hc.rl_dig, ctx->hc.rl_tot, seed, rl, e));
    CHECK(adopt_ksk(ctx, ctx->rlk, rl, rlw));
    if (with_galois) {
        const uint64_t m = 2ull * n; std::vector<uint64_t> elts{m - 1};
        uint64_t p3 = 3, ip3 = 0;
        for (uint64_t x = 1; x < m; x += 2) if (((x * 3) & (m - 1)) == 1) { ip3 = x; break; }
        for (uint32_t i = 0; i + 1 < ctx->hc.logn; i++) { elts.push_back(p3); p3 = (p3 * p3) & (m - 1); elts.push_back(ip3); ip3 = (ip3 * ip3) & (m - 1); }
        size_t gw = cn_key_words(ctx, 1);
        for (uint64_t elt : elts) {
            HIPCHK(hipMemcpyAsync(tmp, ctx->sk, kn * 8, hipMemcpyDeviceToDevice, ctx->stream));
            CHECK(cn_run_ntt(ctx, tmp, k, 0, k, 1));
            hipLaunchKernelGGL(k_galois, dim3(k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, tmp, snew, ctx->dc, ctx->chunks, elt);
            HIPCHK(hipGetLastError());
            CHECK(cn_run_ntt(ctx, snew, k, 0, k, 0));
            uint64_t *gk; HIPCHK(hipMalloc((void **)&gk, gw * 8));
            CHECK(gen_ksk(ctx, snew, ctx->hc.gdbc, ctx->hc.gk_dig, ctx->hc.gk_tot, seed, gk, e));
            CHECK(adopt_ksk(ctx, ctx->gk[elt], gk, gw));
        }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
API_END }
// KeyGenerator.GaloisKeys(dbc, galois_elts) (SEAL 3.2): keys for exactly the listed elements, all of them by ONE k_ksk_gen launch behind one noise launch
// (cn_k_keygen.hip.h) - the words cn_keygen's loop would have produced for these elements from the context's item counter on.  One allocation pass, the
// tables of the call in one upload each, one host wait at the end (the keys that are replaced are released behind it).
static uint32_t brev_bits(uint32_t v, uint32_t bits) { uint32_t r = 0; for (uint32_t i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i); return r; }
extern "C" int cn_keygen_galois(cn_ctx *ctx, uint64_t seed, const uint64_t *galois_elts, uint32_t cnt) { API_BODY
    LOCK; NOT_CAPTURING("cn_keygen_galois"); NOT_LEVEL("cn_keygen_galois");
    if (!cnt) return 0;
    if (!galois_elts) return fail(CN_ERR_ARG, "null argument");
    const uint32_t n = ctx->hc.n, k = ctx->hc.k, logn = ctx->hc.logn, tot = ctx->hc.gk_tot;
    if (!cn_rr_size(logn)) return fail(CN_ERR_ARG, "cn_keygen_galois needs 1024 <= N <= 16384");
    for (uint32_t g = 0; g < cnt; g++) {
        if (!(galois_elts[g] & 1) || galois_elts[g] >= 2ull * n) return fail(CN_ERR_ARG, "invalid Galois element %llu", (unsigned long long)galois_elts[g]);
        for (uint32_t h = 0; h < g; h++) if (galois_elts[h] == galois_elts[g]) return fail(CN_ERR_ARG, "Galois element %llu is listed twice", (unsigned long long)galois_elts[g]);
    }
    if (!ctx->sk) return fail(CN_ERR_NOKEY, "secret key not set");
    const uint64_t items = (uint64_t)cnt * tot, item0 = ctx->rng_item;
    if ((item0 + 2 * items) >> 40) return fail(CN_ERR_ARG, "the sampler's item counter would exceed the 40 item bits of the block counter");
    // host tables: NTT-domain automorphism indices per element, message factors per entry (gen_ksk), sampler items of the noise polynomials
    std::vector<uint16_t> perm((size_t)cnt * n), br(n);
    for (uint32_t i = 0; i < n; i++) br[i] = (uint16_t)brev_bits(i, logn);
    for (uint32_t g = 0; g < cnt; g++) for (uint32_t i = 0; i < n; i++) {
        const uint64_t pt = ((2ull * br[i] + 1) * galois_elts[g]) & (2ull * n - 1);
        perm[(size_t)g * n + i] = br[(pt - 1) >> 1];
    }
    std::vector<KeyFactors> fac(tot);
    {
        uint32_t e = 0;
        for (uint32_t l = 0; l < k; l++) for (uint32_t d = 0; d < ctx->hc.gk_dig[l]; d++, e++) {
            KeyFactors f{};
            for (uint32_t j = 0; j < k; j++) {
                if (!ctx->hc.ks_xi && j != l) continue;
                const uint64_t qj = ctx->hc.q[j].q; unsigned __int128 v = 1;
                for (uint32_t i = 0; i < d; i++) v = (v << ctx->hc.gdbc) % qj;
                if (ctx->hc.ks_xi) v = v * ctx->hc.qhat_q[l][j] % qj;
                f.f[j] = (uint64_t)v;
            }
            fac[e] = f;
        }
        if (e != tot) return fail(CN_ERR_ARG, "internal: %u Galois key entries, expected %u", e, tot);
    }
    std::vector<EncTab> nz(items);
    for (uint64_t i = 0; i < items; i++) nz[i] = EncTab{nullptr, nullptr, seed, item0 + 2 * i + 1};
    const size_t gw = cn_key_words(ctx, 1);
    std::vector<uint64_t *> keys(cnt, nullptr);
    auto release = [&]() { for (uint64_t *p : keys) if (p) (void)hipFree(p); };
    for (uint32_t g = 0; g < cnt; g++) if (hipMalloc((void **)&keys[g], gw * 8) != hipSuccess) { (void)hipGetLastError(); release(); return fail(CN_ERR_HIP, "hipMalloc of a Galois key failed"); }
    const int rc = [&]() -> int {
        CHECK(ensure_scratch(ctx, al(items * n) + al(perm.size() * 2) + al(fac.size() * sizeof(KeyFactors)) + al(nz.size() * sizeof(EncTab)) + al(cnt * sizeof(uint64_t *)) + 1024));
        int8_t *noise = salloc<int8_t>(ctx, items * n);
        uint16_t *dperm = nullptr; KeyFactors *dfac = nullptr; EncTab *dnz = nullptr; uint64_t **douts = nullptr;
        if (!noise) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_keygen_galois");
        CHECK(upload_tmp(ctx, perm.data(), perm.size(), &dperm));
        CHECK(upload_tmp(ctx, fac.data(), fac.size(), &dfac));
        CHECK(upload_tmp(ctx, nz.data(), nz.size(), &dnz));
        CHECK(upload_tmp(ctx, keys.data(), keys.size(), &douts));
        hipLaunchKernelGGL(k_sample_small, dim3((unsigned)((items * (n / 8) + 255) / 256)), dim3(256), 0, ctx->stream, noise, n, 1, 1u, (uint32_t)items, rng_key_of(ctx), seed, 1u, item0,
                           (const EncTab *)dnz, cn_noise_table());
        HIPCHK(hipGetLastError()); launch_count(ctx);
        const KskGenArgs a{douts, dfac, dperm, noise, seed, item0, cnt, tot, keys_as_f64(ctx)};
        CHECK(cn_l_ksk_gen(ctx, a));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return 0;
    }();
    if (rc) { (void)hipStreamSynchronize(ctx->stream); release(); return rc; }
    for (uint32_t g = 0; g < cnt; g++) {
        KsKey &slot = ctx->gk[galois_elts[g]];
        if (slot.owned && slot.d) (void)hipFree(slot.d);
        slot = {keys[g], true, keys_as_f64(ctx)};
    }
    ctx->rng_item = item0 + 2 * items;
    return 0;
API_END }
// the Galois elements this context holds a key for, ascending (a level context: the keys sliced from its parent)
extern "C" int cn_galois_elts(cn_ctx *ctx, uint64_t *elts, uint32_t cap, uint32_t *count) { API_BODY
    LOCK_ONLY;
    if (!count) return fail(CN_ERR_ARG, "null argument");
    uint32_t c = 0;
    for (auto &kv : ctx->gk) if (kv.second.d) c++;
    *count = c;
    if (!elts) return 0;
    if (cap < c) return fail(CN_ERR_ARG, "the context holds %u Galois keys, room for %u", c, cap);
    c = 0;
    for (auto &kv : ctx->gk) if (kv.second.d) elts[c++] = kv.first;          // (std::map: ascending)
    return 0;
API_END }
// the RotateRows steps recorded since cn_set_option("record_steps", 1), ascending and distinct; *columns: was a column rotation asked for
extern "C" int cn_rotation_steps(cn_ctx *ctx, int *steps, uint32_t cap, uint32_t *count, int *columns) { API_BODY
    LOCK_ONLY;
    if (!count) return fail(CN_ERR_ARG, "null argument");
    const uint32_t c = (uint32_t)ctx->rec_set.size();
    *count = c;
    if (columns) *columns = ctx->rec_cols ? 1 : 0;
    if (!steps) return 0;
    if (cap < c) return fail(CN_ERR_ARG, "%u steps recorded, room for %u", c, cap);
    uint32_t i = 0;
    for (int s2 : ctx->rec_set) steps[i++] = s2;
    return 0;
API_END }
// Encryptor.Encrypt (AtomicSealBfvVector.cs:1211,1227): (pk0 u + e1 + Delta m [+ r_t(q)], pk1 u + e2); pt = 0 encrypts zero.
// tab != null: `cnt` encryptions whose outputs / plaintexts / nonces / items come from the table (host copy `htab`), else dense out / ptd
// in_arena: the caller has sized the scratch arena for the whole call (encrypt_scratch_bytes) and carved its own arrays out of it: the arena is neither reset nor grown
size_t encrypt_scratch_bytes(const cn_ctx *ctx, uint32_t cnt, bool tab) {
    const size_t n = ctx->hc.n, kn = (size_t)ctx->hc.k * n;
    return al((size_t)cnt * kn * 8) + al((size_t)cnt * n) + al((size_t)cnt * 2 * n) + (tab ? al(cnt * sizeof(EncTab)) : 0) + 1024;
}
int encrypt_chain(cn_ctx *ctx, uint32_t cnt, const uint64_t *ptd, uint32_t pt_stride_words, uint64_t *out, uint64_t seed, const EncTab *htab, bool in_arena) {
    const uint32_t n = ctx->hc.n, k = ctx->hc.k; const size_t kn = (size_t)k * n;
    if (!in_arena) CHECK(ensure_scratch(ctx, encrypt_scratch_bytes(ctx, cnt, htab != nullptr)));
    uint64_t *u = salloc<uint64_t>(ctx, (size_t)cnt * kn);
    int8_t *us = salloc<int8_t>(ctx, (size_t)cnt * n), *es = salloc<int8_t>(ctx, (size_t)cnt * 2 * n);
    EncTab *dtab = nullptr;
    if (htab) CHECK(upload_tmp(ctx, htab, cnt, &dtab));
    if (!u || !us || !es) return fail(CN_ERR_HIP, "internal: scratch exhausted in encrypt");
    const RngKey key = rng_key_of(ctx);
    const uint64_t item0 = ctx->rng_item;
    hipLaunchKernelGGL(k_sample_small, dim3((unsigned)(((uint64_t)cnt * (n / 16) + 255) / 256)), dim3(256), 0, ctx->stream, us, n, 0, 1u, cnt, key, seed, 0u, item0, (const EncTab *)dtab, cn_noise_table());
    hipLaunchKernelGGL(k_sample_small, dim3((unsigned)(((uint64_t)cnt * 2 * (n / 8) + 255) / 256)), dim3(256), 0, ctx->stream, es, n, 1, 2u, cnt, key, seed, 1u, item0, (const EncTab *)dtab, cn_noise_table());
    if (!htab) ctx->rng_item += cnt;
    CnModRange qr = cn_mod_range(ctx->hc, 0, k);
    if (ctx->opt.enc_fused && !ctx->opt.legacy_ntt) {                 // one kernel behind the samplers: u stays in registers between its transform and the two components
        if (rr_ops[cn_policy(qr, ctx->opt.f64)]->enc_fused(ctx, us, ptd, pt_stride_words, out, cnt, es, dtab)) {
            HIPCHK(hipGetLastError()); launch_count(ctx, 3);
            ctx->st.ntt_forward_limbs += (uint64_t)cnt * k;          // (counted like the three-launch chain)
            return 0;
        }
    }
    hipLaunchKernelGGL(k_expand_small, dim3(cnt * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, us, u, ctx->dc, ctx->chunks);
    HIPCHK(hipGetLastError()); launch_count(ctx, 3);
    CHECK(cn_run_ntt(ctx, u, cnt * k, 0, k, 0));
    qr.light = false;                         // k_encrypt_tail exists for ArU64 and ArF64 only (RR_ENC_TAIL is not defined for the f64l unit): a light range takes ArF64 here
    if (!rr_ops[cn_policy(qr, ctx->opt.f64)]->enc_tail(ctx, u, ptd, pt_stride_words, out, cnt, es, dtab)) return fail(CN_ERR_ARG, "unsupported size");
    HIPCHK(hipGetLastError()); launch_count(ctx);
    return 0;
}
extern "C" int cn_encrypt(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t pt_stride, cn_handle out, uint32_t oi, uint32_t count, uint64_t seed) {
    if (submit_async(ctx) && count && count <= 4) return ring_push(ctx, SUB_ENCRYPT, count, 0, 0, pt, pi, out, oi, pt_stride, seed);
    API_BODY LOCK_ONLY; return encrypt_body(ctx, pt, pi, pt_stride, out, oi, count, seed); API_END
}
int encrypt_body(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t pt_stride, cn_handle out, uint32_t oi, uint32_t count, uint64_t seed) {
    NOT_CAPTURING("cn_encrypt (a replayed graph would reuse its randomness)"); GETCT(O, out, 2);
    if (!ctx->pk) return fail(CN_ERR_NOKEY, "public key not set");
    if (!range_ok(O, oi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!cn_rr_size(ctx->hc.logn)) return fail(CN_ERR_ARG, "device encryption needs 1024 <= N <= 16384");
    const uint64_t *ptd = nullptr;
    if (pt) { Buffer *P = getbuf(ctx, pt, 1); if (!P || !range_ok(P, pi, pt_stride ? count : 1, pt_stride ? pt_stride : 1)) return fail(CN_ERR_ARG, "invalid plaintext range"); ptd = P->d + (size_t)pi * ctx->hc.n; }
    if (!count) return 0;
    // per-ciphertext callers (PoolLayer.ElementAt encrypts a zero vector per padded tap, PoolLayer.cs:67-80): queued like the evaluator calls
    if (deferring(ctx) && count <= 4) return defer_encrypt(ctx, ptd, pt_stride ? ctx->hc.n : 0, O, oi, count, seed);
    CHECK(cn_defer_flush(ctx));
    return encrypt_chain(ctx, count, ptd, pt_stride ? ctx->hc.n : 0, O->d + oi * O->item_words, seed, nullptr);
}
// AllocateCiphertext + Encryptor.Encrypt(PlainZero) in ONE call (the unchanged PoolLayer does both per padded convolution tap, PoolLayer.cs:67-80,
// AtomicSealBfvVector.cs:566): one lock acquisition instead of two, same queue entry / same words as cn_ct_alloc followed by cn_encrypt(pt = 0)
extern "C" int cn_encrypt_zero_new(cn_ctx *ctx, uint64_t seed, cn_handle *out) {
    if (out && submit_async(ctx)) {                     // a ready handle + one record (same queue entry as the locked path below)
        const cn_handle h = ctx->ready->pop();
        if (h) { *out = h; return ring_push(ctx, SUB_ENCRYPT_ZERO, 1, 0, 0, 0, 0, h, 0, 0, seed); }
    }
    API_BODY
    LOCK_ONLY; NOT_CAPTURING("cn_encrypt_zero_new (a replayed graph would reuse its randomness)");
    if (!out) return fail(CN_ERR_ARG, "null argument");
    if (!ctx->pk) return fail(CN_ERR_NOKEY, "public key not set");
    if (!cn_rr_size(ctx->hc.logn)) return fail(CN_ERR_ARG, "device encryption needs 1024 <= N <= 16384");
    cn_handle h = 0;
    CHECK(alloc_buf(ctx, 0, 1, 2, &h));
    if (ctx->defer.load(std::memory_order_relaxed) == 2) ready_refill(ctx);          // (the ring of ready handles had run dry)
    Buffer *O = ctx->bufs.find(h);
    int rc;
    if (deferring(ctx)) rc = defer_encrypt(ctx, nullptr, 0, O, 0, 1, seed);
    else { rc = cn_defer_flush(ctx); if (!rc) rc = encrypt_chain(ctx, 1, nullptr, 0, O->d, seed, nullptr); }
    if (rc) { (void)dev_release(ctx, O->d, O->item_words * 8); ctx->bufs.erase(h); return rc; }
    *out = h;
    return 0;
API_END }
template <int K> static void launch_dec_scale(cn_ctx *c, const uint64_t *c0, size_t stride, const uint64_t *acc, uint64_t *plain, uint32_t cnt) {
    hipLaunchKernelGGL(k_decrypt_scale<K>, dim3(cnt * c->chunks), dim3(c->bs), 0, c->stream, c0, stride, acc, plain, c->dc, c->chunks);
}
// acc[ct][j] <- c1 s (+ c2 s^2) in coefficient form: the part of the decryption phase that needs the secret key
// (extra: bytes of scratch the caller carves out behind it)
int decrypt_phase(cn_ctx *ctx, Buffer *I, uint32_t ci, uint32_t count, uint64_t *&acc, size_t extra) {
    const uint32_t n = ctx->hc.n, k = ctx->hc.k; const size_t kn = (size_t)k * n;
    CHECK(ensure_scratch(ctx, al((size_t)count * kn * 8) * 3 + al(kn * 8) + al(extra)));
    acc = salloc<uint64_t>(ctx, (size_t)count * kn);
    uint64_t *tmp = salloc<uint64_t>(ctx, (size_t)count * kn), *sp = salloc<uint64_t>(ctx, kn);
    const uint64_t *base = I->d + ci * I->item_words;
    HIPCHK(hipMemcpy2DAsync(acc, kn * 8, base + kn, I->item_words * 8, kn * 8, count, hipMemcpyDeviceToDevice, ctx->stream));
    CHECK(cn_run_ntt(ctx, acc, count * k, 0, k, 0));
    hipLaunchKernelGGL(k_mul_limbs_bcast, dim3(count * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, acc, ctx->sk, (const uint64_t *)nullptr, acc, ctx->dc, ctx->chunks);
    if (I->size == 3) {
        hipLaunchKernelGGL(k_mul_limbs, dim3(k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, ctx->sk, ctx->sk, sp, ctx->dc, ctx->chunks);
        HIPCHK(hipMemcpy2DAsync(tmp, kn * 8, base + 2 * kn, I->item_words * 8, kn * 8, count, hipMemcpyDeviceToDevice, ctx->stream));
        CHECK(cn_run_ntt(ctx, tmp, count * k, 0, k, 0));
        hipLaunchKernelGGL(k_mul_limbs_bcast, dim3(count * k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, tmp, sp, acc, acc, ctx->dc, ctx->chunks);
    }
    HIPCHK(hipGetLastError()); launch_count(ctx, 2);
    return cn_run_ntt(ctx, acc, count * k, 0, k, 1);
}
// Decryptor.Decrypt (AtomicSealBfvVector.cs:1042,1085): m = round(t (c0 + c1 s + c2 s^2) / q) mod t
extern "C" int cn_decrypt(cn_ctx *ctx, cn_handle ct, uint32_t ci, uint32_t count, cn_handle pt_out, uint32_t pi) { API_BODY
    LOCK; GETCT(I, ct, 0); GETPT(P, pt_out);
    if (!ctx->sk) return fail(CN_ERR_NOKEY, "secret key not set");
    if (!ctx->hc.inv_g_t) return fail(CN_ERR_ARG, "device decryption needs a prime plain modulus");
    if (!range_ok(I, ci, count) || !range_ok(P, pi, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    uint64_t *acc = nullptr;
    CHECK(decrypt_phase(ctx, I, ci, count, acc));
    DISPATCH_K2(launch_dec_scale, ctx, I->d + ci * I->item_words, I->item_words, acc, P->d + (size_t)pi * ctx->hc.n, count);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    for (uint32_t c = 0; c < count; c++) P->pt_zero[pi + c] = 0;      // unknown: treated as non-zero
    return 0;
API_END }
// Decryptor.InvariantNoiseBudget (CryptoTracker.cs:41-52): the residues of t (c0 + c1 s + c2 s^2) mod q, [count][k][N] to the host
extern "C" int cn_noise_poly(cn_ctx *ctx, cn_handle ct, uint32_t ci, uint32_t count, uint64_t *host) { API_BODY
    LOCK; NOT_CAPTURING("cn_noise_poly"); GETCT(I, ct, 0);
    if (!ctx->sk) return fail(CN_ERR_NOKEY, "secret key not set");
    if (!host || !range_ok(I, ci, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    uint64_t *acc = nullptr;
    CHECK(decrypt_phase(ctx, I, ci, count, acc));
    hipLaunchKernelGGL(k_noise_poly, dim3(count * ctx->hc.k * ctx->chunks), dim3(ctx->bs), 0, ctx->stream, I->d + ci * I->item_words, (size_t)I->item_words, acc, ctx->dc, ctx->chunks);
    HIPCHK(hipGetLastError()); launch_count(ctx);
    HIPCHK(hipMemcpyAsync(host, acc, (size_t)count * ctx->hc.k * ctx->hc.n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
API_END }
// The same probe without the N k words per ciphertext on the host: k_noise_norm (cn_k_noise.hip.h) composes the limbs and reduces the centred
// infinity norm on the device, k words per ciphertext.  At most NOISE_CHUNK_WORDS / (k N) ciphertexts per pass: decrypt_phase's scratch
// (3 x pass x k x N words) stays below 384 MiB whatever the count.
static const size_t NOISE_CHUNK_WORDS = (size_t)1 << 24;
extern "C" int cn_noise_norm(cn_ctx *ctx, cn_handle ct, uint32_t ci, uint32_t count, uint64_t *host) { API_BODY
    LOCK; NOT_CAPTURING("cn_noise_norm"); GETCT(I, ct, 0);
    if (!ctx->sk) return fail(CN_ERR_NOKEY, "secret key not set");
    if (!host || !range_ok(I, ci, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    const uint32_t k = ctx->hc.k; const size_t kn = (size_t)k * ctx->hc.n;
    const uint32_t pass = (uint32_t)std::max<size_t>(1, NOISE_CHUNK_WORDS / kn);
    for (uint32_t c = 0; c < count; c += pass) {
        const uint32_t m = std::min(pass, count - c);
        uint64_t *acc = nullptr;
        CHECK(decrypt_phase(ctx, I, ci + c, m, acc, (size_t)m * k * 8));
        uint64_t *norm = salloc<uint64_t>(ctx, (size_t)m * k);
        if (!norm) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_noise_norm");
        CHECK(cn_l_noise_norm(ctx, I->d + (size_t)(ci + c) * I->item_words, I->item_words, acc, norm, m));
        HIPCHK(hipMemcpyAsync(host + (size_t)c * k, norm, (size_t)m * k * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
API_END }
// ---------------------------------------------------------------- seeded symmetric ciphertexts (include/cnhip.h; kernel: cn_k_seeded.hip.h)
// arguments every seeded entry point shares: size-2 ciphertexts, the transform sizes of device encryption, items inside the 40 bits of the block counter
static int seeded_args_ok(cn_ctx *ctx, const Buffer *B, uint32_t first, uint32_t count, const uint8_t *a_seed32, uint64_t a_item0) {
    if (!a_seed32) return fail(CN_ERR_ARG, "null seed");
    if (!range_ok(B, first, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!cn_rr_size(ctx->hc.logn)) return fail(CN_ERR_ARG, "seeded ciphertexts need 1024 <= N <= 16384");
    if (a_item0 >> 40 || (a_item0 + count) >> 40) return fail(CN_ERR_ARG, "a_item0 + count exceeds the 40 item bits of the block counter");
    return 0;
}
static int expand_body(cn_ctx *ctx, Buffer *B, uint32_t first, uint32_t count, const uint8_t *a_seed32, uint64_t a_nonce, uint64_t a_item0) {
    SeededArgs a{B->d + (size_t)first * B->item_words, B->item_words, count, true, a_seed32, a_nonce, a_item0, nullptr, nullptr, 0};
    return cn_l_seeded(ctx, a);
}
// (c0, c1) = (INTT(-a s) + e + Delta m, INTT(a)): a from the PUBLIC seed, e from the context's own sampler key (stream 1, nonce `seed`, the context's item counter)
extern "C" int cn_encrypt_symmetric(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t pt_stride, cn_handle out, uint32_t oi, uint32_t count, uint64_t seed,
                                    const uint8_t *a_seed32, uint64_t a_nonce, uint64_t a_item0) { API_BODY
    LOCK; NOT_CAPTURING("cn_encrypt_symmetric (a replayed graph would reuse its randomness)"); GETCT(O, out, 2);
    if (!ctx->sk) return fail(CN_ERR_NOKEY, "secret key not set");
    CHECK(seeded_args_ok(ctx, O, oi, count, a_seed32, a_item0));
    const uint32_t n = ctx->hc.n;
    const uint64_t *ptd = nullptr;
    if (pt) { Buffer *P = getbuf(ctx, pt, 1); if (!P || !range_ok(P, pi, pt_stride ? count : 1, pt_stride ? pt_stride : 1)) return fail(CN_ERR_ARG, "invalid plaintext range"); ptd = P->d + (size_t)pi * n; }
    if (!count) return 0;
    CHECK(ensure_scratch(ctx, al((size_t)count * n) + 1024));
    int8_t *es = salloc<int8_t>(ctx, (size_t)count * n);
    if (!es) return fail(CN_ERR_HIP, "internal: scratch exhausted in encrypt");
    hipLaunchKernelGGL(k_sample_small, dim3((unsigned)(((uint64_t)count * (n / 8) + 255) / 256)), dim3(256), 0, ctx->stream, es, n, 1, 1u, count, rng_key_of(ctx), seed, 1u, ctx->rng_item,
                       (const EncTab *)nullptr, cn_noise_table());
    HIPCHK(hipGetLastError()); launch_count(ctx);
    ctx->rng_item += count;
    SeededArgs a{O->d + (size_t)oi * O->item_words, O->item_words, count, false, a_seed32, a_nonce, a_item0, es, ptd, pt_stride ? n : 0};
    return cn_l_seeded(ctx, a);
API_END }
extern "C" int cn_ct_expand(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, const uint8_t *a_seed32, uint64_t a_nonce, uint64_t a_item0) { API_BODY
    LOCK; NOT_CAPTURING("cn_ct_expand"); GETCT(B, h, 2);
    CHECK(seeded_args_ok(ctx, B, first, count, a_seed32, a_item0));
    return expand_body(ctx, B, first, count, a_seed32, a_nonce, a_item0);
API_END }
// c0 words [count][k][N] from the host into poly 0 (ONE strided copy), poly 1 from the seed; synchronises like cn_ct_upload (the host array may be reused)
extern "C" int cn_ct_upload_compact(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, const uint64_t *host_c0, const uint8_t *a_seed32, uint64_t a_nonce, uint64_t a_item0) { API_BODY
    LOCK; NOT_CAPTURING("cn_ct_upload_compact"); GETCT(B, h, 2);
    if (!host_c0) return fail(CN_ERR_ARG, "null argument");
    CHECK(seeded_args_ok(ctx, B, first, count, a_seed32, a_item0));
    if (!count) return 0;
    const size_t row = (size_t)ctx->hc.k * ctx->hc.n * 8;
    HIPCHK(hipMemcpy2DAsync(B->d + (size_t)first * B->item_words, B->item_words * 8, host_c0, row, row, count, hipMemcpyHostToDevice, ctx->stream));
    CHECK(expand_body(ctx, B, first, count, a_seed32, a_nonce, a_item0));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
API_END }
extern "C" int cn_ct_download_compact(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint64_t *host_c0) { API_BODY
    LOCK; NOT_CAPTURING("cn_ct_download_compact"); GETCT(B, h, 2);
    if (!host_c0 || !range_ok(B, first, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    const size_t row = (size_t)ctx->hc.k * ctx->hc.n * 8;
    HIPCHK(hipMemcpy2DAsync(host_c0, row, B->d + (size_t)first * B->item_words, B->item_words * 8, row, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
API_END }
// ---------------------------------------------------------------- packed rows (include/cnhip.h; kernels: cn_k_packed.hip.h)
extern "C" size_t cn_packed_words(cn_ctx *ctx, uint32_t polys) { return ctx ? (size_t)polys * cn_packed_row_words(ctx) : 0; }
// polynomials of a packed call on B: `polys` = 0 every polynomial of B, 1 poly 0 alone; 0 = refused
static uint32_t packed_polys(const Buffer *B, uint32_t polys) { return polys == 0 ? B->size : (polys == 1 ? 1u : 0u); }
extern "C" int cn_ct_download_packed(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint32_t polys, uint64_t *host) { API_BODY
    LOCK; NOT_CAPTURING("cn_ct_download_packed"); GETCT(B, h, 0);
    const uint32_t P = packed_polys(B, polys);
    const size_t pw = cn_packed_row_words(ctx);
    if (!P) return fail(CN_ERR_ARG, "polys: 0 (every polynomial) or 1 (c0 only)");
    if (!pw) return fail(CN_ERR_ARG, "packed rows need N >= 1024");
    if (!host || !range_ok(B, first, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    const size_t words = (size_t)count * P * pw;
    CHECK(ensure_scratch(ctx, al(words * 8)));
    uint64_t *stage = salloc<uint64_t>(ctx, words);
    if (!stage) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_ct_download_packed");
    CHECK(cn_l_pack_rows(ctx, B->d + (size_t)first * B->item_words, B->item_words, stage, count, P));
    HIPCHK(hipMemcpyAsync(host, stage, words * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return 0;
API_END }
extern "C" int cn_ct_upload_packed(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint32_t polys, const uint64_t *host,
                                   const uint8_t *a_seed32, uint64_t a_nonce, uint64_t a_item0) { API_BODY
    LOCK; NOT_CAPTURING("cn_ct_upload_packed"); GETCT(B, h, polys == 1 ? 2 : 0);
    const uint32_t P = packed_polys(B, polys);
    const size_t pw = cn_packed_row_words(ctx);
    if (!P) return fail(CN_ERR_ARG, "polys: 0 (every polynomial) or 1 (c0 only, c1 from the seed)");
    if (!pw) return fail(CN_ERR_ARG, "packed rows need N >= 1024");
    if (!host) return fail(CN_ERR_ARG, "null argument");
    if (polys == 1) CHECK(seeded_args_ok(ctx, B, first, count, a_seed32, a_item0));
    else if (!range_ok(B, first, count)) return fail(CN_ERR_ARG, "index out of range");
    if (!count) return 0;
    const size_t words = (size_t)count * P * pw;
    CHECK(ensure_scratch(ctx, al(words * 8) + 256));
    uint64_t *stage = salloc<uint64_t>(ctx, words);
    uint32_t *flag = salloc<uint32_t>(ctx, 1);
    if (!stage || !flag) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_ct_upload_packed");
    HIPCHK(hipMemcpyAsync(stage, host, words * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(flag, 0, 4, ctx->stream));
    CHECK(cn_l_unpack_rows(ctx, stage, B->d + (size_t)first * B->item_words, B->item_words, count, P, flag));
    if (polys == 1) CHECK(expand_body(ctx, B, first, count, a_seed32, a_nonce, a_item0));
    uint32_t seen = 0;
    HIPCHK(hipMemcpyAsync(&seen, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (seen) { ctx->packed_bad++; return fail(CN_ERR_ARG, "residue not below its modulus"); }
    return 0;
API_END }
// ---------------------------------------------------------------- the reply path (include/cnhip.h: cn_decrypt_join; kernels: cn_k_join.hip.h)
// The constants of a list of contexts: CN_ERR_ARG unless cn_decrypt_join accepts the list (the checks that need no lock: N, device, t are fixed at creation)
static int join_tab_of(cn_ctx *const *ctxs, uint32_t P, uint32_t flags, double scale, JoinTab &T) {
    if (!ctxs || P < 1 || P > CNJ_MAXP) return fail(CN_ERR_ARG, "cn_decrypt_join takes 1 .. %d contexts", CNJ_MAXP);
    uint64_t t[CNJ_MAXP];
    for (uint32_t i = 0; i < P; i++) {
        if (!ctxs[i]) return fail(CN_ERR_ARG, "null context at position %u", i);
        if (ctxs[i]->hc.n != ctxs[0]->hc.n || ctxs[i]->device != ctxs[0]->device) return fail(CN_ERR_ARG, "cn_decrypt_join: context %u has another N or device", i);
        if (!ctxs[i]->hc.inv_g_t) return fail(CN_ERR_ARG, "device decryption needs a prime plain modulus");
        t[i] = ctxs[i]->hc.t.q;
        for (uint32_t h = 0; h < i; h++) if (t[h] == t[i]) return fail(CN_ERR_ARG, "cn_decrypt_join: contexts %u and %u have the same plain modulus", h, i);
    }
    if (cnj_build_tab(t, P, flags, scale, &T)) return fail(CN_ERR_ARG, "cn_decrypt_join: the product of the plain moduli must stay below 2^255");
    return 0;
}
extern "C" int cn_join_words(cn_ctx *const *ctxs, uint32_t P) {
    JoinTab T;
    CHECK(join_tab_of(ctxs, P, 0, 1.0, T));
    return (int)T.W;
}
static bool join_lock_order(const cn_ctx *x, const cn_ctx *y) { return x->hc.k != y->hc.k ? x->hc.k > y->hc.k : x < y; }      // as cn_mod_switch takes two (cn_level.hip)
static int decrypt_join_locked(cn_ctx *const *ctxs, const JoinTab &T, const cn_handle *ct, const uint32_t *ci, uint32_t count, uint32_t nslots,
                               double *values, uint64_t *words, int32_t *argmax) {
    const uint32_t P = T.P, W = T.W, n = ctxs[0]->hc.n;
    const bool dense = !(T.flags & CNJ_COEFF0);
    for (uint32_t i = 0; i < P; i++) { cn_ctx *ctx = ctxs[i]; NOT_CAPTURING("cn_decrypt_join"); }
    // not deferrable: every context's queued calls and published records are submitted first (a handle may come from the lock-free ring)
    for (uint32_t i = 0; i < P; i++) CHECK(flush_all(ctxs[i]));
    Buffer *I[CNJ_MAXP];
    for (uint32_t i = 0; i < P; i++) {
        cn_ctx *ctx = ctxs[i];
        GETCT(B, ct[i], 0);
        if (B->size != 2 && B->size != 3) return fail(CN_ERR_ARG, "cn_decrypt_join: ciphertexts of size 2 or 3");
        if (!range_ok(B, ci ? ci[i] : 0, count)) return fail(CN_ERR_ARG, "index out of range");
        if (!ctx->sk) return fail(CN_ERR_NOKEY, "secret key not set");
        I[i] = B;
    }
    if (!count) return 0;
    cn_ctx *c0 = ctxs[0];
    for (uint32_t i = 0; i < P; i++) if (!ctxs[i]->ev_ms) { CHECK(use(ctxs[i])); HIPCHK(hipEventCreateWithFlags(&ctxs[i]->ev_ms, hipEventDisableTiming)); }
    CHECK(use(c0));
    if (dense) CHECK(ensure_index_map(c0));                   // (the slot order depends on N alone)
    // the arena of the call, in ctxs[0]'s scratch behind the arrays of its own decryption: plaintexts [P][count][N], the constants, the outputs.
    // The other contexts write their slice from their own streams: they start behind whatever ctxs[0]'s stream still runs on that memory.
    HIPCHK(hipEventRecord(c0->ev_ms, c0->stream));
    const size_t slice = (size_t)count * n, total = (size_t)count * nslots;
    const bool want_words = words || argmax;
    const size_t vbytes = values ? total * 8 : 0, wbytes = want_words ? total * W * 8 : 0, abytes = argmax ? (size_t)nslots * 4 : 0;
    uint64_t *plain = nullptr, *dwords = nullptr; JoinTab *dtab = nullptr; double *dvalues = nullptr; int32_t *dargmax = nullptr;
    for (uint32_t i = 0; i < P; i++) {
        cn_ctx *ctx = ctxs[i];
        CHECK(use(ctx));
        if (i && ctx->stream != c0->stream) HIPCHK(hipStreamWaitEvent(ctx->stream, c0->ev_ms, 0));
        uint64_t *acc = nullptr;
        const uint32_t first = ci ? ci[i] : 0;
        CHECK(decrypt_phase(ctx, I[i], first, count, acc, i ? 0 : al(P * slice * 8) + al(sizeof(JoinTab)) + al(vbytes) + al(wbytes) + al(abytes)));
        if (!i) {
            plain = salloc<uint64_t>(ctx, P * slice);
            CHECK(upload_tmp(ctx, &T, 1, &dtab));
            if (vbytes) dvalues = (double *)salloc<char>(ctx, vbytes);
            if (wbytes) dwords = (uint64_t *)salloc<char>(ctx, wbytes);
            if (abytes) dargmax = (int32_t *)salloc<char>(ctx, abytes);
            if (!plain || (vbytes && !dvalues) || (wbytes && !dwords) || (abytes && !dargmax)) return fail(CN_ERR_HIP, "internal: scratch exhausted in cn_decrypt_join");
        }
        uint64_t *mine = plain + (size_t)i * slice;
        DISPATCH_K2(launch_dec_scale, ctx, I[i]->d + first * I[i]->item_words, I[i]->item_words, acc, mine, count);
        HIPCHK(hipGetLastError()); launch_count(ctx);
        if (dense) CHECK(cn_run_ntt(ctx, mine, count, ctx->hc.k + ctx->hc.kb, 1, 0));     // the forward transform mod t of cn_decode_batch
        if (i && ctx->stream != c0->stream) {                                             // ctxs[0]'s stream waits for this slice
            HIPCHK(hipEventRecord(ctx->ev_ms, ctx->stream));
            HIPCHK(hipStreamWaitEvent(c0->stream, ctx->ev_ms, 0));
        }
    }
    CHECK(use(c0));
    CHECK(cn_l_crt_join(c0, plain, c0->d_index_map, dtab, P, W, dvalues, dwords, count, nslots));
    if (argmax) CHECK(cn_l_join_argmax(c0, dwords, W, dargmax, count, nslots));
    if (values) HIPCHK(hipMemcpyAsync(values, dvalues, vbytes, hipMemcpyDeviceToHost, c0->stream));
    if (words) HIPCHK(hipMemcpyAsync(words, dwords, wbytes, hipMemcpyDeviceToHost, c0->stream));
    if (argmax) HIPCHK(hipMemcpyAsync(argmax, dargmax, abytes, hipMemcpyDeviceToHost, c0->stream));
    // the one host wait of the call: ctxs[0]'s stream has waited for every other stream's slice, so nothing of the call is in flight on any of them afterwards
    HIPCHK(hipStreamSynchronize(c0->stream));
    return 0;
}
extern "C" int cn_decrypt_join(cn_ctx *const *ctxs, uint32_t P, const cn_handle *ct, const uint32_t *ci, uint32_t count, uint32_t nslots, uint32_t flags, double scale,
                               double *values, uint64_t *words, int32_t *argmax) {
    JoinTab T;
    CHECK(join_tab_of(ctxs, P, flags, scale, T));
    if (flags & ~(CNJ_SIGNED | CNJ_COEFF0)) return fail(CN_ERR_ARG, "cn_decrypt_join: unknown flag");
    if (!ct) return fail(CN_ERR_ARG, "null argument");
    if (!values && !words && !argmax) return fail(CN_ERR_ARG, "cn_decrypt_join: no output asked for");
    if (nslots == 0 || nslots > ctxs[0]->hc.n) return fail(CN_ERR_ARG, "cn_decrypt_join: 1 .. N slots");
    if ((flags & CNJ_COEFF0) && nslots != 1) return fail(CN_ERR_ARG, "cn_decrypt_join: CN_JOIN_COEFF0 reads one coefficient (nslots = 1)");
    if (!(flags & CNJ_COEFF0)) for (uint32_t i = 0; i < P; i++) if (!ctxs[i]->hc.batching) return fail(CN_ERR_ARG, "plain modulus does not support batching");
    // every lock, in the order cn_mod_switch takes two (more limbs first): calls over one set of contexts cannot deadlock
    std::vector<cn_ctx *> order(ctxs, ctxs + P);
    std::sort(order.begin(), order.end(), join_lock_order);
    HeldLocks locks(order);
    return decrypt_join_locked(ctxs, T, ct, ci, count, nslots, values, words, argmax);
}
// ---------------------------------------------------------------- the request path (include/cnhip.h: cn_split_encode / cn_split_encrypt; kernel: cn_k_split.hip.h)
struct SplitCall {
    const char *what; const void *values; int64_t stride_ct, stride_slot; uint32_t count, nvalues, flags; double scale;
    const cn_handle *h; const uint32_t *first; const uint64_t *seeds; uint8_t *zero; bool encrypt;
};
// the checks that need no lock (N, device and t are fixed at creation)
static int split_args_ok(cn_ctx *const *ctxs, uint32_t P, const SplitCall &a) {
    if (!ctxs || P < 1 || P > CNJ_MAXP) return fail(CN_ERR_ARG, "%s takes 1 .. %d contexts", a.what, CNJ_MAXP);
    for (uint32_t i = 0; i < P; i++) {
        if (!ctxs[i]) return fail(CN_ERR_ARG, "null context at position %u", i);
        if (ctxs[i]->hc.n != ctxs[0]->hc.n || ctxs[i]->device != ctxs[0]->device) return fail(CN_ERR_ARG, "%s: context %u has another N or device", a.what, i);
        for (uint32_t h = 0; h < i; h++) if (ctxs[h] == ctxs[i]) return fail(CN_ERR_ARG, "%s: context %u is listed twice", a.what, i);
        if (ctxs[i]->hc.t.q < 2 || (ctxs[i]->hc.t.q >> 62)) return fail(CN_ERR_ARG, "%s: plain modulus outside [2, 2^62)", a.what);
    }
    if (a.flags & ~(CSP_I64 | CSP_COEFF0)) return fail(CN_ERR_ARG, "%s: unknown flag", a.what);
    if (!a.values || !a.h || (a.encrypt && !a.seeds)) return fail(CN_ERR_ARG, "null argument");
    const uint32_t n = ctxs[0]->hc.n;
    if (a.flags & CSP_COEFF0) { if (a.nvalues != 1) return fail(CN_ERR_ARG, "%s: CN_SPLIT_COEFF0 writes one coefficient (nvalues = 1)", a.what); }
    else {
        if (a.nvalues == 0 || a.nvalues > n) return fail(CN_ERR_ARG, "%s: 1 .. N values per plaintext", a.what);
        for (uint32_t i = 0; i < P; i++) if (!ctxs[i]->hc.batching) return fail(CN_ERR_ARG, "plain modulus does not support batching");
    }
    if (a.encrypt && !cn_rr_size(ctxs[0]->hc.logn)) return fail(CN_ERR_ARG, "device encryption needs 1024 <= N <= 16384");
    return 0;
}
// elements [lo, hi] of `values` that the plaintexts [cb, cb + m) read
static void split_extent(const SplitCall &a, uint32_t cb, uint32_t m, __int128 &lo, __int128 &hi) {
    const __int128 c0 = (__int128)cb * a.stride_ct, c1 = (__int128)(cb + m - 1) * a.stride_ct, s1 = (__int128)(a.nvalues - 1) * a.stride_slot;
    lo = std::min(c0, c1) + std::min<__int128>(0, s1);
    hi = std::max(c0, c1) + std::max<__int128>(0, s1);
}
static int split_locked(cn_ctx *const *ctxs, uint32_t P, const SplitCall &a) {
    const uint32_t n = ctxs[0]->hc.n, count = a.count;
    const bool dense = !(a.flags & CSP_COEFF0);
    for (uint32_t i = 0; i < P; i++) { cn_ctx *ctx = ctxs[i]; NOT_CAPTURING("cn_split_encode / cn_split_encrypt"); }
    // not deferrable: every context's queued calls and published records are submitted first (a handle may come from the lock-free ring)
    for (uint32_t i = 0; i < P; i++) CHECK(flush_all(ctxs[i]));
    Buffer *B[CNJ_MAXP]; uint32_t first[CNJ_MAXP]; uint64_t t[CNJ_MAXP];
    for (uint32_t i = 0; i < P; i++) {
        cn_ctx *ctx = ctxs[i];
        Buffer *b = getbuf(ctx, a.h[i], a.encrypt ? 0 : 1);
        if (!b) return fail(CN_ERR_ARG, "%s: invalid handle at position %u", a.what, i);
        if (a.encrypt && b->size != 2) return fail(CN_ERR_ARG, "%s: fresh ciphertexts have size 2", a.what);
        first[i] = a.first ? a.first[i] : 0;
        if (!range_ok(b, first[i], count)) return fail(CN_ERR_ARG, "index out of range");
        B[i] = b; t[i] = ctx->hc.t.q;
    }
    if (a.encrypt) for (uint32_t i = 0; i < P; i++) if (!ctxs[i]->pk) return fail(CN_ERR_NOKEY, "public key not set");
    if (!count) return 0;
    // passes of at most max(1, 2^24 / N) plaintexts (and of one launch's grid): the arenas stay bounded whatever the count
    const uint32_t pass = (uint32_t)std::min<size_t>(std::max<size_t>(1, NOISE_CHUNK_WORDS / n), 65536), mp = std::min(pass, count);
    size_t stage_bytes = 0;
    for (uint32_t cb = 0; cb < count; cb += pass) {
        __int128 lo, hi; split_extent(a, cb, std::min(pass, count - cb), lo, hi);
        if (hi - lo >= ((__int128)1 << 40)) return fail(CN_ERR_ARG, "%s: the strides span more than 2^40 elements in one pass", a.what);
        stage_bytes = std::max(stage_bytes, (size_t)(hi - lo + 1) * 8);
    }
    cn_ctx *c0 = ctxs[0];
    for (uint32_t i = 0; i < P; i++) if (!ctxs[i]->ev_ms) { CHECK(use(ctxs[i])); HIPCHK(hipEventCreateWithFlags(&ctxs[i]->ev_ms, hipEventDisableTiming)); }
    CHECK(use(c0));
    if (dense) CHECK(ensure_index_map(c0));                   // (the slot order depends on N alone)
    // the arenas of the call.  ctxs[0]: the flags of every pass, then per pass the staged values; every context of cn_split_encrypt: per pass its plaintexts and the
    // arrays of its own encryption.  Sized once for the largest pass, so no arena moves while another stream works in it.
    const size_t flag_words = (size_t)P * count + 1;
    size_t mark[CNJ_MAXP];
    for (uint32_t i = 0; i < P; i++) {
        const size_t own = a.encrypt ? al((size_t)mp * n * 8) + encrypt_scratch_bytes(ctxs[i], mp, false) : 0;
        if (i == 0 || own) { CHECK(use(ctxs[i])); CHECK(ensure_scratch(ctxs[i], own + (i ? 0 : al(flag_words * 4) + al(stage_bytes) + 256))); }
        mark[i] = ctxs[i]->soff;
    }
    uint32_t *dflags = salloc<uint32_t>(c0, flag_words);      // nz [P][count], then the range flag
    if (!dflags) return fail(CN_ERR_HIP, "internal: scratch exhausted in %s", a.what);
    mark[0] = c0->soff;
    uint32_t *dbad = dflags + (size_t)P * count;
    std::vector<uint32_t> hflags(flag_words);
    const int rc = [&]() -> int {
        CHECK(use(c0));
        HIPCHK(hipMemsetAsync(dflags, 0, flag_words * 4, c0->stream));
        for (uint32_t cb = 0; cb < count; cb += pass) {
            const uint32_t m = std::min(pass, count - cb);
            __int128 lo, hi; split_extent(a, cb, m, lo, hi);
            uint64_t *plain[CNJ_MAXP];
            for (uint32_t i = 0; i < P; i++) {
                cn_ctx *ctx = ctxs[i];
                ctx->soff = mark[i];
                plain[i] = a.encrypt ? salloc<uint64_t>(ctx, (size_t)m * n) : B[i]->d + (size_t)(first[i] + cb) * n;
                if (!plain[i]) return fail(CN_ERR_HIP, "internal: scratch exhausted in %s", a.what);
                // ctxs[0]'s stream writes this context's rows: behind whatever the context's own stream still runs on them
                if (i && ctx->stream != c0->stream) { CHECK(use(ctx)); HIPCHK(hipEventRecord(ctx->ev_ms, ctx->stream)); HIPCHK(hipStreamWaitEvent(c0->stream, ctx->ev_ms, 0)); }
            }
            CHECK(use(c0));
            const size_t bytes = (size_t)(hi - lo + 1) * 8;
            char *stage = salloc<char>(c0, bytes);
            if (!stage) return fail(CN_ERR_HIP, "internal: scratch exhausted in %s", a.what);
            HIPCHK(hipMemcpyAsync(stage, (const char *)a.values + (int64_t)lo * 8, bytes, hipMemcpyHostToDevice, c0->stream));
            const void *dvalues = (const void *)((intptr_t)stage - (intptr_t)((int64_t)lo * 8));          // element (c, s) at dvalues[c stride_ct + s stride_slot]
            CHECK(cn_l_crt_split(c0, (const char *)dvalues + (int64_t)cb * a.stride_ct * 8, a.stride_ct, a.stride_slot, m, a.nvalues, a.flags, a.scale, t, plain, P,
                                 dense ? c0->d_index_map : nullptr, dflags + cb, count, dbad));
            HIPCHK(hipEventRecord(c0->ev_ms, c0->stream));
            for (uint32_t i = 0; i < P; i++) {
                cn_ctx *ctx = ctxs[i];
                const bool other = i && ctx->stream != c0->stream;
                CHECK(use(ctx));
                if (other) HIPCHK(hipStreamWaitEvent(ctx->stream, c0->ev_ms, 0));
                if (dense) CHECK(cn_run_ntt(ctx, plain[i], m, ctx->hc.k + ctx->hc.kb, 1, 1));          // the inverse transform mod t of cn_encode_batch
                if (a.encrypt) CHECK(encrypt_chain(ctx, m, plain[i], n, B[i]->d + (size_t)(first[i] + cb) * B[i]->item_words, a.seeds[i], nullptr, true));
                // ctxs[0]'s stream waits for this context: the next pass reuses the arenas, and the call ends with one wait on that stream
                if (other) { HIPCHK(hipEventRecord(ctx->ev_ms, ctx->stream)); HIPCHK(hipStreamWaitEvent(c0->stream, ctx->ev_ms, 0)); }
            }
        }
        CHECK(use(c0));
        HIPCHK(hipMemcpyAsync(hflags.data(), dflags, flag_words * 4, hipMemcpyDeviceToHost, c0->stream));
        HIPCHK(hipStreamSynchronize(c0->stream));              // the one host wait of the call
        return 0;
    }();
    if (rc) { for (uint32_t i = 0; i < P; i++) (void)hipStreamSynchronize(ctxs[i]->stream); return rc; }          // nothing of the call stays in flight on any stream
    for (uint32_t i = 0; i < P; i++) for (uint32_t c = 0; c < count; c++) {
        const uint8_t z = hflags[(size_t)i * count + c] ? 0 : 1;
        if (!a.encrypt) B[i]->pt_zero[first[i] + c] = z;
        if (a.zero) a.zero[(size_t)i * count + c] = z;
    }
    if (hflags[(size_t)P * count]) return fail(CN_ERR_ARG, "%s: value does not fit (NaN, infinite or 2^62 and beyond after scaling)", a.what);
    return 0;
}
static int split_call(cn_ctx *const *ctxs, uint32_t P, const SplitCall &a) {
    CHECK(split_args_ok(ctxs, P, a));
    std::vector<cn_ctx *> order(ctxs, ctxs + P);
    std::sort(order.begin(), order.end(), join_lock_order);      // every lock, in cn_decrypt_join's order
    HeldLocks locks(order);
    return split_locked(ctxs, P, a);
}
extern "C" int cn_split_encode(cn_ctx *const *ctxs, uint32_t P, const void *values, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues, uint32_t flags,
                               double scale, const cn_handle *pt, const uint32_t *pi, uint8_t *zero) {
    return split_call(ctxs, P, SplitCall{"cn_split_encode", values, stride_ct, stride_slot, count, nvalues, flags, scale, pt, pi, nullptr, zero, false});
}
extern "C" int cn_split_encrypt(cn_ctx *const *ctxs, uint32_t P, const void *values, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues, uint32_t flags,
                                double scale, const cn_handle *ct, const uint32_t *ci, const uint64_t *seeds) {
    return split_call(ctxs, P, SplitCall{"cn_split_encrypt", values, stride_ct, stride_slot, count, nvalues, flags, scale, ct, ci, seeds, nullptr, true});
}
