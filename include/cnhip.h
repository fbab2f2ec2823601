/*
 * cnhip.h -- C ABI of libcnhip.so: the MI355X-native BFV evaluator that replaces the
 * SEAL 3.2 native calls issued by microsoft/CryptoNets' AtomicSealBfvEncryptedVector.
 *
 * Boundary being replaced: the managed->native P/Invoke layer inside SEALNet.dll
 * (NuGet Microsoft.Research.SEALNet 3.2.0, `HE Wrapper/packages.config:6`), reached only
 * from `HE Wrapper/AtomicSealBfvVector.cs` through `epenv.evaluator.*`.  Each entry point
 * below cites the reference call sites (file:line under /root/reference) it serves.
 *
 * Conventions:
 *  - plain C, opaque context pointer + 64-bit buffer handles, no C++/torch types;
 *  - every function returns 0 on success, <0 on error; cn_last_error() returns a
 *    thread-local message (the reference throws .NET exceptions at the same points);
 *  - all functions are thread-safe (one mutex per context: the reference calls from
 *    Defaults.ThreadCount threads, `HE Wrapper/Utils.cs:46-88`);
 *  - work is enqueued on the context's HIP stream; results are ordered; host reads
 *    (cn_ct_download) synchronise; cn_sync() waits for everything;
 *  - BATCHED BY CONSTRUCTION: a buffer handle is an ARRAY of ciphertexts (or dense
 *    plaintexts); every op takes (handle, first index, count), so one layer is a handful
 *    of launches instead of 10^5 P/Invokes.  count==1 is the per-ciphertext SEAL call.
 *  - ciphertext layout = SEAL's: [poly][limb][N] u64 canonical residues, coefficient
 *    form; plaintext = N u64 coefficients mod t; keys = NTT form (bit-reversed order):
 *    key-switch key = for limb l, digit d (low->high): [2][k][N], flattened in (l,d) order.
 */
#ifndef CNHIP_H
#define CNHIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cn_ctx cn_ctx;
typedef uint64_t cn_handle;

#define CN_OK 0
#define CN_ERR_ARG (-1)      /* bad argument / shape mismatch (reference: `throw new Exception(...)`) */
#define CN_ERR_HIP (-2)      /* HIP runtime failure */
#define CN_ERR_NOKEY (-3)    /* relin / Galois key missing (SEAL: "Galois key not present") */
#define CN_ERR_ZERO (-4)     /* multiply_plain by an all-zero plaintext (SEAL: "plain cannot be zero") */
#define CN_ERR_NODEV (-5)    /* no HIP device available */
#define CN_STREAM_A (4)      /* sampler stream of the public `a` of seeded symmetric ciphertexts (cn_encrypt_symmetric, cn_ct_expand); 0-3 are the keys' and the noise's */

int cn_version(void);
const char *cn_last_error(void);
int cn_device_count(void);

/* ---- context = AtomicSealBfvEncryptedEnvironment (AtomicSealBfvVector.cs:19-74,140-173):
 * (n, coeff moduli q[k], plain modulus t, DecompositionBitCount, GaloisDecompositionBitCount).  n a power of two up to 16384; every q_j a
 * distinct prime with t < q_j < 2^60 (at most 60 bits, as SEAL 3.2 allows: the 61-bit primes are SEAL's m_sk, gamma and auxiliary base) and
 * q_j == 1 (mod 2n); 1 <= dbc, gdbc <= 60.  Otherwise CN_ERR_ARG and no context. */
int cn_ctx_create(uint32_t n, const uint64_t *q, uint32_t k, uint64_t t, int dbc, int gdbc,
                  int device, cn_ctx **out);
int cn_ctx_destroy(cn_ctx *ctx);      /* CN_ERR_ARG for a member of a recording or a live graph across levels (cn_graph_begin_levels) */
int cn_sync(cn_ctx *ctx);
/* Ordering between contexts without a host wait: everything submitted to `ctx` AFTER this call starts only when everything submitted to
 * `other` BEFORE it has finished (an event on other's stream that ctx's stream waits for; same or different device).  The plaintext-prime
 * channels of one vector are independent contexts (EncryptedSealBfvVector.cs:225-236); a host that issues them from one thread uses this to
 * stagger them - the FP64-bound key switch of one channel then runs beside the HBM-bound layers of the other instead of beside its twin
 * (bench.py --stagger).  Neither context is synchronised with the host. */
int cn_ctx_wait_for(cn_ctx *ctx, cn_ctx *other);
/* ---- modulus switching = Evaluator.ModSwitchToNext(Inplace) / ModSwitchTo (SEAL 3.2 evaluator.h: mod_switch_scale_to_next; the reference
 * never calls it - AtomicSealBfvVector.cs keeps every ciphertext at the first level).  SEAL 3.2 has no special prime: the chain is
 * q[0..k), q[0..k-1), ..., q[0..1).
 * cn_ctx_create_level: a LEVEL CONTEXT over q[0..limbs), 1 <= limbs < k: the parent's N, t, dbc, gdbc, device and settled options ("f64", "ks_xi",
 * "legacy_ntt", the kernel switches; not "defer"), its own stream and tables (transforms, BEHZ, decryption), and a slice of every key the parent holds
 * at the time of the call - relinearisation and Galois keys: entries (l, d) with l < limbs, the first `limbs` limbs of both polynomials; public and
 * secret key: the first `limbs` limbs (device-to-device copies, one per key).  It owns its keys and outlives its parent; a level of a level context
 * works (a chain).  Under "ks_xi" = 1 it decomposes xi_l = [c_l (Q/q_l)^-1]_{q_l} with the chain's TOP modulus Q, which its sliced keys carry.
 * cn_keygen, cn_set_relin_key, cn_set_galois_key, cn_load_key, cn_set_public_key, cn_set_secret_key and changing "ks_xi" return CN_ERR_ARG on it
 * (SEAL 3.2 generates keys at the first level only).
 * ONE-LIMB CONTEXTS (a level of 1, or cn_ctx_create with k = 1) run the linear operations, plaintext products, scalar GEMMs, encryption,
 * decryption and cn_noise_poly.  cn_multiply, cn_relinearize, cn_mul_relin and every rotation (cn_apply_galois, cn_rotate_rows(_many,_add),
 * cn_rotate_columns(_add), cn_sum_slots, cn_rowdot_batch) return CN_ERR_ARG there. */
int cn_ctx_create_level(cn_ctx *parent, uint32_t limbs, cn_ctx **out);
/* out[oi + i] = ModSwitchTo(in[ii + i], level of dst), i < count: k_src - k_dst successive drops of the last prime with rounding,
 * x' = floor((x + floor(q_last / 2)) / q_last) mod Q' per coefficient (x = CRT value), as SEAL's mod_switch_to loops.  Size-2 and size-3
 * ciphertexts (both handles the same size).  dst must be on the chain of src: same device, N and t, q_dst a strict prefix of q_src, the same
 * key-switch convention (and under "ks_xi" = 1 a level of src's chain).  Otherwise, and for bad handles or ranges, or while either context records a
 * graph unless both belong to one recording across levels (cn_graph_begin_levels: the switch is then recorded): CN_ERR_ARG and no switch is
 * enqueued, `out` is not written.  Not deferrable: takes both context locks (more limbs first) and submits both
 * contexts' queued calls first - also when the handle or range checks then refuse the call (handles may come from the lock-free ring, "defer" = 2);
 * the context checks (chain, capture) refuse before anything is submitted.  Ordering without a host wait (events): the switch reads `in` after the work submitted to src before the call, writes `out` after
 * the work submitted to dst before it; later dst calls see the result, later src calls wait for the read.
 * Arithmetic: with "f64" on (both contexts) and every modulus of src below 2^49, the drops run in exact FP64 (k_mod_switch_f64) for the
 * (k_src, k_dst) pairs where that form measured faster - switches of two or more primes; otherwise, and under "f64" = 0 / CN_NO_F64=1, in
 * 64-bit integers (k_mod_switch).  Both produce the same words; cn_get_option "mod_switch_f64" tells which ran last. */
int cn_mod_switch(cn_ctx *src, cn_handle in, uint32_t ii, uint32_t count, cn_ctx *dst, cn_handle out, uint32_t oi);
/* Options of a context.  The tuning switches (A/B testing) all produce identical words.  cn_set_option refuses an unknown name, and a value
 * outside the range of an enumerated switch, with CN_ERR_ARG and keeps the old value; a flag takes any value, non-zero = on.  An environment
 * override is read when the context is created (a value out of range is clamped).  A level context takes its parent's values.
 *
 *   name             values  default               environment      what it selects
 *   "f64"            flag    1                     CN_NO_F64=1: 0   transforms of moduli < 2^49 and key switching in exact FP64; 0 = the integer
 *                                                                   Shoup path everywhere.  Set it BEFORE uploading keys
 *   "legacy_ntt"     flag    0                     CN_LEGACY_NTT    the radix-2 LDS kernels (the only ones below N = 1024)
 *   "gemm_order"     0..1    1                     CN_GEMM_ORDER    VALU scalar GEMM: 1 slice-major workgroup order (every input slice fetched once
 *                                                                   per XCD), 0 group-major
 *   "ks_perm_fused"  flag    1                     -                a rotation of a small batch (two-launch key switch) has no permutation pass: the
 *                                                                   key-switch kernels apply the automorphism while they load c1 and c0; 0 = k_galois_lds
 *   "ks_xcd"         0..2    2 (N <= 8192),        CN_KS_XCD        workgroup order of the fused key switch: 0 (ciphertext, limb), 1 the limbs of a
 *                            1 (N = 16384)                          ciphertext on one XCD, 2 limb-major (one key slice per XCD L2 at a time)
 *   "sq_fused"       flag    1                     CN_SQ_FUSED      transforms and tensor of a squaring (Multiply(a, a): SquareActivation) as one kernel
 *                                                                   per base; 0 = separate launches
 *   "sq_lds"         flag    1                     CN_SQ_LDS        the NTT-form operand of a fused squaring parked in LDS (N <= 8192); 0 = in the
 *                                                                   outputs' place
 *   "sq_pipe"        0..2    1                     CN_SQ_PIPE       1: the fused squaring of a batch on the pipelined resident kernel k_square_pipe (one
 *                                                                   workgroup per CU and modulus, next operand prefetched); 0 k_square_fused; 2
 *                                                                   k_square_pipe for any count
 *   "sq_halves"      0..2    1                     CN_SQ_HALVES     Multiply + Relinearize of a batch pipelined in parts over two streams (below):
 *                                                                   1 cn_mul_relin, 2 also the flush of queued calls (measured slower there), 0 off
 *   "enc_fused"      0..2    2                     CN_ENC_FUSED     Encryptor.Encrypt behind the samplers: 2 one kernel with a block per (ciphertext,
 *                                                                   component, limb) (N <= 8192, FP64 policies); 1 a block per (ciphertext, limb), u in
 *                                                                   registers for both components; 0 expansion + batched transform + tail kernel
 *   "fold_zero"      flag    1                     CN_FOLD_ZERO     queued zero encryptions folded into the scalar product that reads them (below)
 *   "gemm_mfma"      flag    1                     CN_GEMM_MFMA     wide scalar GEMMs (>= 16 outputs per gather list) on the int8 matrix cores; 0 = the
 *                                                                   FP64 kernel.  Affects GEMMs planned after the call
 *   "digit_mfma"     flag    1                     -                the digit GEMM of cn_square_gemm on the int8 matrix cores where the plan's own GEMM
 *                                                                   takes them and a key-switch digit has at most 14 bits; 0 = the FP64 kernel (which
 *                                                                   also serves every other plan).  The same words.  Affects GEMMs planned after the call
 *   "digit_i32"      flag    1                     -                the digit sums cn_square_gemm and cn_mul_relin_sum hand to their key switch are stored
 *                                                                   as int32 words where sum |w| (2^dbc - 1) <= 2^31 - 1; 0 = always doubles.  The same
 *                                                                   words.  Affects GEMMs planned after the call
 *   "mul_sum"        flag    1                     -                cn_mul_relin_sum sums the unrelinearized products and runs one key switch per output
 *                                                                   where it can; 0 = always Multiply + Relinearize per term, then AddMany.  The same words
 *   "gemm_pair"      flag    1                     CN_GEMM_PAIR     cn_scalar_gemm / cn_gemm_plan_create merge gather lists that share at least half of
 *                                                                   their inputs in pairs (small signed weights, lists of <= 64 entries and <= 5
 *                                                                   outputs); 0 = the caller's lists.  Affects GEMMs planned after the call
 *   "mp_fused"       flag    1                     CN_MP_FUSED      a dense MultiplyPlain as two launches (lift + transform of the plaintexts; transform,
 *                                                                   product, inverse transform of the ciphertext limbs); 0 = six
 *   "ks_wide"        -1..2   -1                    -                -1 automatic by batch size, 0 the fused one-launch kernel, 1 two launches with a
 *                                                                   workgroup per digit, 2 two launches with a workgroup per source limb
 *   "ks_split14"     flag    1                     -                N = 16384: the key switch as two 8192-point halves per limb (no register spills);
 *                                                                   0 = the fused 1024-thread kernel
 *   "ks_pair14"      flag    1                     CN_KS_PAIR14     N = 16384, batches: both halves of a limb in ONE launch, a rotation's c1 permuted
 *                                                                   once per ciphertext and its c0 inside the kernel; 0 = permutation pass, two
 *                                                                   workgroups per limb, combining pass
 *   "ks_chain"       flag    1                     CN_KS_CHAIN      every link of a cn_sum_slots / cn_rowdot_batch rotate-and-add chain leaves the next
 *                                                                   link's permuted c1 beside its result (no permutation pass between links)
 *   "mp_bcast"       flag    1                     -                cn_rowdot_batch transforms its ONE ciphertext once and the row plaintexts inside the
 *                                                                   product kernel; 0 = k_lift_ntt + k_mul_plain_fused
 *   "sg_prefloor"    0..2    1                     -                cn_square_gemm: components 0 and 1 of the products take ONE fast floor per dense output
 *                                                                   (sums of their Bsk words in NTT form and of their canonical y on the matrix cores)
 *                                                                   where the plan and the layer size allow; 0 = one floor per product; 2 = for any
 *                                                                   layer size (tests).  The same words
 *   "ptn_order"      0..1    0                     CN_PTN_ORDER     cn_mul_plain_sum on NTT-form plaintexts, workgroup order: 0 limb-major, 1 limb = workgroup
 *                                                                   index mod k (one limb per XCD where k = 8)
 *   "defer"          0..2    0                     -                deferred submission of per-ciphertext calls (below)
 *   "defer_square_gemm" flag 0                     -                queued squarings keep their relinearisation back for the dense layer that
 *                                                                   reads them: one key switch per dense output (below); 0 = every squaring relinearises
 *                                                                   at once
 *   "ks_xi"          flag    0                     -                decomposition convention of the key switch (below)
 *   "record_steps"   flag    0                     -                note the rotation steps the caller asks for (cn_rotation_steps); 0 stops and clears
 *
 * Removed after their variants measured no gain: staggered squaring groups in the flush (profiles/r06_stagger_ab.txt), the q side of a batched
 * squaring on a second stream (profiles/r06_square_overlap.txt), the 128-VGPR fused key switch (profiles/HISTORY.md, round 1).
 *
 * "defer" = 1: DEFERRED SUBMISSION for callers that issue one evaluator call per ciphertext from many threads - the unchanged
 * NeuralNetworks layers of the reference (PoolLayer.cs:67-80,113-121,182,214; EncryptedSealBfvMatrix.cs:79-120,140-154; LLInterleaveLayer.cs;
 * Utils.cs:46-88).  cn_scalar_dot, cn_add, cn_sub, cn_add_plain, cn_mul_relin, cn_encrypt and - on up to 4 ciphertexts per call - cn_mul_plain,
 * cn_rotate_rows(_add), cn_rotate_columns(_add), cn_sum_slots, cn_copy are then queued with their operand addresses, ordered by data dependence,
 * and launched as batched kernels (all pending calls of one dependency level, kind and parameter = one launch chain) at layer boundaries (a
 * scalar product or multiplication that reads the queued result of another one), when the queue is full, or when any other entry point
 * (cn_sync, downloads, ...) needs the results.  Same words as immediate calls; argument errors (ranges, zero plaintexts, missing Galois keys) are
 * reported by the call that made them, device errors by the call that triggered the flush.  cn_free of a handle with pending readers is safe
 * (the array returns to the pool after the flush).
 * "defer" = 2: the same queue, fed WITHOUT THE CONTEXT LOCK.  cn_scalar_dot, cn_add, cn_sub, cn_add_plain, cn_mul_relin (up to 4 ciphertexts per
 * call), cn_encrypt (up to 4), cn_encrypt_zero_new, cn_free, cn_free_many and cn_ct_alloc(1, 2) do not take the lock: a call claims the next slot of a
 * multi-producer ring with one atomic add, writes a 64-byte record (handles and indices as passed) and returns 0; whoever finds the lock free executes
 * the published records in claim order - a total order consistent with happens-before between the caller's threads, which is what the dependence
 * tracking needs.  Single-ciphertext allocations come from a ring of ready handles the executing thread keeps filled.  Every other entry point takes the
 * lock and first executes what was published before it.  DIFFERENCE TO "defer" = 1: the arguments of a published call are checked when it is executed -
 * an error is reported ONCE by the next call that synchronises with the context (cn_sync, downloads, cn_stats_get, any non-deferrable entry point:
 * "a call submitted without the lock (defer = 2) failed ..."), the calls around it are executed.  For callers that come from Defaults.ThreadCount =
 * Environment.ProcessorCount threads (HE Wrapper/Defaults.cs:11-15, Utils.cs:46-88): the unchanged CryptoNets layers run at the same rate from 4, 16 and
 * 256 threads.  cn_live_handles does not count the ready handles.
 * "fold_zero" = 1: a queued fresh encryption of zero (cn_encrypt with pt = 0 / cn_encrypt_zero_new) that only feeds ONE queued scalar
 * product and has been released by the caller (PoolLayer.ElementAt / ReleaseTemp, PoolLayer.cs:67-90) is not materialised: sum_t w_t Enc_t(0) is
 * added onto the scalar product's output by linearity - exact modular arithmetic on the same sampler draws (nonce, item), the SAME words as with
 * "fold_zero" = 0, a fifth of the transforms.  All or nothing per flush (every queued zero encryption must qualify).
 * "defer_square_gemm" = 1 (off by default until it has been measured, profiles/deferred_square_gemm.md): the queue runs the reference's SquareActivation + PoolLayer call sequence (one cn_mul_relin(a, a) per column, then one cn_scalar_dot +
 * cn_add_plain + cn_free per output) in the form of cn_square_gemm.  A flush at a layer boundary runs only the Multiply half of the squarings it launches and keeps
 * the size-3 products in an array of the context (at most a quarter of the scratch limit; the callers' output arrays are not written yet).  The next flush decides
 * once, all or nothing: if the caller has released every such output array (BaseLayer.GetNext disposes a layer's input), only scalar products read them, every
 * gathered term of those scalar products is such an array, no queued call writes one, and the weights pass the test of cn_square_gemm (small signed weights, row sums
 * within the digit bound, FP64 moduli and key, 1024 <= N <= 8192, "ks_xi" = 0), the scalar products run as GEMM + digit GEMM + ONE key switch per OUTPUT - the SAME
 * words.  Otherwise every held-back product is relinearised into its own array first and the flush goes on as with "defer_square_gemm" = 0.  Every flush that is not a
 * layer boundary (cn_sync, downloads, cn_stats_get, any non-deferrable entry point, a full queue, cn_ctx_destroy) settles what is held back and relinearises its own
 * squarings at once: afterwards every array holds its words and the OperationsCount counters read as for the literal calls.  The plan of such a layer is built once
 * and found again by its weights (a handful are kept per context).
 * "sq_halves": cn_mul_relin of >= 512 ciphertexts at N <= 8192 runs in parts software-pipelined over two streams of the context - the Multiply of a part
 * beside the key switch of the part before (its HBM-bound base extension / floor fill what the FP64-bound key switch leaves).  Same words; every later call
 * on the context is ordered behind all parts.  A caller that issues its plaintext primes one after the other (or from parallel tasks) gets what bench.py's
 * half-batch stagger of the primes gets (12.6 -> 12.0 ms per CryptoNets batch); a staggered caller nothing.  A batch runs in parts only if every part takes
 * the fused key switch.  With "ks_wide" 1 or 2, or in automatic mode when a part has at most 160 (ciphertext, limb) blocks, it runs on one stream: the
 * two-launch key switch keeps its partial products in one arena per context.
 * "ks_xi": DECOMPOSITION CONVENTION of the key switch (relinearisation and rotations).  0 (default): base-2^dbc digits of the raw residue c_l of every
 * source limb l; key (l, d) = (-(a s + e) + 2^(dbc d) s' [in limb l only], a) - SURVEY 9.5, the form in which the CRT basis element
 * (q/q_l) [(q/q_l)^-1]_{q_l} is folded into the key.  1: digits of xi_l = [c_l (q/q_l)^-1]_{q_l}; key (l, d) = (-(a s + e) + (q/q_l) 2^(dbc d) s' [in every
 * limb], a) - the xi_q decomposition as the BEHZ paper writes it.  Both are exact key switches and decrypt identically with their own keys; keys of
 * one convention give garbage under the other.  Set it BEFORE cn_keygen / the key uploads; the start-up self-test of the host mirrors
 * (hewrapper.AtomicSealBfvEncryptedEnvironment.SelfTest, the C# twin's SelfTest) picks the one the client's evaluator obeys.
 *
 * Environment switches read once per process (A/B measurements, all default to the measured best): CN_STREAM_PROBE=0 (no hardware-queue selection),
 * CN_TABLES_ZERO_COPY=0 (small operand tables are copied to the device instead of read from the pinned ring), CN_KS_WIDE_MAX / CN_KS_DIGIT_MAX ((ciphertext,
 * limb) blocks up to which a key switch runs as two launches: 160 / with one workgroup per digit: 10), CN_GEMM_ONE_LIMB=0 (the small-weight GEMM kernel
 * keeps its two-limb form), CN_GEMM_RESIDUAL=0 (read whenever a scalar GEMM is planned, not once - a plan that is kept, cn_gemm_plan_create's or a cached plan of the
 * deferred queue, stays in the form it was built in: matrix-core plans with 127 < max |w| <= 254 keep their two base-256 weight planes instead of one clipped plane and
 * a sparse residual; =2: the residual form up to half the K steps instead of one in eight), CN_DEFER_MERGE_GEMM=0 (deferred scalar products of one flush keep their levels: one launch per level instead of one per term
 * count), CN_PIN_RING_MIB (size of the pinned upload ring, 32 MiB), CN_DEFER_TRACE=1 (one stderr line per flushed queue level: calls per kind,
 * launches; one per flush that holds squarings back, runs a dense layer on them or relinearises them after all), CN_LOCK_GRACE_NS / CN_LOCK_COMBINE (the two context-lock experiments that are kept but off, cn_host.cpp). */
int cn_set_option(cn_ctx *ctx, const char *name, int value);
/* reads back every option of cn_set_option's list, or one of these read-only values:
 *   "behz_small_base"          1: auxiliary primes below 2^49 - the FP64 kernels - k+1 of them, or k+2 where k+1 are too few (N = 16384); 0: SEAL's
 *                              61-bit base, taken whenever log2 t + log2 N + log2 q + 2 < log2(B m_sk) does not hold for the small primes or a data
 *                              prime has 49 bits or more
 *   "behz_f64"                 the BEHZ steps run on the FP64 kernels
 *   "mod_switch_f64"           the last cn_mod_switch this context took part in (source or target) ran the exact-FP64 kernel
 *   "aux_primes"               primes of B plus m_sk
 *   "pending_calls"            deferred calls not yet launched
 *   "ready_handles"            single-ciphertext arrays waiting for a lock-free cn_ct_alloc ("defer" = 2)
 *   "pin_laps"                 laps of the context's pinned upload ring (small tables of a flush; a lap waits for the stream once)
 *   "folded_zero_encryptions"  zero encryptions folded so far ("fold_zero")
 *   "mul_relin_pipelined"      cn_mul_relin chunks and flushed groups of queued Multiply + Relinearize calls that ran in parts over the context's two
 *                              streams ("sq_halves"; counts up)
 *   "square_gemm_fused"        cn_square_gemm calls that ran one key switch per output (counts up; the others took the two separate steps)
 *   "square_gemm_prefloor"     ... of which with one fast floor per dense output for components 0 and 1 ("sg_prefloor"; counts up)
 *   "sg_prefloor_min_k"        the smallest K for which cn_square_gemm takes that form under "sg_prefloor" = 1
 *   "defer_square_gemm_fused"  groups of queued scalar products that ran on held-back squarings with one key switch per output ("defer_square_gemm"; counts up)
 *   "defer_pending_products"   squarings whose relinearisation is held back right now (0 after every flush that is not a layer boundary)
 *   "mul_sum_fused"            cn_mul_relin_sum calls that ran one key switch per output (counts up; the others took the literal sequence)
 *   "mul_sum_groups"           output groups of the last cn_mul_relin_sum call (0: it took the literal sequence or had K = 1)
 *   "mul_sum_min_k"            the smallest K for which cn_mul_relin_sum takes the one-key-switch form
 *   "digit_gemm_mfma"          digit GEMMs of cn_square_gemm launched in the matrix-core form ("digit_mfma"; counts up)
 *   "ks_digits_i32"            key switches launched on int32 digit sums ("digit_i32"; counts up)
 *   "scratch_mib"              MiB of the context's scratch arena right now, rounded up (it grows to the largest call's need and stays)
 *   "diag_scan", "diag_encode" launches of k_diag_scan / k_diag_gather (cn_diag_scan, cn_diag_encode; count up)
 *   "pool_arrays"              device arrays cached for reuse (the temporaries of a live graph are reserved out of them)
 *   "stream_tries"             streams cn_ctx_create tried until one had a hardware queue of its own (< 0: none had; CN_STREAM_PROBE=0 takes the first) */
int cn_get_option(cn_ctx *ctx, const char *name, int *value);
/* SEAL DefaultParams.CoeffModulus128(n) (AtomicSealBfvVector.cs:146); returns count, fills q (<=9) */
int cn_default_coeff_modulus(uint32_t n, uint64_t *q);
/* number of u64 words of one key-switch key for this context (relin: which=0, galois: which=1) */
size_t cn_key_words(cn_ctx *ctx, int which);
/* keys.RelinKeys(dbc) / keys.GaloisKeys(gdbc) (AtomicSealBfvVector.cs:68-69): upload from host
 * memory, or adopt a device buffer (e.g. one filled by an RCCL broadcast). */
int cn_set_relin_key(cn_ctx *ctx, const uint64_t *words, size_t count, int is_device_ptr);
int cn_set_galois_key(cn_ctx *ctx, uint64_t galois_elt, const uint64_t *words, size_t count, int is_device_ptr);
int cn_has_galois_key(cn_ctx *ctx, uint64_t galois_elt);
/* Any key in either representation.  which: 0 relin, 1 galois (galois_elt), 2 public, 3 secret - as cn_get_key; a public / secret key is always copied.
 * form 0: NTT form in this library's transform order (what cn_set_relin_key / cn_set_galois_key / cn_set_public_key take: SEAL's in-memory form IF its
 * transform uses the minimal primitive 2N-th root and bit-reversed output).  form 1: COEFFICIENT form - the device transforms the polynomials
 * with its own tables, so the upload does not depend on the root or the output order of the key generator's transform (an adopted device buffer is
 * transformed in place).  The C# twin's start-up self-test falls back to form 1 (Evaluator.TransformFromNTTInplace on the key ciphertexts) when the
 * NTT-form words of the SEAL it runs beside do not reproduce SEAL's own results (integration/GpuAtomicSealBfvEncryptedVector.cs: SelfTest). */
int cn_load_key(cn_ctx *ctx, int which, uint64_t galois_elt, const uint64_t *words, size_t count, int is_device_ptr, int form);
/* Multi-GPU, single process (the path shards by independent batches / plaintext primes, the only exchange is the one-time
 * key broadcast): copies the relinearisation key and every Galois key of ctxs[0] into ctxs[1..n-1] (same encryption parameters, any
 * devices) - ONE RCCL broadcast per key over xGMI to the contexts on other GPUs (librccl is loaded on demand; peer copies without it),
 * device-to-device copies on the root's GPU.  Synchronises all contexts.  (One process per GPU: broadcast with the host framework and
 * adopt the buffers through cn_set_relin_key / cn_set_galois_key with is_device_ptr = 1 instead - bench.py does.) */
int cn_ctx_broadcast_keys(cn_ctx **ctxs, int n);
/* Evaluator/util galois_elt_from_step: steps>0 left, <0 right, 0 = column swap (2N-1) */
uint64_t cn_galois_elt_from_step(cn_ctx *ctx, int steps);

/* ---- buffers = arrays of SEAL Ciphertext / Plaintext objects (ctor/Set/Dispose:
 * AtomicSealBfvVector.cs:373,389-397,413-428) */
int cn_ct_alloc(cn_ctx *ctx, uint32_t count, uint32_t size, cn_handle *out);   /* size = polys per ct (2 or 3) */
int cn_pt_alloc(cn_ctx *ctx, uint32_t count, cn_handle *out);                  /* dense plaintexts, N coeffs each */
int cn_free(cn_ctx *ctx, cn_handle h);
/* n handles with one call (one lock acquisition): ReleaseTemp of the unchanged PoolLayer disposes one zero encryption per padded tap (PoolLayer.cs:83-90),
 * BaseLayer.GetNext one column at a time (BaseLayer.cs:23-49).  All handles are validated first; an invalid or repeated one releases nothing. */
int cn_free_many(cn_ctx *ctx, const cn_handle *h, uint32_t n);
int cn_ct_upload(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, const uint64_t *host);
int cn_ct_download(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint64_t *host);
int cn_pt_upload(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, const uint64_t *host);
int cn_pt_download(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint64_t *host);
/* BatchEncoder.Encode / Decode (AtomicSealBfvVector.cs:644,669,941,1130,1158 / :1050,1093): slot values <-> plaintext
 * coefficients; the (I)NTT mod t runs on the device.  Requires t prime, t == 1 mod 2N. */
int cn_encode(cn_ctx *ctx, const uint64_t *values, uint32_t nvalues, cn_handle pt, uint32_t pi);
int cn_decode(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint64_t *values /* N */);
/* the same for `count` plaintexts in one call (one upload, one scatter launch, one batched transform mod t): values is
 * [count][nvalues] for encode (slots beyond nvalues are zero), [count][N] for decode.  A layer's weight rows / masks / bias vectors
 * (LLDenseLayer.Prepare: thousands of Plaintexts, EncryptedSealBfvMatrix.cs:79-120) are encoded with ONE call. */
int cn_encode_batch(cn_ctx *ctx, const uint64_t *values, uint32_t nvalues, uint32_t count, cn_handle pt, uint32_t pi);
int cn_decode_batch(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t count, uint64_t *values /* [count][N] */);
int cn_copy(cn_ctx *ctx, cn_handle src, uint32_t sfirst, cn_handle dst, uint32_t dfirst, uint32_t count);
/* n single ciphertexts (or dense plaintexts) that live in n arrays -> consecutive places of ONE array with one launch:
 * dst[dfirst + i] = src[i][sfirst[i]] (sfirst NULL = element 0 of every array).  The reference keeps a vector as a list of Ciphertext objects and
 * has no such call; a host that keeps vectors as arrays uses it where the reference copies element by element (GenerateSparseOfArray,
 * AtomicSealBfvVector.cs:1347-1359; the column gather in front of DenseMatrixBySparseVectorMultiply): 25 + 10 copy launches of one LoLa image
 * become 2.  Queued like n cn_copy calls under cn_set_option("defer", 1). */
int cn_copy_many(cn_ctx *ctx, const cn_handle *src, const uint32_t *sfirst, uint32_t n, cn_handle dst, uint32_t dfirst);
int cn_device_ptr(cn_ctx *ctx, cn_handle h, void **ptr, size_t *bytes);
int cn_live_handles(cn_ctx *ctx);                                              /* leak counter */

/* ---- linear ops ---------------------------------------------------------------------- */
/* Evaluator.Add / Sub / Negate (AtomicSealBfvVector.cs:491,646,671,865,1005,1258) */
int cn_add(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count);
int cn_sub(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out, uint32_t oi, uint32_t count);
int cn_negate(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle out, uint32_t oi, uint32_t count);
/* Evaluator.AddMany (AtomicSealBfvVector.cs:502,698,708,902): out[oi] = sum_i in[idx[i]] */
int cn_add_many(cn_ctx *ctx, cn_handle in, const uint32_t *idx, uint32_t n_idx, cn_handle out, uint32_t oi);
/* Evaluator.AddPlain / SubPlain (AtomicSealBfvVector.cs:1019,1267), dense plaintexts */
int cn_add_plain(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, int subtract,
                 cn_handle out, uint32_t oi, uint32_t count);
/* Evaluator.MultiplyPlain with a dense (BatchEncoded) plaintext: lift, NTT, dyadic, INTT
 * (AtomicSealBfvVector.cs:645,670,803,855,942,1455).  pt_stride 0 = same plaintext for all. */
int cn_mul_plain(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle pt, uint32_t pi, uint32_t pt_stride,
                 cn_handle out, uint32_t oi, uint32_t count);
/* Evaluator.MultiplyPlain with a constant (sparse-format) plaintext `Plaintext(hex)`
 * (AtomicSealBfvVector.cs:1136,1164,1179 -> :472,482,571,592): scalars[i] in [0,t). */
int cn_mul_scalar(cn_ctx *ctx, cn_handle a, uint32_t ai, const uint64_t *scalars, uint32_t scalar_stride,
                  cn_handle out, uint32_t oi, uint32_t count);
/* HOT LOOP A: AtomicSealBfvEncryptedVector.DenseMatrixBySparseVectorMultiply for O outputs at
 * once (AtomicSealBfvVector.cs:434-521 as driven by PoolLayer.ConvolveOnce/Apply,
 * NeuralNetworks/PoolLayer.cs:113-121,149-229):
 *   out[oi+o] = sum_k W[o*K+k] * in[idx[o*K+k]]  (+ Delta-scaled dense plaintext bias[bias_idx[o]])
 * idx<0 = padded tap (skipped, PoolLayer.cs:68-80); W in [0,t), zero weights skipped (:468);
 * an output whose weights are all zero is an error like SEAL's AddMany of nothing.
 * `in` and `out` must have the same ciphertext size: 2, or 3 (Evaluator.MultiplyPlain / Add on products that have not been relinearized;
 * cn_gemm_plan_apply likewise - a plan does not depend on the size). */
int cn_scalar_gemm(cn_ctx *ctx, cn_handle in, const int32_t *idx, const uint64_t *W, uint32_t O, uint32_t K,
                   cn_handle bias_pt, const int32_t *bias_idx, cn_handle out, uint32_t oi);
/* The same product for ONE output whose K input ciphertexts are SEPARATE objects - the form the C# twin of
 * AtomicSealBfvEncryptedVector.DenseMatrixBySparseVectorMultiply calls per block i (AtomicSealBfvVector.cs:434-521: denses[k].encData[i]
 * are individually allocated SEAL Ciphertexts): out[oi] = sum_k w[k] * in[k][in_idx[k]].  in[k] == 0: padded tap, skipped
 * (PoolLayer.cs:68-80); in_idx == NULL: all 0; zero weights contribute nothing (:468); an all-zero row is an error.  With
 * cn_set_option("defer", 1) the call is queued (see cn_set_option) and merged with its siblings into one GEMM launch. */
int cn_scalar_dot(cn_ctx *ctx, const cn_handle *in, const uint32_t *in_idx, const uint64_t *w, uint32_t K, cn_handle out, uint32_t oi);
/* The same GEMM planned once: validation, grouping and the weight tiles in kernel layout are built and uploaded by
 * cn_gemm_plan_create (the layer's weights then live in HBM), cn_gemm_plan_apply only launches.  Release with cn_free. */
int cn_gemm_plan_create(cn_ctx *ctx, const int32_t *idx, const uint64_t *W, uint32_t O, uint32_t K, cn_handle bias_pt,
                        const int32_t *bias_idx, cn_handle *plan);
int cn_gemm_plan_apply(cn_ctx *ctx, cn_handle plan, cn_handle in, cn_handle out, uint32_t oi);

/* Captured sequences (HIP graphs) for the launch-bound chains of a single-image inference (LoLa: ~235 small launches per plaintext
 * prime, the reference's LowLatencyCryptoNets loop LoLaCryptonets.cs:236-278): every library call between cn_graph_begin and
 * cn_graph_end is RECORDED on the context stream instead of executed; cn_graph_launch replays the whole sequence with one launch.
 * Rules: run the same sequence once before recording (the scratch arenas then have their size; temporaries come out of the handle pool);
 * nothing that synchronises (cn_sync, uploads / downloads, key changes) between begin and end; handles created while recording stay
 * alive as long as the graph is launched (its kernels carry their addresses); new inputs are written INTO the handles the recorded
 * sequence read (cn_copy, cn_encrypt).  Release with cn_free. */
int cn_graph_begin(cn_ctx *ctx);
int cn_graph_end(cn_ctx *ctx, cn_handle *graph);
int cn_graph_launch(cn_ctx *ctx, cn_handle graph);
/* Recording across levels: cn_graph_begin_levels starts a recording on ctx, the ROOT, that also covers the n level contexts `levels`, the MEMBERS;
 * cn_graph_end(ctx) closes it and returns one graph owned by ctx, cn_graph_launch(ctx) replays the whole chain with one launch.  Every member must be a
 * context cn_mod_switch from ctx would accept as a target (same device, N and t, its coefficient modulus a strict prefix of ctx's, the same
 * key-switch convention and under "ks_xi" = 1 a level of ctx's chain); the members must be distinct, none the root, none recording or a member of
 * another recording.  Otherwise CN_ERR_ARG and nothing starts (n = 0: cn_graph_begin).  Queued calls of the root and the members are submitted first.
 * While recording, the members' calls are recorded on the ROOT's stream (one linear graph) and every member counts as recording: the calls
 * cn_graph_begin refuses are refused on a member too, and cn_graph_begin / cn_graph_end on a member return CN_ERR_ARG.  cn_mod_switch between two
 * contexts of the recording is recorded; a switch to or from any other context is refused.  Each member's temporaries stay reserved out of its own
 * pool while the graph lives.  Launch order without a host wait: the replay starts behind the work submitted to every member before
 * cn_graph_launch, and later calls on a member start behind the replay (a graph without members launches exactly as before).
 * Lifetime: cn_ctx_destroy of a member while the recording runs or a graph recorded with it is alive returns CN_ERR_ARG and frees nothing; free
 * the graph (cn_free on the root) first.  Destroying the root frees its graphs and hands the members' reservations back. */
int cn_graph_begin_levels(cn_ctx *ctx, cn_ctx *const *levels, uint32_t n);

/* ---- non-linear ops ------------------------------------------------------------------ */
/* Evaluator.Multiply (BEHZ), size2 x size2 -> size3 (AtomicSealBfvVector.cs:461,546,786,839,1457) */
int cn_multiply(cn_ctx *ctx, cn_handle a, uint32_t ai, cn_handle b, uint32_t bi, cn_handle out3, uint32_t oi, uint32_t count);
/* Evaluator.Relinearize size3 -> size2 (AtomicSealBfvVector.cs:462,547,787,840) */
int cn_relinearize(cn_ctx *ctx, cn_handle in3, uint32_t ii, cn_handle out, uint32_t oi, uint32_t count);
/* HOT LOOP B: Multiply + Relinearize per block (PointwiseMultiply, AtomicSealBfvVector.cs:839-840;
 * SquareActivation.cs:10-13).  a_stride/b_stride 0 broadcast one operand (PointwiseMultiplySparseDimOne).
 * Overlaps: operand x touches [xi, xi + (count - 1) x_stride] of its handle (one index for x_stride 0).  When x is the output handle, that span must
 * either be disjoint from [oi, oi + count) or be exactly that range (in place: oi == xi, stride 1).  Any other intersection is refused with CN_ERR_ARG
 * and nothing is written - a batch runs in chunks and in parts on two streams, whose results are stored while later ones still read operands.  The
 * operands may overlap each other freely.  The rule is checked when the call is made in every "defer" mode, before a call of up to 4 ciphertexts is
 * published without the lock (defer = 2). */
int cn_mul_relin(cn_ctx *ctx, cn_handle a, uint32_t ai, uint32_t a_stride, cn_handle b, uint32_t bi, uint32_t b_stride,
                 cn_handle out, uint32_t oi, uint32_t count);
/* SquareActivation followed by the PoolLayer behind it, as one call: squares the ciphertexts in[ii .. ii + n_in) (n_in = the largest input index of the plan + 1)
 * and writes the O outputs that cn_mul_relin(in, ii -> tmp) followed by cn_gemm_plan_apply(plan, tmp, out, oi) would write - the same words, bias included; the
 * counters of cn_stats that mirror OperationsCount advance as for those two calls.  The relinearized squares themselves are not produced: a key switch is linear in
 * the digits of its operand, so the layer pair needs one key switch per OUTPUT, fed with the weight-combined digit polynomials S = sum_k w_ok digit(d2_k) - digits
 * taken per input, before the sum, hence the reference's words (unlike relinearizing the sum of size-3 products).  That form runs when the plan's weights are small
 * (|w| < 2^20 centred), max_o sum_k |w_ok| (2^dbc - 1) is below every q_j / 2 and below 2^52, every coefficient modulus and the relinearization key are on the exact-FP64
 * path, 1024 <= N <= 8192 and "ks_xi" is 0; otherwise the call runs the two steps through a temporary - same result, no error.  `in` and `out` must be different
 * handles; with "defer" on, queued calls are submitted first and the call runs at once; under cn_graph_begin it is recorded like its two parts. */
int cn_square_gemm(cn_ctx *ctx, cn_handle plan, cn_handle in, uint32_t ii, cn_handle out, uint32_t oi);
/* Encrypted x encrypted sums of products, as one call: out[oi + i] = sum_{k < K} Relinearize(Multiply(a[k][a_idx[k] + i], b[k][b_idx[k] + i * b_stride])), i < count.
 * DenseMatrixBySparseVectorMultiply with both operands encrypted (AtomicSealBfvVector.cs:459-465,502: Multiply + Relinearize per term, then AddMany - a[k] the dense
 * column k, b[k] the sparse vector's entry k, b_stride 0) and DotProduct of two encrypted dense vectors of several blocks (:963-977: PointwiseMultiply :839-840 and the
 * AddMany at the head of SumAllSlots :888-900 - K = blocks, count 1).  K operand handles on either side, in the form of cn_scalar_dot (a caller's columns are separate
 * arrays; handles may repeat); a_idx / b_idx may be NULL (all zero); b_stride is 0 (one ciphertext of b[k] for every output) or 1.
 * The words, and the counters of cn_stats that mirror OperationsCount, are those of the literal sequence: K calls of cn_mul_relin into a temporary, then cn_add_many
 * per output.  A key switch is linear in the digits of its operand, so the sum needs ONE key switch per output, fed with S = sum_k digit(d2_k) - digits cut per
 * product, before the sum, hence the reference's words (cn_square_gemm with unit weights): K multiplies, one pass that sums the unrelinearized products
 * (components 0 and 1 mod q, the digits of component 2 as integers), one key switch.  That form runs when every coefficient modulus and the relinearization key are on
 * the exact-FP64 path, 1024 <= N <= 8192, "ks_xi" is 0, K (2^dbc - 1) is below every q_j / 2 and below 2^52, K (q_max - 1) < 2^64, a digit has at most 31 bits and a limb at
 * most 8 digits, K >= "mul_sum_min_k", "mul_sum" is 1 and the scratch limit (CN_SCRATCH_GB) leaves room for the K products of one output; the outputs run in groups
 * whose products fit that limit ("mul_sum_groups").  Otherwise the call runs the literal sequence through a temporary - same result, no error.  K = 1 is cn_mul_relin
 * into the outputs.  Level contexts are eligible (their sliced keys are the prefix's key set under "ks_xi" = 0).
 * Refused with CN_ERR_ARG / CN_ERR_NOKEY, nothing written: K = 0, count = 0, b_stride > 1, an index range outside its handle, `out` among the operand handles,
 * operands or outputs not of size 2, no relinearization key, a context with one coefficient modulus.  With "defer" on, queued calls are submitted first and the call
 * runs at once; under cn_graph_begin it is recorded like its parts. */
int cn_mul_relin_sum(cn_ctx *ctx, const cn_handle *a, const uint32_t *a_idx, const cn_handle *b, const uint32_t *b_idx, uint32_t K, uint32_t b_stride,
                     cn_handle out, uint32_t oi, uint32_t count);

/* ---- rotations (HOT LOOP C) ----------------------------------------------------------- */
/* Evaluator.ApplyGalois: automorphism + key switch of c1 */
int cn_apply_galois(cn_ctx *ctx, cn_handle in, uint32_t ii, uint64_t galois_elt, cn_handle out, uint32_t oi, uint32_t count);
/* Evaluator.RotateRows(/Inplace): NAF decomposition when no key exists for the step
 * (AtomicSealBfvVector.cs:625,631,637,660,864,1420,1458).  Operand and result ranges of ONE handle may be the same range (in place), disjoint, or
 * overlap with a shift (cn_rotate_rows, cn_apply_galois, cn_rotate_columns: such a call takes the permutation pass / a staging copy, which reads the whole
 * operand before anything is written).  The _add forms refuse a partial overlap of operand or accumulator with the result (CN_ERR_ARG): their fused
 * accumulator is read where the result is stored.  The hops are planned before anything is copied or launched: a rotation that is refused for a missing
 * key (CN_ERR_NOKEY) or a step count of N/2 or more (CN_ERR_ARG) enqueues nothing and leaves the result range untouched. */
int cn_rotate_rows(cn_ctx *ctx, cn_handle in, uint32_t ii, int steps, cn_handle out, uint32_t oi, uint32_t count);
/* RotateRows of n ciphertexts by n DIFFERENT step counts: out[oi[i]] = RotateRows(in[ii[i]], steps[i]), same words as n cn_rotate_rows calls.
 * The reference rotates the vectors of an Interleave / a Vectorize one Evaluator.RotateRows at a time (AtomicSealBfvVector.cs:628-688); here the
 * hops of all n rotations run in rounds - one two-launch key switch per round over every ciphertext that has a hop left, each with the key
 * and the element of ITS step count - so a single-image network pays the dispatches of the longest rotation instead of the sum (n <= 32 / k; more
 * run one after the other).  in == out is allowed when no result overwrites another rotation's operand or result (its own is fine). */
int cn_rotate_rows_many(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const int *steps, uint32_t n, cn_handle out, const uint32_t *oi);
/* Hoisted rotations: n rotations of ONE ciphertext, out[oi[r]] = the rotation of in[ii] by elts[r] / steps[r], with ONE set of digit transforms.  The reference
 * rotates one ciphertext by many step counts in Duplicate (AtomicSealBfvVector.cs:1370-1396: a rotate-and-add chain over copies of one vector), for the equal-source
 * vectors of Interleave / Vectorize (AtomicSealBfvVector.cs:625-660, 1458) and - through this package's diagonal dense layers - for the baby steps of a matrix-vector
 * product; every Evaluator.RotateRows there cuts c1 into its gk_tot digit polynomials and transforms each of them for each of the k limbs.  The digits do not depend
 * on the rotation and x -> x^g permutes a transform's output without a sign, so this call runs gk_tot k forward transforms once and 2 k inverse transforms per
 * rotation, in two launches (k_ks_digit_ntt, k_ks_hoist_mac).
 * THE WORDS are not those of cn_rotate_rows: SEAL permutes c1 and cuts digits afterwards, and a negated coefficient q_l - x has other digits than x.  With
 *     D_(l,d)[i]          = digit d (base 2^gdbc, low to high) of c1 limb l, coefficient i           ("ks_xi": of [c1_l (q/q_l)^-1]_(q_l))
 *     s_g(D)_j[i g mod N] = +- (D[i] mod q_j), negative when (i g mod 2N) >= N                        (canonical)
 *     out_p limb j        = INTT_j( sum_(l,d) NTT_j(s_g(D_(l,d))_j) . K_g[(l,d)][p][j] )  +  (p == 0 ? s_g(c0)_j : 0)
 * for the Galois key K_g of element g.  The result decrypts to the plaintext of cn_apply_galois; its key-switch noise is a sum over the same digits against the same
 * key errors, permuted (tests/hoisted_model.py states the formula in Python integers, tests/test_gpu_hoisted_rotations.py holds the device to it).
 * The steps form maps a step through cn_galois_elt_from_step's rule; step 0 and element 1 are plain copies.  Every element needs its OWN key - there are no
 * non-adjacent-form hops, a hop chain is sequential: CN_ERR_NOKEY otherwise.  CN_ERR_ARG: a step of N/2 or more, an even element or one >= 2N, n = 0, an output
 * index listed twice, operands not of size 2, an output that is in[ii] itself, N < 1024 or "legacy_ntt", keys loaded in different forms.  A refused call launches
 * nothing and leaves the outputs untouched.  Queued calls ("defer") are submitted first and the call runs at once.  Under cn_graph_begin the lists are captured by
 * value (as for cn_add_many); the transformed digits live in the key-switch arena (gk_tot k N words), which cannot grow while a graph is recorded or alive - run
 * the sequence once before recording.  Works on level contexts with the sliced keys, in both key-switch conventions ("ks_xi") and with keys loaded in either form
 * ("f64"); "record_steps" notes the steps as cn_rotate_rows_many / cn_apply_galois do.  cn_get_option "ks_hoisted" counts the calls that launched the two kernels (counts
 * up, read-only); ntt_forward_limbs / ntt_inverse_limbs grow by gk_tot k and 2 k per rotation.
 * Key memory: direct keys for B - 1 baby steps are (B - 1) gk_tot 2 k N 8 bytes per plaintext prime - 2 GiB at N = 16384, k = gk_tot = 8, B = 128, against the 7 keys
 * of baby steps by doubling. */
int cn_apply_galois_hoisted(cn_ctx *ctx, cn_handle in, uint32_t ii, const uint64_t *elts, uint32_t n, cn_handle out, const uint32_t *oi);
int cn_rotate_rows_hoisted(cn_ctx *ctx, cn_handle in, uint32_t ii, const int *steps, uint32_t n, cn_handle out, const uint32_t *oi);
/* Summed rotations: out[oi + g] = sum over e in [grp_off[g], grp_off[g + 1]) of ApplyGalois(in[ii[e]], elts[e]) / RotateRows(in[ii[e]], steps[e]), g < G - n
 * rotations of n DIFFERENT ciphertexts under one pair of inverse transforms per output limb.  The reference forms such sums in Interleave
 * (AtomicSealBfvVector.cs:600-722: RotateRows of the vectors, AddMany per output block) and Permute (:1436-1474: a rotation and an AddInplace per selection); the
 * giant steps of this package's diagonal dense layers are one more.  A key switch ends in INTT_j(acc) and the inverse transform is linear mod q_j, so
 *     sum_r ( INTT_j(acc_r) + s_(g_r)(c0_r) )  =  INTT_j( sum_r acc_r ) + sum_r s_(g_r)(c0_r)        (mod q_j, canonical)
 * holds exactly: every term runs its forward digit transforms and its key products (the term MAC of the two-launch key switch, operand, key and element per term,
 * the automorphism applied on load), the partial products of all terms of an output are summed and inverted once (k_ks_sum_terms), no rotated term is stored.
 * THE WORDS: cn_apply_galois_sum writes the canonical words of cn_apply_galois per term followed by cn_add_many per group; cn_rotate_rows_sum those of cn_rotate_rows
 * per term (the same hops, in the same order, with the same keys as cn_rotate_rows_many) followed by cn_add_many.  Modular sums are exact: the order of the terms
 * does not matter.  Element 1 / step 0 is a plain addend, both components; a group made only of such terms launches no key-switch kernel (cn_add_many's kernel
 * runs); a group of one rotated term is cn_apply_galois.  grp_off follows cn_mul_plain_sum: G + 1 entries, starts at 0, strictly increasing; indices in ii may
 * repeat inside and across groups.
 * Keys: the element form needs the OWN key of every element (CN_ERR_NOKEY); the steps form runs the non-adjacent-form hops of a step without its own key
 * (cn_rotation.h) - all but the last hop as cn_rotate_rows_many's rounds into a temporary, the last hop inside the sum - and reports CN_ERR_NOKEY only when the
 * planner finds no chain; a step of N/2 or more is CN_ERR_ARG.  CN_ERR_ARG, nothing launched, outputs untouched: G = 0, grp_off[0] != 0, an empty group, an index
 * outside its handle, operands or outputs not of size 2, an output range that contains a ciphertext the call reads, an even element or one >= 2N, a context with
 * one coefficient modulus, keys of the listed elements loaded in different forms.  Hops and refusals are planned before anything is copied or launched.
 * NO REFUSAL FOR A MISSING KERNEL: where the fused form does not run - N < 1024, "legacy_ntt", the integer policy at N = 16384, more rotated terms than the per-digit / per-source-limb term MAC takes
 * (cn_ks_sum_plan, cn_ks_plan.h), partial products that would not fit the key-switch arena - the call composes the literal sequence through a temporary: the same
 * words, no error.  Works on level contexts with the sliced keys, in both key-switch conventions ("ks_xi") and with keys loaded in either form ("f64").  Queued
 * calls ("defer") are submitted first and the call runs at once.  Under cn_graph_begin the lists are captured by value; the partial products live in the
 * key-switch arena, which cannot grow while a graph is recorded or alive - run the sequence once before recording.  "record_steps" notes the steps as
 * cn_rotate_rows_many / cn_apply_galois do.
 * Counters: Rotation grows by one per hop, AddMany by G, AddManyItemCount by the number of terms; ntt_forward_limbs by gk_tot k per hop; ntt_inverse_limbs by 2 k
 * per hop that is not the last of its term plus 2 k per output with at least one rotated term (a composed call: 2 k per hop, what it ran).  cn_get_option
 * "ks_summed" counts the calls that launched the fused form (counts up, read-only). */
int cn_apply_galois_sum(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const uint64_t *elts, const uint32_t *grp_off, uint32_t G, cn_handle out, uint32_t oi);
int cn_rotate_rows_sum(cn_ctx *ctx, cn_handle in, const uint32_t *ii, const int *steps, const uint32_t *grp_off, uint32_t G, cn_handle out, uint32_t oi);
/* Evaluator.RotateColumns(/Inplace) (AtomicSealBfvVector.cs:709,914,1391) */
int cn_rotate_columns(cn_ctx *ctx, cn_handle in, uint32_t ii, cn_handle out, uint32_t oi, uint32_t count);
/* out[i] = acc[i] + RotateRows(in[i], steps) / + RotateColumns(in[i]): the rotate-and-add step of SumAllSlots / RotateRowsAndAdd
 * (AtomicSealBfvVector.cs:862-868, 888-955) with the addition fused into the last key-switch kernel; acc and in may alias
 * out.  Same words as the rotation followed by cn_add. */
int cn_rotate_rows_add(cn_ctx *ctx, cn_handle in, uint32_t ii, int steps, cn_handle acc, uint32_t ai, cn_handle out, uint32_t oi, uint32_t count);
int cn_rotate_columns_add(cn_ctx *ctx, cn_handle in, uint32_t ii, cn_handle acc, uint32_t ai, cn_handle out, uint32_t oi, uint32_t count);
/* HOT LOOP C in one call.  cn_sum_slots: SumAllSlots(length) (AtomicSealBfvVector.cs:888-935) of `count` single-block ciphertexts
 * h[first..], in place: column swap + add when length >= N/2, then RotateRows(-2^s) + AddInplace for 2^s < length; length 0 = all
 * slots.  cn_rowdot_batch: out[oi + r] = SumAllSlots(v[vi] * pt[pi + r], length), r < rows - every row of a row-major plaintext
 * matrix against one packed ciphertext (EncryptedSealBfvMatrix.cs:79-120, LLDenseLayer / LLPackedDenseLayer /
 * LLInterleavedDenseLayer).  Same words as the per-row MultiplyPlain / RotateRows / Add sequence of the reference. */
int cn_sum_slots(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint32_t length);
int cn_rowdot_batch(cn_ctx *ctx, cn_handle v, uint32_t vi, cn_handle pt, uint32_t pi, uint32_t rows, uint32_t length, cn_handle out, uint32_t oi);
/* Sums of plaintext x ciphertext products, as one call: for g < G
 *     out[oi + g] = sum_{e in [grp_off[g], grp_off[g + 1])} MultiplyPlain(ct[ci + ct_idx[e]], pt[pi + e])
 * - the inner loop of a generalized-diagonal (baby-step giant-step) matrix-vector product: the rotated copies of ONE packed input vector against the diagonals of
 * a plaintext matrix (hewrapper.DIAGONAL_DENSE); the encrypted x plaintext sibling of cn_mul_relin_sum.  grp_off has G + 1 entries, starts at 0 and
 * increases strictly (no empty group); ct_idx has grp_off[G] entries, which may repeat inside and across groups; term e takes plaintext pi + e.  Every plaintext is
 * a dense N-coefficient plaintext and none may be zero (CN_ERR_ZERO, like cn_mul_plain).
 * The results are size-2 ciphertexts in coefficient form with canonical words: modular arithmetic is exact, so they are the words of cn_mul_plain per term followed
 * by cn_add in any order.  With the register-radix kernels (1024 <= N <= 16384, every arithmetic policy, level contexts included) the distinct ciphertexts are
 * transformed once and ONE kernel per call lifts and transforms each plaintext, multiplies, accumulates in registers and transforms each sum back once: neither a
 * lifted plaintext nor a product exists in memory.  Other ring sizes, N = 16384 under the integer policy (moduli of 50 bits and more, or "f64" = 0: transform and
 * accumulators do not fit the registers of a 1024-thread workgroup) and "mp_fused" = 0 compose cn_mul_plain and cn_add_many through a temporary - same words.
 * Refused with CN_ERR_ARG, nothing written: G = 0, grp_off[0] != 0, an empty group, an index outside its handle, operands or outputs not of size 2, and an output
 * range that contains one of the ciphertexts the call reads.  Queued calls ("defer") are submitted first; under cn_graph_begin the index lists are captured by
 * value, like those of cn_add_many and cn_copy_many. */
int cn_mul_plain_sum(cn_ctx *ctx, cn_handle ct, uint32_t ci, cn_handle pt, uint32_t pi, const uint32_t *grp_off, const uint32_t *ct_idx, uint32_t G,
                     cn_handle out, uint32_t oi);
/* ---- NTT-form plaintext arrays: the weights of a fixed model, transformed once (Evaluator.TransformToNtt(Plaintext, parms_id), SEAL 3.2 evaluator.cpp; the
 * reference has no such call - every plaintext product of EncryptedSealBfvMatrix.cs:79-120 transforms its plaintext again).
 * An array holds `count` plaintexts as [count][k][N] words of ONE context: limb j of plaintext p is NTT_j(lift_j(m_p)), canonical residues mod q_j in the
 * library's transform order - the words of cn_ct_ntt on a polynomial whose limb j is lift_j(m).  It costs k times the memory of the coefficient form, so it is a
 * form the caller asks for.  A handle belongs to its context: a level context makes its own array (its first `limbs` limbs, transformed again).
 * cn_pt_transform: ptn[oi + i] = TransformToNtt(pt[pi + i]), i < count, with the plaintexts' zero flags; one kernel launch on 1024 <= N <= 16384 (allowed while
 * a graph is recorded and on level contexts); CN_ERR_ARG when either range leaves its handle.
 * cn_ptn_upload / cn_ptn_download move [count][k][N] words (a plan kept on disk or sent to another device); upload returns CN_ERR_ARG, nothing written, when a word
 * is not below its q_j, and derives the zero flags from the words.
 * cn_mul_plain, cn_rowdot_batch and cn_mul_plain_sum accept such a handle where they take `pt` (indices and strides count plaintexts): same words as with the
 * coefficient form, without any transform of the plaintexts - cn_mul_plain runs the product kernel alone (and is never queued under "defer": the queue is
 * flushed and the call runs at once), cn_rowdot_batch multiplies the rows where they lie, cn_mul_plain_sum streams them through one multiply-accumulate kernel
 * (cn_get_option "ptn_sum" / "ptn_bcast" count the launches of the last two; "ptn_sum_interval" is the number of terms between two recentrings of the FP64
 * accumulators).  CN_ERR_ZERO for a zero plaintext as before.  Every other call that takes a plaintext handle (cn_add_plain, cn_encrypt*, cn_decode*,
 * cn_pt_upload / cn_pt_download, the bias of cn_gemm_plan_create, the split / join calls) returns CN_ERR_ARG for one. */
int cn_ptn_alloc(cn_ctx *ctx, uint32_t count, cn_handle *out);
int cn_pt_transform(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t count, cn_handle ptn, uint32_t oi);
int cn_ptn_upload(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, const uint64_t *host);
int cn_ptn_download(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint64_t *host);
/* ---- the plaintexts of a generalized-diagonal dense layer, built where the weights lie (hewrapper.DEVICE_DIAGONAL_PLAN).  The reference encodes weight
 * ROWS (LLDenseLayer.Prepare -> EncryptedSealBfvMatrix.cs:79-120) and has no diagonal form; a host that wants one would decode the rows, index them along the diagonals
 * and encode again - 2 GiB of host traffic per plaintext prime at LoLa-CIFAR shapes.  These two calls read the matrix along its diagonals on the device.
 * rows[ri .. ri + R) are coefficient-form plaintexts of this context; row r holds W[r, x] in slot x for x < dim (W is zero outside R x dim, whatever the slots at dim
 * and above hold).  m = N / 2, slot s = h m + p.
 * cn_diag_scan: nonzero[c m + i] = 1 iff the generalized diagonal diag_(c,i)[h, p] = W[h m + p, (h ^ c) m + (p + i) mod m] has a non-zero slot, else 0 - every
 * non-zero W[h_r m + p_r, h_c m + x] sets flag (h_r ^ h_c, (x - p_r) mod m).  nonzero: N bytes of host memory.
 * cn_diag_encode: out[oi + e] = BatchEncoder.Encode(pre_e), e < count, for terms[e] = (c, J, b):
 *     pre_(c,J,b)[h, p] = W[(h ^ c) m + (p - J) mod m, h m + (p + b) mod m]
 * - diagonal (c, J + b) rotated back by the giant step J, the plaintext a baby-step giant-step product multiplies with the input rotated by b.  `out` is a cn_pt_alloc
 * array (the words of cn_encode_batch on those slot values) or a cn_ptn_alloc array (the words cn_pt_transform would then write; the staging in between is scratch of
 * at most 256 plaintexts).  The zero flags of `out` are those of cn_encode_batch / cn_pt_transform: an all-zero term is legal and leaves a zero plaintext, which the
 * products refuse with CN_ERR_ZERO.  Terms that are neighbours in the list with the same (c, J) and consecutive b - the order of a plan - are gathered 32 at a time
 * from contiguous row segments; any other order gives the same words, more slowly.
 * Both need batching (t == 1 mod 2N) and work on every ring size and on level contexts; an NTT-form `out` takes cn_pt_transform's path.  CN_ERR_ARG with a message that
 * names the argument, and nothing written: R > N, dim = 0 or dim > N, c > 1, J >= m, b >= m, a range that leaves `rows` or `out`, `rows` not a coefficient-form
 * plaintext handle, `out` the handle of `rows`, and under cn_graph_begin.  Queued calls ("defer") are submitted first.  Each call decodes the rows into scratch
 * (2 R N words) and keeps nothing; each waits for the device once, at its end.  cn_get_option "diag_scan" / "diag_encode" count the launches of their kernels. */
int cn_diag_scan(cn_ctx *ctx, cn_handle rows, uint32_t ri, uint32_t R, uint32_t dim, uint8_t *nonzero /* host, [2][N/2] */);
int cn_diag_encode(cn_ctx *ctx, cn_handle rows, uint32_t ri, uint32_t R, uint32_t dim, const uint32_t *terms /* host, [count][3] = c, J, b */, uint32_t count,
                   cn_handle out, uint32_t oi);

/* ---- client side on the device (what SEAL's KeyGenerator / Encryptor / Decryptor do for
 * AtomicSealBfvEncryptedEnvironment.SetKeys / Encrypt / Decrypt, AtomicSealBfvVector.cs:62-74,1030-1110,1202-1232), for data
 * owners that have a GPU.  Randomness: a ChaCha20 counter-mode generator (256-bit key per context, 64-bit nonce per call). ---- */
/* Sampler: ChaCha20 (RFC 7539 block function) in counter mode.  cn_set_rng_key installs the 256-bit key of the context (the data owner draws
 * it from the OS entropy source; default all zero = reproducible, for tests); the `seed` argument of cn_keygen / cn_encrypt is the 64-bit
 * nonce of the call - distinct calls under one key need distinct nonces (a counter or fresh entropy).  cn_set_rng_salt sets only the first
 * 64 key bits (kept for callers of the round-1 interface).
 * Every polynomial drawn takes the next value of the context's item counter (block counter = item | stream | redraw trial | block, as for CN_STREAM_A
 * below): cn_keygen RESETS it to 0 (item 0 = the secret key, 1 / 2 = the public a / noise, then two items per key entry), every other call goes on from it,
 * and a level context has a counter of its own that starts at 0.  Calls that share a nonce are distinct only through the counter: wherever it starts again
 * (a second cn_keygen, a level context) the nonce of an earlier call under the same key must not be used again - item 0 of stream 0 under the nonce of
 * cn_keygen IS the secret key.  tests/sampler_model.py restates every draw; tests/test_gpu_sampler_kat.py holds the device's words to it. */
int cn_set_rng_key(cn_ctx *ctx, const uint8_t *key32);
int cn_set_rng_salt(cn_ctx *ctx, uint64_t salt);
/* known-answer self-test of the generator: one raw block (16 words) for a key, the 64-bit block counter (state words 12-13) and the
 * 64-bit nonce (state words 14-15); RFC 7539 section 2.3.2 is the case counter = 0x0900000000000001, nonce = 0x4a000000 */
int cn_rng_selftest(cn_ctx *ctx, const uint8_t *key32, uint64_t counter, uint64_t nonce, uint32_t *out16);
int cn_keygen(cn_ctx *ctx, uint64_t seed, int with_galois);          /* secret, public, relin (dbc) and default Galois (gdbc) keys */
/* KeyGenerator.GaloisKeys(dbc, galois_elts) of SEAL 3.2: Galois keys for exactly the n listed elements (cn_galois_elt_from_step maps a RotateRows step),
 * generated and installed by ONE kernel launch behind one noise launch (k_ksk_gen) with one host wait at the end.  A rotation by a step whose element has a
 * key is ONE key switch; any other step is split into its non-adjacent form and pays one key switch per term (cn_rotate_rows).  An element the context already
 * holds is replaced.  Layout, convention ("ks_xi", gdbc) and form (FP64 image when the context keeps its keys as doubles) are those of cn_keygen's keys:
 * [(l,d)][2][k][N], NTT form.
 * THE WORDS are those cn_keygen's loop would have produced for these elements, continuing from the context's item counter item0: entry e = (l, d) of the
 * g-th listed element has  a = sample_uniform8(sampler key, seed, stream 3, item0 + 2 (g gk_tot + e), ...)  and its noise from stream 1 at the next item; the
 * counter advances by 2 n gk_tot.  So cn_keygen(seed, 1) on one context and cn_keygen(seed, 0) followed by cn_keygen_galois(seed, the default elements in
 * cn_keygen's order: 2N-1, then 3^(2^i), 3^-(2^i) for i = 0 .. log2(N) - 2) on another with the same sampler key hold identical keys.
 * Needs the secret key (CN_ERR_NOKEY) and 1024 <= N <= 16384.  CN_ERR_ARG - and nothing is installed - for an even element, an element >= 2N, an element
 * listed twice, on a level context and while a graph is recorded.  Flushes deferred work first; n = 0 returns 0. */
int cn_keygen_galois(cn_ctx *ctx, uint64_t seed, const uint64_t *galois_elts, uint32_t n);
/* The Galois elements this context holds a key for, ascending: *count = their number; elts (may be NULL when only the count is asked for) receives them if
 * cap >= *count, else CN_ERR_ARG (with *count set).  A level context reports the keys sliced from its parent. */
int cn_galois_elts(cn_ctx *ctx, uint64_t *elts, uint32_t cap, uint32_t *count);
/* Which rotations does a caller ask for?  cn_set_option(ctx, "record_steps", 1) starts recording, 0 stops and clears (off by default; cn_get_option reads it
 * back; a level context records into its own list and starts with recording off).  While it is on, the context notes every RotateRows step AS REQUESTED -
 * before the split into non-adjacent-form hops - by cn_rotate_rows, cn_rotate_rows_many, cn_rotate_rows_add (immediate or queued; step 0 is a copy and is not
 * noted), the steps -1, -2, -4, .. of cn_sum_slots and cn_rowdot_batch, the step of a cn_apply_galois element 3^s (as s or s - N/2, whichever is smaller in
 * magnitude), and whether a column rotation was asked for (cn_rotate_columns(_add), cn_apply_galois(2N - 1), a cn_sum_slots / cn_rowdot_batch over >= N/2 slots).
 * cn_rotation_steps returns the steps ascending and distinct: *count = their number, steps (may be NULL) receives them if cap >= *count, else CN_ERR_ARG
 * (with *count set); *columns (may be NULL) = 1 if a column rotation was asked for. */
int cn_rotation_steps(cn_ctx *ctx, int *steps, uint32_t cap, uint32_t *count, int *columns);
int cn_set_public_key(cn_ctx *ctx, const uint64_t *words, size_t count);   /* [2][k][N], NTT form */
int cn_set_secret_key(cn_ctx *ctx, const uint64_t *words, size_t count);   /* [k][N], NTT form */
int cn_get_key(cn_ctx *ctx, int which /*0 relin,1 galois,2 public,3 secret*/, uint64_t galois_elt, uint64_t *host, size_t count);
/* Encryptor.Encrypt of `count` dense plaintexts (pt = 0: encryptions of zero; pt_stride 0: the same plaintext).  With
 * cn_set_option("defer", 1) a call for up to 4 ciphertexts is queued like the evaluator calls (the unchanged PoolLayer encrypts a zero
 * vector per padded convolution tap, PoolLayer.cs:67-80: 645 calls per layer and plaintext prime become one launch chain).  Needs
 * 1024 <= N (the samplers run on the register-radix transforms); below, CN_ERR_ARG and nothing written. */
int cn_encrypt(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t pt_stride, cn_handle out, uint32_t oi, uint32_t count, uint64_t seed);
/* AllocateCiphertext + Encryptor.Encrypt(PlainZero) as ONE call: a new one-ciphertext array holding a fresh encryption of zero (PoolLayer.ElementAt per
 * padded tap, PoolLayer.cs:67-80; the IsZero branches of AtomicSealBfvVector.cs:566,587).  Same words and - under "defer" - the same queue entry as
 * cn_ct_alloc followed by cn_encrypt(pt = 0, count = 1, seed). */
int cn_encrypt_zero_new(cn_ctx *ctx, uint64_t seed, cn_handle *out);
/* ---- seeded symmetric ciphertexts: a fresh secret-key encryption whose c1 is regenerated from 32 public bytes, so that only c0 travels (half the
 * bytes of a fresh ciphertext; SEAL >= 3.4 ships the same idea, the framing here is this library's own).  Definition - part of the interface:
 *   a_j, limb j of item i:  sample_uniform8(a_seed, a_nonce, CN_STREAM_A, a_item0 + i, j (N/8) + b, q_j) for b = 0 .. N/8 - 1 - ChaCha20 block
 *       counter = item (40 bits) | stream (4) | redraw trial (4) | block (16), nonce words 14-15 = a_nonce, key = the 32 bytes of a_seed as eight
 *       little-endian words; a block yields 8 consecutive words v = (w[2c] << 32) | w[2c + 1], kept as v mod q_j if v <= 2^64 - 1 - (2^64 - 1) mod q_j - 1,
 *       else redrawn at the next trial - exactly the layout of the `a` of a key from cn_keygen.  It is read as the NTT form in the library's transform order.
 *   c1 = INTT(a),  c0 = INTT(-a . s) + e + Delta m, with the plaintext embedding (rounding term included) of cn_encrypt: cn_decrypt needs no change.
 *   a_seed is PUBLIC and travels with the c0 words; a does not depend on the context's sampler key or salt.  e never comes from a_seed: it is drawn
 *   like cn_encrypt's e1 from the context's secret sampler key (cn_set_rng_key / cn_set_rng_salt), stream 1, nonce `seed`, the context's item counter.
 *   Distinct ciphertexts under one a_seed need distinct (a_nonce, item); a_item0 + count <= 2^40.
 * Streams of the sampler: 0 ternary (secret key, u), 1 / 2 noise, 3 the uniform component of keys, CN_STREAM_A (= 4, defined with the error codes) the public a of
 * seeded ciphertexts. */
/* `count` size-2 ciphertexts out[oi ..) = symmetric encryptions of the plaintexts (pt = 0: of zero; pt_stride 0: the same plaintext).  Two inverse
 * transforms per (ciphertext, limb) against the four transforms of cn_encrypt, and fresh noise e instead of u e_pk + e1 + e2 s.  Needs the secret key
 * (CN_ERR_NOKEY) and 1024 <= N <= 16384; CN_ERR_ARG for a bad range, a null seed or while a graph is recorded.  Flushes deferred work first and is never
 * queued.  A level context encrypts at its own level, as it does with cn_encrypt (its slice of the secret key). */
int cn_encrypt_symmetric(cn_ctx *ctx, cn_handle pt, uint32_t pi, uint32_t pt_stride, cn_handle out, uint32_t oi, uint32_t count, uint64_t seed,
                         const uint8_t *a_seed32, uint64_t a_nonce, uint64_t a_item0);
/* writes poly 1 of the size-2 ciphertexts h[first .. first + count) from the seed; poly 0 is left alone.  Needs no key; works on level contexts (limbs are
 * independent: a level's c1 is the first limbs of its parent's).  Asynchronous on the context stream; CN_ERR_ARG while a graph is recorded. */
int cn_ct_expand(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, const uint8_t *a_seed32, uint64_t a_nonce, uint64_t a_item0);
/* host_c0 [count][k][N] -> poly 0 of h[first ..) with ONE strided copy, then the expansion of poly 1 on the context stream; synchronises like cn_ct_upload */
int cn_ct_upload_compact(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, const uint64_t *host_c0, const uint8_t *a_seed32, uint64_t a_nonce,
                         uint64_t a_item0);
/* poly 0 of the size-2 ciphertexts h[first ..) -> host [count][k][N]; synchronises */
int cn_ct_download_compact(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint64_t *host);
/* Packed rows - the library's own wire form of residues without padding bits (not a SEAL stream).  b_j = bit_length(q_j); the N residues of limb j are one
 * little-endian bit stream, coefficient i in bits [i b_j, (i + 1) b_j) of the row, bit p of the row = bit p % 64 of word p / 64; a row is N b_j / 64 words, a
 * packed ciphertext its rows in [poly][limb] order, a batch [ciphertext][poly][limb].  Needs N >= 1024; works on level contexts with that level's limbs.
 * words of a packed ciphertext of `polys` polynomials: polys * (N / 64) * sum_j b_j (0 when the context has no packed form) */
size_t cn_packed_words(cn_ctx *ctx, uint32_t polys);
/* h[first .. first + count) -> host as packed rows, polys = 1: poly 0 only, 0: every polynomial of h (size 2 or 3); staged through scratch, synchronises */
int cn_ct_download_packed(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint32_t polys, uint64_t *host);
/* packed rows -> h[first ..).  polys = 1: h of size 2, host holds c0 rows, poly 1 is expanded from the seed as in cn_ct_upload_compact; polys = 0: every
 * polynomial of h, the seed arguments are ignored.  Staged through scratch, synchronises like cn_ct_upload_compact.  A row can carry v >= q_j (q_j < 2^b_j):
 * the device stores v - q_j, so the array holds canonical words, and the call returns CN_ERR_ARG ("residue not below its modulus"); the destination is
 * otherwise unspecified then.  cn_get_option "packed_bad_residues" counts such calls. */
int cn_ct_upload_packed(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, uint32_t polys, const uint64_t *host, const uint8_t *a_seed32, uint64_t a_nonce,
                        uint64_t a_item0);
/* Decryptor.Decrypt of size-2 or size-3 ciphertexts into dense plaintexts */
int cn_decrypt(cn_ctx *ctx, cn_handle ct, uint32_t ci, uint32_t count, cn_handle pt_out, uint32_t pi);
/* Decryptor.InvariantNoiseBudget as CryptoTracker.TestBudget probes it (HE Wrapper/CryptoTracker.cs:41-52, BaseLayer.cs:37): writes the
 * residues of t*(c0 + c1 s + c2 s^2) mod q_j, [count][k][N], to `host`; the caller composes the limbs (CRT) and takes
 * budget = log2(q) - log2(centred infinity norm) - 1.  Needs the secret key (client-side context); synchronises. */
int cn_noise_poly(cn_ctx *ctx, cn_handle ct, uint32_t ci, uint32_t count, uint64_t *host);
/* The same probe reduced on the device: writes the exact centred infinity norm of t*(c0 + c1 s [+ c2 s^2]) mod q, k little-endian 64-bit
 * words per ciphertext, [count][k], to `host` (budget = bitcount(q) - bitcount(norm) - 1).  Size-2 and size-3 ciphertexts, any k <= 12, level
 * contexts (their slice of the secret key).  Flushes deferred work first; CN_ERR_NOKEY without the secret key, CN_ERR_ARG for an index out of
 * range, a null `host` or while a graph is recorded; count 0 returns 0.  Processes at most max(1, 2^24 / (k N)) ciphertexts per pass, so its
 * scratch stays bounded; synchronises. */
int cn_noise_norm(cn_ctx *ctx, cn_handle ct, uint32_t ci, uint32_t count, uint64_t *host /* [count][k] */);
/* ---- the reply path on the device: Decryptor.Decrypt + BatchEncoder.Decode + JoinSplitNumbers (EncryptedSealBfvVector.cs:381-411) of `count` ciphertexts per
 * plaintext prime in ONE call - no plaintext and no per-prime slot array reaches the host.  ctxs[i]: the context of plaintext prime t_i, ct[i] / ci[i]: handle and
 * first index in ctxs[i] (ci NULL = 0).
 *   v_i[c][s]  slot s of Decode(Decrypt(ct_i[c])) in the slot order of cn_decode_batch; with CN_JOIN_COEFF0 coefficient 0 of the decrypted plaintext (the wrapper's sparse
 *              format: nslots must be 1, no transform runs)
 *   x          the unique integer in [0, M), M = prod t_i, with x == v_i (mod t_i) for every i; with CN_JOIN_SIGNED, x - M when 2x > M
 *   words      x as W = cn_join_words little-endian 64-bit words, two's complement: [count][nslots][W]
 *   values     double(x) / scale: round-to-nearest-even of the exact integer (up to 255 bits), then the IEEE division - Python's float(x) / scale: [count][nslots]
 *   argmax[s]  the lowest c whose integer x[c][s] is largest (compared as integers, not as doubles): [nslots]
 * Accepted: 1 <= P <= 8 contexts of one device and one N, level contexts included (their slice of the secret key), with pairwise different prime t_i and M < 2^255;
 * size-2 and size-3 ciphertexts.  Refused with CN_ERR_ARG (a missing secret key: CN_ERR_NOKEY), nothing written: P = 0 or P > 8, equal moduli, a different N or device,
 * nslots = 0 or > N, CN_JOIN_COEFF0 with nslots != 1, the dense form on a context without batching, all three outputs NULL, an index range outside its handle, a
 * recording in progress on any context.  count = 0 returns 0.  Takes every context's lock (more limbs first, as cn_mod_switch), submits every context's deferred work
 * first, runs each prime's decryption on its own context's stream into a join buffer of ctxs[0] (ordered by events, no host wait in between), the join on ctxs[0]'s
 * stream, and synchronises once.  cn_join_words: W = ceil((bit_length(M) + 1) / 64), or CN_ERR_ARG for a list cn_decrypt_join refuses. */
#define CN_JOIN_SIGNED (1u)
#define CN_JOIN_COEFF0 (2u)
int cn_join_words(cn_ctx *const *ctxs, uint32_t P);
int cn_decrypt_join(cn_ctx *const *ctxs, uint32_t P, const cn_handle *ct, const uint32_t *ci, uint32_t count, uint32_t nslots, uint32_t flags,
                    double scale, double *values /* [count][nslots] or NULL */, uint64_t *words /* [count][nslots][W] or NULL */,
                    int32_t *argmax /* [nslots] or NULL */);
/* ---- the request path on the device: SplitBigNumbers (EncryptedSealBfvVector.cs:352-365) + BatchEncoder.Encode [+ Encryptor.Encrypt] (AtomicSealBfvVector.cs:1114-1232) of
 * `count` plaintexts per plaintext prime in ONE call - one upload of the values, no per-prime residue array on the host.  ctxs[i]: the context of plaintext prime t_i,
 * pt[i] / pi[i] (ct[i] / ci[i]): handle and first index in ctxs[i] (pi / ci NULL = 0).  For plaintext c < count and slot s < nvalues the input element is
 * values[c * stride_ct + s * stride_slot]; the strides count elements of 8 bytes (a row-major [image][feature] matrix is read as it lies, no host transpose).
 *   w          doubles (the default): r = rint(x * scale) - one IEEE double multiply, then round to nearest even; the call is refused when any r is NaN, infinite or
 *              |r| >= 2^62; w = (int64) r.  CN_SPLIT_I64: the elements are int64_t and w is the element (every int64, INT64_MIN included; scale is ignored)
 *   v_i[c][s]  w mod t_i as the representative in [0, t_i)
 *   plaintext  c of context i: BatchEncoder.Encode of the slots v_i[c][0 .. nvalues), zero beyond, in the slot order and with the transform of cn_encode_batch (equal
 *              words); with CN_SPLIT_COEFF0 the constant polynomial v_i[c][0] (the wrapper's sparse format: nvalues must be 1, no transform runs)
 *   zero       zero[i * count + c] = 1 when every coefficient of that plaintext is zero; cn_split_encode sets the handles' zero flags (what cn_mul_plain refuses
 *              by) to the same exact values
 *   cn_split_encrypt   ct[i][ci[i] + c] = cn_encrypt of that plaintext under the nonce seeds[i]: the words of cn_encode_batch + cn_encrypt(pt, 0, 1, ct[i], ci[i], count,
 *              seeds[i]) on a context in the same sampler state, and the item counter advances as in that call.  Public-key encryption only: the symmetric, compact
 *              and packed forms take cn_split_encode and then their own per-context call.  The plaintexts live in each context's scratch.
 * Accepted: 1 <= P <= 8 different contexts of one device and one N, level contexts included; the t_i need not differ.  Refused with CN_ERR_ARG before anything is
 * enqueued: P = 0 or P > 8, a different N or device, nvalues > N, nvalues = 0 in the dense form, CN_SPLIT_COEFF0 with nvalues != 1, the dense form on a context without
 * batching, a null values / pt / ct / seeds, an index range outside its handle, a ciphertext array of size 3, a recording in progress on any context, cn_split_encrypt
 * with N < 1024 (cn_encrypt's own limit).  cn_split_encrypt without a public key: CN_ERR_NOKEY.  count = 0 returns 0.  A value out of range is found on the device:
 * the call returns CN_ERR_ARG ("value does not fit") and the destinations are unspecified, as for cn_ct_upload_packed's bad residues.
 * Takes every context's lock (the order of cn_decrypt_join), submits every context's deferred work first, uploads the strided extent of the values once into ctxs[0]'s
 * scratch, splits on ctxs[0]'s stream into all P destinations, runs each prime's inverse transform mod t and encryption on its own context's stream (ordered by events,
 * no host wait in between), in passes of at most max(1, 2^24 / N) plaintexts, and synchronises once. */
#define CN_SPLIT_I64    (1u)   /* values are int64_t and are taken as they are; scale is ignored */
#define CN_SPLIT_COEFF0 (2u)   /* the wrapper's sparse format: the value becomes coefficient 0 of a constant plaintext; nvalues must be 1, no transform runs */
int cn_split_encode(cn_ctx *const *ctxs, uint32_t P, const void *values, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues, uint32_t flags,
                    double scale, const cn_handle *pt, const uint32_t *pi /* NULL = 0 */, uint8_t *zero /* [P][count] or NULL */);
int cn_split_encrypt(cn_ctx *const *ctxs, uint32_t P, const void *values, int64_t stride_ct, int64_t stride_slot, uint32_t count, uint32_t nvalues, uint32_t flags,
                     double scale, const cn_handle *ct, const uint32_t *ci /* NULL = 0 */, const uint64_t *seeds /* [P] */);

/* ---- raw transforms (kernel benchmarks / parity tests of the NTT itself) --------------- */
/* in-place negacyclic NTT over `limbs` limbs of N words at a device pointer; limb i uses modulus
 * (i % nmod) of base 0 (coeff moduli q) or base 1 (BEHZ Bsk moduli).  Async on the ctx stream. */
int cn_ntt_forward(cn_ctx *ctx, void *dev_ptr, uint32_t limbs, int base);
int cn_ntt_inverse(cn_ctx *ctx, void *dev_ptr, uint32_t limbs, int base);
int cn_ct_ntt(cn_ctx *ctx, cn_handle h, uint32_t first, uint32_t count, int inverse);   /* same on a ct array */
/* times `iters` back-to-back launches of the forward NTT kernel with HIP events on the ctx
 * stream; returns average milliseconds per launch in *ms. */
int cn_ntt_time(cn_ctx *ctx, void *dev_ptr, uint32_t limbs, int base, int inverse, int iters, float *ms);
/* VALU issue rate of the device at this moment: ns per wave-instruction per SIMD, measured with `launches` launches of a kernel that only
 * runs arithmetic chains (512-thread workgroups, one per CU, two waves per SIMD - the fused key switch's occupancy).  kind 0: FP64, chains
 * of the exact modular multiply (`iters` x 48 instructions per thread); kind 1: full-rate 32-bit integer VALU (`iters` x 24).  bench.py
 * prices the key switch's instruction counts with them. */
int cn_valu_issue_time(cn_ctx *ctx, int kind, int iters, int launches, float *ns_per_instr);
void *cn_stream(cn_ctx *ctx);                       /* hipStream_t of the context */
int cn_event_time_begin(cn_ctx *ctx);               /* HIP-event stopwatch on the ctx stream */
int cn_event_time_end(cn_ctx *ctx, float *ms);

/* ---- statistics = OperationsCount (AtomicSealBfvVector.cs:211-294) ---------------------- */
typedef struct cn_stats {
    uint64_t Multiplication, PlainMultiplication, Addition, PlainAddition, Subtraction, PlainSubtraction,
        Rotation, AddMany, AddManyItemCount, Relinarization;   /* reference names */
    uint64_t ntt_forward_limbs, ntt_inverse_limbs, kernel_launches;
} cn_stats;
int cn_stats_get(cn_ctx *ctx, cn_stats *out, int reset);

#ifdef __cplusplus
}
#endif
#endif
