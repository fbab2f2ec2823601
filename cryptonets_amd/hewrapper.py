"""Host-side mirror of the reference's HE wrapper (`HE Wrapper/*.cs`) on top of libcnhip.

Same names, argument meaning and error behaviour as the C# classes so the parity tests read like the reference's
MSTest suite:
  AtomicSealBfvEncryptedEnvironment / AtomicSealBfvEncryptedVector   <- AtomicSealBfvVector.cs
  EncryptedSealBfvEnvironment / EncryptedSealBfvVector               <- EncryptedSealBfvVector.cs (CRT over plaintext primes)
  EncryptedSealBfvMatrix                                             <- EncryptedSealBfvMatrix.cs
  EncryptedSealBfvFactory                                            <- IFactory.cs:240-410
Every `epenv.evaluator.*` call of the reference becomes a (batched) libcnhip call on device-resident ciphertext
arrays.  What stays on the client in the reference (KeyGenerator, Encryptor, Decryptor - SEAL calls at
AtomicSealBfvVector.cs:62-74,1042,1211) is behind the small `ClientCrypto` interface: the evaluator never sees a
secret key.  BatchEncoder (public math) runs on the device (cn_encode / cn_decode).
"""
import enum
import os
import math

import numpy as np


class EVectorFormat(enum.Enum):
    dense = 0
    sparse = 1


class EMatrixFormat(enum.Enum):
    ColumnMajor = 0
    RowMajor = 1



# LITERAL = True: the matrix- and layer-level conveniences of this mirror (RowsDotProduct, MulColumnsByPlain, the batched LLPoolLayer /
# MulManySparse forms) are switched off and every layer takes the per-vector path the reference's UNCHANGED files take - one
# AtomicSealBfvEncryptedVector method call per row / column / map (EncryptedSealBfvMatrix.cs:79-120, LLPoolLayer.cs, LLInterleaveLayer.cs,
# LLDenseLayer.cs).  That is the call sequence the C# twin receives; tools/call_trace.py records it at the C ABI and
# tools/replay_call_trace.cpp replays it from native code (bench.py --workload lola: `unchanged_caller`).  Same ciphertext words.
# What a vector method does INSIDE is the twin's own business on both sides of the switch: AtomicSealBfvEncryptedVector is the file the twin
# replaces (integration/GpuAtomicSealBfvEncryptedVector.cs), and like it this class gathers with cn_copy_many and rotates the vectors of an
# Interleave / the copies of a Duplicate with one cn_rotate_rows_many.
LITERAL = bool(int(os.environ.get("CN_LITERAL_CALLS", "0")))


def set_literal(on):
    global LITERAL
    LITERAL = bool(on)


# The reply path: EncryptedSealBfvVector.Decrypt / DecryptFullPrecision and EncryptedSealBfvMatrix.Decrypt decrypt, decode and CRT-join on the device with one
# cn_decrypt_join call when every environment's client is a device client (profiles/reply_probe.txt).  False: always the per-prime path (decrypt, download, decode,
# join slot by slot with Python integers) - which host clients, the oracle backends and plaintext vectors take in either case.
DEVICE_JOIN = True


def _device_join_ok(env):
    """may cn_decrypt_join serve this CRT environment?  Device clients on library contexts, at most 8 primes, their product below 2^255"""
    if not DEVICE_JOIN:
        return False
    envs = getattr(env, "Environments", None)
    if not envs or len(envs) > 8 or env.bigFactor >> 255:
        return False
    return all(hasattr(e.client, "decrypt_device") and hasattr(e.ctx, "_h") and hasattr(e.ctx, "L") for e in envs)


# The request path: EncryptedSealBfvVector(...) and EncryptedSealBfvFactory.GetEncryptedMatrix / GetPlainMatrix scale, round, split, encode and encrypt on the
# device with one cn_split_encrypt / cn_split_encode call for all blocks (columns) and plaintext primes when every environment's client is a device client on a
# library context (profiles/request_probe.txt).  False: always the host path (np.rint, one np.mod per prime, then one encode + encrypt per vector and prime) -
# which host clients, the oracle backends, Python integers beyond int64, values of 2^62 and beyond after scaling and sparse plaintext vectors (host lists of
# integers) take in either case.
DEVICE_SPLIT = True


# The dense layers: EncryptedSealBfvMatrix.Mul(..., ForceDenseFormat=True) on a batchable row-major plaintext matrix as a generalized-diagonal product with
# baby-step giant-step rotations (diagonal.py): the input vector is rotated, ONE cn_mul_plain_sum multiplies the rotations by the matrix's diagonals
# and sums them, the sums are rotated and added - instead of one product per row, a SumAllSlots chain on each and a one-hot mask.  Taken if and only if
# diagonal.dense_path_counts counts fewer limb transforms for it (a 10 x 5488 layer keeps the default path).  The decrypted slots are those of the default path
# (the same integer linear map mod t); the ciphertext words and the noise differ.  False (default): the calls and words of the default path, always.
# profiles/diag_dense.md: what was measured.
DIAGONAL_DENSE = False
# NTT_WEIGHTS = True: the weight plaintexts a row-major matrix keeps on the device for its products - the row plaintexts and one-hot masks of RowsDotProduct, the
# pre-rotated diagonals of DiagonalDense - are kept in NTT form (cn_pt_transform): every later product multiplies without transforming them again.
# Same ciphertext words.  The arrays are k times the coefficient form (CIFAR: rows 5.4 GiB, diagonals 16 GiB per prime), so this is asked for, never a default;
# a backend without pt_transform (the CPU oracle of the tests) keeps the coefficient form.
NTT_WEIGHTS = False
# DEVICE_DIAGONAL_PLAN = True: the pre-rotated diagonals of DiagonalDense are built where the weights lie (cn_diag_scan, cn_diag_encode): one scan of the row
# plaintexts for the non-zero diagonals, the plan from those flags (diagonal.plan_from_flags), an array of exactly plan.terms plaintexts and ONE call that fills it -
# instead of decode_batch to the host, numpy index arrays and encode_batch per chunk of 256 candidates.  The same plan and plaintext words, hence the same ciphertext
# words.  False (default) until the two routes have been measured side by side (profiles/diag_device_plan.md); a backend without diag_scan (the CPU oracle of the
# tests) keeps the host route.
DEVICE_DIAGONAL_PLAN = False


# HOISTED_ROTATIONS = True: the places that rotate ONE ciphertext by many step counts - the copies of Duplicate, the baby steps of DiagonalDense - ask for one hoisted
# call (cn_rotate_rows_hoisted, DESIGN 6j: the digit transforms of the input once, two launches, every copy one key switch away from the input) when the context
# holds the own Galois key of every step; the baby steps are then never "by doubling".  A context that lacks a key (CN_ERR_NOKEY) or has no kernel for the call (the
# planner's refusals for the ring size / "legacy_ntt" and for the integer policy at N = 16384) takes the present route; any other error is raised.  The decrypted slots are the same; the ciphertext words and the noise differ (the words of tests/hoisted_model.py).  Direct
# keys for B - 1 baby steps cost (B - 1) digits 2 k N 8 bytes per plaintext prime (2 GiB at the CIFAR layer, against the 7 keys of doubling): networks.rotation_steps
# reports the direct steps under this switch, so GenerateEncryptionKeys(steps=...) makes exactly them.  False (default): nothing changes - the switch stays off until
# the routes have been measured side by side (profiles/hoisted_rotations.md).
HOISTED_ROTATIONS = False


def _rotate_hoisted(ctx, h, first, steps, out_h, out_idx):
    """out_h[out_idx[r]] = the rotation of h[first] by steps[r] through one hoisted call; False (nothing written): the switch is off, the backend has no such
    call, a key is missing (CN_ERR_NOKEY) or the context has no kernel for it (the two refusals of the planner: ring size / "legacy_ntt", the integer policy at
    N = 16384) - the caller takes its present route.  Every other error is the caller's and is raised.  While the context records steps, a call that lacks a key
    still notes the steps it asked for (Context.note_hoisted_steps; rotation_steps returns them): the keys to generate are those of the direct steps."""
    if not HOISTED_ROTATIONS or not hasattr(ctx, "rotate_rows_hoisted"):
        return False
    from ._native import CN_ERR_ARG, CN_ERR_NOKEY, HOISTED_UNAVAILABLE, CnError
    steps = [int(s) for s in steps]
    try:
        ctx.rotate_rows_hoisted(h, first, steps, out_h, list(out_idx))
        return True
    except CnError as e:
        if e.code == CN_ERR_NOKEY:
            ctx.note_hoisted_steps(steps)
            return False
        if e.code == CN_ERR_ARG and any(text in str(e) for text in HOISTED_UNAVAILABLE):
            return False
        raise


# SUMMED_ROTATIONS = True: the places that add up rotations of DIFFERENT ciphertexts - the output blocks of Interleave, the selections of Permute, the giant steps
# of DiagonalDense - ask for one summed call (cn_rotate_rows_sum, DESIGN 6k: every term its forward digit transforms and key products, ONE pair of inverse
# transforms per output limb, no rotated term stored, no dependence between the terms).  The call writes the words of the rotations followed by AddMany, so Interleave
# and Permute return the ciphertext words of the switch-off run; DiagonalDense returns the same slots with other words where the present route folds (folding
# rotates sums).  A step without its own key runs its non-adjacent-form hops inside the call; with "record_steps" on the giant steps are noted, so
# networks.rotation_steps and GenerateEncryptionKeys(steps=...) make their direct keys.  A backend without the call (the CPU oracle of the tests) keeps the present
# route.  False (default): nothing changes - the switch stays off until the routes have been measured side by side (profiles/rotation_sum.md).
SUMMED_ROTATIONS = False


def _summed(ctx):
    return SUMMED_ROTATIONS and hasattr(ctx, "rotate_rows_sum")


def _hoisted_keys_held(ctx, B):
    """does the context hold the own Galois key of every baby step 1 .. B - 1 (what a hoisted call of DiagonalDense needs)?"""
    return hasattr(ctx, "rotate_rows_hoisted") and all(ctx.has_galois_key(ctx.galois_elt_from_step(s)) for s in range(1, B))


def _device_split_ok(env, encrypt):
    """may cn_split_encode / cn_split_encrypt serve this CRT environment?  Device clients on library contexts, at most 8 primes; encryption on the ring
    sizes cn_encrypt takes"""
    if not DEVICE_SPLIT:
        return False
    envs = getattr(env, "Environments", None)
    if not envs or len(envs) > 8:
        return False
    if not all(hasattr(e.client, "encrypt_device") and hasattr(e.client, "_call_seed") and hasattr(e.ctx, "_h") and hasattr(e.ctx, "L") for e in envs):
        return False
    if any("encode_batch" in vars(e.ctx) for e in envs):          # a call-trace recorder wraps the context's methods (tools/call_trace.py): it records the per-context calls
        return False
    return not encrypt or 1024 <= envs[0].ctx.n <= 16384


def _device_split(env, values, encrypt, coeff0, scale):
    """values [count][nvalues] (float64 or int64, any strides) -> per environment a view of ONE fresh array of `count` ciphertexts (or plaintexts) and the zero
    flags [P][count] (None for ciphertexts); None when a value does not fit (2^62 and beyond after scaling, NaN): the caller's host path reports or handles it"""
    from . import _native
    envs = env.Environments
    ctxs = [e.ctx for e in envs]
    views = [_Buf(c, "ct" if encrypt else "pt", values.shape[0]).view() for c in ctxs]
    try:
        if encrypt:
            _native.split_encrypt(ctxs, values, [v.h for v in views], None, [e.client._call_seed() for e in envs], scale=scale, coeff0=coeff0)
            return views, None
        return views, _native.split_encode(ctxs, values, [v.h for v in views], None, scale=scale, coeff0=coeff0)
    except BaseException as ex:
        for v in views:
            v.release()
        if isinstance(ex, _native.CnError) and ex.code == -1 and "does not fit" in str(ex):
            return None
        raise


class ClientCrypto:
    """The client-side SEAL objects of AtomicSealBfvEncryptedEnvironment.SetKeys (AtomicSealBfvVector.cs:62-74):
    KeyGenerator / Encryptor / Decryptor for ONE plaintext modulus."""

    def generate_keys(self, with_galois=True, steps=None, columns=True):
        """steps: None = the default Galois key set; a list of RotateRows step counts = KeyGenerator.GaloisKeys(dbc, steps) (+ the column swap when
        `columns`).  A client that cannot generate keys for a list of its own keeps the one-argument form: GenerateEncryptionKeys(steps=...) is
        refused for it with a message, not with a TypeError from the call."""
        raise NotImplementedError

    def relin_key(self):            # u64 words, layout of include/cnhip.h
        raise NotImplementedError

    def galois_keys(self):          # dict galois_elt -> u64 words
        raise NotImplementedError

    def encrypt(self, plain):       # N plaintext coefficients -> size-2 ciphertext words
        raise NotImplementedError

    def decrypt(self, ct):          # ciphertext words -> N plaintext coefficients
        raise NotImplementedError

    def reference_evaluator(self):
        """The client's OWN evaluator on host words, or None.  AtomicSealBfvEncryptedEnvironment keeps a live SEAL `Evaluator` next to
        the keys (AtomicSealBfvVector.cs:22,66); the start-up self-test (AtomicSealBfvEncryptedEnvironment.SelfTest) runs a handful of
        operations through it and through the device and compares ciphertext WORDS.  Methods, all on flat u64 word arrays:
        multiply_plain(ct, plain_coeffs) (a length-1 plain = constant plaintext), add_plain(ct, plain_coeffs), multiply(a, b) -> size 3,
        relinearize(c3), rotate_rows(ct, steps), rotate_columns(ct)."""
        return None

    def relin_key_coeff_form(self):   # the relinearisation key with every polynomial in COEFFICIENT form (Evaluator.TransformFromNTTInplace), or None
        return None

    def galois_keys_coeff_form(self):
        return None


# ------------------------------------------------------------------------------------------------ device buffers
class _Buf:
    """Ref-counted device array of ciphertexts (kind 'ct'), dense plaintexts (kind 'pt') or NTT-form plaintexts (kind 'ptn')."""

    def __init__(self, ctx, kind, count, size=2):
        self.ctx, self.kind, self.count, self.size, self.refs = ctx, kind, count, size, 0
        self.h = ctx.ct_alloc(count, size) if kind == "ct" else (ctx.ptn_alloc(count) if kind == "ptn" else ctx.pt_alloc(count))

    def view(self, first=0, count=None):
        return _View(self, first, self.count - first if count is None else count)


class _View:
    def __init__(self, buf, first, count):
        self.buf, self.first, self.count = buf, first, count
        buf.refs += 1
        self.live = True

    def release(self):
        if self.live:
            self.live = False
            self.buf.refs -= 1
            if self.buf.refs == 0 and self.buf.h is not None:
                self.buf.ctx.free(self.buf.h)
                self.buf.h = None

    def sub(self, i, count=1):
        return _View(self.buf, self.first + i, count)

    @property
    def h(self):
        return self.buf.h


def _gather(ctx, views):
    """Return (buffer handle, [index per ciphertext], temp view or None) with every ciphertext of `views` in ONE device
    array: in place when they already share a buffer, otherwise packed into a temporary (device-to-device copies)."""
    b0 = views[0].buf
    if all(v.buf is b0 for v in views):
        return b0.h, [v.first + i for v in views for i in range(v.count)], None
    total = sum(v.count for v in views)
    tmp = _Buf(ctx, "ct", total).view()
    if hasattr(ctx, "copy_many"):                          # one launch for the whole gather (cn_copy_many) instead of one per vector
        ctx.copy_many([v.h for v in views for _ in range(v.count)], [v.first + i for v in views for i in range(v.count)], tmp.h, 0)
        return tmp.h, list(range(total)), tmp
    pos, idx = 0, []
    for v in views:
        ctx.copy(v.h, v.first, tmp.h, pos, v.count)
        idx.extend(range(pos, pos + v.count))
        pos += v.count
    return tmp.h, idx, tmp


# ------------------------------------------------------------------------------------------------ CRT fan-out
PARALLEL_PRIMES = os.environ.get("CN_PARALLEL_PRIMES", "0") != "0"
_crt_pool = None


def _fan_out(envs, fn):
    """ForEveryEncryptedVector (EncryptedSealBfvVector.cs:225-236): the reference issues every operation as one Task per
    plaintext prime.  Here each prime is a device context with its own HIP stream and every libcnhip call only ENQUEUES work, so
    one host thread walking the primes in turn already keeps the streams busy; the Task-per-prime form (CN_PARALLEL_PRIMES=1,
    one host thread per prime, ctypes drops the GIL inside libcnhip) was measured SLOWER for single-image LoLa - 27 ms vs 17.7 ms
    per image - the four threads spend their time handing the GIL to each other between ~25 us calls."""
    global _crt_pool
    if len(envs) == 1 or not PARALLEL_PRIMES:
        return [fn(i, e) for i, e in enumerate(envs)]
    if _crt_pool is None:
        from concurrent.futures import ThreadPoolExecutor
        _crt_pool = ThreadPoolExecutor(max_workers=8, thread_name_prefix="crt")
    futures = [_crt_pool.submit(fn, i, e) for i, e in enumerate(envs)]
    results, first_error = [], None
    for f in futures:                       # wait for every prime before raising: no task may outlive the call
        try:
            results.append(f.result())
        except Exception as ex:             # noqa: BLE001 - re-raised below
            first_error = first_error or ex
            results.append(None)
    if first_error is not None:
        raise first_error
    return results


# ------------------------------------------------------------------------------------------------ levels (modulus switching)
def _level_lift(ctx, parent_ctx, ctwords):
    """a ciphertext at the level q[:l] of `parent_ctx`'s chain -> a ciphertext over all of q that decrypts to the SAME plaintext with the same noise
    budget: x -> (Q/Q') x mod Q per coefficient (limb j < l: x_j (Q/Q' mod q_j); the other limbs: 0, since q_j divides Q/Q').  Exact: t (Q/Q') x mod Q =
    (Q/Q') (t x mod Q'), so round(t v / Q) and the centred norm relative to Q are those of the level.  A host-side client (SEAL at the first level)
    decrypts and probes level ciphertexts through it."""
    l, k, n = ctx.k, parent_ctx.k, ctx.n
    w = np.ascontiguousarray(ctwords, dtype=np.uint64).reshape(-1, l, n)
    P = 1
    for qj in parent_ctx.q[l:]:
        P *= int(qj)
    out = np.zeros((w.shape[0], k, n), dtype=np.uint64)
    for j in range(l):
        qj = int(parent_ctx.q[j])
        out[:, j] = ((w[:, j].astype(object) * (P % qj)) % qj).astype(np.uint64)
    return out.reshape(-1)


class _LevelClient:
    """The data owner's side of a level environment (Decryptor / noise probes of ciphertexts at the level; keys and encryption stay at the
    first level, as in SEAL 3.2).  Host clients see the exact lift of the ciphertext to the first level (_level_lift)."""

    def __init__(self, ctx, root_ctx, parent):
        self.ctx, self.root_ctx, self.parent = ctx, root_ctx, parent

    def decrypt(self, ct):
        return self.parent.decrypt(_level_lift(self.ctx, self.root_ctx, ct))

    def noise_budget_words(self, ct):
        return self.parent.noise_budget_words(_level_lift(self.ctx, self.root_ctx, ct))


class _LevelDeviceClient(_LevelClient):
    """... of a device client: the level context holds the slice of the secret key, decryption and probes run where the ciphertext lives"""

    def decrypt_device(self, ct_handle, first, count):
        pt = self.ctx.pt_alloc(count)
        try:
            self.ctx.decrypt(ct_handle, first, count, pt, 0)
            return self.ctx.pt_download(pt, 0, count)
        finally:
            self.ctx.free(pt)

    def noise_budget(self, ct_handle, first=0, count=1):
        return self.ctx.invariant_noise_budget(ct_handle, first, count, exact_bits=True)

    def decrypt(self, ct):
        w = np.ascontiguousarray(ct, dtype=np.uint64)
        h = self.ctx.ct_alloc(1, w.size // (self.ctx.k * self.ctx.n))
        try:
            self.ctx.ct_upload(h, 0, w[None, :])
            return self.decrypt_device(h, 0, 1)[0]
        finally:
            self.ctx.free(h)


def _ctx_limbs(ctx):
    return getattr(ctx, "k", None)


def _env_at(env, limbs):
    """the environment of level `limbs` on env's chain (env itself for None - plaintext operands - or an environment without levels)"""
    if limbs is None or not hasattr(env, "Level"):
        return env
    return env.Level(limbs)


def _check_level(env, *vectors):
    """SEAL's parameter-mismatch check (Evaluator: "encrypted1 and encrypted2 parameter mismatch"): every ciphertext operand must be at the
    level of the environment the operation runs in"""
    want = _ctx_limbs(env.ctx)
    for v in vectors:
        d = getattr(v, "encData", None)
        if d is not None and want is not None and _ctx_limbs(d.buf.ctx) not in (None, want):
            raise Exception("parameter mismatch: an operand is at level %d, the environment at level %d (ModSwitchTo first)" % (_ctx_limbs(d.buf.ctx), want))


# ------------------------------------------------------------------------------------------------ atomic layer
class AtomicSealBfvEncryptedEnvironment:
    """One plaintext modulus = one device context + its evaluation keys (AtomicSealBfvVector.cs:19-206)."""

    def __init__(self, ctx, client=None):
        self.ctx, self.client = ctx, client
        self.plainmodulusValue = ctx.t
        self.ParentFactory = None
        self._root, self._levels = self, {}

    # -- levels (SEAL 3.2 has no special prime: every prefix q[:l] of the coefficient modulus is a level) -------------------------------
    @property
    def Limbs(self):
        """coefficient moduli of this environment (its level)"""
        return self.ctx.k

    def Level(self, limbs):
        """the environment of the level q[:limbs] of this environment's chain (created once, cached at the first level): a level context
        (keys sliced from the first level's, cn_ctx_create_level) and the client's side of it.  Level(Limbs of the first level) is the first level."""
        root = self._root
        limbs = int(limbs)
        if limbs == root.ctx.k:
            return root
        if limbs not in root._levels:
            if not hasattr(root.ctx, "level"):
                raise Exception("this context has no modulus-switching chain")
            lctx = root.ctx.level(limbs)
            cls = _LevelDeviceClient if hasattr(root.client, "decrypt_device") else _LevelClient
            e = AtomicSealBfvEncryptedEnvironment(lctx, cls(lctx, root.ctx, root.client))
            e.ParentFactory, e._root = root.ParentFactory, root
            root._levels[limbs] = e
        return root._levels[limbs]

    @property
    def SlotCount(self):
        return self.ctx.n

    @property
    def PlaintextCapacity(self):
        return self.ctx.n

    @property
    def Primes(self):
        return [self.plainmodulusValue]

    def GenerateEncryptionKeys(self, with_galois=True, steps=None):
        """KeyGenerator + SetKeys (AtomicSealBfvVector.cs:62-74,163-173): keys are made by the client, the public
        evaluation keys are uploaded to HBM.  steps: None = the default Galois key set (the reference's); a list of RotateRows step counts =
        KeyGenerator.GaloisKeys(dbc, steps), keys for exactly these rotations and the column swap (client.DeviceClient.generate_keys)."""
        if steps is None:
            self.client.generate_keys(with_galois)
        else:
            import inspect
            if "steps" not in inspect.signature(self.client.generate_keys).parameters:
                raise Exception("%s cannot generate Galois keys for a list of steps (its generate_keys takes no `steps`)" % type(self.client).__name__)
            self.client.generate_keys(with_galois, steps=[int(x) for x in steps])
        rk = self.client.relin_key()
        if rk is not None:                       # a device-side client has already installed its keys in the context
            self.ctx.set_relin_key(rk)
        if with_galois:
            for elt, words in self.client.galois_keys().items():
                self.ctx.set_galois_key(elt, words)
        self.SelfTest(with_galois, steps=steps)

    # what the last SelfTest found: None (not run: the client has no evaluator of its own), or a dict
    #   {"ks_xi": 0 | 1, "key_form": "ntt" | "coeff", "ops": [names compared], "tried": [(ks_xi, key_form, first failing op or None), ...],
    #    "warnings": [key-less operations whose words differ from the client's evaluator while their decrypted slots agree]}
    self_test_report = None

    def SelfTest(self, with_galois=True, steps=None):
        """Start-up agreement check of the drop-in with the evaluator it replaces (the C# twin does the same at the end of
        CreateDevice, integration/GpuAtomicSealBfvEncryptedVector.cs).  Two fresh ciphertexts go through the client's own evaluator and
        through the device: MultiplyPlain (dense and constant), AddPlain, Multiply - then the key-switching operations Relinearize,
        RotateRows(+1), RotateRows(-1), RotateColumns.  WORDS are compared.  Two things about real SEAL 3.2 keys cannot be read off
        the reference (SEAL is an un-vendored dependency): which decomposition convention the key switch uses (cn_set_option "ks_xi")
        and whether the NTT-form key words are in this library's transform order.  So when a key-switching operation disagrees the test
        retries with the other convention, then with coefficient-form keys (cn_load_key form 1: the device transforms them itself),
        and keeps the first combination that reproduces the client's words.  Nothing matches: an exception that names the operation -
        never rc 0 and garbage.  With keys for a caller's own steps (GenerateEncryptionKeys(steps=...)) the two row rotations are by steps of
        that list - rotations the context can serve - and RotateColumns is compared when the column-swap key exists; what is compared does not change."""
        ev = self.client.reference_evaluator() if hasattr(self.client, "reference_evaluator") else None
        if ev is None:
            return None
        ctx, n, t = self.ctx, self.ctx.n, self.ctx.t
        rot = (1, -1) if steps is None else tuple(dict.fromkeys(int(x) for x in steps if int(x)))[:2]
        cols = steps is None or ctx.has_galois_key(2 * n - 1)
        # deterministic operands (the encryption randomness is the client's): slot-like values over the whole range of t
        v0 = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) % np.uint64(t)
        v1 = (np.arange(n, dtype=np.uint64) * np.uint64(40503) + np.uint64(7)) % np.uint64(t)
        ca, cb = self.client.encrypt(v0), self.client.encrypt(v1)
        h2, h3, o2, pt = ctx.ct_alloc(2), ctx.ct_alloc(1, 3), ctx.ct_alloc(1), ctx.pt_alloc(1)
        try:
            ctx.ct_upload(h2, 0, np.stack([ca, cb]))
            ctx.pt_upload(pt, 0, v1)
            const = int(v1[1]) or 1

            def dev(op):
                if op == "MultiplyPlain":
                    ctx.mul_plain(h2, 0, pt, 0, o2, 0)
                elif op == "MultiplyPlain(constant)":
                    ctx.mul_scalar(h2, 0, [const], o2, 0)
                elif op == "AddPlain":
                    ctx.add_plain(h2, 0, pt, 0, o2, 0)
                elif op == "Multiply":
                    ctx.multiply(h2, 0, h2, 1, h3, 0)
                    return ctx.ct_download(h3, 0, 1, size=3)[0]
                elif op == "Relinearize":
                    ctx.multiply(h2, 0, h2, 1, h3, 0)
                    ctx.relinearize(h3, 0, o2, 0)
                elif op.startswith("RotateRows("):
                    ctx.rotate_rows(h2, 0, int(op[11:-1]), o2, 0)
                elif op == "RotateColumns":
                    ctx.rotate_columns(h2, 0, o2, 0)
                return ctx.ct_download(o2, 0, 1)[0]

            c3 = ev.multiply(ca, cb)
            want = {"MultiplyPlain": lambda: ev.multiply_plain(ca, v1), "MultiplyPlain(constant)": lambda: ev.multiply_plain(ca, np.array([const], dtype=np.uint64)),
                    "AddPlain": lambda: ev.add_plain(ca, v1), "Multiply": lambda: c3, "Relinearize": lambda: ev.relinearize(c3),
                    **{"RotateRows(%d)" % r: (lambda r=r: ev.rotate_rows(ca, r)) for r in rot}}
            if cols:
                want["RotateColumns"] = lambda: ev.rotate_columns(ca)
            want = {k: np.asarray(f(), dtype=np.uint64).reshape(-1) for k, f in want.items()
                    if with_galois or not k.startswith("Rotate")}
            # Operations without keys.  Equal WORDS is what the restatement of SEAL 3.2 predicts; a product whose words differ from the client's but which
            # DECRYPTS to the same slots is still a valid drop-in for these operations (an evaluator may pick another valid BEHZ auxiliary base, another
            # representative in a lift: nothing downstream depends on it - only the key-switch convention is an interoperability property): recorded as a
            # warning in self_test_report, the start-up goes on.  Different slots: fatal, as before.
            warnings = []
            for op in ("MultiplyPlain", "MultiplyPlain(constant)", "AddPlain", "Multiply"):
                got = dev(op)
                if np.array_equal(got, want[op]):
                    continue
                try:
                    same = np.array_equal(np.asarray(self.client.decrypt(got)), np.asarray(self.client.decrypt(want[op])))
                except Exception:
                    same = False
                if not same:
                    raise Exception("libcnhip self-test: %s differs from the client's evaluator (plaintext modulus %d), words AND decrypted slots - the device "
                                    "does not implement this evaluator's arithmetic; no key convention can repair that" % (op, t))
                warnings.append("%s: ciphertext words differ from the client's evaluator, decrypted slots are equal (another valid representative; "
                                "not an interoperability property)" % op)
                # never silent: the operator sees at start-up that this device and the client's evaluator disagree on words
                import sys as _sys
                print("libcnhip self-test warning (plaintext modulus %d): %s" % (t, warnings[-1]), file=_sys.stderr)
            ks_ops = [op for op in ("Relinearize", *("RotateRows(%d)" % r for r in rot), "RotateColumns") if op in want]

            # Key-switching operations: WORDS again - unless the product itself already differs in words (then Relinearize inherits the difference and only
            # its decrypted slots can be compared; the rotations still compare words)
            by_slots = {"Relinearize"} if any(w.startswith("Multiply:") for w in warnings) else set()

            def first_failure():
                for op in ks_ops:
                    got = dev(op)
                    if op in by_slots:
                        if not np.array_equal(np.asarray(self.client.decrypt(got)), np.asarray(self.client.decrypt(want[op]))):
                            return op
                    elif not np.array_equal(got, want[op]):
                        return op
                return None

            xi0 = ctx.get_option("ks_xi")
            tried = []
            for form in ("ntt", "coeff"):
                if form == "coeff":
                    rk = self.client.relin_key_coeff_form() if hasattr(self.client, "relin_key_coeff_form") else None
                    if rk is None:
                        break
                    ctx.load_key(0, rk, coeff_form=True)
                    for elt, words in (self.client.galois_keys_coeff_form() or {}).items() if with_galois else ():
                        ctx.load_key(1, words, elt=elt, coeff_form=True)
                for xi in (xi0, 1 - xi0):
                    ctx.set_option("ks_xi", xi)
                    bad = first_failure()
                    tried.append((xi, form, bad))
                    if bad is None:
                        self.self_test_report = {"ks_xi": xi, "key_form": form, "ops": list(want), "tried": tried, "warnings": warnings}
                        return self.self_test_report
            ctx.set_option("ks_xi", xi0)
            raise Exception("libcnhip self-test: no key-switch convention reproduces the client's evaluator (plaintext modulus %d); tried (ks_xi, key form, "
                            "first differing operation): %s" % (t, tried))
        finally:
            for h in (h2, h3, o2, pt):
                ctx.free(h)

    def encode(self, values):
        """BatchEncoder.Encode into a fresh device plaintext; returns a pt view."""
        v = _Buf(self.ctx, "pt", 1).view()
        self.ctx.encode(np.asarray(values, dtype=np.uint64), v.h, 0)
        return v

    def mask_plain(self, kind, count):
        """Selection masks of the packing ops (ones over the first `count` slots: Interleave's row-boundary split,
        AtomicSealBfvVector.cs:628-688; a single one in slot `count`: ForceOutputInColumn, :936-945), encoded once per environment and
        kept in HBM: the reference re-encodes them on every call; here that would also put a host upload + synchronisation into the
        middle of an inference (and a recorded evaluation could not contain it).  The caller must NOT release the view."""
        cache = self.__dict__.setdefault("_mask_plains", {})
        key = (kind, int(count))
        if key not in cache:
            if kind == "ones":
                vals = np.ones(count, dtype=np.uint64)
            else:
                vals = np.zeros(count + 1, dtype=np.uint64)
                vals[count] = 1
            cache[key] = self.encode(vals)
        return cache[key]


class AtomicSealBfvEncryptedVector:
    """A vector under ONE plaintext modulus: ceil(Dim/N) ciphertexts (dense) or Dim ciphertexts holding one constant
    polynomial each (sparse) - or the same as plaintexts (AtomicSealBfvVector.cs:303-326)."""

    def __init__(self, v=None, env=None, Scale=1.0, SignedNumbers=True, EncryptData=True, Format=EVectorFormat.dense):
        self.encData = None          # _View over a ciphertext array
        self.plainDense = None       # _View over a device plaintext array (dense format)
        self.plainZero = None        # per dense plaintext: IsZero
        self.plainSparse = None      # list of ints, one constant polynomial each (sparse format)
        self.Scale, self.IsSigned, self.Format, self.Dim = Scale, SignedNumbers, Format, 0
        if v is not None:
            if EncryptData:
                self._Encrypt(v, Format, env)
            else:
                self._Plain(v, Format, env)

    # -- construction -----------------------------------------------------------------------------------------
    @classmethod
    def _new(cls, **kw):
        r = cls()
        for k, val in kw.items():
            setattr(r, k, val)
        return r

    @classmethod
    def Copy(cls, v, env):
        """copy constructor (AtomicSealBfvVector.cs:365-374): deep copy"""
        r = cls._new(Scale=v.Scale, Dim=v.Dim, IsSigned=v.IsSigned, Format=v.Format)
        if v.encData is not None:
            r.encData = _Buf(env.ctx, "ct", v.encData.count).view()
            env.ctx.copy(v.encData.h, v.encData.first, r.encData.h, 0, v.encData.count)
        if v.plainDense is not None:
            pd = v._pd(env.ctx)
            r.plainDense = _Buf(env.ctx, "pt", pd.count).view()
            env.ctx.copy(pd.h, pd.first, r.plainDense.h, 0, pd.count)
            r.plainZero = list(v.plainZero)
        if v.plainSparse is not None:
            r.plainSparse = list(v.plainSparse)
        return r

    def _values(self, v, env):
        """VectorToPlaintext value mapping (AtomicSealBfvVector.cs:1120-1122): round(v*Scale), negatives -> t + x.
        Returns a uint64 numpy array (vectorised: weight matrices have 10^8 entries)."""
        t = env.plainmodulusValue
        a = np.asarray(v)
        if a.dtype == np.uint64:
            return np.ascontiguousarray(a)
        if self.Scale == 0:
            self.Scale = 1
        r = np.rint(np.asarray(v, dtype=np.float64) * self.Scale)
        if r.size and float(np.max(np.abs(r))) >= 2.0 ** 62:
            raise Exception("value does not fit the plaintext modulus")
        w = r.astype(np.int64)
        if self.IsSigned:
            if w.size and (int(w.min()) <= -t or int(w.max()) >= t):
                raise Exception("value does not fit the plaintext modulus")
            w = np.where(w < 0, w + t, w)
        elif w.size and int(w.min()) < 0:
            raise Exception("value does not fit the plaintext modulus")
        return w.astype(np.uint64)

    def _to_plaintexts(self, v, env):
        values = self._values(v, env)
        t = env.plainmodulusValue
        if values.size and int(values.max()) >= t:
            raise Exception("value does not fit the plaintext modulus")
        self.Dim = len(values)
        if self.Format == EVectorFormat.dense:
            slots = env.SlotCount
            blocks = -(-len(values) // slots)
            if blocks == 0:
                raise Exception("empty vector")
            pv = _Buf(env.ctx, "pt", blocks).view()
            padded = np.zeros(blocks * slots, dtype=np.uint64)          # all blocks in ONE BatchEncoder call (cn_encode_batch)
            padded[:len(values)] = values
            padded = padded.reshape(blocks, slots)
            env.ctx.encode_batch(padded, pv.h, 0)
            zero = [not bool(padded[b].any()) for b in range(blocks)]
            return pv, zero, None
        return None, None, [int(x) for x in values]

    def _Plain(self, v, Format, env):
        self.Format = Format
        self.plainDense, self.plainZero, self.plainSparse = self._to_plaintexts(v, env)
        self.encData = None

    def _Encrypt(self, v, Format, env):
        """Encrypt (AtomicSealBfvVector.cs:1202-1232): one Encryptor.Encrypt per plaintext, done by the client."""
        self.Format = Format
        pv, _, sparse = self._to_plaintexts(v, env)
        ctx = env.ctx
        if sparse is not None:
            polys = np.zeros((len(sparse), ctx.n), dtype=np.uint64)
            polys[:, 0] = np.array(sparse, dtype=np.uint64)                # Plaintext(hex) = constant polynomial
            pv = _Buf(ctx, "pt", len(sparse)).view()
            ctx.pt_upload(pv.h, 0, polys)
        self.encData = _Buf(ctx, "ct", pv.count).view()
        if hasattr(env.client, "encrypt_device"):                          # Encryptor on the device: no host round trip
            env.client.encrypt_device(pv.h, 0, pv.count, self.encData.h, 0)
        else:
            plains = ctx.pt_download(pv.h, 0, pv.count)
            ctx.ct_upload(self.encData.h, 0, np.stack([env.client.encrypt(p) for p in plains]))
        pv.release()

    # -- modulus switching (SEAL 3.2 Evaluator.ModSwitchToNext / ModSwitchTo) --------------------------------------------------------
    @property
    def Limbs(self):
        """level of the ciphertexts (coefficient moduli kept), None for a plaintext vector"""
        return None if self.encData is None else _ctx_limbs(self.encData.buf.ctx)

    def ModSwitchTo(self, limbs, env):
        """a NEW vector at the level q[:limbs], bound to env.Level(limbs) (operate on it, decrypt it and write it with that environment);
        `env` is the environment this vector is at.  Plaintext vectors are level-free and are returned as they are."""
        if self.encData is None:
            return self
        _check_level(env, self)
        lenv = env.Level(limbs)
        if lenv is env:
            return self
        if limbs >= env.ctx.k:
            raise Exception("ModSwitchTo: level %d is not below the vector's level %d" % (limbs, env.ctx.k))
        d = self.encData
        t = AtomicSealBfvEncryptedVector._new(Scale=self.Scale, Dim=self.Dim, Format=self.Format, IsSigned=self.IsSigned)
        t.encData = _Buf(lenv.ctx, "ct", d.count, d.buf.size).view()
        env.ctx.mod_switch(d.h, d.first, d.count, lenv.ctx, t.encData.h, 0)
        return t

    def ModSwitchToNext(self, env):
        """ModSwitchTo one prime down (the last prime of the vector's level is dropped)"""
        return self.ModSwitchTo(env.ctx.k - 1, env)

    # -- persistence (AtomicSealBfvVector.cs:1273-1345) ------------------------------------------------------------
    def Write(self, stream, env):
        from . import serialization
        serialization.write_atomic_vector(stream, self, env)

    @staticmethod
    def Read(stream, env):
        from . import serialization
        return serialization.read_atomic_vector(stream, env)

    # -- properties -------------------------------------------------------------------------------------------
    @property
    def IsEncrypted(self):
        return self.encData is not None

    def _blocks(self):
        if self.encData is not None:
            return self.encData.count
        return self.plainDense.count if self.plainDense is not None else len(self.plainSparse)

    def RegisterDim(self, dim):
        self.Dim = dim

    def RegisterScale(self, scale):
        self.Scale = scale

    def Dispose(self):
        cached = [c[1] for c in self.__dict__.pop("_sparse_as_dense", {}).values()] + list(self.__dict__.pop("_pd_levels", {}).values())
        for v in [self.encData, self.plainDense] + cached:
            if v is not None:
                v.release()
        self.encData = self.plainDense = self.plainSparse = None

    def _pd(self, ctx):
        """the dense plaintexts as a view of `ctx`'s handles.  A plaintext is level-free (N words mod t), but a device handle belongs to one
        context: at the context they were encoded with, the vector's own; at a level of its chain, a copy made on first use and kept with the
        vector (once per vector and level, never per call; released by Dispose)"""
        pd = self.plainDense
        if pd.buf.ctx is ctx:
            return pd
        cache = self.__dict__.setdefault("_pd_levels", {})
        v = cache.get(ctx)
        if v is None or not v.live:
            v = _Buf(ctx, "pt", pd.count).view()
            ctx.pt_upload(v.h, 0, pd.buf.ctx.pt_download(pd.h, pd.first, pd.count))
            cache[ctx] = v
        return v

    def _plain_is_zero(self, i):
        return self.plainZero[i] if self.plainDense is not None else self.plainSparse[i] == 0

    # -- HOT LOOP A -------------------------------------------------------------------------------------------
    @staticmethod
    def DenseMatrixBySparseVectorMultiply(denses, sparse, env):
        """AtomicSealBfvVector.cs:434-521: out_block[i] = sum_k denses[k].block[i] * sparse[k]."""
        _check_level(env, sparse, *denses)
        if len(denses) != sparse.Dim:
            raise Exception("dimensions do not match")
        if sparse.Format != EVectorFormat.sparse:
            raise Exception("expecting a sparse vector")
        if not denses[0].IsEncrypted and not sparse.IsEncrypted:
            raise Exception("at least one parameter has to be encrypted")
        if denses[0].IsSigned != sparse.IsSigned:
            raise Exception("can't mix signed and unsigned messages")
        ctx = env.ctx
        l = denses[0]._blocks()
        K = len(denses)
        res = _Buf(ctx, "ct", l).view()
        if denses[0].IsEncrypted and sparse.IsEncrypted:
            # Multiply + Relinearize per term, then AddMany (:459-465,502).  The twin's form: ONE cn_mul_relin_sum over the K columns where they lie - the same
            # words and counters, one key switch per output block where the context allows it
            if hasattr(ctx, "mul_relin_sum"):
                ctx.mul_relin_sum([d.encData.h for d in denses], [d.encData.first for d in denses], [sparse.encData.h] * K,
                                  [sparse.encData.first + k for k in range(K)], 0, res.h, 0, l)
                return AtomicSealBfvEncryptedVector._new(Format=EVectorFormat.dense, Scale=denses[0].Scale * sparse.Scale, IsSigned=sparse.IsSigned,
                                                         encData=res, Dim=denses[0].Dim)
            # (backends without cn_mul_relin_sum - the CPU test harness): the literal loop
            terms = _Buf(ctx, "ct", K * l).view()
            for k in range(K):
                ctx.mul_relin(denses[k].encData.h, denses[k].encData.first, sparse.encData.h, sparse.encData.first + k,
                              terms.h, k * l, l, a_stride=1, b_stride=0)
            for i in range(l):
                ctx.add_many(terms.h, [k * l + i for k in range(K)], res.h, i)
            terms.release()
        elif denses[0].IsEncrypted:
            # ct blocks x constant plaintexts.  The twin's form (integration/GpuAtomicSealBfvEncryptedVector.cs): ONE cn_scalar_dot per output block
            # over the K ciphertexts where they lie - no gather copies
            if hasattr(ctx, "scalar_dot"):
                w = np.array(sparse.plainSparse, dtype=np.uint64)
                for i in range(l):
                    ctx.scalar_dot([d.encData.h for d in denses], [d.encData.first + i for d in denses], w, res.h, i)
                return AtomicSealBfvEncryptedVector._new(Format=EVectorFormat.dense, Scale=denses[0].Scale * sparse.Scale, IsSigned=sparse.IsSigned,
                                                         encData=res, Dim=denses[0].Dim)
            # (backends without cn_scalar_dot - the CPU test harness): one scalar GEMM with l outputs over a gathered array
            h, idx, tmp = _gather(ctx, [d.encData for d in denses])
            W = np.tile(np.array(sparse.plainSparse, dtype=np.uint64), (l, 1))
            gidx = np.array([[idx[k * l + i] for k in range(K)] for i in range(l)], dtype=np.int32)
            try:
                ctx.scalar_gemm(h, W, res.h, 0, idx=gidx)
            finally:
                if tmp is not None:
                    tmp.release()
        else:
            # plain dense columns x encrypted sparse entries (:476-485): MultiplyPlain(sparse.enc[k], denses[k].plain[i])
            terms = _Buf(ctx, "ct", K).view()
            for i in range(l):
                used = []
                for k in range(K):
                    if denses[k]._plain_is_zero(i):
                        continue
                    pd = denses[k]._pd(ctx)
                    ctx.mul_plain(sparse.encData.h, sparse.encData.first + k, pd.h, pd.first + i, terms.h, k, 1)
                    used.append(k)
                if not used:
                    raise Exception("AddMany of an empty list")
                ctx.add_many(terms.h, used, res.h, i)
            terms.release()
        return AtomicSealBfvEncryptedVector._new(Format=EVectorFormat.dense, Scale=denses[0].Scale * sparse.Scale, IsSigned=sparse.IsSigned,
                                                 encData=res, Dim=denses[0].Dim)

    # -- packing ops (slot movement) ----------------------------------------------------------------------------
    @staticmethod
    def _Inteleave(vecs, shift, outputBlockCount, env):
        """AtomicSealBfvVector.cs:600-722.  vecs: list of single-ciphertext views."""
        ctx = env.ctx
        blockSize = env.SlotCount
        absShift = -shift if shift < 0 else shift
        if shift < 0 and outputBlockCount > 1:
            raise Exception("Negative shifts with multiple output blocks are not implemented yet")
        if absShift > blockSize // 2 and outputBlockCount > 1:
            raise Exception("Shifts of more than half block size with multiple output blocks are not implemented yet")
        if absShift * len(vecs) > blockSize * outputBlockCount:
            raise Exception("not enough room for interleaving")
        n = len(vecs)
        work = _Buf(ctx, "ct", 2 * n).view()               # slot k: v, slot n + k: v2 (the split-off part)
        lower = [[] for _ in range(outputBlockCount)]
        upper = [[] for _ in range(outputBlockCount)]
        half = blockSize // 2

        def ones_mask(count):
            return env.mask_plain("ones", count)

        def geometry(k):
            thisShift = shift * k
            if thisShift < 0:
                thisShift = half + thisShift
            inBlockShift = thisShift % blockSize
            return thisShift, inBlockShift, thisShift // blockSize, (thisShift + absShift) // blockSize

        def steps_of(k):
            """the RotateRows step count of vector k (0: none)"""
            thisShift, inBlockShift, _, _ = geometry(k)
            if inBlockShift == 0:
                return 0
            if inBlockShift + absShift < half:
                return -thisShift
            return -(inBlockShift - half) if inBlockShift >= half else -inBlockShift

        # work[k] = RotateRows(vecs[k], steps_of(k)).  The reference copies and rotates vector by vector (:628-660); here - as in the C# twin - all
        # rotations of the interleave are ONE library call (cn_rotate_rows_many: the hops of the 13 differently rotated vectors run in rounds,
        # the same hops and words), straight from the source array when the vectors share one, behind one gather launch otherwise
        steps = [steps_of(k) for k in range(n)]
        if _summed(ctx) and n > 1:
            res = AtomicSealBfvEncryptedVector._interleave_summed(vecs, steps, geometry, ones_mask, absShift, outputBlockCount, env)
            work.release()
            return res
        if hasattr(ctx, "rotate_rows_many") and n > 1:
            if all(x.buf is vecs[0].buf for x in vecs):
                ctx.rotate_rows_many(vecs[0].h, [x.first for x in vecs], steps, work.h, list(range(n)))
            else:
                ctx.copy_many([x.h for x in vecs], [x.first for x in vecs], work.h, 0)
                ctx.rotate_rows_many(work.h, list(range(n)), steps, work.h, list(range(n)))
        else:
            for k, src in enumerate(vecs):
                if steps[k] == 0:
                    ctx.copy(src.h, src.first, work.h, k, 1)
                else:
                    ctx.rotate_rows(src.h, src.first, steps[k], work.h, k, 1)
        for k in range(n):
            thisShift, inBlockShift, startBlock, endBlock = geometry(k)
            v, v2 = k, n + k
            if inBlockShift == 0:
                lower[startBlock].append(v)
            elif inBlockShift + absShift < half:
                lower[startBlock].append(v)
            elif inBlockShift >= half:
                if startBlock == endBlock:
                    upper[startBlock].append(v)
                else:
                    upperPartSize = inBlockShift + absShift - blockSize
                    ctx.copy(work.h, v, work.h, v2, 1)
                    p = ones_mask(upperPartSize)
                    ctx.mul_plain(work.h, v, p.h, 0, work.h, v, 1)
                    ctx.sub(work.h, v2, work.h, v, work.h, v2, 1)
                    upper[startBlock].append(v2)
                    lower[endBlock].append(v)
            else:
                upperPartSize = inBlockShift + absShift - half
                if upperPartSize > 0:
                    ctx.copy(work.h, v, work.h, v2, 1)
                    p = ones_mask(upperPartSize)
                    ctx.mul_plain(work.h, v, p.h, 0, work.h, v, 1)
                    ctx.sub(work.h, v2, work.h, v, work.h, v2, 1)
                    upper[startBlock].append(v)
                    lower[startBlock].append(v2)
                else:
                    lower[startBlock].append(v)
        res = _Buf(ctx, "ct", outputBlockCount).view()
        tmp = _Buf(ctx, "ct", 1).view()
        for i in range(outputBlockCount):
            if not lower[i]:
                raise Exception("AddMany of an empty list")
            ctx.add_many(work.h, lower[i], res.h, i)
            if upper[i]:
                ctx.add_many(work.h, upper[i], tmp.h, 0)
                ctx.rotate_columns(tmp.h, 0, tmp.h, 0, 1)
                ctx.add(res.h, i, tmp.h, 0, res.h, i, 1)
        tmp.release()
        work.release()
        return res

    @staticmethod
    def _interleave_summed(vecs, steps, geometry, ones_mask, absShift, outputBlockCount, env):
        """_Inteleave under SUMMED_ROTATIONS: a vector that goes into a sum unmodified is a TERM of one cn_rotate_rows_sum (two groups per output block, its
        `lower` list and its `upper` list) and is never stored rotated; a vector that is split (v2, the mask products) is rotated into `work` by the present code
        and enters the sums as plain addends.  Straight from the source array when nothing is split and the vectors share one, behind copy_many otherwise.  Then
        the present rotate_columns + add.  The words are those of the switch-off route."""
        ctx = env.ctx
        blockSize = env.SlotCount
        half = blockSize // 2
        n = len(vecs)
        lower = [[] for _ in range(outputBlockCount)]      # (slot, step): slot k = vector k unrotated, slot n + k: its split-off part (step 0, like a split slot k)
        upper = [[] for _ in range(outputBlockCount)]
        split = []                                         # (vector, mask length, the list its masked part goes to, the list the rest goes to)
        for k in range(n):
            thisShift, inBlockShift, startBlock, endBlock = geometry(k)
            if inBlockShift == 0 or inBlockShift + absShift < half:
                lower[startBlock].append((k, steps[k]))
            elif inBlockShift >= half:
                if startBlock == endBlock:
                    upper[startBlock].append((k, steps[k]))
                else:
                    split.append((k, inBlockShift + absShift - blockSize, lower[endBlock], upper[startBlock]))
            else:
                upperPartSize = inBlockShift + absShift - half
                if upperPartSize > 0:
                    split.append((k, upperPartSize, upper[startBlock], lower[startBlock]))
                else:
                    lower[startBlock].append((k, steps[k]))
        shared = all(x.buf is vecs[0].buf for x in vecs)
        work = None
        if split or not shared:
            work = _Buf(ctx, "ct", 2 * n).view()
            ctx.copy_many([x.h for x in vecs], [x.first for x in vecs], work.h, 0)
            ks = [k for k, _, _, _ in split]
            if ks:                                           # the vectors that are split: rotated in place, as the present route rotates them
                ctx.rotate_rows_many(work.h, ks, [steps[k] for k in ks], work.h, ks)
            for k, size, masked_to, rest_to in split:        # slot k: the masked part, slot n + k: the rest - the present route's operations
                v, v2 = k, n + k
                ctx.copy(work.h, v, work.h, v2, 1)
                p = ones_mask(size)
                ctx.mul_plain(work.h, v, p.h, 0, work.h, v, 1)
                ctx.sub(work.h, v2, work.h, v, work.h, v2, 1)
                masked_to.append((v, 0))
                rest_to.append((v2, 0))
            src_h, slot = work.h, (lambda k: k)
        else:
            src_h, slot = vecs[0].h, (lambda k: vecs[k].first)
        groups = []                                          # (block, is_upper)
        ii, st, off = [], [], [0]
        for i in range(outputBlockCount):
            if not lower[i]:
                raise Exception("AddMany of an empty list")
            for is_upper, lst in ((False, lower[i]), (True, upper[i])):
                if lst:
                    groups.append((i, is_upper))
                    ii += [slot(k) if k < n else k for k, _ in lst]
                    st += [s_ for _, s_ in lst]
                    off.append(len(ii))
        sums = _Buf(ctx, "ct", len(groups)).view()
        ctx.rotate_rows_sum(src_h, ii, st, off, sums.h, 0)
        res = _Buf(ctx, "ct", outputBlockCount).view()
        at = {g: x for x, g in enumerate(groups)}
        for i in range(outputBlockCount):
            if (i, True) in at:
                ctx.rotate_columns(sums.h, at[(i, True)], sums.h, at[(i, True)], 1)
                ctx.add(sums.h, at[(i, False)], sums.h, at[(i, True)], res.h, i, 1)
            else:
                ctx.copy(sums.h, at[(i, False)], res.h, i, 1)
        sums.release()
        if work is not None:
            work.release()
        return res

    @staticmethod
    def Interleave(vecs, shift, env):
        """AtomicSealBfvVector.cs:729-750"""
        if vecs[0].Format != EVectorFormat.dense:
            raise Exception("Expecting dense vector")
        blockSize = env.SlotCount
        outputBlocks = 1
        if shift > 0:
            outputBlocks = int(math.ceil(vecs[0].Dim * len(vecs) / float(blockSize)))
        subs = [v.encData.sub(0) for v in vecs]
        try:
            enc = AtomicSealBfvEncryptedVector._Inteleave(subs, shift, outputBlocks, env)
        finally:
            for sv in subs:                              # (these views used to stay alive: every Interleave / Stack kept its inputs' arrays)
                sv.release()
        return AtomicSealBfvEncryptedVector._new(encData=enc, Dim=vecs[0].Dim, Scale=vecs[0].Scale, IsSigned=vecs[0].IsSigned,
                                                 Format=EVectorFormat.dense)

    @staticmethod
    def Stack(vecs, env):
        """AtomicSealBfvVector.cs:756-761"""
        res = AtomicSealBfvEncryptedVector.Interleave(vecs, int(vecs[0].Dim), env)
        res.Dim = vecs[0].Dim * len(vecs)
        return res

    # -- HOT LOOP B -------------------------------------------------------------------------------------------
    def _PointwiseMultiplySparseDimOne(self, ev, env):
        """AtomicSealBfvVector.cs:774-810: multiply every block by one constant"""
        ctx = env.ctx
        t = AtomicSealBfvEncryptedVector._new(Scale=self.Scale * ev.Scale, Dim=self.Dim, Format=self.Format, IsSigned=self.IsSigned)
        if self.encData is not None and ev.encData is not None:
            t.encData = _Buf(ctx, "ct", self.encData.count).view()
            ctx.mul_relin(ev.encData.h, ev.encData.first, self.encData.h, self.encData.first, t.encData.h, 0, self.encData.count,
                          a_stride=0, b_stride=1)
            return t
        if self.encData is not None:                 # enc blocks x plain constant
            t.encData = _Buf(ctx, "ct", self.encData.count).view()
            w = ev.plainSparse[0]
            if w == 0:
                raise Exception("plain cannot be zero")
            ctx.mul_scalar(self.encData.h, self.encData.first, np.array([w], dtype=np.uint64), t.encData.h, 0, self.encData.count, broadcast=True)
        else:                                        # plain blocks x encrypted constant
            pd = self._pd(ctx)
            cnt = pd.count
            t.encData = _Buf(ctx, "ct", cnt).view()
            for i in range(cnt):
                ctx.mul_plain(ev.encData.h, ev.encData.first, pd.h, pd.first + i, t.encData.h, i, 1)
        return t

    def _encrypt_zero_into(self, env, buf_h, index):
        """encryptor.Encrypt(PlainZero) (AtomicSealBfvVector.cs:566,588): a fresh encryption of zero from the client"""
        ctx = env.ctx
        if hasattr(env.client, "encrypt_device"):
            z = _Buf(ctx, "pt", 1).view()
            ctx.pt_upload(z.h, 0, np.zeros((1, ctx.n), dtype=np.uint64))
            env.client.encrypt_device(z.h, 0, 1, buf_h, index)
            z.release()
        else:
            ctx.ct_upload(buf_h, index, np.asarray(env.client.encrypt(np.zeros(ctx.n, dtype=np.uint64)))[None, :])

    def SparseMultiply(self, v, colIndex, env):
        """AtomicSealBfvVector.cs:529-598: every block of this (dense) vector times ELEMENT colIndex of the sparse vector v.
        (No caller in the reference's networks - kept for interface parity)"""
        _check_level(env, self, v)
        ev = v
        if colIndex >= ev.Dim:
            raise Exception("index exceeds dimension")
        if ev.Format != EVectorFormat.sparse:
            raise Exception("expecting sparse format")
        if ev.encData is None and self.encData is None:
            raise Exception("at least one argument is expected to be encrypted")
        if self.IsSigned != ev.IsSigned:
            raise Exception("can't mix signed and unsigned numbers.")
        ctx = env.ctx
        t = AtomicSealBfvEncryptedVector._new(Scale=self.Scale * ev.Scale, Dim=self.Dim, Format=EVectorFormat.dense, IsSigned=self.IsSigned)
        if self.encData is not None and ev.encData is not None:
            n = self.encData.count
            t.encData = _Buf(ctx, "ct", n).view()
            ctx.mul_relin(ev.encData.h, ev.encData.first + colIndex, self.encData.h, self.encData.first, t.encData.h, 0, n, a_stride=0, b_stride=1)
            return t
        if self.encData is None:                       # plain dense blocks x one encrypted element
            n = self.plainDense.count
            t.encData = _Buf(ctx, "ct", n).view()
            for i in range(n):
                if self.plainZero[i]:
                    self._encrypt_zero_into(env, t.encData.h, i)
                else:
                    pd = self._pd(ctx)
                    ctx.mul_plain(ev.encData.h, ev.encData.first + colIndex, pd.h, pd.first + i, t.encData.h, i, 1)
            return t
        n = self.encData.count                         # encrypted blocks x one plain constant
        t.encData = _Buf(ctx, "ct", n).view()
        w = ev.plainSparse[colIndex]
        if w == 0:
            for i in range(n):
                self._encrypt_zero_into(env, t.encData.h, i)
        else:
            ctx.mul_scalar(self.encData.h, self.encData.first, np.array([w], dtype=np.uint64), t.encData.h, 0, n, broadcast=True)
        return t

    def PointwiseMultiply(self, v, env):
        """AtomicSealBfvVector.cs:813-860"""
        _check_level(env, self, v)
        ev = v
        if self.IsSigned != ev.IsSigned:
            raise Exception("Can't mix signed and unsigned numbers.")
        if not self.IsEncrypted and not ev.IsEncrypted:
            raise Exception("multiplying two plaintexts is not implemented")
        if self.Dim == 1 and self.Format == EVectorFormat.sparse:
            return ev._PointwiseMultiplySparseDimOne(self, env)
        if ev.Dim == 1 and ev.Format == EVectorFormat.sparse:
            return self._PointwiseMultiplySparseDimOne(ev, env)
        if self.Dim != v.Dim:
            raise Exception("Dimensions do not match")
        if self.Format != ev.Format:
            raise Exception("Format mismatch")
        ctx = env.ctx
        t = AtomicSealBfvEncryptedVector._new(Scale=self.Scale * ev.Scale, Dim=self.Dim, Format=self.Format, IsSigned=self.IsSigned)
        if self.encData is not None and ev.encData is not None:
            n = ev.encData.count
            t.encData = _Buf(ctx, "ct", n).view()
            ctx.mul_relin(ev.encData.h, ev.encData.first, self.encData.h, self.encData.first, t.encData.h, 0, n)
            return t
        enc = self.encData if self.encData is not None else ev.encData
        pl = self if self.encData is None else ev
        t.encData = _Buf(ctx, "ct", enc.count).view()
        if pl.plainDense is not None:
            pd = pl._pd(ctx)
            ctx.mul_plain(enc.h, enc.first, pd.h, pd.first, t.encData.h, 0, enc.count)
        else:
            if any(w == 0 for w in pl.plainSparse):
                raise Exception("plain cannot be zero")
            ctx.mul_scalar(enc.h, enc.first, np.array(pl.plainSparse, dtype=np.uint64), t.encData.h, 0, enc.count)
        return t

    # -- HOT LOOP C -------------------------------------------------------------------------------------------
    @staticmethod
    def _RotateRowsAndAdd(ctx, c_h, c_i, steps, agg_h, agg_i, tmp_h, tmp_i):
        """AtomicSealBfvVector.cs:862-868: agg += RotateRows(c, -steps)"""
        ctx.rotate_rows_add(c_h, c_i, -steps, agg_h, agg_i, agg_h, agg_i, 1)      # rotation + AddInplace in one launch chain

    def SumAllSlots(self, env, length=None, ForceOutputInColumn=None, _consume=False):
        """AtomicSealBfvVector.cs:877-955 (length None = Int32.MaxValue = full sum).  _consume: the caller owns this vector as a temporary (the
        product inside DotProduct) - the sum is built in its array instead of in a copy, and this object must not be used or disposed afterwards"""
        INT_MAX = 2 ** 31 - 1
        if length is None:
            length = INT_MAX
        if self.Format != EVectorFormat.dense:
            raise Exception("Expecting dense vector format")
        if length != INT_MAX and ForceOutputInColumn is not None:
            raise Exception("forcing output in a column works only when doing complete sum")
        if self.encData is None:
            raise Exception("SumAllSlots can be applied to encrypted data only")
        if length <= 0:
            raise Exception("Can't sum over less then one element")
        if length == 1:
            return self
        ctx, slots = env.ctx, env.SlotCount
        if _consume and self.encData.count == 1 and self.encData.first == 0 and self.encData.buf.refs == 1:
            res, self.encData = self.encData, None
        else:
            res = _Buf(ctx, "ct", 1).view()        # the sum is built where it is returned (as in the twin: one copy, not three)
            if self.encData.count > 1:
                ctx.add_many(self.encData.h, [self.encData.first + i for i in range(self.encData.count)], res.h, 0)
            else:
                ctx.copy(self.encData.h, self.encData.first, res.h, 0, 1)
            if _consume:
                self.Dispose()
        ctx.sum_slots(res.h, 0, 1, 0 if length >= slots else length)      # column swap + log2 rotate-and-add steps in one call
        if length >= slots // 2:
            length = slots // 2
        if ForceOutputInColumn is not None:
            p = env.mask_plain("slot", ForceOutputInColumn)
            ctx.mul_plain(res.h, 0, p.h, 0, res.h, 0, 1)
            length = 1
        return AtomicSealBfvEncryptedVector._new(IsSigned=self.IsSigned, Scale=self.Scale, Dim=1 if length >= slots // 2 else self.Dim, encData=res,
                                                 Format=EVectorFormat.sparse if length >= slots else EVectorFormat.dense)

    def DotProduct(self, v, env, length=None, ForceOutputInColumn=None):
        """AtomicSealBfvVector.cs:963-977"""
        full = length is None or length > 1
        if (full and self.encData is not None and v.encData is not None and self.Format == v.Format == EVectorFormat.dense and self.Dim == v.Dim
                and self.IsSigned == v.IsSigned and v.encData.count > 1 and self.encData.count == v.encData.count and hasattr(env.ctx, "mul_relin_sum")):
            # two encrypted dense vectors of several blocks: PointwiseMultiply (:839-840) and the AddMany at the head of SumAllSlots (:888-900) as ONE
            # cn_mul_relin_sum - the same words and counters - into the array the slot sum is then built in
            _check_level(env, self, v)
            n = v.encData.count
            mul = AtomicSealBfvEncryptedVector._new(Scale=self.Scale * v.Scale, Dim=self.Dim, Format=self.Format, IsSigned=self.IsSigned)
            mul.encData = _Buf(env.ctx, "ct", 1).view()
            env.ctx.mul_relin_sum([v.encData.h] * n, [v.encData.first + i for i in range(n)], [self.encData.h] * n,
                                  [self.encData.first + i for i in range(n)], 1, mul.encData.h, 0, 1)
            return mul.SumAllSlots(env, length, ForceOutputInColumn, _consume=True)
        mul = self.PointwiseMultiply(v, env)
        if (length is None or length > 1) and mul.encData is not None and mul.Format == EVectorFormat.dense:
            return mul.SumAllSlots(env, length, ForceOutputInColumn, _consume=True)       # the product is a temporary: summed in its own array
        res = mul.SumAllSlots(env, length, ForceOutputInColumn)
        if res is not mul:
            mul.Dispose()
        return res

    # -- linear ---------------------------------------------------------------------------------------------
    def Add(self, v, env):
        """AtomicSealBfvVector.cs:983-1024"""
        _check_level(env, self, v)
        if self.Scale == 0:
            return v
        if v.Scale == 0:
            return self
        if self.Scale != v.Scale:
            raise Exception("Scales do not match.")
        if self.Dim != v.Dim:
            raise Exception("Dimensions do not match")
        if self.Format != v.Format:
            raise Exception("Format mismatch")
        if self.IsSigned != v.IsSigned:
            raise Exception("can't mix signed and unsigned numbers.")
        if not self.IsEncrypted and not v.IsEncrypted:
            raise Exception("adding two plaintexts is not supported")
        ctx = env.ctx
        t = AtomicSealBfvEncryptedVector._new(Scale=self.Scale, Dim=self.Dim, Format=self.Format, IsSigned=self.IsSigned)
        if self.IsEncrypted and v.IsEncrypted:
            n = self.encData.count
            t.encData = _Buf(ctx, "ct", n).view()
            ctx.add(v.encData.h, v.encData.first, self.encData.h, self.encData.first, t.encData.h, 0, n)
            return t
        enc, pl = (self.encData, v) if self.IsEncrypted else (v.encData, self)
        t.encData = _Buf(ctx, "ct", enc.count).view()
        pv, tmp = pl._dense_plain_view(env)
        ctx.add_plain(enc.h, enc.first, pv.h, pv.first, t.encData.h, 0, pv.count)
        if tmp:
            pv.release()
        return t

    def Subtract(self, v, env):
        """AtomicSealBfvVector.cs:1238-1271"""
        _check_level(env, self, v)
        if v.Scale == 0:
            return self
        if self.Scale != v.Scale:
            raise Exception("Scales do not match.")
        if self.Dim != v.Dim:
            raise Exception("Dimensions do not match")
        if self.Format != v.Format:
            raise Exception("Format mismatch")
        if self.IsSigned != v.IsSigned:
            raise Exception("Can't mix signed and unsigned numbers.")
        if not self.IsEncrypted:
            raise Exception("the first argument for subtraction must be encrypted")
        ctx = env.ctx
        n = self.encData.count
        t = AtomicSealBfvEncryptedVector._new(Scale=self.Scale, Dim=self.Dim, Format=self.Format, IsSigned=self.IsSigned)
        t.encData = _Buf(ctx, "ct", n).view()
        if v.IsEncrypted:
            ctx.sub(self.encData.h, self.encData.first, v.encData.h, v.encData.first, t.encData.h, 0, n)
        else:
            pv, tmp = v._dense_plain_view(env)
            ctx.add_plain(self.encData.h, self.encData.first, pv.h, pv.first, t.encData.h, 0, n, subtract=True)
            if tmp:
                pv.release()
        return t

    def _dense_plain_view(self, env):
        """Plaintexts as device polynomials: dense plaintexts as they are; sparse ones as constant polynomials."""
        if self.plainDense is not None:
            return self._pd(env.ctx), False
        # sparse plaintexts (biases) are constants of the network: their polynomial form is uploaded once per context (level) and kept with
        # the vector - no host upload + synchronisation in the middle of every inference (a recorded evaluation could not contain one either)
        key = tuple(int(x) for x in self.plainSparse)
        per_ctx = self.__dict__.setdefault("_sparse_as_dense", {})
        cached = per_ctx.get(env.ctx)
        if cached is None or cached[0] != key or not cached[1].live:
            if cached is not None:
                cached[1].release()
            pv = _Buf(env.ctx, "pt", len(self.plainSparse)).view()
            polys = np.zeros((len(self.plainSparse), env.ctx.n), dtype=np.uint64)
            polys[:, 0] = np.array(self.plainSparse, dtype=np.uint64)
            env.ctx.pt_upload(pv.h, 0, polys)
            per_ctx[env.ctx] = cached = (key, pv)
        return cached[1], False

    # -- decryption (client side) -------------------------------------------------------------------------------
    def _decrypt_ints(self, env):
        """Unsigned residues per element, exactly as Decrypt / DecryptFullPrecision read them (AtomicSealBfvVector.cs:1030-1110)."""
        ctx = env.ctx
        res = []
        n_items = self._blocks()
        if self.encData is not None:
            if hasattr(env.client, "decrypt_device"):
                plains = env.client.decrypt_device(self.encData.h, self.encData.first, self.encData.count)
            else:
                cts = ctx.ct_download(self.encData.h, self.encData.first, self.encData.count)
                plains = np.stack([env.client.decrypt(c) for c in cts])
        elif self.plainDense is not None:
            plains = self.plainDense.buf.ctx.pt_download(self.plainDense.h, self.plainDense.first, self.plainDense.count)
        else:
            plains = None
        if self.Format == EVectorFormat.dense:
            tmp = _Buf(ctx, "pt", n_items).view()
            ctx.pt_upload(tmp.h, 0, np.asarray(plains)[:n_items])
            slots = ctx.decode_batch(tmp.h, 0, n_items)                               # every block in one BatchEncoder.Decode call
            for i in range(n_items):
                left = int(self.Dim) - len(res)
                res.extend(int(x) for x in slots[i][:min(left, slots.shape[1])])
            tmp.release()
        else:
            for i in range(n_items):
                res.append(int(plains[i][0]) if plains is not None else int(self.plainSparse[i]))
        return res

    def DecryptFullPrecision(self, env):
        t = env.plainmodulusValue
        return [(v - t) if (self.IsSigned and v * 2 > t) else v for v in self._decrypt_ints(env)]

    def Decrypt(self, env):
        mod = float(env.plainmodulusValue)
        t = env.plainmodulusValue
        return np.array([((float(v) - mod) if (self.IsSigned and v * 2 > t) else float(v)) / self.Scale for v in self._decrypt_ints(env)])

    # -- misc -------------------------------------------------------------------------------------------------
    @staticmethod
    def GenerateSparseOfArray(encryptedVector, env):
        """AtomicSealBfvVector.cs:1347-1359: first block of every vector becomes one entry of a sparse vector"""
        ctx = env.ctx
        res = _Buf(ctx, "ct", len(encryptedVector)).view()
        if hasattr(ctx, "copy_many"):
            ctx.copy_many([e.encData.h for e in encryptedVector], [e.encData.first for e in encryptedVector], res.h, 0)
        else:
            for i, e in enumerate(encryptedVector):
                ctx.copy(e.encData.h, e.encData.first, res.h, i, 1)
        return AtomicSealBfvEncryptedVector._new(Scale=encryptedVector[0].Scale, Dim=len(encryptedVector), Format=EVectorFormat.sparse,
                                                 IsSigned=encryptedVector[0].IsSigned, encData=res)

    def Duplicate(self, count, env):
        """AtomicSealBfvVector.cs:1370-1408"""
        shift = 1
        while shift < self.Dim:
            shift *= 2
        if self.encData is None:
            raise Exception("Duplicate operates only on encrypted data")
        if self.Format == EVectorFormat.sparse:
            raise Exception("Duplicate operates only on dense vectors")
        slots, ctx = env.SlotCount, env.ctx
        if shift * count > slots:
            raise Exception("Packed vector must fit in a single ciphertext")
        if hasattr(ctx, "rotate_rows_many") and int(count) > 2:
            # every copy is a rotation of the SAME ciphertext (or of its column-swapped form) and they are only added up: the count - 1 rotations
            # are one library call (their hops share rounds), the sum one AddMany - the words of the reference's rotate-and-add chain (modular
            # addition is exact in any order), 6 dispatches instead of 2 per copy
            n = int(count) - 1
            work = _Buf(ctx, "ct", 2 + n).view()    # 0: the vector, 1: its column-swapped form, 2 ..: the rotated copies
            ctx.copy(self.encData.h, self.encData.first, work.h, 0, 1)
            srcs, steps = [], []
            for i in range(1, int(count)):
                target = i * shift
                if target * 2 >= slots:
                    srcs.append(1)
                    target -= slots // 2
                else:
                    srcs.append(0)
                steps.append(-target)
            if 1 in srcs:
                ctx.rotate_columns(self.encData.h, self.encData.first, work.h, 1, 1)
            # HOISTED_ROTATIONS: the copies of each of the two sources are one hoisted call; a refusal of either leaves the present route for all
            by_src = [[i for i in range(n) if srcs[i] == c] for c in (0, 1)]
            if not all(_rotate_hoisted(ctx, work.h, c, [steps[i] for i in idx], work.h, [2 + i for i in idx]) for c, idx in enumerate(by_src) if idx):
                ctx.rotate_rows_many(work.h, srcs, steps, work.h, [2 + i for i in range(n)])
            res = _Buf(ctx, "ct", 1).view()
            ctx.add_many(work.h, [0] + [2 + i for i in range(n)], res.h, 0)
            work.release()
            return AtomicSealBfvEncryptedVector._new(IsSigned=self.IsSigned, Scale=self.Scale, Dim=count * shift, encData=res, Format=EVectorFormat.dense)
        work = _Buf(ctx, "ct", 3).view()            # 0: res, 1: rotator, 2: tmp
        ctx.copy(self.encData.h, self.encData.first, work.h, 0, 1)
        ctx.copy(self.encData.h, self.encData.first, work.h, 1, 1)
        columnRotated = False
        for i in range(1, int(count)):
            target = i * shift
            if target * 2 >= slots:
                if not columnRotated:
                    columnRotated = True
                    ctx.rotate_columns(self.encData.h, self.encData.first, work.h, 1, 1)
                target -= slots // 2
            self._RotateRowsAndAdd(ctx, work.h, 1, target, work.h, 0, work.h, 2)
        res = _Buf(ctx, "ct", 1).view()
        ctx.copy(work.h, 0, res.h, 0, 1)
        work.release()
        return AtomicSealBfvEncryptedVector._new(IsSigned=self.IsSigned, Scale=self.Scale, Dim=count * shift, encData=res, Format=EVectorFormat.dense)

    def Rotate(self, amount, env):
        """AtomicSealBfvVector.cs:1414-1430"""
        if self.encData is None:
            raise Exception("Rotate operates only on encrypted data")
        if self.Format == EVectorFormat.sparse:
            raise Exception("Rotate operates only on dense vectors")
        res = _Buf(env.ctx, "ct", 1).view()
        env.ctx.rotate_rows(self.encData.h, self.encData.first, amount, res.h, 0, 1)
        return AtomicSealBfvEncryptedVector._new(IsSigned=self.IsSigned, Scale=self.Scale, Dim=self.Dim, encData=res, Format=EVectorFormat.dense)

    def Permute(self, selections, shifts, outputDim, env):
        """AtomicSealBfvVector.cs:1436-1475: sum_i rotL(x * sel_i, shifts[i])"""
        if self.Format != EVectorFormat.dense:
            raise Exception("Permute works only on dense vectors")
        if len(selections) != len(shifts):
            raise Exception("number of selection vectors and number of shifts does not match")
        if self.encData is None:
            raise Exception("can permute only encrypted vectors")
        if self.encData.count > 1:
            raise Exception("can permute only a single block")
        ctx = env.ctx
        if _summed(ctx):
            return self._permute_summed(selections, shifts, outputDim, env)
        work = _Buf(ctx, "ct", 3).view()            # 0: res, 1: t, 2: t3->relin tmp
        first = -1
        for i, s in enumerate(selections):
            if s is None:
                continue
            if first < 0:
                first = i
            if s.Dim != self.Dim:
                raise Exception("dimension of selection vector does not match dimension of data vector")
            if s.Scale != selections[first].Scale:
                raise Exception("scales of all selection vectors should be the same")
            if s.plainDense is not None:
                pd = s._pd(ctx)
                ctx.mul_plain(self.encData.h, self.encData.first, pd.h, pd.first, work.h, 1, 1)
            else:
                # the reference multiplies without relinearising here (:1457) and would then fail to rotate a size-3
                # ciphertext; encrypted selections are therefore relinearised
                ctx.mul_relin(self.encData.h, self.encData.first, s.encData.h, s.encData.first, work.h, 1, 1)
            if i == first:
                ctx.rotate_rows(work.h, 1, shifts[i], work.h, 0, 1)
            else:
                ctx.rotate_rows_add(work.h, 1, shifts[i], work.h, 0, work.h, 0, 1)     # res += rot(x * sel_i)
        if first < 0:
            raise Exception("permuting with no selected values is illigal")
        res = _Buf(ctx, "ct", 1).view()
        ctx.copy(work.h, 0, res.h, 0, 1)
        work.release()
        return AtomicSealBfvEncryptedVector._new(IsSigned=self.IsSigned, Scale=self.Scale * selections[first].Scale, Dim=outputDim, encData=res,
                                                 Format=EVectorFormat.dense)

    def _permute_summed(self, selections, shifts, outputDim, env):
        """Permute under SUMMED_ROTATIONS: the selection products as they are, then ONE cn_rotate_rows_sum instead of a rotation and an addition per selection -
        the same words"""
        ctx = env.ctx
        chosen = [i for i, s in enumerate(selections) if s is not None]
        if not chosen:
            raise Exception("permuting with no selected values is illigal")
        first = chosen[0]
        work = _Buf(ctx, "ct", len(chosen)).view()
        try:
            for x, i in enumerate(chosen):
                s = selections[i]
                if s.Dim != self.Dim:
                    raise Exception("dimension of selection vector does not match dimension of data vector")
                if s.Scale != selections[first].Scale:
                    raise Exception("scales of all selection vectors should be the same")
                if s.plainDense is not None:
                    pd = s._pd(ctx)
                    ctx.mul_plain(self.encData.h, self.encData.first, pd.h, pd.first, work.h, x, 1)
                else:
                    ctx.mul_relin(self.encData.h, self.encData.first, s.encData.h, s.encData.first, work.h, x, 1)
            res = _Buf(ctx, "ct", 1).view()
            ctx.rotate_rows_sum(work.h, list(range(len(chosen))), [int(shifts[i]) for i in chosen], [0, len(chosen)], res.h, 0)
        finally:
            work.release()
        return AtomicSealBfvEncryptedVector._new(IsSigned=self.IsSigned, Scale=self.Scale * selections[first].Scale, Dim=outputDim, encData=res,
                                                 Format=EVectorFormat.dense)


# ------------------------------------------------------------------------------------------------ CRT layer
class EncryptedSealBfvEnvironment:
    """All plaintext-prime channels + CRT coefficients (EncryptedSealBfvVector.cs:17-149)."""

    def __init__(self, environments, ParentFactory=None):
        self.Environments = environments
        self.ParentFactory = ParentFactory
        primes = [e.plainmodulusValue for e in environments]
        self.bigFactor = 1
        for p in primes:
            self.bigFactor *= p
        # PreCompute (:79-90): coef_i = (M/p_i) * ((M/p_i)^-1 mod p_i)
        self.preComputedCoefficients = [(self.bigFactor // p) * pow((self.bigFactor // p) % p, -1, p) for p in primes]

    @property
    def Primes(self):
        return [e.plainmodulusValue for e in self.Environments]

    @property
    def Limbs(self):
        return self.Environments[0].Limbs

    def Level(self, limbs):
        """the environment of the level q[:limbs] for every plaintext prime (cached: the same object for the same level)"""
        root = self.__dict__.get("_root", self)
        if int(limbs) == root.Environments[0].ctx.k:
            return root
        cache = root.__dict__.setdefault("_levels", {})
        if int(limbs) not in cache:
            e = EncryptedSealBfvEnvironment([x.Level(limbs) for x in root.Environments], root.ParentFactory)
            e.bigFactor, e.preComputedCoefficients, e._root = root.bigFactor, root.preComputedCoefficients, root
            cache[int(limbs)] = e
        return cache[int(limbs)]


class EncryptedSealBfvVector:
    """Values split over the plaintext primes; every op fans out to eVectors[i] (EncryptedSealBfvVector.cs:150-573)."""

    def __init__(self, v=None, env=None, Scale=1.0, EncryptData=True, Format=EVectorFormat.dense, integers=None):
        self.eVectors = None
        self.Scale = Scale
        self.IsSigned = True
        if v is not None or integers is not None:
            if self._device_split(v, env, Scale, EncryptData, Format, integers):
                return
            primes = [e.plainmodulusValue for e in env.Environments]
            res = None
            if integers is None:
                r = np.rint(np.asarray(v, dtype=np.float64) * Scale)              # SplitBigNumbers (:352-365)
                if r.size == 0 or float(np.max(np.abs(r))) < 2.0 ** 62:
                    w = r.astype(np.int64)                                        # vectorised: (X mod M) mod p = X mod p
                    res = [np.mod(w, p).astype(np.uint64) for p in primes]
                else:
                    integers = [int(x) for x in r]
            if res is None:
                z = [int(x) + env.bigFactor if int(x) < 0 else int(x) for x in integers]
                res = [np.array([x % p for x in z], dtype=np.uint64) for p in primes]
            self.eVectors = [AtomicSealBfvEncryptedVector(res[i], e, Scale=1, SignedNumbers=False, EncryptData=EncryptData, Format=Format)
                             for i, e in enumerate(env.Environments)]

    def _device_split(self, v, env, Scale, EncryptData, Format, integers):
        """the constructor's work as ONE cn_split_encrypt / cn_split_encode call for all blocks and primes (DEVICE_SPLIT); False: the host path has to do it"""
        sparse = Format != EVectorFormat.dense
        if not _device_split_ok(env, EncryptData) or (sparse and not EncryptData):       # (a sparse plaintext vector is a host list of integers)
            return False
        try:
            x = np.asarray(v, dtype=np.float64) if integers is None else np.array([int(i) for i in integers], dtype=np.int64)
        except OverflowError:                                                             # Python integers beyond int64
            return False
        if x.ndim != 1 or x.size == 0:
            return False
        slots = env.Environments[0].SlotCount
        if sparse:
            x2 = x.reshape(-1, 1)
        elif x.size <= slots or x.size % slots == 0:
            x2 = x.reshape(-1, min(x.size, slots))
        else:                                                                             # a partial last block: zero padded, like the host path's blocks
            x2 = np.zeros(-(-x.size // slots) * slots, dtype=x.dtype)
            x2[:x.size] = x
            x2 = x2.reshape(-1, slots)
        done = _device_split(env, x2, EncryptData, sparse, Scale)
        if done is None:
            return False
        views, zero = done
        self.eVectors = [AtomicSealBfvEncryptedVector._new(Scale=1, IsSigned=False, Format=Format, Dim=int(x.size), encData=vw if EncryptData else None,
                                                           plainDense=None if EncryptData else vw, plainZero=None if EncryptData else [bool(z) for z in zero[i]])
                         for i, vw in enumerate(views)]
        return True

    @classmethod
    def _of(cls, vecs, Scale=1.0):
        r = cls()
        r.eVectors, r.Scale = vecs, Scale
        return r

    @classmethod
    def Copy(cls, v, env):
        return cls._of([AtomicSealBfvEncryptedVector.Copy(x, e) for x, e in zip(v.eVectors, env.Environments)], v.Scale)

    Dim = property(lambda self: 0 if self.eVectors is None else self.eVectors[0].Dim)
    Limbs = property(lambda self: None if self.eVectors is None else self.eVectors[0].Limbs)     # level of the ciphertexts, None for plaintexts
    IsEncrypted = property(lambda self: False if self.eVectors is None else self.eVectors[0].IsEncrypted)
    Format = property(lambda self: self.eVectors[0].Format)
    BlockSize = property(lambda self: None)

    def Dispose(self):
        if self.eVectors is not None:
            for v in self.eVectors:
                if v is not None:
                    v.Dispose()
        self.eVectors = None

    def RegisterScale(self, scale):
        self.Scale = scale

    def RegisterDim(self, dim):
        for v in self.eVectors:
            v.RegisterDim(dim)

    def _each(self, fn, env):
        return _fan_out(env.Environments, fn)

    @staticmethod
    def Interleave(vecs, shift, env):
        return EncryptedSealBfvVector._of([AtomicSealBfvEncryptedVector.Interleave([v.eVectors[i] for v in vecs], shift, e)
                                           for i, e in enumerate(env.Environments)], vecs[0].Scale)

    @staticmethod
    def Stack(vecs, env):
        return EncryptedSealBfvVector._of([AtomicSealBfvEncryptedVector.Stack([v.eVectors[i] for v in vecs], e)
                                           for i, e in enumerate(env.Environments)], vecs[0].Scale)

    def Add(self, v, env):
        if self.Scale == 0:
            return v
        if v.Scale == 0:
            return self
        if self.Scale != v.Scale:
            raise Exception("Scales do not match.")
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].Add(v.eVectors[i], e), env), self.Scale)

    def Subtract(self, v, env):
        if v.Scale == 0:
            return self
        if self.Scale != v.Scale:
            raise Exception("Scales do not match.")
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].Subtract(v.eVectors[i], e), env), self.Scale)

    @staticmethod
    def GenerateSpareOfArray(SparseVectors, env):
        return EncryptedSealBfvVector._of([AtomicSealBfvEncryptedVector.GenerateSparseOfArray([v.eVectors[i] for v in SparseVectors], e)
                                           for i, e in enumerate(env.Environments)], SparseVectors[0].Scale)

    @staticmethod
    def DenseMatrixBySparseVectorMultiply(denses, sparse, env):
        return EncryptedSealBfvVector._of([AtomicSealBfvEncryptedVector.DenseMatrixBySparseVectorMultiply([d.eVectors[i] for d in denses],
                                                                                                           sparse.eVectors[i], e)
                                           for i, e in enumerate(env.Environments)], denses[0].Scale * sparse.Scale)

    def PointwiseMultiply(self, v, env):
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].PointwiseMultiply(v.eVectors[i], e), env), self.Scale * v.Scale)

    def SumAllSlots(self, env, length=None):
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].SumAllSlots(e, length), env), self.Scale)

    def DotProduct(self, v, env, length=None, ForceOutputInColumn=None):
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].DotProduct(v.eVectors[i], e, length, ForceOutputInColumn), env),
                                          self.Scale * v.Scale)

    def Duplicate(self, count, env):
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].Duplicate(count, e), env), self.Scale)

    def Rotate(self, amount, env):
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].Rotate(amount, e), env), self.Scale)

    def Permute(self, selections, shifts, outputDim, env):
        I = [i for i, s in enumerate(selections) if s is not None]
        sel, sh = [selections[i] for i in I], [shifts[i] for i in I]
        return EncryptedSealBfvVector._of(self._each(lambda i, e: self.eVectors[i].Permute([x.eVectors[i] for x in sel], sh, outputDim, e), env), self.Scale)

    def ModSwitchTo(self, limbs, env):
        """every plaintext prime's vector switched to the level q[:limbs]; the result belongs to env.Level(limbs)"""
        return EncryptedSealBfvVector._of([v.ModSwitchTo(limbs, e) for v, e in zip(self.eVectors, env.Environments)], self.Scale)

    def ModSwitchToNext(self, env):
        return self.ModSwitchTo(env.Limbs - 1, env)

    def Write(self, stream, env):
        """EncryptedSealBfvVector.cs:430-439"""
        from . import serialization
        serialization.write_vector(stream, self, env)

    @staticmethod
    def Read(stream, env):
        """EncryptedSealBfvVector.cs:414-429"""
        from . import serialization
        return serialization.read_vector(stream, env)

    def _join(self, split, env, signed=True):
        """JoinSplitNumbers (EncryptedSealBfvVector.cs:381-411)"""
        out = []
        for j in range(len(split[0])):
            x = sum(int(split[i][j]) * env.preComputedCoefficients[i] for i in range(len(split))) % env.bigFactor
            if signed and x * 2 > env.bigFactor:
                x -= env.bigFactor
            out.append(x)
        return out

    def _device_join(self, env, signed, scale=1.0, words=False):
        """Decrypt + Decode + JoinSplitNumbers of this vector as ONE cn_decrypt_join call (dense: every block, cut to Dim; sparse: coefficient 0 of every
        entry), or None when the present path has to run: DEVICE_JOIN off, a plaintext vector, a host client or an oracle backend, a prime set
        cn_decrypt_join does not take."""
        if not self.IsEncrypted or not _device_join_ok(env):
            return None
        views = [v.encData for v in self.eVectors]
        count = views[0].count
        if any(v.count != count for v in views):
            return None
        from . import _native
        dim = int(self.Dim)
        if self.Format == EVectorFormat.dense:
            nslots = env.Environments[0].ctx.n if count > 1 else max(1, min(dim, env.Environments[0].ctx.n))
            coeff0 = False
        else:
            nslots, coeff0 = 1, True
        r = _native.decrypt_join([e.ctx for e in env.Environments], [v.h for v in views], [v.first for v in views], count, nslots,
                                 signed=signed, scale=scale, coeff0=coeff0, words=words, values=not words)
        if words:
            return [x for row in r.ints() for x in row][:dim if self.Format == EVectorFormat.dense else count]
        return r.values.reshape(-1)[:dim if self.Format == EVectorFormat.dense else count].copy()

    def DecryptFullPrecision(self, env):
        env = _env_at(env, self.Limbs)
        joined = self._device_join(env, self.IsSigned, words=True)
        if joined is not None:
            return joined
        return self._join([v.DecryptFullPrecision(e) for v, e in zip(self.eVectors, env.Environments)], env, self.IsSigned)

    def Decrypt(self, env):
        env = _env_at(env, self.Limbs)
        joined = self._device_join(env, True, scale=self.Scale)
        if joined is not None:
            return joined
        ints = self._join([v._decrypt_ints(e) for v, e in zip(self.eVectors, env.Environments)], env)
        return np.array([float(x) / self.Scale for x in ints])


# ------------------------------------------------------------------------------------------------ matrix
class EncryptedSealBfvMatrix:
    """Array of CRT vectors, column- or row-major (EncryptedSealBfvMatrix.cs)."""

    def __init__(self, columns=None, env=None, CopyVectors=True, Format=EMatrixFormat.ColumnMajor):
        self.Format = Format
        self.DataDisposedExternaly = False
        self.leVectors = None
        if columns is not None:
            if any(c.Dim != columns[0].Dim for c in columns):
                raise Exception("all columns of a matrix should have the same size")
            self.leVectors = [EncryptedSealBfvVector.Copy(c, env) for c in columns] if CopyVectors else list(columns)

    RowCount = property(lambda self: len(self.leVectors) if self.Format == EMatrixFormat.RowMajor else self.leVectors[0].Dim)
    ColumnCount = property(lambda self: len(self.leVectors) if self.Format == EMatrixFormat.ColumnMajor else self.leVectors[0].Dim)
    Scale = property(lambda self: self.leVectors[0].Scale)
    IsEncrypted = property(lambda self: all(v.IsEncrypted for v in self.leVectors))

    @property
    def Limbs(self):
        """level of the matrix's ciphertexts (coefficient moduli kept), None for a plaintext matrix"""
        for v in self.leVectors:
            if v.IsEncrypted:
                return v.Limbs
        return None

    def ModSwitchTo(self, limbs, env):
        """a NEW matrix at the level q[:limbs], bound to env.Level(limbs); `env` is the environment this matrix is at.  Per plaintext prime
        ONE cn_mod_switch over all columns: in place when they lie in one range of one array (as the batched layers produce them), otherwise
        after one gather (cn_copy_many).  A plaintext matrix is level-free and returned as it is."""
        if self.Limbs is None:
            return self
        lenv = env.Level(limbs)
        if lenv is env:
            return self
        if limbs >= env.Limbs:
            raise Exception("ModSwitchTo: level %d is not below the matrix's level %d" % (limbs, env.Limbs))
        cols = self.leVectors
        if not all(c.IsEncrypted for c in cols):
            raise Exception("ModSwitchTo: a matrix with both encrypted and plaintext columns")

        def one_prime(i, e):
            views = [c.eVectors[i].encData for c in cols]
            _check_level(e, *[c.eVectors[i] for c in cols])
            size = views[0].buf.size
            if any(v.buf.size != size for v in views):
                return None                                          # mixed ciphertext sizes: column by column below
            b0 = views[0].buf
            idx = [v.first + j for v in views for j in range(v.count)]
            total = len(idx)
            tmp = None
            if all(v.buf is b0 for v in views) and idx == list(range(idx[0], idx[0] + total)):
                h, first = b0.h, idx[0]
            else:
                tmp = _Buf(e.ctx, "ct", total, size).view()
                if hasattr(e.ctx, "copy_many"):
                    e.ctx.copy_many([v.h for v in views for _ in range(v.count)], idx, tmp.h, 0)
                else:
                    pos = 0
                    for v in views:
                        e.ctx.copy(v.h, v.first, tmp.h, pos, v.count)
                        pos += v.count
                h, first = tmp.h, 0
            out = _Buf(lenv.Environments[i].ctx, "ct", total, size)
            try:
                e.ctx.mod_switch(h, first, total, lenv.Environments[i].ctx, out.h, 0)
            finally:
                if tmp is not None:
                    tmp.release()
            return out
        per_prime = _fan_out(env.Environments, one_prime)
        r = EncryptedSealBfvMatrix(Format=self.Format)
        if any(x is None for x in per_prime):
            for x in per_prime:
                if x is not None:
                    x.view().release()
            r.leVectors = [c.ModSwitchTo(limbs, env) for c in cols]
            return r
        vecs, pos = [], 0
        for c in cols:
            cnt = c.eVectors[0].encData.count
            atoms = [AtomicSealBfvEncryptedVector._new(Scale=a.Scale, Dim=a.Dim, Format=a.Format, IsSigned=a.IsSigned, encData=per_prime[i].view(pos, cnt))
                     for i, a in enumerate(c.eVectors)]
            vecs.append(EncryptedSealBfvVector._of(atoms, c.Scale))
            pos += cnt
        r.leVectors = vecs
        return r

    def Dispose(self):
        for cache in ("_rowpt", "_rowmask", "_rowptn"):
            for buf in self.__dict__.pop(cache, {}).values():
                buf.release()
        for (_, pts) in self.__dict__.pop("_diagplan", {}).values():
            pts.release()
        if self.leVectors is not None and not self.DataDisposedExternaly:
            for v in self.leVectors:
                if v is not None:
                    v.Dispose()
        self.leVectors = None

    def _device_join(self, env):
        """every column decrypted, decoded and joined by ONE cn_decrypt_join call - when the columns are dense, encrypted and lie in one range of one
        array per plaintext prime (the batched layers' form) - as the list of the columns' value arrays; else None (column by column)"""
        cols = self.leVectors
        if not cols or not all(c.IsEncrypted and c.Format == EVectorFormat.dense for c in cols) or not _device_join_ok(env):
            return None
        if any(c.Scale != cols[0].Scale or c.Dim != cols[0].Dim for c in cols):
            return None
        P = len(env.Environments)
        blocks = cols[0].eVectors[0].encData.count
        firsts = []
        for i in range(P):
            views = [c.eVectors[i].encData for c in cols]
            if any(v.buf is not views[0].buf or v.count != blocks for v in views) or [v.first for v in views] != [views[0].first + j * blocks for j in range(len(cols))]:
                return None
            firsts.append(views[0].first)
        from . import _native
        n, dim = env.Environments[0].ctx.n, int(cols[0].Dim)
        nslots = n if blocks > 1 else max(1, min(dim, n))
        r = _native.decrypt_join([e.ctx for e in env.Environments], [cols[0].eVectors[i].encData.h for i in range(P)], firsts, blocks * len(cols), nslots,
                                 signed=True, scale=cols[0].Scale)
        return [v[:dim] for v in r.values.reshape(len(cols), blocks * nslots)]

    def Decrypt(self, env):
        env = _env_at(env, self.Limbs)
        vecs = self._device_join(env)
        if vecs is None:
            vecs = [v.Decrypt(env) for v in self.leVectors]
        return np.stack(vecs, axis=0) if self.Format == EMatrixFormat.RowMajor else np.stack(vecs, axis=1)

    def Mul(self, v, env, ForceDenseFormat=False):
        """EncryptedSealBfvMatrix.cs:70-121"""
        if self.Format == EMatrixFormat.ColumnMajor:
            if ForceDenseFormat:
                raise Exception("Forcing dense format is available only in RowMajor mode")
            return EncryptedSealBfvVector.DenseMatrixBySparseVectorMultiply(self.leVectors, v, env)
        if self._can_batch_rows(v):
            if ForceDenseFormat:
                if DIAGONAL_DENSE and self.DiagonalDenseWins(v, env):
                    return self.DiagonalDense(v, env)
                return self.RowsDotProduct(v, env, ForceOutputInColumns=True)
            temp = self.RowsDotProduct(v, env)
            res = EncryptedSealBfvVector.GenerateSpareOfArray(temp, env)
            for t in temp:
                t.Dispose()
            return res
        if not ForceDenseFormat:
            temp = [row.DotProduct(v, env) for row in self.leVectors]
            res = EncryptedSealBfvVector.GenerateSpareOfArray(temp, env)
            for t in temp:
                t.Dispose()
            return res
        total = None
        for colIndex, row in enumerate(self.leVectors):
            t = row.DotProduct(v, env, ForceOutputInColumn=colIndex)
            if total is None:
                total = t
            else:
                s = total.Add(t, env)
                total.Dispose()
                t.Dispose()
                total = s
        total.RegisterDim(len(self.leVectors))
        if total.Format != EVectorFormat.dense:
            raise Exception("Internal probloem: expecting the output to be dense")
        return total

    def _check(self, m):
        if m.Format != self.Format:
            raise Exception("Format mismatch")
        if m.RowCount != self.RowCount:
            raise Exception("Row count mismatch")
        if m.ColumnCount != self.ColumnCount:
            raise Exception("Column count mismatch")

    def Add(self, m, env):
        self._check(m)
        r = EncryptedSealBfvMatrix(Format=self.Format)
        r.leVectors = [a.Add(b, env) for a, b in zip(self.leVectors, m.leVectors)]
        return r

    def ElementWiseMultiply(self, m, env):
        """EncryptedSealBfvMatrix.cs:140-154; on the GPU all columns of one prime go through ONE cn_mul_relin launch chain."""
        self._check(m)
        r = EncryptedSealBfvMatrix(Format=self.Format)
        cols = len(self.leVectors)
        batched = all(a.IsEncrypted and b.IsEncrypted and a.Format == b.Format and a.Dim == b.Dim for a, b in zip(self.leVectors, m.leVectors))
        if not batched:
            r.leVectors = [a.PointwiseMultiply(b, env) for a, b in zip(self.leVectors, m.leVectors)]
            return r
        out = [[None] * len(env.Environments) for _ in range(cols)]

        def one_prime(i, e):
            ctx = e.ctx
            av = [c.eVectors[i] for c in self.leVectors]
            bv = [c.eVectors[i] for c in m.leVectors]
            for x, y in zip(av, bv):
                if x.IsSigned != y.IsSigned:
                    raise Exception("Can't mix signed and unsigned numbers.")
            ha, ia, ta = _gather(ctx, [x.encData for x in av])
            if m is self:
                hb, ib, tb = ha, ia, None
            else:
                hb, ib, tb = _gather(ctx, [y.encData for y in bv])
            total = len(ia)
            res = _Buf(ctx, "ct", total)
            contiguous = ia == list(range(ia[0], ia[0] + total)) and ib == list(range(ib[0], ib[0] + total))
            if contiguous:
                ctx.mul_relin(ha, ia[0], hb, ib[0], res.h, 0, total)
            else:
                for j in range(total):
                    ctx.mul_relin(ha, ia[j], hb, ib[j], res.h, j, 1)
            pos = 0
            for c, x in enumerate(av):
                cnt = x.encData.count
                out[c][i] = AtomicSealBfvEncryptedVector._new(Scale=x.Scale * bv[c].Scale, Dim=x.Dim, Format=x.Format, IsSigned=x.IsSigned,
                                                              encData=res.view(pos, cnt))
                pos += cnt
            for t in (ta, tb):
                if t is not None:
                    t.release()
        _fan_out(env.Environments, one_prime)
        r.leVectors = [EncryptedSealBfvVector._of(out[c], self.leVectors[c].Scale * m.leVectors[c].Scale) for c in range(cols)]
        return r

    def GetColumn(self, columnNumber):
        if columnNumber >= len(self.leVectors):
            raise Exception("Column does not exist")
        if self.Format != EMatrixFormat.ColumnMajor:
            raise Exception("Columns can be extracted only from a column major matrix")
        return self.leVectors[columnNumber]

    def GetRow(self, rowNumber):
        if rowNumber >= len(self.leVectors):
            raise Exception("Row does not exist")
        if self.Format != EMatrixFormat.RowMajor:
            raise Exception("Rows can be extracted only from a row major matrix")
        return self.leVectors[rowNumber]

    def SetColumn(self, columnNumber, vector):
        if columnNumber >= len(self.leVectors):
            raise Exception("Column does not exist")
        if self.Format != EMatrixFormat.ColumnMajor:
            raise Exception("Columns can be set only from a column major matrix")
        old = self.leVectors[columnNumber]
        if vector.Dim != old.Dim:
            raise Exception("dimension of vector does not match the dimension of the vector it is replacing")
        if vector.Scale != old.Scale:
            raise Exception("Scale of vector does not match the scale of the vector it is replacing")
        if vector.IsEncrypted != old.IsEncrypted:
            raise Exception("can't exchange encrypted and not encrypted vectors")
        self.leVectors[columnNumber] = vector

    def RegisterScale(self, scale):
        for v in self.leVectors:
            v.RegisterScale(scale)

    def Write(self, stream, env):
        """EncryptedSealBfvMatrix.cs:199-208"""
        from . import serialization
        serialization.write_matrix(stream, self, env)

    @staticmethod
    def Read(stream, env):
        """EncryptedSealBfvMatrix.cs:182-197"""
        from . import serialization
        return serialization.read_matrix(stream, env)

    def ConvertToColumnVector(self, env):
        return EncryptedSealBfvVector.Stack(self.leVectors, env)

    def Interleave(self, shift, env):
        if self.Format != EMatrixFormat.ColumnMajor:
            raise Exception("Expecting ColumnMajor matrix")
        return EncryptedSealBfvVector.Interleave(self.leVectors, shift, env)

    def MulColumnsByPlain(self, plain, env):
        """Every column PointwiseMultiply(plain) with ONE MultiplyPlain launch chain per plaintext prime (LLInterleaveLayer masks all
        its columns with the same selection vector, LLInterleaveLayer.cs:40-47).  Same words as the per-column loop."""
        if self.Format != EMatrixFormat.ColumnMajor:
            raise Exception("Expecting ColumnMajor matrix")
        cols = self.leVectors
        ok = (not LITERAL) and all(c.IsEncrypted and c.Format == EVectorFormat.dense and all(a.encData.count == 1 for a in c.eVectors) and c.Dim == cols[0].Dim
                 for c in cols) and (not plain.IsEncrypted) and plain.Format == EVectorFormat.dense and plain.Dim == cols[0].Dim \
            and all(a.plainDense is not None and a.plainDense.count == 1 and not a.plainZero[0] for a in plain.eVectors)
        if not ok:
            r = EncryptedSealBfvMatrix(Format=self.Format)
            r.leVectors = [c.PointwiseMultiply(plain, env) for c in cols]
            return r

        def one_prime(i, e):
            ctx = e.ctx
            h, idx, tmp = _gather(ctx, [c.eVectors[i].encData for c in cols])
            res = _Buf(ctx, "ct", len(cols))
            pd = plain.eVectors[i]._pd(ctx)
            try:
                if idx == list(range(idx[0], idx[0] + len(idx))):
                    ctx.mul_plain(h, idx[0], pd.h, pd.first, res.h, 0, len(cols), pt_stride=0)
                else:
                    for j, src in enumerate(idx):
                        ctx.mul_plain(h, src, pd.h, pd.first, res.h, j, 1)
            finally:
                if tmp is not None:
                    tmp.release()
            return res
        per_prime = _fan_out(env.Environments, one_prime)
        vecs = []
        for j, c in enumerate(cols):
            atoms = [AtomicSealBfvEncryptedVector._new(Scale=c.eVectors[i].Scale * plain.eVectors[i].Scale, Dim=c.eVectors[i].Dim, Format=EVectorFormat.dense,
                                                       IsSigned=c.eVectors[i].IsSigned, encData=per_prime[i].view(j, 1)) for i in range(len(env.Environments))]
            vecs.append(EncryptedSealBfvVector._of(atoms, c.Scale * plain.Scale))
        r = EncryptedSealBfvMatrix(Format=self.Format)
        r.leVectors = vecs
        return r

    # ---- batched HOT LOOP C: every row of a RowMajor plaintext matrix against one packed ciphertext ---------------------
    def _row_plaintexts(self, i, env_i):
        """contiguous device array with the (single-block, dense) plaintext of every row for prime i - built once per context (level)"""
        cache = self.__dict__.setdefault("_rowpt", {})
        key = (i, env_i.ctx)
        if key not in cache:
            rows = [r.eVectors[i] for r in self.leVectors]
            buf = _Buf(env_i.ctx, "pt", len(rows)).view()
            if rows[0].plainDense.buf.ctx is env_i.ctx:
                for k, r in enumerate(rows):
                    env_i.ctx.copy(r.plainDense.h, r.plainDense.first, buf.h, k, 1)
            else:                                                    # at a level: one upload of the rows (not a copy per row per level)
                src = [r.plainDense for r in rows]
                env_i.ctx.pt_upload(buf.h, 0, np.concatenate([v.buf.ctx.pt_download(v.h, v.first, 1) for v in src]))
            cache[key] = buf
        return cache[key]

    def _row_ptn(self, i, env_i):
        """the rows of _row_plaintexts in NTT form (NTT_WEIGHTS): what RowsDotProduct hands to rowdot_batch - transformed once per context (level).  The
        coefficient-form rows stay: _diagonal_plan and the bias path read them"""
        cache = self.__dict__.setdefault("_rowptn", {})
        key = (i, env_i.ctx)
        if key not in cache:
            rows = self._row_plaintexts(i, env_i)
            buf = _Buf(env_i.ctx, "ptn", rows.count).view()
            env_i.ctx.pt_transform(rows.h, rows.first, rows.count, buf.h, 0)
            cache[key] = buf
        return cache[key]

    def _can_batch_rows(self, v):
        return (not LITERAL and self.Format == EMatrixFormat.RowMajor and v.IsEncrypted and v.Format == EVectorFormat.dense
                and all(a.encData.count == 1 for a in v.eVectors)
                and all((not r.IsEncrypted) and r.Format == EVectorFormat.dense and r.Dim == v.Dim
                        and all(a.plainDense is not None and a.plainDense.count == 1 and not a.plainZero[0] for a in r.eVectors)
                        for r in self.leVectors))

    def RowsDotProduct(self, v, env, length=None, ForceOutputInColumns=False, bias=None):
        """[row_r . v for every row r] with ONE launch chain per plaintext prime: the packed ciphertext is replicated R times,
        multiplied by the R row plaintexts (cn_mul_plain, count R) and reduced by the rotate-and-add tree of
        AtomicSealBfvEncryptedVector.SumAllSlots (:888-955) applied to all R ciphertexts at once (cn_rotate_rows / cn_add, count R).
        Same ciphertext words as R sequential DotProduct calls.  Returns the list of R result vectors (or, with
        ForceOutputInColumns, their mask-accumulated dense sum as a single vector, EncryptedSealBfvMatrix.cs:91-120);
        `bias`: optional RowMajor plaintext matrix added row-wise (LLPackedDenseLayer.cs:72)."""
        INT_MAX = 2 ** 31 - 1
        R = len(self.leVectors)
        full = length is None

        def one_prime(i, e):
            ctx, slots = e.ctx, e.SlotCount
            src = v.eVectors[i].encData
            ntt = NTT_WEIGHTS and hasattr(ctx, "pt_transform")
            pts = self._row_ptn(i, e) if ntt else self._row_plaintexts(i, e)
            work = _Buf(ctx, "ct", R)
            wv = work.view()
            ln = INT_MAX if full else int(length)
            if ln <= 0:
                raise Exception("Can't sum over less then one element")
            # replicate + MultiplyPlain + the SumAllSlots rotate-and-add tree for all R rows: ONE library call per prime
            ctx.rowdot_batch(src.h, src.first, pts.h, pts.first, R, 0 if ln >= slots else ln, work.h, 0)
            if ln >= slots // 2:
                ln = slots // 2
            dim = 1 if ln >= slots // 2 else v.Dim
            fmt = EVectorFormat.sparse if ln >= slots else EVectorFormat.dense
            if ForceOutputInColumns:
                mcache = self.__dict__.setdefault("_rowmask", {})
                if (i, ctx, ntt) not in mcache:                      # one-hot masks e_r (SumAllSlots ForceOutputInColumn, :936-945), per context (level) and form
                    masks = _Buf(ctx, "pt", R).view()
                    ctx.encode_batch(np.eye(R, dtype=np.uint64), masks.h, 0)          # e_0 .. e_{R-1} in one call
                    if ntt:
                        coeff, masks = masks, _Buf(ctx, "ptn", R).view()
                        ctx.pt_transform(coeff.h, 0, R, masks.h, 0)
                        coeff.release()
                    mcache[(i, ctx, ntt)] = masks
                masks = mcache[(i, ctx, ntt)]
                ctx.mul_plain(work.h, 0, masks.h, 0, work.h, 0, R)
                tot = _Buf(ctx, "ct", 1)
                ctx.add_many(work.h, list(range(R)), tot.h, 0)
                wv.release()
                work, wv = tot, tot.view()
            elif bias is not None:
                bp = bias._row_plaintexts(i, e)
                ctx.add_plain(work.h, 0, bp.h, bp.first, work.h, 0, R)
            return work, wv, dim, fmt
        done = _fan_out(env.Environments, one_prime)
        per_prime = [(w, x) for (w, x, _, _) in done]
        out_dim, out_fmt = done[0][2], done[0][3]
        signed = v.eVectors[0].IsSigned
        if ForceOutputInColumns:
            atoms = [AtomicSealBfvEncryptedVector._new(Scale=1, Dim=R, Format=EVectorFormat.dense, IsSigned=signed, encData=wv)
                     for (_, wv) in per_prime]
            return EncryptedSealBfvVector._of(atoms, self.leVectors[0].Scale * v.Scale)
        res = []
        for r in range(R):
            atoms = [AtomicSealBfvEncryptedVector._new(Scale=1, Dim=out_dim, Format=out_fmt, IsSigned=signed, encData=work.view(r, 1))
                     for (work, _) in per_prime]
            res.append(EncryptedSealBfvVector._of(atoms, self.leVectors[r].Scale * v.Scale))
        for (_, wv) in per_prime:
            wv.release()
        return res

    # ---- the dense product by generalized diagonals (DIAGONAL_DENSE; diagonal.py) ---------------------------
    def DiagonalDenseCounts(self, v, env):
        """diagonal.dense_path_counts for this matrix against the packed vector v in `env` (None: the matrix has more rows than a ciphertext has slots)"""
        from . import diagonal
        ctx = env.Environments[0].ctx
        R, n = len(self.leVectors), ctx.n
        if R > n or v.Dim > n:
            return None
        args = (R, int(v.Dim), n, len(ctx.q), diagonal.ks_digits(ctx.q, ctx.gdbc))
        c = diagonal.dense_path_counts(*args, ntt_weights=NTT_WEIGHTS and hasattr(ctx, "pt_transform"))
        # HOISTED_ROTATIONS: the baby steps are priced as one hoisted call only where the context holds their direct keys - without them the run goes by doubling.
        # (Not foreseen here: a context whose planner refuses the call - the integer policy at N = 16384 - is still priced as hoisted when it holds the keys.)
        hoisted = HOISTED_ROTATIONS and _hoisted_keys_held(ctx, c["B"])
        if hoisted or _summed(ctx):                                  # SUMMED_ROTATIONS: the giant steps of a column class share one pair of inverse transforms per limb
            c = diagonal.dense_path_counts(*args, B=c["B"], ntt_weights=NTT_WEIGHTS and hasattr(ctx, "pt_transform"), hoisted=hoisted, summed=_summed(ctx))
        return c

    def DiagonalDenseWins(self, v, env):
        c = self.DiagonalDenseCounts(v, env)
        return c is not None and c["choice"] == "diagonal"

    def _diagonal_plan(self, i, env_i, B=None):
        """(plan, device array of its pre-rotated diagonal plaintexts) for prime i - built once per context (level), like _row_plaintexts: the weights are the
        integers the row plaintexts hold, rotated in slot space on the host and encoded in chunks.  Under NTT_WEIGHTS the array holds the diagonals in NTT form: each
        chunk is encoded into a chunk-sized plaintext buffer and transformed into the array, so the resident footprint is k times the coefficient form, not k + 1.
        Under DEVICE_DIAGONAL_PLAN (and a context with diag_scan) nothing travels: the same plan from the flags of cn_diag_scan, the same words from cn_diag_encode"""
        from . import diagonal
        cache = self.__dict__.setdefault("_diagplan", {})
        ntt = NTT_WEIGHTS and hasattr(env_i.ctx, "pt_transform")
        dev = DEVICE_DIAGONAL_PLAN and hasattr(env_i.ctx, "diag_scan")
        key = (i, env_i.ctx, B, ntt, dev)
        if key not in cache and dev:                                 # scan, plan, an array of exactly its terms, one call that fills it
            ctx = env_i.ctx
            R, dim = len(self.leVectors), int(self.leVectors[0].Dim)
            rows = self._row_plaintexts(i, env_i)
            plan, terms = diagonal.plan_from_flags(ctx.diag_scan(rows.h, rows.first, R, dim), ctx.n, R, dim, B=B)
            pts = _Buf(ctx, "ptn" if ntt else "pt", plan.terms).view()
            try:
                ctx.diag_encode(rows.h, rows.first, R, dim, terms, pts.h, pts.first)
            except BaseException:
                pts.release()
                raise
            cache[key] = (plan, pts)
        if key not in cache:
            ctx = env_i.ctx
            R, dim = len(self.leVectors), int(self.leVectors[0].Dim)
            rows = self._row_plaintexts(i, env_i)
            W = np.ascontiguousarray(ctx.decode_batch(rows.h, rows.first, R)[:, :dim])
            bound = int(diagonal.structural_diagonals(R, dim, ctx.n).sum())
            chunk = 256
            pts = _Buf(ctx, "ptn" if ntt else "pt", bound).view()
            stage = _Buf(ctx, "pt", min(chunk, bound)).view() if ntt else None

            def emit(first, slots):
                if ntt:
                    ctx.encode_batch(slots, stage.h, 0)
                    ctx.pt_transform(stage.h, 0, len(slots), pts.h, pts.first + first)
                else:
                    ctx.encode_batch(slots, pts.h, pts.first + first)
            try:
                plan = diagonal.build_plan(W, ctx.n, emit, B=B, chunk=chunk)
            except BaseException:
                pts.release()
                raise
            finally:
                if stage is not None:
                    stage.release()
            cache[key] = (plan, pts)
        return cache[key]

    def DiagonalDense(self, v, env, B=None):
        """Mul(v, ForceDenseFormat=True) by generalized diagonals: per plaintext prime the baby steps rho_b(v) (by doubling: log2 B cn_rotate_rows calls), ONE
        cn_mul_plain_sum for the 2 Gs sums of diagonal x rotation products (contexts without it: mul_plain + add_many per group), the giant steps by folding (log2 Gs
        cn_rotate_rows_add calls over both column groups) and one cn_rotate_columns_add; cn_rotate_rows_many / cn_add_many where zero diagonals leave gaps.  The result
        is the vector RowsDotProduct(ForceOutputInColumns=True) returns: row r in slot r, zero elsewhere, same Scale, Dim, format and sign."""
        R = len(self.leVectors)

        def one_prime(i, e):
            ctx = e.ctx
            plan, pts = self._diagonal_plan(i, e, B)
            src = v.eVectors[i].encData
            nb, ng, Bs, Gs = len(plan.babies), len(plan.groups), plan.B, plan.Gs
            bab, u = _Buf(ctx, "ct", nb), _Buf(ctx, "ct", ng)
            bv, uv = bab.view(), u.view()
            ctx.copy(src.h, src.first, bab.h, 0, 1)
            if nb > 1 and _rotate_hoisted(ctx, bab.h, 0, plan.babies[1:], bab.h, range(1, nb)):
                pass                                                 # HOISTED_ROTATIONS: every baby step one key switch away from the input, never by doubling
            elif plan.babies_by_doubling:
                s = 1
                while s < Bs:                                        # rho_(b + s)(v) = rho_s(rho_b(v)) for all b < s at once
                    ctx.rotate_rows(bab.h, 0, s, bab.h, s, s)
                    s *= 2
            elif nb > 1:
                ctx.rotate_rows_many(bab.h, [0] * (nb - 1), plan.babies[1:], bab.h, list(range(1, nb)))
            if hasattr(ctx, "mul_plain_sum"):
                ctx.mul_plain_sum(bab.h, 0, pts.h, pts.first, plan.grp_off, plan.ct_idx, u.h, 0)
            else:                                                    # (the CPU backend): the composed loop
                for g in range(ng):
                    e0, e1 = plan.grp_off[g], plan.grp_off[g + 1]
                    tmp = _Buf(ctx, "ct", e1 - e0)
                    tv = tmp.view()
                    for x in range(e0, e1):
                        ctx.mul_plain(bab.h, plan.ct_idx[x], pts.h, pts.first + x, tmp.h, x - e0, 1)
                    ctx.add_many(tmp.h, list(range(e1 - e0)), u.h, g)
                    tv.release()
            bv.release()
            res = _Buf(ctx, "ct", 1)
            if _summed(ctx):                                         # SUMMED_ROTATIONS: the giant steps of every column class in ONE call - term (u[g], j B), j = 0 as step 0
                members = [[g for g, (_, c) in enumerate(plan.groups) if c == cc] for cc in (0, 1)]
                used = [cc for cc in (0, 1) if members[cc]]
                idx = [g for cc in used for g in members[cc]]
                off = [0]
                for cc in used:
                    off.append(off[-1] + len(members[cc]))
                tot = _Buf(ctx, "ct", len(used))
                tv = tot.view()
                ctx.rotate_rows_sum(u.h, idx, [plan.groups[g][0] * Bs for g in idx], off, tot.h, 0)
                if len(used) == 2:
                    ctx.rotate_columns_add(tot.h, 1, tot.h, 0, res.h, 0, 1)
                elif used == [1]:
                    ctx.rotate_columns(tot.h, 0, res.h, 0, 1)
                else:
                    ctx.copy(tot.h, 0, res.h, 0, 1)
                tv.release()
            elif plan.giants_by_folding:                               # u[nc j + x] += rho_(half B)(u[nc (j + half) + x]) for j < half, every column class at once
                nc, half = len(plan.classes), Gs // 2
                while half >= 1:
                    ctx.rotate_rows_add(u.h, nc * half, half * Bs, u.h, 0, u.h, 0, nc * half)
                    half //= 2
                if nc == 2:
                    ctx.rotate_columns_add(u.h, 1, u.h, 0, res.h, 0, 1)
                elif plan.classes == [1]:
                    ctx.rotate_columns(u.h, 0, res.h, 0, 1)
                else:
                    ctx.copy(u.h, 0, res.h, 0, 1)
            else:
                far = [g for g, (j, _) in enumerate(plan.groups) if j]
                if far:
                    ctx.rotate_rows_many(u.h, far, [plan.groups[g][0] * Bs for g in far], u.h, far)
                tot = _Buf(ctx, "ct", 2)
                tv = tot.view()
                members = [[g for g, (_, c) in enumerate(plan.groups) if c == cc] for cc in (0, 1)]
                for cc in (0, 1):
                    if members[cc]:
                        ctx.add_many(u.h, members[cc], tot.h, cc)
                if members[0] and members[1]:
                    ctx.rotate_columns_add(tot.h, 1, tot.h, 0, res.h, 0, 1)
                elif members[1]:
                    ctx.rotate_columns(tot.h, 1, res.h, 0, 1)
                else:
                    ctx.copy(tot.h, 0, res.h, 0, 1)
                tv.release()
            uv.release()
            return res.view()
        views = _fan_out(env.Environments, one_prime)
        signed = v.eVectors[0].IsSigned
        atoms = [AtomicSealBfvEncryptedVector._new(Scale=1, Dim=R, Format=EVectorFormat.dense, IsSigned=signed, encData=wv) for wv in views]
        return EncryptedSealBfvVector._of(atoms, self.leVectors[0].Scale * v.Scale)

    # ---- batched HOT LOOP A for a whole PoolLayer (PoolLayer.cs:149-229 issues one Mul per output) -----------------
    def MulManySparse(self, gather, weights, bias, out_scale, env, cache=None, bias_vectors=None):
        """out[o] = sum_k weights[o][k] * column[gather[o][k]] + bias[o]  for all outputs in one scalar GEMM per prime.
        gather: int32 [O,K] (-1 = padded tap), weights: integer rows (scaled, signed), bias: integers or None.
        Equivalent to O calls of Mul(sparse plain weight window) followed by Add(dense plain bias).  `cache`: a dict owned by the
        calling layer - the planned GEMM (weight tiles, gather tables, bias plaintexts in HBM) is kept there per plaintext prime and
        only launched on the next inference (cn_gemm_plan_create / cn_gemm_plan_apply).  `bias_vectors`: instead of integer
        constants, one dense plaintext vector per output (LLPoolLayer adds `hot * bias`, LLPoolLayer.cs:128-134)."""
        if self.Format != EMatrixFormat.ColumnMajor:
            raise Exception("Expecting ColumnMajor matrix")
        O = len(weights)

        def one_prime(i, e):
            ctx, p = e.ctx, e.plainmodulusValue
            cols = [c.eVectors[i] for c in self.leVectors]
            if any(c.encData is None or c.encData.count != 1 for c in cols):
                raise Exception("batched PoolLayer expects single-block encrypted columns")
            h, idx, tmp = _gather(ctx, [c.encData for c in cols])
            res = _Buf(ctx, "ct", O)
            key = (i, _ctx_limbs(ctx), tuple(idx), None if bias is None else tuple(int(b) for b in bias), bias_vectors is not None)   # the bias depends on the input scale; plans belong to one context (level)
            if cache is not None and key in cache and hasattr(ctx, "gemm_apply"):
                try:
                    ctx.gemm_apply(cache[key][0], h, res.h, 0)
                finally:
                    if tmp is not None:
                        tmp.release()
                return res
            g = np.asarray(gather, dtype=np.int64)
            gidx = np.where(g >= 0, np.asarray(idx, dtype=np.int64)[np.maximum(g, 0)], -1).astype(np.int32)
            W = np.array([[int(x) % p for x in row] for row in weights], dtype=np.uint64)
            bh, bidx = 0, None
            if bias_vectors is not None:
                bp = _Buf(ctx, "pt", O).view()
                for o_, bv in enumerate(bias_vectors):
                    pd = bv.eVectors[i]._pd(ctx)
                    ctx.copy(pd.h, pd.first, bp.h, o_, 1)
                bh, bidx = bp.h, np.arange(O, dtype=np.int32)
            elif bias is not None:
                bvals = [int(b) % p for b in bias]
                uniq = sorted(set(bvals))
                pos = {v: j for j, v in enumerate(uniq)}
                bp = _Buf(ctx, "pt", len(uniq)).view()
                polys = np.zeros((len(uniq), ctx.n), dtype=np.uint64)
                polys[:, 0] = np.array(uniq, dtype=np.uint64)      # Encode(constant vector) = constant polynomial
                ctx.pt_upload(bp.h, 0, polys)
                bh, bidx = bp.h, np.array([pos[v] for v in bvals], dtype=np.int32)
            if cache is not None and hasattr(ctx, "gemm_plan"):
                try:
                    plan = ctx.gemm_plan(W, idx=gidx, bias_pt=bh, bias_idx=bidx)
                    cache[key] = (plan, bp if (bias is not None or bias_vectors is not None) else None)      # the plan references the bias plaintexts: keep both
                    ctx.gemm_apply(plan, h, res.h, 0)
                finally:
                    if tmp is not None:
                        tmp.release()
                return res
            try:
                ctx.scalar_gemm(h, W, res.h, 0, idx=gidx, bias_pt=bh, bias_idx=bidx)
            finally:
                if tmp is not None:
                    tmp.release()
                if bias is not None or bias_vectors is not None:
                    bp.release()
            return res
        per_prime = _fan_out(env.Environments, one_prime)
        dim = self.leVectors[0].Dim
        vecs = []
        for o in range(O):
            atoms = [AtomicSealBfvEncryptedVector._new(Scale=1, Dim=dim, Format=EVectorFormat.dense, IsSigned=False, encData=per_prime[i].view(o, 1))
                     for i in range(len(env.Environments))]
            vecs.append(EncryptedSealBfvVector._of(atoms, out_scale))
        r = EncryptedSealBfvMatrix(Format=EMatrixFormat.ColumnMajor)
        r.leVectors = vecs
        return r


# ------------------------------------------------------------------------------------------------ factory
class CapturedEvaluation:
    """A recorded evaluation (one HIP graph per plaintext-prime context, `cn_graph_begin/end/launch`): the launch-bound chain of a
    single-image inference - LoLa issues ~235 small launches per prime (`LoLaCryptonets.cs:236-278`) - replayed with one launch per
    prime.  `fn(inputs)` is the evaluation (layer `Apply` chain) on encrypted matrices; it must have run once before on data of the same
    shapes (temporaries then come out of the handle pools).  `run(new_inputs)` writes the new ciphertext words into the buffers the
    recording read, launches the graphs and returns the matrix the recording produced (same object every time: decrypt or copy it
    before the next run).  Everything the recording created stays alive until `Dispose`.
    A chain that switches levels (ModSwitchLayer) is recorded across them: each prime's graph covers its context and its level contexts
    (cn_graph_begin_levels) and replays with one launch on the first level.  `levels`: the limb counts of those level contexts (the levels the
    rehearsal ran at); None: every level the environment has cached (`Level(limbs)`); (): none (cn_graph_begin)."""

    def __init__(self, env, fn, inputs, levels=None):
        self.env, self.inputs = env, list(inputs)
        ctxs = [e.ctx for e in env.Environments]
        pick = (lambda e: sorted(e._levels)) if levels is None else (lambda e: sorted(set(int(x) for x in levels), reverse=True))
        levels = [[e.Level(lv).ctx for lv in pick(e)] for e in env.Environments]
        import gc
        gc.collect()                                  # temporaries of the rehearsal that only the collector frees go back to the pools first
        self.graphs, begun, failure = [], [], None
        try:
            for c, lv in zip(ctxs, levels):
                if lv:
                    c.graph_begin(levels=lv)
                else:
                    c.graph_begin()
                begun.append(c)
            self.result = fn(*self.inputs)
        except BaseException as ex:                   # noqa: BLE001 - re-raised below, after every context has left capture mode
            failure = ex
        for c in begun:                               # every context that entered capture mode leaves it, whatever happened
            try:
                self.graphs.append((c, c.graph_end()))
            except Exception as ex:                   # noqa: BLE001
                failure = failure or ex
        if failure is not None:                       # a failed recording keeps nothing: its graphs would pin the scratch arenas
            for c, g in self.graphs:
                c.free(g)
            self.graphs = []
            raise failure
        self.graphs = [g for _, g in self.graphs]

    @staticmethod
    def _views(m):
        return [[a.encData for a in v.eVectors] for v in m.leVectors]

    def run(self, *new_inputs):
        for dst, src in zip(self.inputs, new_inputs):
            if src is dst:
                continue
            for dv, sv in zip(self._views(dst), self._views(src)):
                for e, d, s_ in zip(self.env.Environments, dv, sv):
                    if d.count != s_.count:
                        raise Exception("a captured evaluation takes inputs of the shapes it was recorded with")
                    e.ctx.copy(s_.h, s_.first, d.h, d.first, d.count)
        for e, g in zip(self.env.Environments, self.graphs):
            e.ctx.graph_launch(g)
        return self.result

    def Dispose(self):
        """frees the graphs (on the first-level contexts that own them): the level contexts they cover can be closed after this"""
        for e, g in zip(self.env.Environments, self.graphs):
            e.ctx.free(g)
        self.graphs = []


class EncryptedSealBfvFactory:
    """IFactory.cs:240-410.  `client_factory(t, n, q, dbc, gdbc)` builds the client-side SEAL objects for one plaintext
    prime; the device contexts are libcnhip contexts (`context_factory` is only overridden by the CPU test harness)."""
    DefaultDecompositionBitCount = 10
    DefaultGaloisDecompositionBitCount = 20

    def __init__(self, primes=None, n=4096, DecompositionBitCount=10, GaloisDecompositionBitCount=20, SmallModulusCount=-1,
                 client_factory=None, context_factory=None, device=0, galois=True, client_seed=None, device_client_factory=None, steps=None):
        """client_seed: None (default) = keys and encryption randomness from the OS entropy source; an integer makes the default
        DeviceClient reproducible (tests only - whoever knows it can regenerate the secret key).  device_client_factory(ctx, t): a client
        that lives on the context (e.g. client.SharedKeyDeviceClient: one rank generates, the others receive the keys by RCCL broadcast).
        steps: None = the default Galois key set; a list of RotateRows step counts = keys for exactly these rotations and the column swap
        (KeyGenerator.GaloisKeys(dbc, steps); networks.rotation_steps finds the list of a network)."""
        if primes is None:
            primes = [40961, 65537, 114689, 147457, 188417]
            n = 4096
        if context_factory is None:
            from ._native import Context, default_coeff_modulus

            def context_factory(n_, t_, q_, dbc_, gdbc_):
                return Context(n_, t_, q=q_, dbc=dbc_, gdbc=gdbc_, device=device)
            q = default_coeff_modulus(n)
        else:
            q = context_factory.default_coeff_modulus(n)
        if SmallModulusCount > 0:
            q = q[:SmallModulusCount]
        envs = []
        for t in primes:
            ctx = context_factory(n, t, q, DecompositionBitCount, GaloisDecompositionBitCount)
            if client_factory is not None:
                client = client_factory(t, n, q, DecompositionBitCount, GaloisDecompositionBitCount)
            elif device_client_factory is not None:
                client = device_client_factory(ctx, t)
            else:
                from .client import DeviceClient                   # keygen / encrypt / decrypt on the device, seeded from os.urandom
                client = DeviceClient(ctx, seed=None if client_seed is None else client_seed ^ t)
            e = AtomicSealBfvEncryptedEnvironment(ctx, client)
            if client is not None:
                e.GenerateEncryptionKeys(with_galois=galois, steps=steps)
            envs.append(e)
        self.referenceEnvironment = EncryptedSealBfvEnvironment(envs, ParentFactory=self)

    @classmethod
    def Load(cls, source, device=0, context_factory=None, client_factory=None):
        """EncryptedSealBfvFactory(string fileName) / (Stream stream) (IFactory.cs:262-276): environments from the zip key
        container.  `client_factory(ctx)` overrides the client built on each loaded context (default DeviceClient)."""
        from . import serialization
        if context_factory is None:
            from ._native import Context

            def context_factory(n_, t_, q_, dbc_, gdbc_):
                return Context(n_, t_, q=q_, dbc=dbc_, gdbc=gdbc_, device=device)
        self = cls.__new__(cls)
        if isinstance(source, (str, bytes)):
            with open(source, "rb") as f:
                envs = serialization.load_environments(f, context_factory, client_factory)
        else:
            envs = serialization.load_environments(source, context_factory, client_factory)
        self.referenceEnvironment = EncryptedSealBfvEnvironment(envs, ParentFactory=self)
        return self

    def Save(self, target, withPrivateKeys=False):
        """IFactory.cs:296-304: zip of one key stream per plaintext prime; the secret keys only on request"""
        from . import serialization
        if isinstance(target, (str, bytes)):
            with open(target, "wb") as f:
                serialization.save_environments(f, self.referenceEnvironment.Environments, withPrivateKeys)
            return None
        return serialization.save_environments(target, self.referenceEnvironment.Environments, withPrivateKeys)

    def LoadVector(self, stream):
        return EncryptedSealBfvVector.Read(stream, self.referenceEnvironment)

    def LoadMatrix(self, stream):
        return EncryptedSealBfvMatrix.Read(stream, self.referenceEnvironment)

    def AllocateComputationEnv(self):
        return self.referenceEnvironment

    def FreeComputationEnv(self, env):
        pass

    def CopyVector(self, v):
        return EncryptedSealBfvVector.Copy(v, self.referenceEnvironment)

    def GetPlainVector(self, v, format, scale=None):
        if scale is None:
            return EncryptedSealBfvVector(env=self.referenceEnvironment, EncryptData=False, Format=format, integers=v)
        return EncryptedSealBfvVector(v, self.referenceEnvironment, scale, EncryptData=False, Format=format)

    def GetEncryptedVector(self, v, format, scale=None):
        if scale is None:
            return EncryptedSealBfvVector(env=self.referenceEnvironment, EncryptData=True, Format=format, integers=v)
        return EncryptedSealBfvVector(v, self.referenceEnvironment, scale, EncryptData=True, Format=format)

    def _matrix(self, m, format, scale, encrypt):
        m = np.asarray(m, dtype=np.float64)
        rows = m.T if format == EMatrixFormat.ColumnMajor else m                 # (a view: the column-major request reaches the device as transposed strides)
        env = self.referenceEnvironment
        if rows.ndim == 2 and rows.shape[0] and 0 < rows.shape[1] <= env.Environments[0].SlotCount and _device_split_ok(env, encrypt):
            # ONE call for the whole matrix: all vectors of a prime lie in one array, in order, each a view of it - the form the batched layers produce and
            # EncryptedSealBfvMatrix.ModSwitchTo / Decrypt take without a gather
            done = _device_split(env, rows, encrypt, False, scale)
            if done is not None:
                views, zero = done
                vecs = []
                for j in range(rows.shape[0]):
                    atoms = [AtomicSealBfvEncryptedVector._new(Scale=1, IsSigned=False, Format=EVectorFormat.dense, Dim=int(rows.shape[1]),
                                                               encData=vw.sub(j) if encrypt else None, plainDense=None if encrypt else vw.sub(j),
                                                               plainZero=None if encrypt else [bool(zero[i][j])]) for i, vw in enumerate(views)]
                    vecs.append(EncryptedSealBfvVector._of(atoms, scale))
                for vw in views:
                    vw.release()                                                 # (the columns' views keep the arrays alive)
                return EncryptedSealBfvMatrix(vecs, env, CopyVectors=False, Format=format)
        vecs = [EncryptedSealBfvVector(r, self.referenceEnvironment, scale, EncryptData=encrypt, Format=EVectorFormat.dense) for r in rows]
        return EncryptedSealBfvMatrix(vecs, self.referenceEnvironment, CopyVectors=False, Format=format)

    def GetPlainMatrix(self, m, format, scale):
        return self._matrix(m, format, scale, False)

    def GetEncryptedMatrix(self, m, format, scale):
        return self._matrix(m, format, scale, True)

    def GetMatrix(self, vectors, format, CopyVectors=True):
        return EncryptedSealBfvMatrix(list(vectors), self.referenceEnvironment, CopyVectors=CopyVectors, Format=format)

    def GetValueFromString(self, s):
        f = [int(x) for x in s.split(",")]
        env = self.referenceEnvironment
        return sum(c * x for c, x in zip(env.preComputedCoefficients, f)) % env.bigFactor

    def GetStringFromValue(self, value):
        return ",".join(str(value % e.plainmodulusValue) for e in self.referenceEnvironment.Environments)
