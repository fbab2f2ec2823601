"""ctypes binding of libcnhip.so (C ABI declared in include/cnhip.h).

There is NO CPU fallback: if the HIP library is missing or no GPU is present, the
operations raise.  The oracle under oracle/ is never imported from this package.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_PKG, "lib", "libcnhip.so")
CSRC = os.path.join(_PKG, "csrc")
# one translation unit per kernel family: hipcc compiles them in parallel (the register-radix kernels alone are ~180 instantiations)
SOURCES = [os.path.join(CSRC, f) for f in (
    "cn_api.hip", "cn_eval.hip", "cn_client.hip", "cn_defer.hip", "cn_multi.hip", "cn_host.cpp", "cn_tables.cpp", "cn_l_gemm.hip", "cn_l_behz.hip",
    "cn_l_rr_u64.hip", "cn_l_rr_f64.hip", "cn_l_rr_f64l.hip", "cn_l_ks_u64.hip", "cn_l_ks_f64.hip", "cn_l_ks_f64l.hip", "cn_level.hip", "cn_l_modswitch.hip",
    "cn_l_modswitch_f64.hip", "cn_l_noise.hip", "cn_l_seeded.hip", "cn_l_keygen.hip", "cn_l_packed.hip", "cn_l_join.hip",
    "cn_l_split.hip", "cn_l_diag.hip", "cn_l_ptn.hip", "cn_l_diagplan.hip")]
OBJ_DIR = os.path.join(_PKG, "lib", "obj")

U64P = C.POINTER(C.c_uint64)
I32P = C.POINTER(C.c_int32)
U32P = C.POINTER(C.c_uint32)


CN_ERR_ARG, CN_ERR_NOKEY = -1, -3                            # include/cnhip.h
# the two refusals of the hoisted-rotation planner (cn_ks_hoist_plan, cn_ks_plan.h) that mean "this context has no kernel for the call", as they begin
HOISTED_UNAVAILABLE = ("hoisted rotations need the register-radix kernels", "hoisted rotations: no kernel under the integer policy")


class CnError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libcnhip error %d: %s" % (code, msg))
        self.code = code


class CnStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "Multiplication", "PlainMultiplication", "Addition", "PlainAddition", "Subtraction", "PlainSubtraction",
        "Rotation", "AddMany", "AddManyItemCount", "Relinarization",
        "ntt_forward_limbs", "ntt_inverse_limbs", "kernel_launches")]


def _deps(path, seen=None):
    """`path` and every header it includes (transitively, quoted includes only)"""
    import re
    seen = set() if seen is None else seen
    if path in seen or not os.path.exists(path):
        return seen
    seen.add(path)
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
        _deps(os.path.normpath(os.path.join(os.path.dirname(path), inc)), seen)
    return seen


# Instruction-scheduling strategy of the compiler per translation unit (-mllvm -amdgpu-sched-strategy=...), measured on the MI355X against the default
# (profiles/r03_sched_strategy.txt, one box, alternating runs): the key-switch unit of the moduli up to 44 bits (CryptoNets / LoLa: N <= 8192) under
# "max-memory-clause" (fused key switch 3.37-3.41 -> 3.27-3.31 ms, the same 212 VGPRs; batch -0.7 %); under "max-ilp" the key switch is 18 % SLOWER (224
# VGPRs).  The unit of the 48-49-bit moduli (N = 16384) stays with the default: the split key switch of the LoLa-CIFAR shapes lost 29 % under
# "max-memory-clause" (1.77 against 1.37 s per image).  The transform units stay with the default: "max-ilp" makes the forward
# N=8192 kernel of the roofline line 7 % faster (0.46-0.47 -> 0.50 of the HBM peak at 115 VGPRs) but takes the inverse kernel to 162 VGPRs (one workgroup
# per CU instead of two) and makes the N=16384 kernels spill.  CN_SCHED_STRATEGY=0 builds everything with the default.
SCHED_STRATEGY = {"cn_l_ks_f64l.hip": "max-memory-clause"}


def _unit_flags(src):
    if os.environ.get("CN_SCHED_STRATEGY", "1") == "0":
        return []
    st = SCHED_STRATEGY.get(os.path.basename(src))
    return ["-mllvm", "-amdgpu-sched-strategy=" + st] if st else []


def build(force=False, verbose=False, defines=(), out=None):
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU): the translation units are compiled in
    parallel into lib/obj/ (only those whose sources changed), then linked.  `defines` / `out`: A/B builds of tools/ (-D switches,
    another library name - their objects go to a directory of their own)."""
    from concurrent.futures import ThreadPoolExecutor
    if defines and out is None:
        raise ValueError("build(defines=...) needs `out`: an A/B build must not share objects or the library name with the default build")
    lib_path = out or LIB_PATH
    obj_dir = OBJ_DIR
    if out is not None:                  # objects of another flag set never mix: the directory name carries a digest of the -D switches
        import hashlib
        obj_dir = os.path.splitext(out)[0] + "_obj" + ("_" + hashlib.sha1(" ".join(sorted(defines)).encode()).hexdigest()[:8] if defines else "")
    os.makedirs(obj_dir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function", *["-D" + d for d in defines]]
    jobs, stamps = [], {}
    for src in SOURCES:
        obj = os.path.join(obj_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        newest = max(os.path.getmtime(d) for d in _deps(src))
        cmd = [hipcc, *flags, *_unit_flags(src), "-c", src, "-o", obj]
        # the command line is part of the staleness key (toggling CN_SCHED_STRATEGY used to reuse objects built with the other setting)
        stamp = obj + ".cmd"
        same_cmd = os.path.exists(stamp) and open(stamp).read() == " ".join(cmd)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < newest or not same_cmd:
            jobs.append(cmd)
            stamps[obj] = (stamp, " ".join(cmd))
    objs = [os.path.join(obj_dir, os.path.splitext(os.path.basename(src))[0] + ".o") for src in SOURCES]
    if not jobs and os.path.exists(lib_path) and all(os.path.getmtime(lib_path) >= os.path.getmtime(o) for o in objs):
        return lib_path

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1) or 1) as ex:
        list(ex.map(run, jobs))
    for stamp, text in stamps.values():
        with open(stamp, "w") as f:
            f.write(text)
    run([hipcc, "-shared", "--offload-arch=gfx950", *objs, "-o", lib_path])
    return lib_path


# every exported symbol of include/cnhip.h: name -> (restype, argtypes)
_H = C.c_uint64
_CTX = C.c_void_p
_u32 = C.c_uint32
SIGNATURES = {
    "cn_version": (C.c_int, []),
    "cn_last_error": (C.c_char_p, []),
    "cn_device_count": (C.c_int, []),
    "cn_ctx_create": (C.c_int, [_u32, U64P, _u32, C.c_uint64, C.c_int, C.c_int, C.c_int, C.POINTER(_CTX)]),
    "cn_ctx_destroy": (C.c_int, [_CTX]),
    "cn_sync": (C.c_int, [_CTX]),
    "cn_ctx_wait_for": (C.c_int, [_CTX, _CTX]),
    "cn_ctx_create_level": (C.c_int, [_CTX, _u32, C.POINTER(_CTX)]),
    "cn_mod_switch": (C.c_int, [_CTX, _H, _u32, _u32, _CTX, _H, _u32]),
    "cn_set_option": (C.c_int, [_CTX, C.c_char_p, C.c_int]),
    "cn_get_option": (C.c_int, [_CTX, C.c_char_p, C.POINTER(C.c_int)]),
    "cn_default_coeff_modulus": (C.c_int, [_u32, U64P]),
    "cn_key_words": (C.c_size_t, [_CTX, C.c_int]),
    "cn_set_relin_key": (C.c_int, [_CTX, C.c_void_p, C.c_size_t, C.c_int]),
    "cn_set_galois_key": (C.c_int, [_CTX, C.c_uint64, C.c_void_p, C.c_size_t, C.c_int]),
    "cn_ctx_broadcast_keys": (C.c_int, [C.POINTER(_CTX), C.c_int]),
    "cn_has_galois_key": (C.c_int, [_CTX, C.c_uint64]),
    "cn_load_key": (C.c_int, [_CTX, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t, C.c_int, C.c_int]),
    "cn_galois_elt_from_step": (C.c_uint64, [_CTX, C.c_int]),
    "cn_ct_alloc": (C.c_int, [_CTX, _u32, _u32, C.POINTER(_H)]),
    "cn_pt_alloc": (C.c_int, [_CTX, _u32, C.POINTER(_H)]),
    "cn_free": (C.c_int, [_CTX, _H]),
    "cn_free_many": (C.c_int, [_CTX, C.POINTER(_H), _u32]),
    "cn_encrypt_zero_new": (C.c_int, [_CTX, C.c_uint64, C.POINTER(_H)]),
    "cn_ct_upload": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_ct_download": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_pt_upload": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_pt_download": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_encode": (C.c_int, [_CTX, U64P, _u32, _H, _u32]),
    "cn_decode": (C.c_int, [_CTX, _H, _u32, U64P]),
    "cn_encode_batch": (C.c_int, [_CTX, U64P, _u32, _u32, _H, _u32]),
    "cn_decode_batch": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_copy": (C.c_int, [_CTX, _H, _u32, _H, _u32, _u32]),
    "cn_copy_many": (C.c_int, [_CTX, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), _u32, _H, _u32]),
    "cn_device_ptr": (C.c_int, [_CTX, _H, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "cn_live_handles": (C.c_int, [_CTX]),
    "cn_add": (C.c_int, [_CTX, _H, _u32, _H, _u32, _H, _u32, _u32]),
    "cn_sub": (C.c_int, [_CTX, _H, _u32, _H, _u32, _H, _u32, _u32]),
    "cn_negate": (C.c_int, [_CTX, _H, _u32, _H, _u32, _u32]),
    "cn_add_many": (C.c_int, [_CTX, _H, U32P, _u32, _H, _u32]),
    "cn_add_plain": (C.c_int, [_CTX, _H, _u32, _H, _u32, C.c_int, _H, _u32, _u32]),
    "cn_mul_plain": (C.c_int, [_CTX, _H, _u32, _H, _u32, _u32, _H, _u32, _u32]),
    "cn_mul_scalar": (C.c_int, [_CTX, _H, _u32, U64P, _u32, _H, _u32, _u32]),
    "cn_scalar_gemm": (C.c_int, [_CTX, _H, I32P, U64P, _u32, _u32, _H, I32P, _H, _u32]),
    "cn_scalar_dot": (C.c_int, [_CTX, C.POINTER(_H), U32P, U64P, _u32, _H, _u32]),
    "cn_gemm_plan_create": (C.c_int, [_CTX, I32P, U64P, _u32, _u32, _H, I32P, C.POINTER(_H)]),
    "cn_gemm_plan_apply": (C.c_int, [_CTX, _H, _H, _H, _u32]),
    "cn_graph_begin": (C.c_int, [_CTX]),
    "cn_graph_end": (C.c_int, [_CTX, C.POINTER(_H)]),
    "cn_graph_launch": (C.c_int, [_CTX, _H]),
    "cn_graph_begin_levels": (C.c_int, [_CTX, C.POINTER(_CTX), _u32]),
    "cn_multiply": (C.c_int, [_CTX, _H, _u32, _H, _u32, _H, _u32, _u32]),
    "cn_relinearize": (C.c_int, [_CTX, _H, _u32, _H, _u32, _u32]),
    "cn_mul_relin": (C.c_int, [_CTX, _H, _u32, _u32, _H, _u32, _u32, _H, _u32, _u32]),
    "cn_square_gemm": (C.c_int, [_CTX, _H, _H, _u32, _H, _u32]),
    "cn_mul_relin_sum": (C.c_int, [_CTX, C.POINTER(_H), U32P, C.POINTER(_H), U32P, _u32, _u32, _H, _u32, _u32]),
    "cn_apply_galois": (C.c_int, [_CTX, _H, _u32, C.c_uint64, _H, _u32, _u32]),
    "cn_rotate_rows": (C.c_int, [_CTX, _H, _u32, C.c_int, _H, _u32, _u32]),
    "cn_rotate_rows_many": (C.c_int, [_CTX, _H, C.POINTER(C.c_uint32), C.POINTER(C.c_int), _u32, _H, C.POINTER(C.c_uint32)]),
    "cn_apply_galois_hoisted": (C.c_int, [_CTX, _H, _u32, U64P, _u32, _H, C.POINTER(C.c_uint32)]),
    "cn_rotate_rows_hoisted": (C.c_int, [_CTX, _H, _u32, C.POINTER(C.c_int), _u32, _H, C.POINTER(C.c_uint32)]),
    "cn_apply_galois_sum": (C.c_int, [_CTX, _H, C.POINTER(C.c_uint32), U64P, C.POINTER(C.c_uint32), _u32, _H, _u32]),
    "cn_rotate_rows_sum": (C.c_int, [_CTX, _H, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_uint32), _u32, _H, _u32]),
    "cn_rotate_columns": (C.c_int, [_CTX, _H, _u32, _H, _u32, _u32]),
    "cn_rotate_rows_add": (C.c_int, [_CTX, _H, _u32, C.c_int, _H, _u32, _H, _u32, _u32]),
    "cn_rotate_columns_add": (C.c_int, [_CTX, _H, _u32, _H, _u32, _H, _u32, _u32]),
    "cn_sum_slots": (C.c_int, [_CTX, _H, _u32, _u32, _u32]),
    "cn_rowdot_batch": (C.c_int, [_CTX, _H, _u32, _H, _u32, _u32, _u32, _H, _u32]),
    "cn_mul_plain_sum": (C.c_int, [_CTX, _H, _u32, _H, _u32, U32P, U32P, _u32, _H, _u32]),
    "cn_ptn_alloc": (C.c_int, [_CTX, _u32, C.POINTER(_H)]),
    "cn_pt_transform": (C.c_int, [_CTX, _H, _u32, _u32, _H, _u32]),
    "cn_ptn_upload": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_ptn_download": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_diag_scan": (C.c_int, [_CTX, _H, _u32, _u32, _u32, C.POINTER(C.c_uint8)]),
    "cn_diag_encode": (C.c_int, [_CTX, _H, _u32, _u32, _u32, U32P, _u32, _H, _u32]),
    "cn_set_rng_salt": (C.c_int, [_CTX, C.c_uint64]),
    "cn_set_rng_key": (C.c_int, [_CTX, C.c_char_p]),
    "cn_rng_selftest": (C.c_int, [_CTX, C.c_char_p, C.c_uint64, C.c_uint64, U32P]),
    "cn_keygen": (C.c_int, [_CTX, C.c_uint64, C.c_int]),
    "cn_keygen_galois": (C.c_int, [_CTX, C.c_uint64, U64P, _u32]),
    "cn_galois_elts": (C.c_int, [_CTX, U64P, _u32, U32P]),
    "cn_rotation_steps": (C.c_int, [_CTX, C.POINTER(C.c_int), _u32, U32P, C.POINTER(C.c_int)]),
    "cn_set_public_key": (C.c_int, [_CTX, U64P, C.c_size_t]),
    "cn_set_secret_key": (C.c_int, [_CTX, U64P, C.c_size_t]),
    "cn_get_key": (C.c_int, [_CTX, C.c_int, C.c_uint64, U64P, C.c_size_t]),
    "cn_encrypt": (C.c_int, [_CTX, _H, _u32, _u32, _H, _u32, _u32, C.c_uint64]),
    "cn_encrypt_symmetric": (C.c_int, [_CTX, _H, _u32, _u32, _H, _u32, _u32, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64]),
    "cn_ct_expand": (C.c_int, [_CTX, _H, _u32, _u32, C.c_char_p, C.c_uint64, C.c_uint64]),
    "cn_ct_upload_compact": (C.c_int, [_CTX, _H, _u32, _u32, U64P, C.c_char_p, C.c_uint64, C.c_uint64]),
    "cn_ct_download_compact": (C.c_int, [_CTX, _H, _u32, _u32, U64P]),
    "cn_packed_words": (C.c_size_t, [_CTX, _u32]),
    "cn_ct_download_packed": (C.c_int, [_CTX, _H, _u32, _u32, _u32, U64P]),
    "cn_ct_upload_packed": (C.c_int, [_CTX, _H, _u32, _u32, _u32, U64P, C.c_char_p, C.c_uint64, C.c_uint64]),
    "cn_decrypt": (C.c_int, [_CTX, _H, _u32, _u32, _H, _u32]),
    "cn_noise_poly": (C.c_int, [_CTX, _H, _u32, _u32, C.POINTER(C.c_uint64)]),
    "cn_noise_norm": (C.c_int, [_CTX, _H, _u32, _u32, C.POINTER(C.c_uint64)]),
    "cn_join_words": (C.c_int, [C.POINTER(_CTX), _u32]),
    "cn_decrypt_join": (C.c_int, [C.POINTER(_CTX), _u32, C.POINTER(_H), U32P, _u32, _u32, _u32, C.c_double, C.POINTER(C.c_double), U64P, I32P]),
    "cn_split_encode": (C.c_int, [C.POINTER(_CTX), _u32, C.c_void_p, C.c_int64, C.c_int64, _u32, _u32, _u32, C.c_double, C.POINTER(_H), U32P, C.POINTER(C.c_uint8)]),
    "cn_split_encrypt": (C.c_int, [C.POINTER(_CTX), _u32, C.c_void_p, C.c_int64, C.c_int64, _u32, _u32, _u32, C.c_double, C.POINTER(_H), U32P, U64P]),
    "cn_ntt_forward": (C.c_int, [_CTX, C.c_void_p, _u32, C.c_int]),
    "cn_ntt_inverse": (C.c_int, [_CTX, C.c_void_p, _u32, C.c_int]),
    "cn_ct_ntt": (C.c_int, [_CTX, _H, _u32, _u32, C.c_int]),
    "cn_ntt_time": (C.c_int, [_CTX, C.c_void_p, _u32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "cn_valu_issue_time": (C.c_int, [_CTX, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "cn_stream": (C.c_void_p, [_CTX]),
    "cn_event_time_begin": (C.c_int, [_CTX]),
    "cn_event_time_end": (C.c_int, [_CTX, C.POINTER(C.c_float)]),
    "cn_stats_get": (C.c_int, [_CTX, C.POINTER(CnStats), C.c_int]),
}

_lib = None


def lib():
    """Load libcnhip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "cryptonets_amd: %s is missing - run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(os.environ.get("CNHIP_LIB", LIB_PATH))    # CNHIP_LIB: developer override for A/B kernel builds (tools/)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the ABI and the header diverge
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _p64(a):
    if a.dtype != np.uint64 or not a.flags["C_CONTIGUOUS"]:
        raise ValueError("expected contiguous uint64 array")
    return a.ctypes.data_as(U64P)


def broadcast_keys(contexts):
    """evaluation keys of contexts[0] into the others (cn_ctx_broadcast_keys: RCCL across GPUs, device copies on one GPU)"""
    arr = (_CTX * len(contexts))(*[c._h for c in contexts])
    rc = lib().cn_ctx_broadcast_keys(arr, len(contexts))
    if rc:
        raise CnError(rc, lib().cn_last_error().decode())


def join_words(contexts):
    """64-bit words of one joined integer of these plaintext-prime contexts: ceil((bit_length(prod t_i) + 1) / 64) (cn_join_words)"""
    arr = (_CTX * len(contexts))(*[c._h for c in contexts])
    w = lib().cn_join_words(arr, len(contexts))
    if w <= 0:
        raise CnError(w, lib().cn_last_error().decode())
    return w


class JoinResult:
    """what decrypt_join returns: values [count, nslots] float64, words [count, nslots, W] uint64 (two's complement, little-endian) or None,
    argmax [nslots] int32 or None"""

    def __init__(self, values, words, argmax):
        self.values, self.words, self.argmax = values, words, argmax

    def ints(self):
        """the joined integers as Python ints, [count][nslots]"""
        W = self.words.shape[2]
        out = []
        for row in self.words.reshape(self.words.shape[0], -1).tolist():
            r = []
            for i in range(0, len(row), W):
                x = 0
                for w in range(W - 1, -1, -1):
                    x = (x << 64) | row[i + w]
                r.append(x - (1 << (64 * W)) if x >> (64 * W - 1) else x)
            out.append(r)
        return out


def decrypt_join(contexts, handles, firsts, count, nslots, signed=True, scale=1.0, coeff0=False, words=False, argmax=False, values=True):
    """Decrypt + BatchEncoder.Decode + JoinSplitNumbers of `count` ciphertexts per plaintext prime in one call (cn_decrypt_join): contexts[i] holds
    the ciphertexts handles[i][firsts[i] : firsts[i] + count] of prime t_i (firsts None = 0).  Dense form: the first `nslots` slots of every
    ciphertext; coeff0: coefficient 0 of every plaintext (nslots = 1, the wrapper's sparse format).  Joined value x in [0, M), or centred under
    `signed`; values = float(x) / scale."""
    L = lib()
    P = len(contexts)
    arr = (_CTX * P)(*[c._h for c in contexts])
    hs = (_H * P)(*[int(h) for h in handles])
    fs = None if firsts is None else (_u32 * P)(*[int(f) for f in firsts])
    flags = (1 if signed else 0) | (2 if coeff0 else 0)
    out_v = np.empty((count, nslots), dtype=np.float64) if values else None
    out_w = None
    if words:
        out_w = np.empty((count, nslots, join_words(contexts)), dtype=np.uint64)
    out_a = np.empty(nslots, dtype=np.int32) if argmax else None
    rc = L.cn_decrypt_join(arr, P, hs, fs, count, nslots, flags, float(scale),
                           None if out_v is None else out_v.ctypes.data_as(C.POINTER(C.c_double)),
                           None if out_w is None else out_w.ctypes.data_as(U64P),
                           None if out_a is None else out_a.ctypes.data_as(I32P))
    if rc:
        raise CnError(rc, L.cn_last_error().decode())
    return JoinResult(out_v, out_w, out_a)


def _split_args(contexts, values, handles, firsts, transpose, coeff0):
    """the arguments cn_split_encode and cn_split_encrypt share: values[c, s] (after `transpose`: values[s, c]) is slot s of plaintext c; float64 or int64 with any
    numpy strides that are whole elements - the strides are passed on, no host copy is made"""
    v = values if isinstance(values, np.ndarray) else np.asarray(values)
    if v.dtype not in (np.float64, np.int64):
        v = v.astype(np.float64)
    if v.ndim == 1:
        v = v.reshape(1, -1)
    if transpose:
        v = v.T
    if v.ndim != 2 or v.strides[0] % 8 or v.strides[1] % 8:
        raise ValueError("expected a 2-D float64 / int64 array with element-aligned strides")
    P = len(contexts)
    arr = (_CTX * P)(*[c._h for c in contexts])
    hs = (_H * P)(*[int(h) for h in handles])
    fs = None if firsts is None else (_u32 * P)(*[int(f) for f in firsts])
    flags = (1 if v.dtype == np.int64 else 0) | (2 if coeff0 else 0)
    return v, P, arr, hs, fs, flags


def split_encode(contexts, values, handles, firsts=None, scale=1.0, coeff0=False, transpose=False):
    """SplitBigNumbers + BatchEncoder.Encode of values.shape[0] plaintexts of values.shape[1] slots per plaintext prime in one call (cn_split_encode) into the plaintext
    handles handles[i][firsts[i] : ...] of contexts[i].  float64: rint(x * scale); int64: taken as they are.  coeff0: one value per plaintext, the constant
    polynomial (the wrapper's sparse format).  Returns the zero flags, [P, count] bool."""
    L = lib()
    v, P, arr, hs, fs, flags = _split_args(contexts, values, handles, firsts, transpose, coeff0)
    count, nvalues = v.shape
    zero = np.zeros((P, count), dtype=np.uint8)
    rc = L.cn_split_encode(arr, P, C.c_void_p(v.ctypes.data), v.strides[0] // 8, v.strides[1] // 8, count, nvalues, flags, float(scale), hs, fs,
                           zero.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc:
        raise CnError(rc, L.cn_last_error().decode())
    return zero.astype(bool)


def split_encrypt(contexts, values, handles, firsts, seeds, scale=1.0, coeff0=False, transpose=False):
    """the same split and encoding followed by the public-key encryption of every plaintext under the nonce seeds[i] (cn_split_encrypt) into the size-2 ciphertext
    handles handles[i][firsts[i] : ...] of contexts[i]"""
    L = lib()
    v, P, arr, hs, fs, flags = _split_args(contexts, values, handles, firsts, transpose, coeff0)
    count, nvalues = v.shape
    sd = (C.c_uint64 * P)(*[int(x) & (2 ** 64 - 1) for x in seeds])
    rc = L.cn_split_encrypt(arr, P, C.c_void_p(v.ctypes.data), v.strides[0] // 8, v.strides[1] // 8, count, nvalues, flags, float(scale), hs, fs, sd)
    if rc:
        raise CnError(rc, L.cn_last_error().decode())


def default_coeff_modulus(n):
    buf = (C.c_uint64 * 16)()
    cnt = lib().cn_default_coeff_modulus(n, buf)
    if cnt <= 0:
        raise ValueError("no default coefficient modulus for n=%d" % n)
    return [int(buf[i]) for i in range(cnt)]


class Context:
    """One BFV evaluation context resident on one MI355X (HBM tables, keys, buffers, stream)."""

    def __init__(self, n, t, q=None, dbc=10, gdbc=20, device=0):
        self.L = lib()
        if q is None:
            q = default_coeff_modulus(n)
        self.n, self.t, self.q, self.k = int(n), int(t), [int(x) for x in q], len(q)
        self.dbc, self.gdbc, self.device = dbc, gdbc, device
        qa = (C.c_uint64 * self.k)(*self.q)
        h = _CTX()
        self._h = None
        self._chk(self.L.cn_ctx_create(self.n, qa, self.k, self.t, dbc, gdbc, device, C.byref(h)))
        self._adopt(h, None)

    def _adopt(self, h, parent):
        """the state every context object carries besides its parameters (also the constructor of a level context: Context.level)"""
        self.ctw = 2 * self.k * self.n
        self._ct_size = {}
        self._h = h
        self._parent, self._levels = parent, {}
        self._hoisted_wanted = set()     # note_hoisted_steps: steps a hoisted call asked for while "record_steps" was on and a key was missing

    # ---- modulus switching (SEAL 3.2 ModSwitchToNext / ModSwitchTo; include/cnhip.h: cn_ctx_create_level, cn_mod_switch)
    @property
    def limbs(self):
        """number of coefficient moduli of this context (its level)"""
        return self.k

    @property
    def parent(self):
        """the context this level context was sliced from (None for a context of its own)"""
        return self._parent

    def level(self, limbs):
        """the level context over q[:limbs] (1 <= limbs < k), created once per context and cached: the parent's options and a slice of every
        key the parent holds when it is created.  A level context owns its keys and its stream and outlives its parent (cn_ctx_create_level):
        close() of the parent leaves its levels open - each is released by its own close() (or when it is collected)."""
        limbs = int(limbs)
        if limbs not in self._levels:
            h = _CTX()
            self._chk(self.L.cn_ctx_create_level(self._h, limbs, C.byref(h)))
            c = Context.__new__(Context)
            c.L, c.n, c.t, c.q, c.k = self.L, self.n, self.t, self.q[:limbs], limbs
            c.dbc, c.gdbc, c.device = self.dbc, self.gdbc, self.device
            c._adopt(h, self)
            if self.get_option("record_steps"):                 # a level created while its parent records (networks.rotation_steps) records too, into its own list
                c.set_option("record_steps", 1)
            self._levels[limbs] = c
        return self._levels[limbs]

    def mod_switch(self, src, ii, count, dst, out, oi):
        """out[oi:oi+count] (a handle of `dst`, a context on this one's chain with fewer limbs) = the ciphertexts src[ii:ii+count] of this context
        switched down to dst's level (successive drops of the last prime with rounding); ordered on the device, no host wait"""
        self._chk(self.L.cn_mod_switch(self._h, src, ii, count, dst._h, out, oi))

    def _chk(self, rc):
        if rc:
            raise CnError(rc, self.L.cn_last_error().decode())

    def set_option(self, name, value):
        self._chk(self.L.cn_set_option(self._h, name.encode(), int(value)))
        if name == "record_steps" and not int(value):        # switching the recording off clears it: the library's list and the steps noted here
            self._hoisted_wanted.clear()

    def note_hoisted_steps(self, steps):
        """a hoisted call (rotate_rows_hoisted) was refused for a missing key: while "record_steps" is on, its non-zero steps count as asked for - rotation_steps
        returns them beside the library's list, so that keys for exactly the direct steps can be generated.  Nothing is noted while recording is off."""
        if self.get_option("record_steps"):
            self._hoisted_wanted.update(int(s) for s in steps if int(s))

    def get_option(self, name):
        v = C.c_int()
        self._chk(self.L.cn_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def close(self):
        """release the context.  A member of a live graph recorded across levels (graph_begin(levels=...)) is refused and stays open: free the graph first"""
        if self._h is not None:
            self._chk(self.L.cn_ctx_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- keys
    def key_words(self, galois=False):
        return int(self.L.cn_key_words(self._h, int(galois)))

    def set_relin_key(self, words):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self._chk(self.L.cn_set_relin_key(self._h, w.ctypes.data, w.size, 0))

    def set_relin_key_device(self, dev_ptr, words):
        self._chk(self.L.cn_set_relin_key(self._h, dev_ptr, words, 1))

    def set_galois_key(self, elt, words):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self._chk(self.L.cn_set_galois_key(self._h, elt, w.ctypes.data, w.size, 0))

    def set_galois_key_device(self, elt, dev_ptr, words):
        self._chk(self.L.cn_set_galois_key(self._h, elt, dev_ptr, words, 1))

    def has_galois_key(self, elt):
        return bool(self.L.cn_has_galois_key(self._h, elt))

    def load_key(self, which, words, elt=0, coeff_form=False):
        """cn_load_key: which 0 relin, 1 galois (elt), 2 public, 3 secret; coeff_form: the polynomials are in coefficient form and the
        device transforms them with its own tables"""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self._chk(self.L.cn_load_key(self._h, which, elt, w.ctypes.data, w.size, 0, int(bool(coeff_form))))

    def galois_elt_from_step(self, steps):
        return int(self.L.cn_galois_elt_from_step(self._h, steps))

    # ---- buffers
    def ct_alloc(self, count, size=2):
        h = _H()
        self._chk(self.L.cn_ct_alloc(self._h, count, size, C.byref(h)))
        self._ct_size[h.value] = size
        return h.value

    def pt_alloc(self, count):
        h = _H()
        self._chk(self.L.cn_pt_alloc(self._h, count, C.byref(h)))
        return h.value

    def free(self, h):
        if self._h is None:                                # context closed: its arrays went with it
            return
        self._chk(self.L.cn_free(self._h, h))
        self._ct_size.pop(h, None)

    def free_many(self, handles):
        if self._h is None or not len(handles):
            return
        a = (_H * len(handles))(*[int(h) for h in handles])
        self._chk(self.L.cn_free_many(self._h, a, len(handles)))
        for h in handles:
            self._ct_size.pop(int(h), None)

    def encrypt_zero_new(self, seed=1):
        """a new one-ciphertext array holding a fresh encryption of zero (cn_ct_alloc + cn_encrypt(pt = 0) in one call)"""
        h = _H()
        self._chk(self.L.cn_encrypt_zero_new(self._h, seed, C.byref(h)))
        self._ct_size[h.value] = 2
        return h.value

    def ct_upload(self, h, first, data):
        d = np.ascontiguousarray(data, dtype=np.uint64)
        count = d.shape[0] if d.ndim > 1 else 1
        _, nbytes = self.device_ptr(h)                     # the library reads count * item words from the host pointer: check the row width here
        row = d.size // count if count else 0
        size = self._ct_size.get(h)                        # polynomials per ciphertext of this handle, when it was allocated through this object
        if count == 0 or d.size != count * row or row % (self.k * self.n) or row // (self.k * self.n) not in (2, 3) \
                or (size is not None and row != size * self.k * self.n) or nbytes % (row * 8) or first + count > nbytes // (row * 8):
            raise ValueError("ct_upload: data of shape %s does not fit the ciphertexts of this handle" % (d.shape,))
        self._chk(self.L.cn_ct_upload(self._h, h, first, count, _p64(d)))

    def ct_download(self, h, first, count, size=2):
        out = np.empty((count, size * self.k * self.n), dtype=np.uint64)
        self._chk(self.L.cn_ct_download(self._h, h, first, count, _p64(out)))
        return out

    def pt_upload(self, h, first, data):
        d = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, self.n)
        self._chk(self.L.cn_pt_upload(self._h, h, first, d.shape[0], _p64(d)))

    def pt_download(self, h, first, count):
        out = np.empty((count, self.n), dtype=np.uint64)
        self._chk(self.L.cn_pt_download(self._h, h, first, count, _p64(out)))
        return out

    def ptn_alloc(self, count):
        """an array of `count` NTT-form plaintexts, [count][k][N] words (Evaluator.TransformToNtt): the operand mul_plain, rowdot_batch and mul_plain_sum take
        in place of a coefficient-form handle, k times its size"""
        h = _H()
        self._chk(self.L.cn_ptn_alloc(self._h, count, C.byref(h)))
        return h.value

    def pt_transform(self, pt, pi, count, ptn, oi):
        """ptn[oi + i] = NTT form of pt[pi + i], i < count (cn_pt_transform)"""
        self._chk(self.L.cn_pt_transform(self._h, pt, pi, count, ptn, oi))

    def ptn_upload(self, h, first, data):
        d = np.ascontiguousarray(data, dtype=np.uint64).reshape(-1, self.k * self.n)
        self._chk(self.L.cn_ptn_upload(self._h, h, first, d.shape[0], _p64(d)))

    def ptn_download(self, h, first, count):
        out = np.empty((count, self.k, self.n), dtype=np.uint64)
        self._chk(self.L.cn_ptn_download(self._h, h, first, count, _p64(out)))
        return out

    def diag_scan(self, rows, ri, R, dim):
        """bool [2, N / 2]: does the generalized diagonal (c, i) of the R x dim matrix whose rows are the plaintexts rows[ri .. ri + R) hold a non-zero?  (cn_diag_scan)"""
        out = np.zeros((2, self.n // 2), dtype=np.uint8)
        self._chk(self.L.cn_diag_scan(self._h, rows, ri, R, dim, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.astype(bool)

    def diag_encode(self, rows, ri, R, dim, terms, out, oi):
        """out[oi + e] = the encoded pre-rotated diagonal diagonal.pre_rotated_rows(W, n, [terms[e]]) of that matrix, terms = [(c, J, b)]; out: a pt_alloc or a
        ptn_alloc array (cn_diag_encode)"""
        t = np.ascontiguousarray(terms, dtype=np.uint32).reshape(-1, 3)
        self._chk(self.L.cn_diag_encode(self._h, rows, ri, R, dim, t.ctypes.data_as(U32P), t.shape[0], out, oi))

    def encode(self, values, pt, pi):
        v = np.ascontiguousarray(values, dtype=np.uint64)
        self._chk(self.L.cn_encode(self._h, _p64(v), v.size, pt, pi))

    def decode(self, pt, pi):
        out = np.empty(self.n, dtype=np.uint64)
        self._chk(self.L.cn_decode(self._h, pt, pi, _p64(out)))
        return out

    def encode_batch(self, values, pt, pi):
        """BatchEncoder.Encode of values[count, nvalues] into pt[pi .. pi + count) with one library call"""
        v = np.ascontiguousarray(values, dtype=np.uint64)
        if v.ndim != 2:
            raise ValueError("encode_batch expects a [count, nvalues] array")
        self._chk(self.L.cn_encode_batch(self._h, _p64(v), v.shape[1], v.shape[0], pt, pi))

    def decode_batch(self, pt, pi, count):
        """slot values [count, N] of pt[pi .. pi + count)"""
        out = np.empty((count, self.n), dtype=np.uint64)
        self._chk(self.L.cn_decode_batch(self._h, pt, pi, count, _p64(out)))
        return out

    def copy(self, src, sfirst, dst, dfirst, count):
        self._chk(self.L.cn_copy(self._h, src, sfirst, dst, dfirst, count))

    def copy_many(self, srcs, sfirsts, dst, dfirst):
        """dst[dfirst + i] = srcs[i][sfirsts[i]]: single ciphertexts (or plaintexts) of many arrays into one array with one launch"""
        hs = np.ascontiguousarray(srcs, dtype=np.uint64)
        fs = np.ascontiguousarray(sfirsts, dtype=np.uint32)
        self._chk(self.L.cn_copy_many(self._h, hs.ctypes.data_as(C.POINTER(C.c_uint64)), fs.ctypes.data_as(C.POINTER(C.c_uint32)), len(hs), dst, dfirst))

    def device_ptr(self, h):
        p, b = C.c_void_p(), C.c_size_t()
        self._chk(self.L.cn_device_ptr(self._h, h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def live_handles(self):
        return self.L.cn_live_handles(self._h)

    def sync(self):
        self._chk(self.L.cn_sync(self._h))

    def wait_for(self, other):
        """work submitted to this context from now on starts after everything submitted to `other` so far (device-side ordering)"""
        self._chk(self.L.cn_ctx_wait_for(self._h, other._h))

    # ---- evaluator
    def add(self, a, ai, b, bi, out, oi, count=1):
        self._chk(self.L.cn_add(self._h, a, ai, b, bi, out, oi, count))

    def sub(self, a, ai, b, bi, out, oi, count=1):
        self._chk(self.L.cn_sub(self._h, a, ai, b, bi, out, oi, count))

    def negate(self, a, ai, out, oi, count=1):
        self._chk(self.L.cn_negate(self._h, a, ai, out, oi, count))

    def add_many(self, src, idx, out, oi):
        ia = np.ascontiguousarray(idx, dtype=np.uint32)
        self._chk(self.L.cn_add_many(self._h, src, ia.ctypes.data_as(U32P), ia.size, out, oi))

    def add_plain(self, a, ai, pt, pi, out, oi, count=1, subtract=False):
        self._chk(self.L.cn_add_plain(self._h, a, ai, pt, pi, int(subtract), out, oi, count))

    def mul_plain(self, a, ai, pt, pi, out, oi, count=1, pt_stride=1):
        self._chk(self.L.cn_mul_plain(self._h, a, ai, pt, pi, pt_stride, out, oi, count))

    def mul_scalar(self, a, ai, scalars, out, oi, count=1, broadcast=False):
        s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1)
        self._chk(self.L.cn_mul_scalar(self._h, a, ai, _p64(s), 0 if broadcast else 1, out, oi, count))

    def scalar_gemm(self, src, W, out, oi, idx=None, bias_pt=0, bias_idx=None):
        W = np.ascontiguousarray(W, dtype=np.uint64)
        O, K = W.shape
        ip = None
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            if idx.shape != (O, K):
                raise ValueError("gather table must have the shape of the weight matrix")
            ip = idx.ctypes.data_as(I32P)
        bp = None
        if bias_pt:
            bias_idx = np.ascontiguousarray(bias_idx, dtype=np.int32)
            if bias_idx.shape != (O,):
                raise ValueError("one bias index per output expected")
            bp = bias_idx.ctypes.data_as(I32P)
        self._chk(self.L.cn_scalar_gemm(self._h, src, ip, _p64(W), O, K, bias_pt, bp, out, oi))

    def scalar_dot(self, handles, indices, weights, out, oi):
        """out[oi] = sum_k weights[k] * handles[k][indices[k]]: one output of DenseMatrixBySparseVectorMultiply whose input ciphertexts
        are separate arrays (handle 0 = padded tap)"""
        hs = np.ascontiguousarray(handles, dtype=np.uint64)
        ix = np.ascontiguousarray(indices, dtype=np.uint32)
        w = np.ascontiguousarray(weights, dtype=np.uint64)
        if not (hs.shape == ix.shape == w.shape) or hs.ndim != 1:
            raise ValueError("scalar_dot: handles, indices and weights must be 1-d arrays of one length")
        self._chk(self.L.cn_scalar_dot(self._h, hs.ctypes.data_as(C.POINTER(_H)), ix.ctypes.data_as(U32P), _p64(w), hs.size, out, oi))

    def gemm_plan(self, W, idx=None, bias_pt=0, bias_idx=None):
        """plan a scalar GEMM once (weights and gather tables stay in HBM); returns a handle for gemm_apply / free"""
        W = np.ascontiguousarray(W, dtype=np.uint64)
        O, K = W.shape
        ip = None
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            if idx.shape != (O, K):
                raise ValueError("gather table must have the shape of the weight matrix")
            ip = idx.ctypes.data_as(I32P)
        bp = None
        if bias_pt:
            bias_idx = np.ascontiguousarray(bias_idx, dtype=np.int32)
            if bias_idx.shape != (O,):
                raise ValueError("one bias index per output expected")
            bp = bias_idx.ctypes.data_as(I32P)
        h = _H()
        self._chk(self.L.cn_gemm_plan_create(self._h, ip, _p64(W), O, K, bias_pt, bp, C.byref(h)))
        return h.value

    def gemm_apply(self, plan, src, out, oi):
        self._chk(self.L.cn_gemm_plan_apply(self._h, plan, src, out, oi))

    def multiply(self, a, ai, b, bi, out3, oi, count=1):
        self._chk(self.L.cn_multiply(self._h, a, ai, b, bi, out3, oi, count))

    def relinearize(self, in3, ii, out, oi, count=1):
        self._chk(self.L.cn_relinearize(self._h, in3, ii, out, oi, count))

    def mul_relin(self, a, ai, b, bi, out, oi, count=1, a_stride=1, b_stride=1):
        self._chk(self.L.cn_mul_relin(self._h, a, ai, a_stride, b, bi, b_stride, out, oi, count))

    def square_gemm(self, plan, src, ii, out, oi):
        """SquareActivation of the plan's inputs src[ii..] + the planned PoolLayer behind it: the words of mul_relin followed by gemm_apply"""
        self._chk(self.L.cn_square_gemm(self._h, plan, src, ii, out, oi))

    def mul_relin_sum(self, a_handles, a_idx, b_handles, b_idx, b_stride, out, oi, count=1):
        """out[oi + i] = sum_k Relinearize(Multiply(a_handles[k][a_idx[k] + i], b_handles[k][b_idx[k] + i * b_stride])), i < count: the words of mul_relin per
        term followed by add_many, with one key switch per output where the context allows it (a_idx / b_idx None = all zero)"""
        ha = np.ascontiguousarray(a_handles, dtype=np.uint64)
        hb = np.ascontiguousarray(b_handles, dtype=np.uint64)
        if ha.ndim != 1 or ha.shape != hb.shape:
            raise ValueError("mul_relin_sum: one handle per term on either side")
        ia = ib = None
        if a_idx is not None:
            ia = np.ascontiguousarray(a_idx, dtype=np.uint32)
            if ia.shape != ha.shape:
                raise ValueError("mul_relin_sum: one index per term expected")
        if b_idx is not None:
            ib = np.ascontiguousarray(b_idx, dtype=np.uint32)
            if ib.shape != hb.shape:
                raise ValueError("mul_relin_sum: one index per term expected")
        self._chk(self.L.cn_mul_relin_sum(self._h, ha.ctypes.data_as(C.POINTER(_H)), ia.ctypes.data_as(U32P) if ia is not None else None,
                                          hb.ctypes.data_as(C.POINTER(_H)), ib.ctypes.data_as(U32P) if ib is not None else None, ha.size, b_stride, out, oi, count))

    def apply_galois(self, src, ii, elt, out, oi, count=1):
        self._chk(self.L.cn_apply_galois(self._h, src, ii, elt, out, oi, count))

    def rotate_rows(self, src, ii, steps, out, oi, count=1):
        self._chk(self.L.cn_rotate_rows(self._h, src, ii, steps, out, oi, count))

    def rotate_rows_many(self, src, iis, steps, out, ois):
        """out[ois[i]] = RotateRows(src[iis[i]], steps[i]): n rotations by n different step counts as one launch chain"""
        a = np.ascontiguousarray(iis, dtype=np.uint32)
        st = np.ascontiguousarray(steps, dtype=np.int32)
        o = np.ascontiguousarray(ois, dtype=np.uint32)
        self._chk(self.L.cn_rotate_rows_many(self._h, src, a.ctypes.data_as(C.POINTER(C.c_uint32)), st.ctypes.data_as(C.POINTER(C.c_int)), len(a), out,
                                             o.ctypes.data_as(C.POINTER(C.c_uint32))))

    def rotate_rows_hoisted(self, src, ii, steps, out, ois):
        """out[ois[r]] = the hoisted rotation of src[ii] by steps[r] (0: a copy): n rotations of ONE ciphertext on one set of digit transforms, every step
        with its own Galois key (CN_ERR_NOKEY otherwise).  The words are those of tests/hoisted_model.py, not cn_rotate_rows'; the plaintext is the same"""
        st = np.ascontiguousarray(steps, dtype=np.int32)
        o = np.ascontiguousarray(ois, dtype=np.uint32)
        assert len(st) == len(o)
        self._chk(self.L.cn_rotate_rows_hoisted(self._h, src, ii, st.ctypes.data_as(C.POINTER(C.c_int)), len(st), out, o.ctypes.data_as(C.POINTER(C.c_uint32))))

    def apply_galois_hoisted(self, src, ii, elts, out, ois):
        """the same by Galois elements (1: a copy)"""
        e = np.ascontiguousarray(elts, dtype=np.uint64)
        o = np.ascontiguousarray(ois, dtype=np.uint32)
        assert len(e) == len(o)
        self._chk(self.L.cn_apply_galois_hoisted(self._h, src, ii, e.ctypes.data_as(U64P), len(e), out, o.ctypes.data_as(C.POINTER(C.c_uint32))))

    def rotate_rows_sum(self, src, iis, steps, grp_off, out, oi):
        """out[oi + g] = the sum over e in [grp_off[g], grp_off[g + 1]) of RotateRows(src[iis[e]], steps[e]) (step 0: a plain addend): rotations of DIFFERENT
        ciphertexts under one inverse transform per output limb.  The words of rotate_rows per term followed by add_many; a step without its own key runs its
        non-adjacent-form hops"""
        i = np.ascontiguousarray(iis, dtype=np.uint32)
        st = np.ascontiguousarray(steps, dtype=np.int32)
        g = np.ascontiguousarray(grp_off, dtype=np.uint32)
        assert len(st) == len(i) and (len(g) < 2 or int(g[-1]) == len(i))
        self._chk(self.L.cn_rotate_rows_sum(self._h, src, i.ctypes.data_as(C.POINTER(C.c_uint32)), st.ctypes.data_as(C.POINTER(C.c_int)),
                                            g.ctypes.data_as(C.POINTER(C.c_uint32)), max(len(g), 1) - 1, out, oi))

    def apply_galois_sum(self, src, iis, elts, grp_off, out, oi):
        """the same by Galois elements (1: a plain addend), every element with its own key"""
        i = np.ascontiguousarray(iis, dtype=np.uint32)
        e = np.ascontiguousarray(elts, dtype=np.uint64)
        g = np.ascontiguousarray(grp_off, dtype=np.uint32)
        assert len(e) == len(i) and (len(g) < 2 or int(g[-1]) == len(i))
        self._chk(self.L.cn_apply_galois_sum(self._h, src, i.ctypes.data_as(C.POINTER(C.c_uint32)), e.ctypes.data_as(U64P), g.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             max(len(g), 1) - 1, out, oi))

    def rotate_rows_add(self, src, ii, steps, acc, ai, out, oi, count=1):
        """out = acc + RotateRows(src, steps) (fused rotate-and-add of SumAllSlots)"""
        self._chk(self.L.cn_rotate_rows_add(self._h, src, ii, steps, acc, ai, out, oi, count))

    def sum_slots(self, h, first, count, length=0):
        """in-place SumAllSlots(length) of `count` single-block ciphertexts (length 0 = every slot)"""
        self._chk(self.L.cn_sum_slots(self._h, h, first, count, length))

    def rowdot_batch(self, v, vi, pt, pi, rows, length, out, oi):
        """out[oi + r] = SumAllSlots(v[vi] * pt[pi + r], length) for r < rows"""
        self._chk(self.L.cn_rowdot_batch(self._h, v, vi, pt, pi, rows, length, out, oi))

    def mul_plain_sum(self, ct, ci, pt, pi, grp_off, ct_idx, out, oi):
        """out[oi + g] = sum_{e in [grp_off[g], grp_off[g + 1])} MultiplyPlain(ct[ci + ct_idx[e]], pt[pi + e]) for g < len(grp_off) - 1: the words of mul_plain per
        term followed by add_many, in one kernel on the register-radix sizes (cn_mul_plain_sum)"""
        go = np.ascontiguousarray(grp_off, dtype=np.uint32).reshape(-1)
        ix = np.ascontiguousarray(ct_idx, dtype=np.uint32).reshape(-1)
        if go.size < 1 or int(go[-1]) != ix.size:
            raise ValueError("mul_plain_sum: grp_off has one entry per group plus one and ends at len(ct_idx)")
        self._chk(self.L.cn_mul_plain_sum(self._h, ct, ci, pt, pi, go.ctypes.data_as(U32P), ix.ctypes.data_as(U32P), go.size - 1, out, oi))

    def rotate_columns_add(self, src, ii, acc, ai, out, oi, count=1):
        self._chk(self.L.cn_rotate_columns_add(self._h, src, ii, acc, ai, out, oi, count))

    def rotate_columns(self, src, ii, out, oi, count=1):
        self._chk(self.L.cn_rotate_columns(self._h, src, ii, out, oi, count))

    # ---- client side on the device
    def set_rng_salt(self, salt):
        self._chk(self.L.cn_set_rng_salt(self._h, salt))

    def set_rng_key(self, key32):
        """256-bit ChaCha20 key of the context's sampler (bytes of length 32)"""
        key32 = bytes(key32)
        if len(key32) != 32:
            raise ValueError("the sampler key has 32 bytes")
        self._chk(self.L.cn_set_rng_key(self._h, key32))

    def rng_block(self, key32, counter, nonce):
        """one raw block (16 words) of the device sampler's generator (known-answer tests)"""
        out = np.zeros(16, dtype=np.uint32)
        self._chk(self.L.cn_rng_selftest(self._h, bytes(key32), counter, nonce, out.ctypes.data_as(U32P)))
        return out

    def keygen(self, seed, galois=True):
        self._chk(self.L.cn_keygen(self._h, seed, int(galois)))

    def keygen_galois(self, seed, elts):
        """cn_keygen_galois: Galois keys for exactly the listed elements, generated by one kernel launch (needs the secret key of a keygen(...) before it)"""
        e = np.ascontiguousarray(list(elts), dtype=np.uint64)
        self._chk(self.L.cn_keygen_galois(self._h, seed, _p64(e), e.size))

    def galois_elts(self):
        """the Galois elements this context holds a key for, ascending (cn_galois_elts)"""
        cnt = C.c_uint32()
        self._chk(self.L.cn_galois_elts(self._h, None, 0, C.byref(cnt)))
        out = np.zeros(max(1, cnt.value), dtype=np.uint64)
        self._chk(self.L.cn_galois_elts(self._h, _p64(out), out.size, C.byref(cnt)))
        return [int(x) for x in out[:cnt.value]]

    def rotation_steps(self):
        """(sorted distinct RotateRows steps, was a column rotation asked for) recorded since set_option("record_steps", 1) (cn_rotation_steps), with the steps of
        note_hoisted_steps among them"""
        cnt, cols = C.c_uint32(), C.c_int()
        self._chk(self.L.cn_rotation_steps(self._h, None, 0, C.byref(cnt), C.byref(cols)))
        out = (C.c_int * max(1, cnt.value))()
        self._chk(self.L.cn_rotation_steps(self._h, out, len(out), C.byref(cnt), C.byref(cols)))
        return sorted({int(out[i]) for i in range(cnt.value)} | self._hoisted_wanted), bool(cols.value)

    def set_public_key(self, words):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self._chk(self.L.cn_set_public_key(self._h, _p64(w), w.size))

    def set_secret_key(self, words):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        self._chk(self.L.cn_set_secret_key(self._h, _p64(w), w.size))

    def get_key(self, which, elt=0):
        words = {0: self.key_words(False), 1: self.key_words(True), 2: self.ctw, 3: self.ctw // 2}[which]
        out = np.empty(words, dtype=np.uint64)
        self._chk(self.L.cn_get_key(self._h, which, elt, _p64(out), words))
        return out

    def encrypt(self, pt, pi, out, oi, count=1, seed=1, pt_stride=1):
        self._chk(self.L.cn_encrypt(self._h, pt, pi, pt_stride, out, oi, count, seed))

    # ---- seeded symmetric ciphertexts (include/cnhip.h): c1 = INTT(a), a regenerated from 32 public bytes
    @staticmethod
    def _seed32(a_seed):
        a_seed = bytes(a_seed)
        if len(a_seed) != 32:
            raise ValueError("the public seed has 32 bytes")
        return a_seed

    def encrypt_symmetric(self, pt, pi, out, oi, count=1, *, a_seed, seed=1, a_nonce=0, a_item0=0, pt_stride=1):
        """secret-key encryptions whose c1 is the expansion of (a_seed, a_nonce, a_item0 + i); `seed` is the nonce of the noise draw under the
        context's own sampler key.  a_seed has no default: two ciphertexts under one (a_seed, a_nonce, item) share their a, and their difference
        then shows the difference of the messages"""
        self._chk(self.L.cn_encrypt_symmetric(self._h, pt, pi, pt_stride, out, oi, count, seed, self._seed32(a_seed), a_nonce, a_item0))

    def ct_expand(self, h, first, count, a_seed, a_nonce=0, a_item0=0):
        """poly 1 of h[first : first + count] from the public seed (needs no key)"""
        self._chk(self.L.cn_ct_expand(self._h, h, first, count, self._seed32(a_seed), a_nonce, a_item0))

    def ct_upload_compact(self, h, first, c0, a_seed, a_nonce=0, a_item0=0):
        """c0 words [count, k * n] into poly 0 of h[first ..) (one strided copy), poly 1 expanded from the seed on the device"""
        d = np.ascontiguousarray(c0, dtype=np.uint64)
        count = d.shape[0] if d.ndim > 1 else 1
        _, nbytes = self.device_ptr(h)                     # the library reads count * k * n words from the host pointer: check the row width here
        size = self._ct_size.get(h)
        if count == 0 or d.size != count * self.k * self.n or (size is not None and size != 2) or nbytes % (self.ctw * 8) or first + count > nbytes // (self.ctw * 8):
            raise ValueError("ct_upload_compact: data of shape %s is not [count, %d] c0 words for the size-2 ciphertexts of this handle" % (d.shape, self.k * self.n))
        self._chk(self.L.cn_ct_upload_compact(self._h, h, first, count, _p64(d), self._seed32(a_seed), a_nonce, a_item0))

    def ct_download_compact(self, h, first, count):
        """the c0 words [count, k * n] of h[first : first + count]"""
        out = np.empty((count, self.k * self.n), dtype=np.uint64)
        self._chk(self.L.cn_ct_download_compact(self._h, h, first, count, _p64(out)))
        return out

    # ---- packed rows (include/cnhip.h): residues in bit_length(q_j) bits each
    def packed_words(self, polys=1):
        """words of one packed ciphertext of `polys` polynomials: polys * (n / 64) * sum of the moduli's bit lengths"""
        return int(self.L.cn_packed_words(self._h, polys))

    def ct_download_packed(self, h, first, count, polys=1, size=None):
        """packed rows [count, words] of h[first : first + count]: poly 0 alone (polys = 1) or every polynomial of the handle (polys = 0; `size`: its
        polynomials per ciphertext when the handle was not allocated through this object)"""
        if polys not in (0, 1):
            raise ValueError("polys: 0 (every polynomial of the handle) or 1 (c0 only)")
        size = 1 if polys else (size or self._ct_size.get(h))
        if size is None:
            raise ValueError("ct_download_packed(polys=0): pass `size`, the handle was not allocated through this object")
        out = np.empty((count, self.packed_words(size)), dtype=np.uint64)
        self._chk(self.L.cn_ct_download_packed(self._h, h, first, count, polys, _p64(out)))
        return out

    def ct_upload_packed(self, h, first, packed, polys=1, a_seed=None, a_nonce=0, a_item0=0, size=None):
        """packed rows [count, words] into h[first ..): polys = 1 - c0 rows, poly 1 expanded from the seed (ct_upload_compact's arguments); polys = 0 - every
        polynomial of the handle, no seed; `size`: its polynomials per ciphertext when the handle was not allocated through this object.  Raises CnError (CN_ERR_ARG) when a row held a residue that is not below its modulus"""
        if polys not in (0, 1):
            raise ValueError("polys: 0 (every polynomial of the handle) or 1 (c0 only)")
        d = np.ascontiguousarray(packed, dtype=np.uint64)
        count = d.shape[0] if d.ndim > 1 else 1
        size = self._ct_size.get(h) or size
        _, nbytes = self.device_ptr(h)                     # the library reads count * packed words from the host pointer: check the row width here
        if size is None or (polys == 1 and size != 2) or count == 0 or d.size != count * self.packed_words(1 if polys else size) \
                or first + count > nbytes // (size * self.k * self.n * 8):
            raise ValueError("ct_upload_packed: data of shape %s does not fit the ciphertexts of this handle" % (d.shape,))
        seed = self._seed32(a_seed) if polys == 1 else None
        self._chk(self.L.cn_ct_upload_packed(self._h, h, first, count, polys, _p64(d), seed, a_nonce, a_item0))

    def decrypt(self, ct, ci, count, pt_out, pi):
        self._chk(self.L.cn_decrypt(self._h, ct, ci, count, pt_out, pi))

    def noise_poly(self, ct, ci=0, count=1):
        """residues of t*(c0 + c1 s + c2 s^2) mod q_j, uint64 [count, k, n] (needs the secret key)"""
        out = np.empty((count, self.k, self.n), dtype=np.uint64)
        self._chk(self.L.cn_noise_poly(self._h, ct, ci, count, _p64(out)))
        return out

    def noise_norm(self, ct, ci=0, count=1):
        """exact centred infinity norms || t*(c0 + c1 s + c2 s^2) mod q ||_inf of `count` ciphertexts, as Python ints (cn_noise_norm: composed
        and reduced on the device, k words per ciphertext; needs the secret key)"""
        out = np.zeros((max(count, 1), self.k), dtype=np.uint64)
        self._chk(self.L.cn_noise_norm(self._h, ct, ci, count, _p64(out)))
        return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in out[:count]]

    def invariant_noise_budget(self, ct, ci=0, count=1, exact_bits=False):
        """Decryptor.InvariantNoiseBudget (what CryptoTracker.TestBudget reads, CryptoTracker.cs:41-52) of `count` ciphertexts:
        log2(q) - log2(|| t (c0 + c1 s + c2 s^2) mod q ||_inf, centred) - 1, in bits (float); with `exact_bits` SEAL's integer
        max(0, bitcount(q) - bitcount(norm) - 1).  Both from the exact norm of noise_norm."""
        import math
        Q = 1
        for qj in self.q:
            Q *= qj
        out = []
        for norm in self.noise_norm(ct, ci, count):
            if exact_bits:
                out.append(max(0, Q.bit_length() - norm.bit_length() - 1))
            else:
                out.append(math.log2(Q) - (math.log2(norm) if norm else 0.0) - 1.0)
        return out

    # ---- raw transforms / timing / stats
    def ct_ntt(self, h, first, count, inverse=False):
        self._chk(self.L.cn_ct_ntt(self._h, h, first, count, int(inverse)))

    def ntt_forward(self, dev_ptr, limbs, base=0):
        self._chk(self.L.cn_ntt_forward(self._h, dev_ptr, limbs, base))

    def ntt_inverse(self, dev_ptr, limbs, base=0):
        self._chk(self.L.cn_ntt_inverse(self._h, dev_ptr, limbs, base))

    def ntt_time(self, dev_ptr, limbs, base=0, inverse=False, iters=10):
        ms = C.c_float()
        self._chk(self.L.cn_ntt_time(self._h, dev_ptr, limbs, base, int(inverse), iters, C.byref(ms)))
        return ms.value

    def fp64_issue_ns(self, iters=2048, launches=4):
        """ns per FP64 wave-instruction per SIMD right now (cn_valu_issue_time, kind 0)"""
        ns = C.c_float()
        self._chk(self.L.cn_valu_issue_time(self._h, 0, iters, launches, C.byref(ns)))
        return ns.value

    def valu32_issue_ns(self, iters=8192, launches=4):
        """ns per full-rate 32-bit VALU wave-instruction per SIMD right now (cn_valu_issue_time, kind 1)"""
        ns = C.c_float()
        self._chk(self.L.cn_valu_issue_time(self._h, 1, iters, launches, C.byref(ns)))
        return ns.value

    def stream(self):
        return self.L.cn_stream(self._h)

    # ---- captured sequences (HIP graphs): see include/cnhip.h
    def graph_begin(self, levels=()):
        """start recording; `levels`: level contexts of this context's chain the recording also covers (cn_graph_begin_levels) - their calls
        and the cn_mod_switch calls between them and this context are recorded into the one graph graph_end returns"""
        levels = list(levels)
        if not levels:
            self._chk(self.L.cn_graph_begin(self._h))
            return
        arr = (_CTX * len(levels))(*[c._h for c in levels])
        self._chk(self.L.cn_graph_begin_levels(self._h, arr, len(levels)))

    def graph_end(self):
        h = _H()
        self._chk(self.L.cn_graph_end(self._h, C.byref(h)))
        return h.value

    def graph_launch(self, graph):
        self._chk(self.L.cn_graph_launch(self._h, graph))

    def time_begin(self):
        self._chk(self.L.cn_event_time_begin(self._h))

    def time_end(self):
        ms = C.c_float()
        self._chk(self.L.cn_event_time_end(self._h, C.byref(ms)))
        return ms.value

    def stats(self, reset=False):
        s = CnStats()
        self._chk(self.L.cn_stats_get(self._h, C.byref(s), int(reset)))
        return {n: int(getattr(s, n)) for n, _ in CnStats._fields_}

