#!/usr/bin/env python
"""FP64 instruction counts of the fused key-switch kernel, read from the BUILT code object (not from constants in a script).

`llvm-objdump --offloading` extracts the gfx950 code object from the key-switch translation unit's object file, `llvm-objdump -d`
disassembles it; the kernel's loops are recovered from its backward branches (limb loop > digit loop; the loop over the two inverse
transforms) and every `v_*_f64` instruction is weighted with the trip counts of the loops that contain it.  `fp64_per_thread(k, digits
per limb)` is what bench.py prices against the FP64 issue rate (one wave-instruction per ~4.4 cycles per SIMD,
profiles/r01_ubench_mulmod.txt) to get the key switch's arithmetic floor.

    python tools/ks_isa_counts.py            # prints the structure found in k_keyswitch_rr<13, ArF64T<0>, 1, true, false>
"""
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
KERNEL = "_Z14k_keyswitch_rrILi13E6ArF64TILi0EELi1ELb1ELb0EE"          # k_keyswitch_rr<13, ArF64T<0>, 1, true, false>


def disassemble(obj, kernel=KERNEL):
    """[(address, mnemonic, operands)] of `kernel` in the device code object bundled in `obj`"""
    with tempfile.TemporaryDirectory() as td:
        tmp = os.path.join(td, os.path.basename(obj))
        os.symlink(obj, tmp)
        subprocess.check_call([OBJDUMP, "--offloading", tmp], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in glob.glob(tmp + ".*") if "amdgcn" in f]
        if not co:
            raise RuntimeError("no gfx950 code object in %s" % obj)
        txt = subprocess.check_output([OBJDUMP, "-d", co[0]], text=True)
    ins, on = [], False
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            on = m.group(1).startswith(kernel)
            continue
        if not on:
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), m.group(2)))
    if not ins:
        raise RuntimeError("kernel %s not found" % kernel)
    return ins


def loops(ins):
    """{header address: [addresses of its back edges]}: backward branches, minus the compiler's out-of-line trampolines (an s_branch that
    directly follows another s_branch is the landing pad of a forward conditional branch jumping back into the body, not a loop)"""
    out = {}
    end = min([a for a, op, _ in ins if op == "s_endpgm"] or [ins[-1][0]])      # blocks the compiler places behind the kernel's end jump back into it: no loops
    for k, (addr, op, args) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            m = re.search(r"(-?\d+)", args)
            if not m or addr > end or (op == "s_branch" and k and ins[k - 1][1] == "s_branch"):
                continue
            nxt = ins[k + 1][0] if k + 1 < len(ins) else addr + 4
            off = int(m.group(1))
            off = off - 65536 if off >= 32768 else off         # simm16, in dwords from the next instruction
            tgt = nxt + 4 * off
            if tgt <= addr:
                out.setdefault(tgt, []).append(addr)
    return out


def structure(obj=None, kernel=KERNEL):
    obj = obj or os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_ks_f64l.o")
    ins = disassemble(obj, kernel)
    f64 = [a for a, op, _ in ins if op.startswith("v_") and "_f64" in op]
    other = [a for a, op, _ in ins if op.startswith("v_") and "_f64" not in op and not op.startswith("v_readfirstlane")]   # the rest of the VALU stream
    within = lambda lo, hi: sum(lo <= a <= hi for a in f64)
    owithin = lambda lo, hi: sum(lo <= a <= hi for a in other)
    # the kernel has two loop nests with FP64 work: (limb loop > digit loop), which the compiler rotates onto ONE header with two back
    # edges (digit: the nearer one, limb: the farther one), and behind it the loop over the two inverse transforms
    big = sorted((h, sorted(e)) for h, e in loops(ins).items() if within(h, max(e)) > 100)
    if len(big) == 3 and len(big[0][1]) == 1 and len(big[1][1]) == 2 and big[0][0] < big[1][0] and max(big[1][1]) < big[0][1][0]:
        # since the source words of a limb are requested a limb ahead (round 5) the limb loop has a header of its own: limb loop > digit loop with two back
        # edges (the nearer one: next digit; the farther one: the end of the recentring block that runs every `accmax` terms - counted once per limb, as before)
        (h0, (limb_end,)), (h1, (digit_end, _settle_end)), (h2, e2) = big
    elif len(big) == 2 and len(big[0][1]) == 2:
        (h1, (digit_end, limb_end)), (h2, e2) = big
        h0 = h1
    else:
        raise RuntimeError("unrecognised loop structure in the key-switch kernel: %s" % [(hex(h), [hex(x) for x in e]) for h, e in big])
    tail_end = max(e2)
    limb_only = lambda f: f(h0, limb_end) - f(h1, digit_end)
    return dict(kernel="k_keyswitch_rr<13, ArF64T<0>, 1, true, false>", instructions=len(ins), fp64_total=len(f64),
                fp64_digit_loop=within(h1, digit_end), fp64_limb_loop_only=limb_only(within),
                fp64_tail_loop=within(h2, tail_end), fp64_once=len(f64) - within(h0, limb_end) - within(h2, tail_end),
                valu_digit_loop=owithin(h1, digit_end), valu_limb_loop_only=limb_only(owithin),
                valu_tail_loop=owithin(h2, tail_end), valu_once=len(other) - owithin(h0, limb_end) - owithin(h2, tail_end))


def fp64_per_thread(k, digits_per_limb, obj=None, kernel=KERNEL):
    """FP64 instructions one thread executes for one (ciphertext, output limb): k source limbs x their digits, 2 inverse transforms"""
    s = structure(obj, kernel)
    return sum(d * s["fp64_digit_loop"] + s["fp64_limb_loop_only"] for d in digits_per_limb) + 2 * s["fp64_tail_loop"] + s["fp64_once"], s


def valu_per_thread(digits_per_limb, s):
    """non-FP64 VALU instructions of the same thread (digit extraction, selects, addressing; every one at least a full-rate issue slot)"""
    return sum(d * s["valu_digit_loop"] + s["valu_limb_loop_only"] for d in digits_per_limb) + 2 * s["valu_tail_loop"] + s["valu_once"]


def digit_loop(obj=None, kernel=KERNEL):
    """the instructions of the digit loop (header .. the nearer back edge), in program order"""
    obj = obj or os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_ks_f64l.o")
    ins = disassemble(obj, kernel)
    is64 = lambda op: op.startswith("v_") and "_f64" in op
    big = sorted((h, sorted(e)) for h, e in loops(ins).items() if sum(h <= a <= max(e) and is64(op) for a, op, _ in ins) > 100)
    h1, edges = big[1] if len(big) == 3 else big[0]
    return [i for i in ins if h1 <= i[0] <= edges[0]]


def _regs(tok):
    """VGPR numbers named by one operand"""
    m = re.match(r"^-?\|?v\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^-?\|?v(\d+)\b", tok)
    return [int(m.group(1))] if m else []


BUCKETS = ("digit extraction", "u64 -> f64 image", "LDS address arithmetic (exchanges, LDS twiddles)", "key address arithmetic", "register moves", "other")


def digit_loop_buckets(obj=None, kernel=KERNEL):
    """The non-FP64 VALU instructions of one digit, by what their result is used for.  A backward slice over the loop body (one basic block but for the
    recentring that runs every `accmax` terms): the address operands of ds_* instructions and of global loads, and the operands of FP64 instructions, are the
    sinks; an integer instruction belongs to the sink its result reaches first (walking up from the end of the body).  Inside the FP64 slice the
    shifts and masks are the digit extraction and the `or` with the exponent pattern 0x43300000 is the u64 -> f64 image."""
    body = digit_loop(obj, kernel)
    want, out = {}, {b: 0 for b in BUCKETS}
    hist = {b: {} for b in BUCKETS}
    for addr, op, args in reversed(body):
        toks = [t.strip() for t in args.split(",")] if args else []
        if op.startswith("ds_") or op.startswith("global_") or op.startswith("flat_"):
            store = "write" in op or "store" in op
            a = toks[0] if (store or op.startswith("ds_write")) else (toks[1] if len(toks) > 1 else "")
            if op.startswith("global_load") or op.startswith("flat_load") or op.startswith("ds_read"):
                a = toks[1] if len(toks) > 1 else ""
                for r in _regs(toks[0]):
                    want.pop(r, None)
            for r in _regs(a):
                want[r] = BUCKETS[2] if op.startswith("ds_") else BUCKETS[3]
            continue
        if not op.startswith("v_"):
            continue
        dst, src = _regs(toks[0]) if toks else [], [r for t in toks[1:] for r in _regs(t)]
        if "_f64" in op:
            for r in dst:
                want.pop(r, None)
            for r in src:
                want.setdefault(r, "value")
            continue
        if op.startswith("v_readfirstlane"):
            continue
        use = next((want[r] for r in dst if r in want), None)
        for r in dst:
            want.pop(r, None)
        if op.startswith("v_mov") or op.startswith("v_accvgpr"):
            b = BUCKETS[4]
        elif use == "value":
            b = BUCKETS[1] if (op.startswith("v_or") and "0x4330" in args) else BUCKETS[0]
        elif use in (BUCKETS[2], BUCKETS[3]):
            b = use
        else:
            b = BUCKETS[5]
        out[b] += 1
        hist[b][op] = hist[b].get(op, 0) + 1
        for r in src:
            want.setdefault(r, use if use else "other")
    return out, hist


def resources(obj, pattern):
    """{kernel symbol: (VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes)} of the kernels whose mangled name contains `pattern`, from the code object's notes"""
    with tempfile.TemporaryDirectory() as td:
        tmp = os.path.join(td, os.path.basename(obj))
        os.symlink(os.path.abspath(obj), tmp)
        subprocess.check_call([OBJDUMP, "--offloading", tmp], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        co = [f for f in glob.glob(tmp + ".*") if "amdgcn" in f]
        txt = subprocess.check_output([os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf"), "--notes", co[0]], text=True)
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        f = lambda key: (re.search(r"\.%s:\s*(\S+)" % key, blk) or [None, "?"])[1]
        name = f("name")
        if pattern in name:
            out[name] = dict(vgpr=int(f("vgpr_count")), agpr=int(blk.split()[0]), sgpr=int(f("sgpr_count")), scratch=int(f("private_segment_fixed_size")),
                             lds=int(f("group_segment_fixed_size")))
    return out


def static_counts(obj, kernel):
    """instructions / FP64 / other VALU / v_rndne_f64 (one per modular product or recentring) in the whole kernel body, unweighted"""
    ins = disassemble(obj, kernel)
    return dict(instructions=len(ins), fp64=sum(op.startswith("v_") and "_f64" in op for _, op, _ in ins),
                valu_other=sum(op.startswith("v_") and "_f64" not in op and not op.startswith("v_readfirstlane") for _, op, _ in ins),
                rndne=sum(op.startswith("v_rndne_f64") for _, op, _ in ins))


PIPE_KERNEL = "_Z13k_square_pipeILi13E6ArF64TILi0EEJEE"               # k_square_pipe<13, ArF64T<0>>: the squaring of the CryptoNets batches
SQUARE_KERNEL = "_Z14k_square_fusedILi13E6ArF64TILi0EELb1EJEE"        # k_square_fused<13, ArF64T<0>, true>: fused squaring, operand parked in LDS


def _branches(ins):
    """[(index, address, mnemonic, target address)] of every branch of the kernel"""
    out = []
    for k, (addr, op, args) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            m = re.search(r"(-?\d+)", args)
            if not m:
                continue
            off = int(m.group(1))
            off = off - 65536 if off >= 32768 else off
            nxt = ins[k + 1][0] if k + 1 < len(ins) else addr + 4
            out.append((k, addr, op, nxt + 4 * off))
    return out


def square_structure(obj=None, kernel=SQUARE_KERNEL):
    """FP64 / other VALU instructions ONE THREAD of k_square_fused executes for one (ciphertext, limb) block, from the built code object.
    The kernel is one rolled loop over the three steps (cn_k_rr.hip.h); the compiler rotates it so that the body starts with the inverse
    transform + store (all three steps), followed by the exit test, then EITHER the forward transform with the step-0 / step-1 tensor
    variants (each variant skipped by one forward branch in the other step) OR the step-2 block (A1^2 out of LDS).  Weights: inverse part
    x 3, forward part x 2, each skippable variant block x 1, step-2 block x 1."""
    obj = obj or os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_rr_f64l.o")
    ins = disassemble(obj, kernel)
    addrs = [a for a, _, _ in ins]
    is64 = lambda op: op.startswith("v_") and "_f64" in op
    isv = lambda op: op.startswith("v_") and "_f64" not in op and not op.startswith("v_readfirstlane")
    br = _branches(ins)
    back = [(a, t) for _, a, _, t in br if t <= a and a - t > 4096]
    if not back:
        raise RuntimeError("no step loop found in %s" % kernel)
    head = min(t for _, t in back)
    last = max(a for a, _ in back)
    end = addrs[-1]
    body = [(k, a, op, t) for k, a, op, t in br if head <= a <= last]
    exit_br = [(a, t) for _, a, op, t in body if op.startswith("s_cbranch") and t > last]
    if len(exit_br) != 1:
        raise RuntimeError("unrecognised exit structure in %s: %s" % (kernel, [(hex(a), hex(t)) for a, t in exit_br]))
    exit_at = exit_br[0][0]
    # the first forward conditional branch behind the exit test selects the step-2 block
    sel = [(a, t) for _, a, op, t in body if op.startswith("s_cbranch") and a > exit_at and exit_at < t <= last]
    if not sel:
        raise RuntimeError("no step selector found in %s" % kernel)
    sel_at, step2_at = sel[0]
    variants = [(a, t) for a, t in sel[1:] if a < step2_at and t <= step2_at + 8]
    if len(variants) != 2:
        raise RuntimeError("expected the step-0 / step-1 tensor variants in %s, found %s" % (kernel, [(hex(a), hex(t)) for a, t in variants]))

    def count(pred, lo, hi):                 # instructions with lo <= address < hi
        return sum(1 for a, op, _ in ins if lo <= a < hi and pred(op))
    res = {}
    for name, pred in (("fp64", is64), ("valu", isv)):
        inv = count(pred, head, exit_at)
        var = [count(pred, a + 4, t) for a, t in variants]
        fwd = count(pred, sel_at, step2_at) - sum(var)
        st2 = count(pred, step2_at, last + 4)
        once = count(pred, addrs[0], head) + count(pred, last + 4, end + 4)
        res[name] = dict(inverse_part=inv, forward_part=fwd, tensor_variants=var, step2_block=st2, once=once,
                         per_thread=3 * inv + 2 * fwd + sum(var) + st2 + once)
    if not 4500 <= res["fp64"]["per_thread"] <= 7500:
        raise RuntimeError("implausible FP64 count %d for k_square_fused (2 forward + 3 inverse 8192-point transforms are ~5600)" % res["fp64"]["per_thread"])
    res["kernel"] = "k_square_fused<13, ArF64T<0>, true>"
    res["instructions"] = len(ins)
    return res


if __name__ == "__main__":
    # python tools/ks_isa_counts.py [OBJ_DIR]: OBJ_DIR holds cn_l_ks_f64l.o / cn_l_rr_f64l.o / cn_l_behz.o of the build to read (default: the in-tree build)
    od = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "cryptonets_amd", "lib", "obj")
    ks, rr = os.path.join(od, "cn_l_ks_f64l.o"), os.path.join(od, "cn_l_rr_f64l.o")
    s = structure(ks)
    print(json.dumps(s, indent=1))
    print(json.dumps(square_structure(rr), indent=1))
    print(json.dumps(dict(kernel="k_square_pipe<13, ArF64T<0>>", **static_counts(rr, PIPE_KERNEL)), indent=1))
    b, hist = digit_loop_buckets(ks)
    print("\nnon-FP64 VALU instructions of one digit of %s: %d" % (s["kernel"], sum(b.values())))
    print("| bucket | instructions | opcodes |\n|---|---|---|")
    for name in BUCKETS:
        print("| %s | %d | %s |" % (name, b[name], ", ".join("%s x%d" % kv for kv in sorted(hist[name].items(), key=lambda kv: -kv[1]))))
    print("\n| kernel | VGPRs | AGPRs | scratch | LDS (static) |\n|---|---|---|---|---|")
    for obj, pat in ((ks, "k_keyswitch_rrILi13E6ArF64TILi0EE"), (rr, "k_square_pipeILi13E"), (rr, "k_square_fusedILi13E"), (rr, "k_intt_tensorILi13E"),
                     (os.path.join(od, "cn_l_rr_f64.o"), "k_square_pipeILi13E"), (os.path.join(od, "cn_l_behz.o"), "k_behz_floor_f64ILi5ELi5E")):
        for name, r in sorted(resources(obj, pat).items()):
            print("| %s | %d | %d | %d | %d |" % (name, r["vgpr"], r["agpr"], r["scratch"], r["lds"]))
