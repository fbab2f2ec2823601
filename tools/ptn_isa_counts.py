#!/usr/bin/env python
"""Instruction counts of the term loop of k_mul_ptn_sum (cn_k_ptn.hip.h), read from the BUILT code object like tools/ks_isa_counts.py: the loop is the kernel's
one backward branch in front of the inverse transforms; per trip (one term of a group, one thread) it prints the FP64 instructions, the other VALU
instructions and the global loads.  With a device it prices the FP64 instructions of a whole call against the issue rate measured in the same process
(cn_valu_issue_time: ns per FP64 wave-instruction per SIMD) - the kernel's arithmetic floor - beside the time the plaintext bytes take at the HBM's rate.

    python tools/ptn_isa_counts.py [--logn 14] [--policy 1] [--terms 16384] [--k 8] [--floor] [--counts 272,96,69,24,408]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ks_isa_counts

OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_ptn.o")
FORMS = {10: (2, 4, 1), 11: (2, 4, 1), 12: (2, 4, 1), 13: (2, 4, 1), 14: (2, 1, 2)}      # (polynomials per block, register pairs per chunk, chunks ahead) of the FP64 policies: PtnForm, cn_l_ptn.hip
HBM_BYTES_PER_S = 8e12                                                   # the MI355X's specified HBM bandwidth


def term_loop(logn, policy):
    """{"fp64", "valu", "loads", "instructions"} per trip of the term loop of k_mul_ptn_sum<logn, ArF64T<policy>, NP, WS>"""
    np_, ws, depth = FORMS[logn]
    kernel = "_Z13k_mul_ptn_sumILi%dE6ArF64TILi%dEELi%dELi%dELi%dEE" % (logn, policy, np_, ws, depth)
    ins = ks_isa_counts.disassemble(OBJ, kernel)
    found = ks_isa_counts.loops(ins)
    span = lambda lo, hi: [(a, op) for a, op, _ in ins if lo <= a <= hi]
    cands = [(h, sorted(e)) for h, e in found.items() if any(op.startswith("global_load") for _, op in span(h, max(e)))]
    if len(cands) != 1 or len(cands[0][1]) != 2:
        raise RuntimeError("expected ONE loop with global loads and two back edges (a term; a term that ends an interval) in %s, found %s" % (kernel, cands))
    h, (near, far) = cands[0]
    b, settle = span(h, near), span(near + 1, far)                     # behind the nearer back edge: the recentring of the accumulators, run every `interval` terms
    f64 = lambda x: sum(op.startswith("v_") and "_f64" in op for _, op in x)
    return {"fp64": f64(b), "settle_fp64": f64(settle), "valu": sum(op.startswith("v_") and "_f64" not in op for _, op in b),
            "loads": sum(op.startswith("global_load") for _, op in b), "instructions": len(b), "polys": np_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=14)
    ap.add_argument("--policy", type=int, default=1, help="1 = ArF64 (moduli below 2^49.4), 0 = ArF64L (up to 44 bits)")
    ap.add_argument("--terms", type=int, default=16384, help="terms of the call (diagonals of the plan)")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--interval", type=int, default=11, help="terms between two recentrings (cn_get_option \"ptn_sum_interval\": 11 at 49 bits)")
    ap.add_argument("--floor", action="store_true", help="measure the FP64 issue rate on the device and print the two floors of a call")
    ap.add_argument("--counts", default=None, help="fp64,settle_fp64,valu,loads,instructions of a term, as an earlier run printed them (a machine without the object files)")
    a = ap.parse_args()
    if a.counts:
        c = dict(zip(("fp64", "settle_fp64", "valu", "loads", "instructions"), (int(x) for x in a.counts.split(","))), polys=FORMS[a.logn][0])
    else:
        c = term_loop(a.logn, a.policy)
    print("k_mul_ptn_sum<%d, ArF64T<%d>>: per term and thread %d FP64 + %d other VALU instructions, %d global loads (%d instructions in the loop), %d FP64 more per recentring; "
          "%d polynomials per block" % (a.logn, a.policy, c["fp64"], c["valu"], c["loads"], c["instructions"], c["settle_fp64"], c["polys"]))
    n = 1 << a.logn
    waves = (n // 16) // 64                                               # per block
    blocks = a.terms * a.k * (2 // c["polys"])                            # block-terms of the call
    wave_instr = (c["fp64"] + c["settle_fp64"] / a.interval) * waves * blocks
    bytes_pt = a.terms * a.k * n * 8
    print("a call of %d terms, k = %d: %.3g FP64 wave-instructions; plaintext bytes %.2f GiB = %.2f ms at %.0f TB/s"
          % (a.terms, a.k, wave_instr, bytes_pt / 2 ** 30, bytes_pt / HBM_BYTES_PER_S * 1e3, HBM_BYTES_PER_S / 1e12))
    if a.floor:
        from cryptonets_amd._native import Context
        from oracle.cno import COEFF_MODULUS_128
        g = Context(1 << 13, 557057, q=COEFF_MODULUS_128[1 << 13], dbc=10, gdbc=20, device=0)
        ns = g.fp64_issue_ns()
        simds = 4 * 256                                                   # 256 CUs of four SIMDs
        print("FP64 issue: %.3f ns per wave-instruction per SIMD -> FP64 issue floor of the call %.2f ms on %d SIMDs" % (ns, wave_instr * ns / simds * 1e-6, simds))
        g.close()


if __name__ == "__main__":
    main()
