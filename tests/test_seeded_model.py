"""CPU: the model of the seeded draw (tests/seeded_model.py) against RFC 7539, its rejection path, the four seeded entry points in header, binding and
library, and the register budget of the seeded kernel."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import seeded_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ENTRY_POINTS = ["cn_encrypt_symmetric", "cn_ct_expand", "cn_ct_upload_compact", "cn_ct_download_compact"]

RFC7539_232 = [0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
               0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2]


def test_model_block_function_is_rfc7539_section_2_3_2():
    """the block the device sampler's known-answer test uses: key 00..1f, counter word 1, nonce 00:00:00:09:00:00:00:4a:00:00:00:00"""
    got = sm.chacha20_block(bytes(range(32)), 0x0900000000000001, 0x000000004a000000)
    assert [int(x) for x in got[0]] == RFC7539_232
    both = sm.chacha20_block(bytes(range(32)), [0x0900000000000001, 5], 0x000000004a000000)        # vectorised over counters
    assert [int(x) for x in both[0]] == RFC7539_232 and [int(x) for x in both[1]] != RFC7539_232


def test_counter_layout():
    assert sm.rng_counter(1, 0, 0, 0) == 1 << 24
    assert sm.rng_counter(0, sm.STREAM_A, 0, 0) == 4 << 20
    assert sm.rng_counter(0, 0, 3, 0xffff) == (3 << 16) | 0xffff
    assert sm.rng_counter((1 << 40) - 1, 15, 15, 0xffff) == (1 << 64) - 1


def test_rejection_path_redraws_the_word_at_the_next_trial():
    """q = 2^63 + 29: every word above 2^64 - 1 - (2^64 - 1) mod q - 1 = 2^63 + 28 ... i.e. about half of all words is rejected.  Search (seed, block) on the
    CPU for a block with a rejected word and check the redraw by hand: the word keeps its position and comes from the block of the next trial."""
    q = (1 << 63) + 29
    lim = (1 << 64) - 1 - ((1 << 64) - 1) % q - 1
    seed = bytes(range(32, 64))
    found = False
    for blk in range(64):
        out, rej = sm.sample_uniform8(seed, 7, sm.STREAM_A, 3, [blk], q)
        trials = [sm.chacha20_block(seed, sm.rng_counter(3, sm.STREAM_A, tr, blk), 7)[0] for tr in range(16)]
        words = [[(int(w[2 * c]) << 32) | int(w[2 * c + 1]) for c in range(8)] for w in trials]
        expect_rej = 0
        for c in range(8):
            tr = 0
            while words[tr][c] > lim:
                tr += 1
                expect_rej += 1
            assert int(out[0, c]) == words[tr][c] % q
            found = found or tr > 0
        assert rej == expect_rej
    assert found
    # a modulus the library accepts (< 2^60) rejects only if 2^64 mod q is large: q near 2^64 / 16.5 drops about 3 % of the words
    q59 = (1 << 64) * 2 // 33
    _, rej = sm.sample_uniform8(seed, 7, sm.STREAM_A, 0, np.arange(64), q59)
    assert q59 < 1 << 60 and rej > 0


def test_seeded_a_has_the_layout_of_a_key_polynomial():
    """limb j takes blocks j N/8 .. (j + 1) N/8 - 1, block b the positions 8 b .. 8 b + 7; limbs of one item differ, items differ"""
    qs, n = [0xffffee001, 0xffffc4001], 64
    a = sm.seeded_a(bytes(32), 9, 5, n, qs)
    assert a.shape == (2, n) and all(int(a[j].max()) < qs[j] for j in range(2))
    one, _ = sm.sample_uniform8(bytes(32), 9, sm.STREAM_A, 5, [n // 8 + 2], qs[1])
    assert np.array_equal(a[1, 16:24], one[0])
    assert not np.array_equal(a, sm.seeded_a(bytes(32), 9, 6, n, qs)) and not np.array_equal(a, sm.seeded_a(bytes(32), 8, 5, n, qs))


def test_header_binding_and_library_have_the_seeded_entry_points():
    from cryptonets_amd import _native
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cnhip.h")).read(), flags=re.S)
    _native.build()
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in include/cnhip.h"
        assert name in _native.SIGNATURES, name
        assert hasattr(L, name), name + " is not exported by the built library"
    assert re.search(r"#define\s+CN_STREAM_A\s+\(?%d\)?" % sm.STREAM_A, open(os.path.join(ROOT, "include", "cnhip.h")).read())
    for meth in ("encrypt_symmetric", "ct_expand", "ct_upload_compact", "ct_download_compact"):
        assert callable(getattr(_native.Context, meth))
    cs = open(os.path.join(ROOT, "integration", "CnHip.cs")).read()
    assert all(name in cs for name in ENTRY_POINTS)


# ---- register budget of the BUILT seeded kernel (in the manner of tests/test_build_resources.py)
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj", "cn_l_seeded.o")
SEEDED = [("void k_seeded<%d, %s>" % (L, pol), 128) for L in (10, 11, 12, 13, 14) for pol in ("ArF64T<0> ", "ArF64T<1> ", "ArU64")]


@pytest.fixture(scope="module")
def seeded_resources():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    return kernel_resources.resources(OBJ)


@pytest.mark.parametrize("kernel,budget", SEEDED)
def test_seeded_kernel_stays_inside_its_register_budget(seeded_resources, kernel, budget):
    """128 VGPRs: four waves per SIMD - two 512-thread workgroups per CU at N = 8192, the one 1024-thread workgroup at N = 16384 - and no scratch"""
    assert kernel in seeded_resources, "%s not found (have e.g. %s)" % (kernel, sorted(seeded_resources)[:3])
    r = seeded_resources[kernel]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, "%s spills: %s" % (kernel, r)
    assert r["vgpr"] + r["agpr"] <= budget, "%s: %d registers, budget %d" % (kernel, r["vgpr"] + r["agpr"], budget)


def test_seeded_kernel_uses_global_not_flat_memory_instructions():
    from cryptonets_amd import _native
    _native.build()
    import kernel_resources
    flat = kernel_resources.flat_instructions(OBJ)
    assert not flat, flat


def test_compact_batch_framing_round_trip_and_rejections():
    import io
    from cryptonets_amd import serialization as ser
    parms = ser.Parameters(1024, [0xffffee001, 0xffffc4001, 0x1ffffe0001], 12289)
    rng = np.random.default_rng(1)
    for limbs in (3, 2):
        lv = parms.level(limbs)
        c0 = rng.integers(0, 1 << 36, size=(4, limbs * 1024), dtype=np.uint64)
        d = ser.CompactDescriptor(os.urandom(32), 11, 1000, 4, lv.parms_id())
        f = io.BytesIO()
        ser.save_compact_batch(f, c0, d)
        raw = f.getvalue()
        assert raw[:8] == b"CNHIPSC1" and len(raw) == 8 + 4 + 32 + 24 + 32 + 8 + c0.nbytes
        got, d2, l2 = ser.load_compact_batch(io.BytesIO(raw), parms)
        assert np.array_equal(got, c0) and d2 == d and l2 == limbs
        with pytest.raises(ser.BadStream):
            ser.load_compact_batch(io.BytesIO(raw[:-8]), parms)
        with pytest.raises(ser.BadStream):
            ser.load_compact_batch(io.BytesIO(b"X" + raw[1:]), parms)
        with pytest.raises(ser.BadStream):
            ser.load_compact_batch(io.BytesIO(raw), ser.Parameters(1024, [0xffffee001], 40961))
