"""CPU: packed batches (serialization.save_packed_batch / load_packed_batch) - round trips at two levels of a chain and the streams the loader refuses."""
import io
import struct

import numpy as np
import pytest

import packed_model as pm
from conftest import PARAMS
from cryptonets_amd import serialization as ser

SEED = bytes(range(32))


def chain():
    p = PARAMS["tiny"]
    return ser.Parameters(p["n"], p["q"], p["t"])


def batch(parms, rng, count=3, item0=5):
    words = pm.random_words(rng, parms.q, parms.n, count, 1)
    packed = ser.pack_ciphertexts(words, parms.q, parms.n)
    return packed, ser.PackedDescriptor(SEED, 9, item0, count, parms.parms_id(), ser.packed_bits(parms.q)), words


def stream_of(packed, desc):
    f = io.BytesIO()
    ser.save_packed_batch(f, packed, desc)
    return f.getvalue()


@pytest.mark.parametrize("limbs", [3, 2])
def test_round_trip_at_two_levels(limbs, rng):
    top = chain()
    packed, desc, words = batch(top.level(limbs), rng)
    raw = stream_of(packed, desc)
    assert len(raw) == 8 + 4 + 32 + 24 + 32 + 4 + limbs + 8 + packed.size * 8
    got, d, l = ser.load_packed_batch(io.BytesIO(raw), top)
    assert l == limbs and d == desc and d.bits == ser.packed_bits(top.q[:limbs])
    assert got.dtype == np.uint64 and np.array_equal(got, packed)
    assert np.array_equal(ser.unpack_ciphertexts(got, top.q[:limbs], top.n, 1), words)


# offsets of the fields in the stream
O_VERSION, O_ITEM0, O_COUNT, O_PID, O_LIMBS = 8, 8 + 4 + 32 + 8, 8 + 4 + 32 + 16, 8 + 4 + 32 + 24, 8 + 4 + 32 + 24 + 32


def test_loader_refuses_bad_streams(rng):
    top = chain()
    packed, desc, _ = batch(top, rng)
    raw = stream_of(packed, desc)
    ser.load_packed_batch(io.BytesIO(raw), top)

    def refused(b, parms=top):
        with pytest.raises(ser.BadStream):
            ser.load_packed_batch(io.BytesIO(bytes(b)), parms)

    refused(b"CNHIPSC1" + raw[8:])                                                        # wrong magic (a compact batch's)
    refused(raw[:O_VERSION] + struct.pack("<I", 2) + raw[O_VERSION + 4:])                 # wrong version
    refused(raw, ser.Parameters(top.n, top.q, 40961))                                     # foreign parms_id: another plain modulus
    refused(raw[:O_PID] + bytes(32) + raw[O_PID + 32:])
    wrong = bytearray(raw)
    wrong[O_LIMBS + 4] = 37                                                                # wrong widths: 37 bits for a 36-bit modulus
    refused(wrong)
    refused(raw[:O_LIMBS] + struct.pack("<I", 2) + raw[O_LIMBS + 4:])                     # ... or another number of them
    refused(raw[:-8])                                                                      # short array: truncated
    short = stream_of(packed[:2], ser.PackedDescriptor(SEED, 9, 5, 2, desc.parms_id, desc.bits))
    refused(short[:O_COUNT] + struct.pack("<Q", 3) + short[O_COUNT + 8:])                 # ... or fewer words than the count asks for
    refused(raw[:O_ITEM0] + struct.pack("<Q", (1 << 40) - 2) + raw[O_ITEM0 + 8:])         # item overflow: a_item0 + count beyond 40 bits


def test_save_checks_the_shape(rng):
    top = chain()
    packed, desc, _ = batch(top, rng)
    with pytest.raises(ValueError):
        ser.save_packed_batch(io.BytesIO(), packed[:2], desc)
    with pytest.raises(ValueError):
        ser.save_packed_batch(io.BytesIO(), packed[:, :-1], desc)
