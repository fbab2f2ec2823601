"""The wrapper's request path on the device (hewrapper.DEVICE_SPLIT): EncryptedSealBfvVector and EncryptedSealBfvFactory.GetEncryptedMatrix / GetPlainMatrix through
one cn_split_encrypt / cn_split_encode call against the host path, and cryptonets_mnist.encrypt_images.  Every comparison is exact."""
import os

import numpy as np
import pytest

from conftest import PARAMS

pytestmark = pytest.mark.gpu

TINY_PRIMES = (12289, 18433)


@pytest.fixture(scope="module")
def factory():
    from cryptonets_amd import hewrapper as hw
    from cryptonets_amd._native import Context
    from cryptonets_amd.client import DeviceClient
    p = PARAMS["tiny"]

    def context_factory(n, t, q, dbc, gdbc):
        return Context(n, t, q=q, dbc=dbc, gdbc=gdbc, device=0)
    context_factory.default_coeff_modulus = lambda n: p["q"]
    return hw.EncryptedSealBfvFactory(primes=list(TINY_PRIMES), n=1024, context_factory=context_factory, galois=False,
                                      device_client_factory=lambda ctx, t: DeviceClient(ctx, seed=0xC0FFEE ^ t))


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


MATRIX = np.array([[-3.25, 0.5, 7.0, -0.03125, 1.5],
                   [2.5, -2.5, 0.0, 100.0625, -77.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0],
                   [1000.5, -1000.5, 3.0, -4.0, 0.0625],
                   [-0.0, 12.75, -12.75, 1.0, -1.0],
                   [5.0, 6.0, -7.0, 8.0, 0.03125]])              # 6 x 5, signed, ties after the scale 16; products below M / 2 = 113 million


@pytest.mark.parametrize("fmt", ["ColumnMajor", "RowMajor"])
def test_encrypted_matrix_is_one_array_per_prime_and_decrypts_the_same(factory, monkeypatch, fmt):
    from cryptonets_amd import hewrapper as hw
    F, env = factory, factory.AllocateComputationEnv()
    fmt = getattr(hw.EMatrixFormat, fmt)
    ctxs = [e.ctx for e in env.Environments]
    live = [g.live_handles() for g in ctxs]
    got = {}
    for on in (True, False):
        monkeypatch.setattr(hw, "DEVICE_SPLIT", on)
        m = F.GetEncryptedMatrix(MATRIX, fmt, 16.0)
        got[on] = m.Decrypt(env)
        vecs = m.leVectors
        assert len(vecs) == (5 if fmt == hw.EMatrixFormat.ColumnMajor else 6) and m.Scale == 16.0
        for i in range(len(ctxs)):
            views = [v.eVectors[i].encData for v in vecs]
            one_array = all(v.buf is views[0].buf for v in views) and [v.first for v in views] == list(range(len(views))) and all(v.count == 1 for v in views)
            assert one_array == on
        if on:
            assert [g.live_handles() for g in ctxs] == [x + 1 for x in live]
        for j, v in enumerate(vecs):                               # the columns go one by one; the array goes with the last of them
            v.Dispose()
            if on:
                assert [g.live_handles() for g in ctxs] == [x + (j + 1 < len(vecs)) for x in live]
        assert [g.live_handles() for g in ctxs] == live
    assert got[True].shape == MATRIX.shape and np.array_equal(bits(got[True]), bits(got[False]))
    assert np.array_equal(got[True], np.rint(MATRIX * 16.0) / 16.0)


@pytest.mark.parametrize("fmt", ["ColumnMajor", "RowMajor"])
def test_plain_matrix_words_and_zero_flags_agree(factory, monkeypatch, fmt):
    from cryptonets_amd import hewrapper as hw
    F, env = factory, factory.AllocateComputationEnv()
    fmt = getattr(hw.EMatrixFormat, fmt)
    words, zeros = {}, {}
    for on in (True, False):
        monkeypatch.setattr(hw, "DEVICE_SPLIT", on)
        m = F.GetPlainMatrix(MATRIX, fmt, 16.0)
        words[on] = [[a.plainDense.buf.ctx.pt_download(a.plainDense.h, a.plainDense.first, a.plainDense.count) for a in v.eVectors] for v in m.leVectors]
        zeros[on] = [[list(a.plainZero) for a in v.eVectors] for v in m.leVectors]
        assert all(a.Dim == (6 if fmt == hw.EMatrixFormat.ColumnMajor else 5) and not a.IsEncrypted for v in m.leVectors for a in v.eVectors)
        m.Dispose()
    rows = MATRIX.T if fmt == hw.EMatrixFormat.ColumnMajor else MATRIX
    want = [[[all(int(x) % t == 0 for x in np.rint(r * 16.0))] for t in TINY_PRIMES] for r in rows]        # (the all-zero row of the row-major form is one of them)
    assert zeros[True] == zeros[False] == want
    for a, b in zip(words[True], words[False]):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_vectors_agree_with_the_host_path(factory, monkeypatch):
    """a dense vector of two blocks (the last one partial), a sparse one, given as doubles with a scale and as Python integers; encrypted and plain"""
    from cryptonets_amd import hewrapper as hw
    F, env = factory, factory.AllocateComputationEnv()
    M = env.bigFactor
    rng = np.random.default_rng(6)
    dense = rng.integers(-2 ** 20, 2 ** 20, size=1500).astype(np.float64) / 64.0
    ints = [int(x) for x in rng.integers(-(M // 2), M // 2, size=1100)] + [-(M // 2), M // 2, 0, -1]
    sparse = [-3.5, 2.5, 0.0, 1000.25, -0.03125, 7.0]
    live = [e.ctx.live_handles() for e in env.Environments]
    got = {}
    for on in (True, False):
        monkeypatch.setattr(hw, "DEVICE_SPLIT", on)
        vs = [F.GetEncryptedVector(dense, hw.EVectorFormat.dense, 16.0), F.GetEncryptedVector(ints, hw.EVectorFormat.dense),
              F.GetEncryptedVector(sparse, hw.EVectorFormat.sparse, 16.0), F.GetEncryptedVector(ints[:9], hw.EVectorFormat.sparse),
              F.GetEncryptedVector([2 ** 70, -2 ** 70, 5], hw.EVectorFormat.dense),                  # beyond int64: the host path in either case
              F.GetEncryptedVector([2.0 ** 63, -1.0], hw.EVectorFormat.dense, 1.0)]                  # 2^62 and beyond: the host path in either case
        assert [v.Dim for v in vs] == [1500, 1104, 6, 9, 3, 2] and [v.eVectors[0].encData.count for v in vs] == [2, 2, 6, 9, 1, 1]
        got[on] = [vs[0].Decrypt(env), vs[1].DecryptFullPrecision(env), vs[2].Decrypt(env), vs[3].DecryptFullPrecision(env), vs[4].DecryptFullPrecision(env),
                   vs[5].DecryptFullPrecision(env)]
        pv = F.GetPlainVector(dense, hw.EVectorFormat.dense, 16.0)
        got[on].append([(a.plainDense.buf.ctx.pt_download(a.plainDense.h, a.plainDense.first, 2).tolist(), list(a.plainZero), a.Dim) for a in pv.eVectors])
        ps = F.GetPlainVector(sparse, hw.EVectorFormat.sparse, 16.0)
        got[on].append([list(a.plainSparse) for a in ps.eVectors])
        for v in vs + [pv, ps]:
            v.Dispose()
        assert [e.ctx.live_handles() for e in env.Environments] == live
    a, b = got[True], got[False]
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[0], np.rint(dense * 16.0) / 16.0)
    assert a[1] == b[1] == ints
    assert np.array_equal(bits(a[2]), bits(b[2])) and a[3] == b[3] == ints[:9]
    assert a[4] == b[4] and a[5] == b[5]
    assert a[6] == b[6] and a[7] == b[7]


def test_encrypt_images_then_forward_and_predict_equal_the_integer_model():
    """8 synthetic images in the first 8 slots of the 8192-slot batch of the CryptoNets configuration: the predicted classes are the arg max of the exact integer logits"""
    from cryptonets_amd import cryptonets_mnist as cm
    from cryptonets_amd._native import Context, default_coeff_modulus
    from cryptonets_amd.client import DeviceClient
    w = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cryptonets_weights.npz"))
    layers = cm.layer_tables(w["Weights_0"], w["Weights_1"], w["Biases_2"], w["Weights_3"], w["Biases_3"])
    images = cm.synthetic_images(8, seed=5)
    channels = []
    for p in cm.PLAIN_PRIMES:
        g = Context(cm.N, p, q=default_coeff_modulus(cm.N), dbc=10, gdbc=20, device=0)
        DeviceClient(g, seed=0x51CE ^ p).generate_keys(with_galois=False)
        channels.append(cm.CryptoNetsChannel(g, layers, cm.constant_plaintext(cm.N)))
    cm.encrypt_images(channels, images * cm.NORMALIZATION, cm.INPUT_SCALE, seeds=[7, 8])
    for ch in channels:
        ch.forward()
    got = cm.predict(channels, nslots=8)
    want = []
    for s in range(8):
        logits = cm.int_logits(w, images[s])
        want.append(max(range(10), key=lambda c: (logits[c], -c)))
    assert got.tolist() == want
    with pytest.raises(ValueError):
        cm.encrypt_images(channels, images[:, :783], cm.INPUT_SCALE)
    for ch in channels:
        ch.g.close()
