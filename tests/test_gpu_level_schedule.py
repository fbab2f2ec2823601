"""GPU: modulus-switching schedules - the exact-FP64 switch kernel word for word against the model and the integer kernel, every layer type
of the networks on an input at a lower level against the same layer at the top level, one network object run at the top level, scheduled
and at the top level again, networks planned on calibration records and run on others against their integer models, and the refusal of
a recorded evaluation of a scheduled chain."""
import os

import numpy as np
import pytest

from conftest import PARAMS
from modswitch_model import switch_residues

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cryptonets_weights.npz")
# LoLa-CIFAR's chain at 9 limbs: all of CoeffModulus128(16384)
C9 = list(PARAMS["c5"]["q"]) + [0x1ffffffe48001]           # = COEFF_MODULUS_128[16384]


def make_factory(backend, primes, n, dbc=10, gdbc=20, small_modulus_count=-1, galois=True):
    """a factory with the device client (keys, encryption, decryption and noise budgets on the device; reproducible seed)"""
    from cryptonets_amd.hewrapper import EncryptedSealBfvFactory
    assert backend == "gpu"
    return EncryptedSealBfvFactory(list(primes), n, dbc, gdbc, small_modulus_count, galois=galois, client_seed=1234)


def qs(name):
    p = PARAMS[name]
    if p["q"] is not None:
        return list(p["q"])
    from oracle.cno import COEFF_MODULUS_128
    return list(COEFF_MODULUS_128[p["n"]])


def ctx(name, q=None):
    from cryptonets_amd._native import Context
    p = PARAMS[name]
    return Context(p["n"], p["t"], q=q or qs(name), dbc=p["dbc"], gdbc=p["gdbc"], device=0)


def rand_cts(rng, q, n, count, size):
    return np.stack([np.concatenate([rng.integers(0, m, size=n, dtype=np.uint64) for _ in range(size) for m in q]) for _ in range(count)])


def f64_pair(ks, kd):
    """the (KS, KD) pairs cn_l_mod_switch runs in FP64 (cn_l_modswitch.hip: cn_ms_f64_pair)"""
    return ks - kd >= 2


# ------------------------------------------------------------------ the FP64 kernel, word for word
@pytest.mark.parametrize("name", ["c3", "c4", "c5", "c9"])
def test_fp64_mod_switch_words_every_pair(name):
    g = ctx("c5", C9) if name == "c9" else ctx(name)
    q, n = g.q, g.n
    assert g.get_option("f64") == 1
    rng = np.random.default_rng(17)
    chains = [g] + [g.level(k) for k in range(g.k - 1, 1, -1)]          # every source level KS <= k of the chain
    for size in (2, 3):
        for src_ctx in chains:
            ks, sq = src_ctx.k, src_ctx.q
            count = 5 if n == 8192 else 3                                # 5 x 2 x 4096 / 256 = 160 workgroups: the last is partial for odd counts
            src = rand_cts(rng, sq, n, count, size)
            src[0, :n] = [m - 1 for m in sq[:1]] * n                     # a limb of q - 1 words
            h = src_ctx.ct_alloc(count + 1, size)
            src_ctx.ct_upload(h, 1, src)
            for kd in range(ks - 1, 0, -1):
                lv = g.level(kd)
                out = lv.ct_alloc(count + 2, size)
                src_ctx.mod_switch(h, 1, count, lv, out, 2)              # non-zero offsets on both sides
                assert src_ctx.get_option("mod_switch_f64") == f64_pair(ks, kd) and lv.get_option("mod_switch_f64") == f64_pair(ks, kd)
                got = lv.ct_download(out, 2, count, size)
                exp = switch_residues(src, sq, n, kd).reshape(count, -1)
                assert np.array_equal(got, exp), (name, size, ks, kd)
                lv.free(out)
            src_ctx.free(h)


def test_fp64_and_integer_switch_give_the_same_words_for_845_ciphertexts():
    words = {}
    for f64 in (1, 0):
        g = ctx("c3")
        g.set_option("f64", f64)
        src = rand_cts(np.random.default_rng(18), g.q, g.n, 845, 2)
        h = g.ct_alloc(845, 2)
        for s in range(0, 845, 169):
            g.ct_upload(h, s, src[s:s + 169])
        for kd in (4, 2):
            lv = g.level(kd)
            out = lv.ct_alloc(845, 2)
            g.mod_switch(h, 0, 845, lv, out, 0)
            assert g.get_option("mod_switch_f64") == (f64 and f64_pair(5, kd))
            words[(f64, kd)] = lv.ct_download(out, 0, 845)
            lv.free(out)
        if f64:
            for kd in (4, 2):
                assert np.array_equal(words[(1, kd)], switch_residues(src, g.q, g.n, kd).reshape(845, -1))
        g.free(h)
        g.close()
    for kd in (4, 2):
        assert np.array_equal(words[(1, kd)], words[(0, kd)])


# ------------------------------------------------------------------ layers at a lower level
def _top_handles(env):
    return [e.ctx.live_handles() for e in env.Environments]


def _layers(head):
    from cryptonets_amd.networks import _chain
    return list(_chain(head))[::-1]


def _each_layer_at_a_level(head, Factory, check, drop=1):
    """for every layer after the EncryptLayer: its top-level input, and a copy of it switched `drop` limbs down, through the layer; the two
    outputs must decrypt to the same values.  Returns the layer types covered."""
    from cryptonets_amd.levels import _DeviceOracle
    o = _DeviceOracle(head, Factory, 1)
    env = Factory.AllocateComputationEnv()
    covered = []
    try:
        x = o.inputs[0]
        o.inputs = []
        for p in range(o.k + 1, len(o.layers)):
            L = o.layers[p]
            lv = o._switch(o._copy(x), env.Limbs - drop)
            assert lv.Limbs == env.Limbs - drop
            y_lv = o._step(L, lv)
            y = o._step(L, x)
            if type(L).__name__ in check:
                assert y_lv.Limbs == env.Limbs - drop
                assert np.array_equal(np.asarray(y_lv.Decrypt(env)), np.asarray(y.Decrypt(env))), type(L).__name__
                covered.append(type(L).__name__)
            y_lv.Dispose()
            x = y
        x.Dispose()
    finally:
        o.close()
    return covered


def test_every_lola_layer_type_at_a_level():
    from test_lola import PRIMES, lola
    Factory = make_factory("gpu", primes=PRIMES, n=8192, galois=True)
    img = np.where(np.random.default_rng(4).random(784) < 0.81, 0, np.random.default_rng(5).integers(1, 256, size=784)).astype(float)
    net = lola(Factory, img)
    names = {"LLPoolLayer", "LLVectorizeLayer", "SquareActivation", "LLDuplicateLayer", "LLPackedDenseLayer", "LLInterleaveLayer",
             "LLInterleavedDenseLayer"}
    assert set(_each_layer_at_a_level(net, Factory, names)) == names


def test_cryptonets_layer_types_at_a_level():
    from test_cryptonets_mnist import build_network, synthetic_images
    from cryptonets_amd import cryptonets_mnist as cm
    Factory = make_factory("gpu", primes=cm.PLAIN_PRIMES, n=cm.N, galois=False)
    net, _ = build_network(Factory, synthetic_images(16, seed=7))
    assert set(_each_layer_at_a_level(net, Factory, {"PoolLayer", "SquareActivation"})) == {"PoolLayer", "SquareActivation"}


@pytest.mark.parametrize("force", [False, True])
def test_lldense_layer_at_a_level(force):
    from cryptonets_amd import networks
    from cryptonets_amd.hewrapper import EVectorFormat
    from cryptonets_amd.layers import LLDenseLayer, LLPoolLayer, LLVectorizeLayer, SquareActivation, EncryptLayer
    w = np.load(os.path.join(os.path.dirname(GOLD), "small_model_weights.npz"))
    Factory = make_factory("gpu", primes=(2277377, 2424833), n=8192, dbc=40, gdbc=40, small_modulus_count=5, galois=True)
    reader = networks.lola_reader("LoLaSmall", Factory=Factory)
    reader.Features = np.where(np.random.default_rng(9).random(784) < 0.81, 0, 128.0) / 256.0
    enc = EncryptLayer(Source=reader, Factory=Factory)
    c1 = LLPoolLayer(Source=enc, MapCount=[5, 1], WeightsScale=64, Weights=w["Weights_0"], **networks.MNIST_CONV)
    a3 = SquareActivation(Source=LLVectorizeLayer(Source=c1))
    d4 = LLDenseLayer(Source=a3, Bias=w["Biases_1"], Weights=w["Weights_1"], WeightsScale=64, InputFormat=EVectorFormat.dense, ForceDenseFormat=force)
    assert "LLDenseLayer" in _each_layer_at_a_level(d4, Factory, {"LLDenseLayer"})


def test_llpreconv_layer_at_a_level(tmp_path):
    from test_lola import image, lola_dense
    img = image(5)
    nz = np.nonzero(img)[0]
    tsv = tmp_path / "one_image.tsv"
    tsv.write_text("7\t784\t" + "\t".join("%d:%d" % (i, int(img[i])) for i in nz) + "\n")
    Factory = make_factory("gpu", primes=(34359771137, 34360754177), n=16384, dbc=60, gdbc=60, small_modulus_count=8, galois=True)
    _, net = lola_dense(Factory, str(tsv))
    pre = _layers(net)[2]
    assert type(pre).__name__ == "LLPreConvLayer"
    assert _each_layer_at_a_level(pre, Factory, {"LLPreConvLayer"}) == ["LLPreConvLayer"]


def test_one_network_top_scheduled_top_again():
    """the same LoLa object at the top level, under a schedule, at the top level again: exact each time; the top contexts' handles come back
    (the per-level plaintext weights live on the level contexts)"""
    from test_lola import PRIMES, int_logits, lola
    from cryptonets_amd import networks
    from cryptonets_amd.layers import ModSwitchLayer
    Factory = make_factory("gpu", primes=PRIMES, n=8192, galois=True)
    env = Factory.AllocateComputationEnv()
    img = np.where(np.random.default_rng(2).random(784) < 0.81, 0, np.random.default_rng(3).integers(1, 256, size=784)).astype(float)
    net = lola(Factory, img)
    reader = _layers(net)[0]
    exp = int_logits(img)
    M = env.bigFactor
    exp = [((v % M) - M) if (v % M) * 2 > M else (v % M) for v in exp]

    def run(head):
        reader.Features = img / 256.0
        head.PrepareNetwork()
        out = head.GetNext()
        got = [int(x) for x in out.GetColumn(0).DecryptFullPrecision(env)]
        limbs = out.Limbs
        out.Dispose()
        return got, limbs
    assert run(net) == (exp, env.Limbs)
    live = _top_handles(env)
    layers = _layers(net)
    last = len(layers) - 1
    sources = [p.Source for p in layers]
    head = networks.with_levels(net, [(last - 2, env.Limbs - 1), (last, env.Limbs - 2)])
    assert run(head) == (exp, env.Limbs - 2)
    for p, s in zip(layers, sources):                          # undo the rewiring: the same objects, the top-level chain again
        p.Source = s
    assert not any(isinstance(p, ModSwitchLayer) for p in _layers(net))
    assert run(net) == (exp, env.Limbs)
    assert _top_handles(env) == live


# ------------------------------------------------------------------ planned schedules end to end
def _budget(m, Factory):
    from cryptonets_amd.levels import min_budget
    return min_budget([m], Factory)


def test_cryptonets_mnist_planned_then_run_on_other_records():
    from test_cryptonets_mnist import build_network, int_model_mod_p, synthetic_images, weights
    from cryptonets_amd import cryptonets_mnist as cm
    from cryptonets_amd import networks
    from cryptonets_amd.levels import plan_levels
    Factory = make_factory("gpu", primes=cm.PLAIN_PRIMES, n=cm.N, galois=False)
    env = Factory.AllocateComputationEnv()
    net, _ = build_network(Factory, synthetic_images(64, seed=21))
    net.PrepareNetwork()
    net.GetNext().Dispose()                      # the layers plan their GEMMs and upload their plaintexts at the top level once
    live = _top_handles(env)
    plan = plan_levels(net, Factory, records=1, margin_bits=8)
    print(plan)
    assert _top_handles(env) == live             # the planner frees every ciphertext it made
    assert plan.final_budget >= 8 and plan.tail_runs >= 0
    images = synthetic_images(64, seed=22)                               # other records
    _layers(net)[0].data = images
    head = networks.with_levels(net, plan.schedule)
    head.PrepareNetwork()
    out = head.GetNext()
    assert _budget(out, Factory) >= 1
    L = cm.layer_tables(*weights())
    x_int = np.rint(images / 256.0 * 16.0).astype(np.int64)
    lenv = env.Level(out.Limbs)
    for i, e in enumerate(lenv.Environments):
        model = int_model_mod_p(x_int, L, e.plainmodulusValue)
        for c in range(10):
            got = np.array(out.GetColumn(c).eVectors[i]._decrypt_ints(e), dtype=np.uint64)
            assert np.array_equal(got, model[:, c]), (c, e.plainmodulusValue)
    out.Dispose()


def test_lola_mnist_planned_then_run_on_other_records():
    from test_lola import PRIMES, int_logits, lola
    from cryptonets_amd import networks
    from cryptonets_amd.levels import plan_levels
    Factory = make_factory("gpu", primes=PRIMES, n=8192, galois=True)
    env = Factory.AllocateComputationEnv()
    cal = np.where(np.random.default_rng(30).random(784) < 0.81, 0, np.random.default_rng(31).integers(1, 256, size=784)).astype(float)
    net = lola(Factory, cal)
    plan = plan_levels(net, Factory, records=1, margin_bits=8)
    print(plan)
    head = networks.with_levels(net, plan.schedule)
    reader = _layers(net)[0]
    M = env.bigFactor
    for seed in (32, 33):
        img = np.where(np.random.default_rng(seed).random(784) < 0.81, 0, np.random.default_rng(seed + 10).integers(1, 256, size=784)).astype(float)
        reader.Features = img / 256.0
        out = head.GetNext()
        assert _budget(out, Factory) >= 1
        exp = [((v % M) - M) if (v % M) * 2 > M else (v % M) for v in int_logits(img)]
        assert [int(x) for x in out.GetColumn(0).DecryptFullPrecision(env)] == exp
        out.Dispose()


def test_lola_cifar_9_limbs_planned_after_the_first_square():
    from cryptonets_amd import networks
    from cryptonets_amd.levels import plan_levels
    from test_lola_cifar import PRIMES, mulmod
    rng = np.random.default_rng(5)
    Factory = make_factory("gpu", primes=PRIMES, n=16384, dbc=60, gdbc=60, small_modulus_count=9, galois=True)
    env = Factory.AllocateComputationEnv()
    w0 = np.rint(rng.normal(0, 0.05, 83 * 192) * 256) / 256
    b0 = np.rint(rng.normal(0, 0.05, 83) * 256) / 256
    w1 = np.rint(rng.normal(0, 0.02, 112 * 8300) * 512) / 512
    b1 = np.rint(rng.normal(0, 0.05, 112) * 512) / 512
    w2 = np.rint(rng.normal(0, 0.05, 10 * 5488) * 512) / 512
    b2 = np.rint(rng.normal(0, 0.05, 10) * 512) / 512
    reader = networks.cifar_reader(Factory=Factory)
    cal = rng.integers(0, 256, size=3 * 32 * 32).astype(float)
    reader.Features = cal / 256.0
    d6 = networks.LoLaCifar(Factory, reader, [w0, w1, w2], [b0, b1, b2], timing=False)
    layers = _layers(d6)
    sq = next(i for i, p in enumerate(layers) if type(p).__name__ == "SquareActivation")
    plan = plan_levels(d6, Factory, records=1, margin_bits=8, boundaries=range(sq, len(layers)))
    print(plan)
    assert all(b >= sq for b, _ in plan.schedule) and plan.final_budget >= 8
    head = networks.with_levels(d6, plan.schedule)
    img = rng.integers(0, 256, size=3 * 32 * 32).astype(float)
    reader.Features = img / 256.0
    out = head.GetNext()
    c1 = layers[2]
    W2i = np.rint(w2.reshape(10, 5488) * 512).astype(np.int64)
    s2 = ((8 * 256) ** 2 * 512) ** 2
    B2i = [int(round(float(b) * s2 * 512)) for b in b2]
    lenv = env.Level(out.Limbs)
    for i, e in enumerate(lenv.Environments):
        p = np.uint64(e.plainmodulusValue)
        a2 = networks.lola_cifar_dense_model(reader, c1, [w0, w1, w2], [b0, b1, b2], img, int(p))
        a2 = mulmod(a2, a2, p)
        W2p = np.mod(W2i, int(p)).astype(np.uint64)
        lg = np.zeros(10, dtype=np.uint64)
        for c0 in range(0, 5488, 512):
            lg = (lg + (mulmod(W2p[:, c0:c0 + 512], a2[None, c0:c0 + 512], p) % p).sum(axis=1) % p) % p
        lg = (lg + np.array([b % int(p) for b in B2i], dtype=np.uint64)) % p
        assert [int(v) for v in out.GetColumn(0).eVectors[i]._decrypt_ints(e)] == [int(v) for v in lg], "logits, prime %d" % int(p)
    out.Dispose()


# ------------------------------------------------------------------ recording
def test_recorded_evaluation_of_a_scheduled_chain_raises_before_capturing():
    from test_lola import PRIMES, lola
    from cryptonets_amd import networks
    Factory = make_factory("gpu", primes=PRIMES, n=8192, galois=True)
    env = Factory.AllocateComputationEnv()
    net = lola(Factory, np.zeros(784))
    head = networks.with_levels(net, [(len(_layers(net)) - 1, env.Limbs - 1)])
    launches = [e.ctx.stats()["kernel_launches"] for e in env.Environments]
    with pytest.raises(Exception, match="ModSwitchLayer"):
        networks.evaluate_single_recorded(head, Factory, records=2, report=None)
    assert [e.ctx.stats()["kernel_launches"] for e in env.Environments] == launches
