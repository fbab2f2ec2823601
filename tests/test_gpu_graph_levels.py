"""GPU: recording across levels (cn_graph_begin_levels) - a chain that switches levels recorded into one graph on the first-level context and
replayed word for word like the eager chain, the launch ordering against the level contexts' streams, the refusals, the lifetime of the
members' arrays, and LoLa-MNIST recorded under a modulus-switching schedule."""
import numpy as np
import pytest

from modswitch_model import switch_residues
from test_gpu_mod_switch import keyed, level_oracle

pytestmark = pytest.mark.gpu

STEP0, STEP1 = 3, -5


class Chain:
    """c4: mul_plain + rotate_rows at 5 limbs -> switch to 4 -> rotate_rows_add + mul_relin at 4 -> switch to 2 -> add at 2"""

    def __init__(self, f64, ks_xi):
        self.o, self.g = keyed("c4", f64=f64, ks_xi=ks_xi)
        g = self.g
        self.lv4, self.lv2 = g.level(4), g.level(2)
        rng = np.random.default_rng(21)
        self.plain_vals = rng.integers(0, 4, size=g.n, dtype=np.uint64)
        self.plain = self.o.encode(self.plain_vals)
        self.pt = g.pt_alloc(1)
        g.pt_upload(self.pt, 0, self.plain[None, :])
        self.x, self.a, self.b = g.ct_alloc(1), g.ct_alloc(1), g.ct_alloc(1)
        self.c, self.d, self.e = self.lv4.ct_alloc(1), self.lv4.ct_alloc(1), self.lv4.ct_alloc(1)
        self.f, self.out = self.lv2.ct_alloc(1), self.lv2.ct_alloc(1)

    def run(self):
        g, lv4, lv2 = self.g, self.lv4, self.lv2
        g.mul_plain(self.x, 0, self.pt, 0, self.a, 0, 1, pt_stride=0)
        g.rotate_rows(self.a, 0, STEP0, self.b, 0)
        g.mod_switch(self.b, 0, 1, lv4, self.c, 0)
        lv4.rotate_rows_add(self.c, 0, STEP1, self.c, 0, self.d, 0)
        lv4.mul_relin(self.d, 0, self.d, 0, self.e, 0)
        lv4.mod_switch(self.e, 0, 1, lv2, self.f, 0)
        lv2.add(self.f, 0, self.f, 0, self.out, 0)

    def inputs(self, count, seed):
        """(plaintext slot values, ciphertexts of them under this chain's keys)"""
        rng = np.random.default_rng(seed)
        vals = rng.integers(0, 8, size=(count, self.g.n), dtype=np.uint64)
        return vals, [self.o.encrypt(self.o.encode(v)) for v in vals]

    def eager(self, cts):
        """the chain run call by call on every input (the first run is also the rehearsal of a recording)"""
        out = []
        for ct in cts:
            self.g.ct_upload(self.x, 0, ct[None, :])
            self.run()
            out.append(self.lv2.ct_download(self.out, 0, 1)[0])
        return out

    def slots(self, words):
        """slots of a level-2 result, decrypted on the host with the slice of the secret key"""
        lo2 = level_oracle(self.o, "c4", 2, galois=False)
        return lo2.decode(lo2.decrypt(words))

    def usage(self):
        """live handles and cached pool arrays of the three contexts"""
        return [(c.live_handles(), c.get_option("pool_arrays")) for c in (self.g, self.lv4, self.lv2)]


def oracle_chain(o, ct, plain):
    """the same chain on the CPU oracle over q and its prefixes (sliced keys; ks_xi = 0)"""
    q, n = o.q, o.n
    lo4, lo2 = level_oracle(o, "c4", 4), level_oracle(o, "c4", 2, galois=False)
    b = o.rotate_rows(o.multiply_plain(ct, plain), STEP0)
    c = switch_residues(b[None, :], q, n, 4).reshape(-1)
    d = lo4.add(c, lo4.rotate_rows(c, STEP1))
    e = lo4.mul_relin_batch(d[None, :], d[None, :])[0]
    f = switch_residues(e[None, :], q[:4], n, 2).reshape(-1)
    return lo2.add(f, f)


def refused(call):
    from cryptonets_amd._native import CnError
    with pytest.raises(CnError) as e:
        call()
    assert e.value.code == -1


@pytest.mark.parametrize("f64,ks_xi", [(True, False), (False, False), (True, True), (False, True)])
def test_recorded_chain_across_levels_equals_the_eager_chain(f64, ks_xi):
    ch = Chain(f64, ks_xi)
    g, lv4, lv2 = ch.g, ch.lv4, ch.lv2
    vals, cts = ch.inputs(4, seed=5)
    eager = ch.eager(cts)
    if not ks_xi:                                    # word for word against the prefix oracle
        assert np.array_equal(eager[1], oracle_chain(ch.o, cts[1], ch.plain))
    # the slots: those of the prefix oracle's chain (ks_xi = 0, its own keys) on the same plaintexts
    from conftest import get_oracle
    o = get_oracle("c4", galois=True)
    ref = oracle_chain(o, o.encrypt(o.encode(vals[1])), o.encode(ch.plain_vals))
    lo2 = level_oracle(o, "c4", 2, galois=False)
    assert np.array_equal(ch.slots(eager[1]), lo2.decode(lo2.decrypt(ref)))
    src = g.ct_alloc(3)
    g.ct_upload(src, 0, np.stack(cts[1:]))
    g.ct_upload(ch.x, 0, cts[0][None, :])
    g.graph_begin(levels=[lv4, lv2])
    try:
        ch.run()
    finally:
        graph = g.graph_end()
    launches = [c.stats()["kernel_launches"] for c in (g, lv4, lv2)]
    for i in (0, 1, 2):
        g.copy(src, i, ch.x, 0, 1)
        g.graph_launch(graph)
        assert np.array_equal(lv2.ct_download(ch.out, 0, 1)[0], eager[i + 1]), i
    after = [c.stats()["kernel_launches"] for c in (g, lv4, lv2)]
    assert after[1:] == launches[1:]                 # nothing launched on the level contexts
    assert 3 <= after[0] - launches[0] <= 6          # one graph launch (+ the input copy) per replay
    g.free(graph)


def test_launch_is_ordered_against_the_level_contexts():
    ch = Chain(True, False)
    g, lv4, lv2 = ch.g, ch.lv4, ch.lv2
    _, cts = ch.inputs(3, seed=6)
    eager = ch.eager(cts)
    src = g.ct_alloc(3)
    g.ct_upload(src, 0, np.stack(cts))
    g.graph_begin(levels=[lv2, lv4])                 # (any order)
    ch.run()
    graph = g.graph_end()
    # a download on the level context right behind the launch, no cn_sync between: the result of that launch
    g.copy(src, 1, ch.x, 0, 1)
    g.graph_launch(graph)
    assert np.array_equal(lv2.ct_download(ch.out, 0, 1)[0], eager[1])
    # two launches back to back with an eager level-2 read of the result queued between them: the read sees the first replay
    snap = lv2.ct_alloc(1)
    g.copy(src, 2, ch.x, 0, 1)
    g.graph_launch(graph)
    lv2.copy(ch.out, 0, snap, 0, 1)
    g.copy(src, 0, ch.x, 0, 1)
    g.graph_launch(graph)
    assert np.array_equal(lv2.ct_download(snap, 0, 1)[0], eager[2])
    assert np.array_equal(lv2.ct_download(ch.out, 0, 1)[0], eager[0])
    g.free(graph)


def test_refusals_leave_root_and_members_usable():
    from cryptonets_amd._native import Context
    ch = Chain(True, False)
    g, lv4, lv2 = ch.g, ch.lv4, ch.lv2
    _, cts = ch.inputs(1, seed=7)
    want = ch.eager(cts)[0]
    foreign = Context(g.n, 65537, q=g.q, dbc=10, gdbc=20, device=0)                       # another t
    other = Context(g.n, g.t, q=[g.q[1], g.q[0]] + g.q[2:], dbc=10, gdbc=20, device=0)     # another chain
    for levels in ([foreign.level(2)], [g], [lv4, lv4], [lv4, other.level(2)], [other]):
        refused(lambda: g.graph_begin(levels=levels))
    lv4.add(ch.c, 0, ch.c, 0, ch.d, 0)
    lv4.graph_begin()                                                                     # a member that is already recording
    lv4.add(ch.c, 0, ch.c, 0, ch.d, 0)
    refused(lambda: g.graph_begin(levels=[lv4, lv2]))
    lv4.free(lv4.graph_end())
    g.graph_begin(levels=[lv4])
    try:
        refused(lambda: g.graph_begin(levels=[lv2]))                                      # the root is recording
        refused(lambda: lv2.graph_begin(levels=[lv4]))                                    # lv4 is a member of a recording
        refused(lambda: g.mod_switch(ch.b, 0, 1, lv2, ch.f, 0))                           # a switch to a non-member
        refused(lambda: lv4.mod_switch(ch.c, 0, 1, lv2, ch.f, 0))                         # ... from a member
        refused(lambda: lv4.sync())
        refused(lambda: lv4.ct_upload(ch.c, 0, np.zeros((1, 2 * 4 * g.n), dtype=np.uint64)))
        refused(lambda: lv4.ct_download(ch.c, 0, 1))
        refused(lambda: lv4.graph_end())
        refused(lambda: lv4.graph_begin())
        refused(lambda: lv4.close())                                                      # a member of a running recording
        g.mod_switch(ch.b, 0, 1, lv4, ch.c, 0)                                            # recorded
    finally:
        graph = g.graph_end()
    refused(lambda: lv4.close())                                                          # its graph is alive
    g.graph_launch(graph)
    g.free(graph)
    g.graph_begin()                                                                       # plain cn_graph_begin still refuses every switch
    try:
        refused(lambda: g.mod_switch(ch.b, 0, 1, lv4, ch.c, 0))
    finally:
        g.free(g.graph_end())
    assert ch.eager(cts)[0].tolist() == want.tolist()                                     # root and members usable, the same words
    lv2.sync()
    lv4.close()                                                                           # accepted once the graph is freed
    foreign.close()
    other.close()


def test_members_arrays_return_when_the_graph_is_freed():
    ch = Chain(True, False)
    g, lv4, lv2 = ch.g, ch.lv4, ch.lv2
    _, cts = ch.inputs(1, seed=8)
    ch.eager(cts)
    before = ch.usage()
    g.graph_begin(levels=[lv4, lv2])
    ch.run()
    graph = g.graph_end()
    g.graph_launch(graph)
    alive = ch.usage()
    assert [h for h, _ in alive] == [before[0][0] + 1, before[1][0], before[2][0]]      # + the graph's handle on the root
    assert all(p1 <= p0 for (_, p0), (_, p1) in zip(before, alive))
    g.free(graph)
    assert ch.usage() == before


def test_lola_mnist_recorded_under_a_schedule():
    """LoLa-MNIST with the schedule the probe plans: the recorded scheduled chain decrypts to the unrecorded scheduled chain's logits and the
    integer model's; a replay adds one launch per prime on the first level (besides the input copies) and none on the levels"""
    from test_lola import PRIMES, image, int_logits, lola
    from cryptonets_amd import networks
    from cryptonets_amd.hewrapper import CapturedEvaluation, EncryptedSealBfvFactory
    schedule = [(5, 4), (6, 3), (8, 2), (9, 1)]
    Factory = EncryptedSealBfvFactory(list(PRIMES), 8192, 10, 20, -1, galois=True, client_seed=1234)
    env = Factory.AllocateComputationEnv()
    imgs = [image(3), image(4), image(5), image(6)]
    net = lola(Factory, imgs[0])
    head = networks.with_levels(net, schedule)
    head.PrepareNetwork()
    layers = list(networks._chain(head))[::-1]
    reader, encrypt = layers[0], layers[1]
    M = env.bigFactor

    def centred(v):
        return [((x % M) - M) if (x % M) * 2 > M else (x % M) for x in v]

    def encrypted(img):
        reader.Features = np.asarray(img) / 256.0
        return encrypt.Apply(reader.GetNext())

    def evaluate(x, keep):
        for L in layers[2:]:
            y = L.Apply(x)
            if y is not x and x is not keep:
                x.Dispose()
            x = y
        return x

    def logits(m):
        return [int(v) for v in m.GetColumn(0).DecryptFullPrecision(env)]

    unrecorded = []
    for img in imgs:
        y = evaluate(encrypted(img), None)
        assert y.Limbs == 1
        unrecorded.append(logits(y))
        y.Dispose()
    assert unrecorded == [centred(int_logits(img)) for img in imgs]
    first = encrypted(imgs[0])
    evaluate(first, first).Dispose()                 # rehearsal
    cap = CapturedEvaluation(env, lambda x: evaluate(x, first), [first])
    levels = [lv.ctx for e in env.Environments for lv in e._levels.values()]
    assert len(levels) == 4 * len(PRIMES)
    copies = None
    for i in (1, 2, 3):
        fresh = encrypted(imgs[i])
        top = [e.ctx.stats()["kernel_launches"] for e in env.Environments]
        low = [c.stats()["kernel_launches"] for c in levels]
        out = cap.run(fresh)
        added = [e.ctx.stats()["kernel_launches"] - t for e, t in zip(env.Environments, top)]
        assert [c.stats()["kernel_launches"] for c in levels] == low
        copies = added if copies is None else copies
        assert added == copies and all(a - 1 in (0, len(first.leVectors)) for a in added), added     # the graph + the input copies
        assert logits(out) == unrecorded[i]
        fresh.Dispose()
    cap.result.Dispose()
    cap.Dispose()
    first.Dispose()
    # through the network driver, on a reader of three records: the schedule applied, rehearsed, recorded and replayed - and the chain
    # wired back as it was
    import tempfile
    from test_lola import GOLD
    with tempfile.TemporaryDirectory() as tmp:
        tsv = tmp + "/three.tsv"
        with open(tsv, "w") as f:
            for img in imgs[1:]:
                f.write("7\t784\t" + "\t".join("%d:%d" % (i, int(img[i])) for i in np.nonzero(img)[0]) + "\n")
        net2 = networks.LoLa(Factory, networks.lola_reader("LoLa", tsv, Factory=Factory), np.load(GOLD))
        lines = []
        errs, count = networks.evaluate_single_recorded(net2, Factory, 3, report=lines.append, schedule=schedule)
    assert count == 3 and sum("(recorded)" in s for s in lines) == 2, lines
    assert [int(s.split("prediction ")[1].split()[0]) for s in lines] == [int(np.argmax(u[:10])) for u in unrecorded[1:]]
    assert not any(isinstance(p, networks.ModSwitchLayer) for p in networks._chain(net2))
