#!/usr/bin/env python
"""Recorded evaluation under a modulus-switching schedule on one MI355X: LoLa-MNIST "Prediction-Time" per image (after encryption .. before
decryption, every stream of the first-level and level contexts synchronised) in four forms:

    unrecorded top level      the layers call by call at all limbs
    unrecorded scheduled      ... under the schedule (ModSwitchLayers, networks.with_levels)
    recorded top level        one HIP graph per plaintext prime (hewrapper.CapturedEvaluation), replayed per image
    recorded scheduled        one graph per prime recorded across its level contexts (cn_graph_begin_levels), replayed per image

    python tools/recorded_levels_probe.py [--records 50] [--rounds 3]

Each form is warmed up (and rehearsed / recorded) once, then the forms take turns for --rounds rounds of --records images each; prints the
median and range per form.  Every form's decrypted logits are checked against the integer model on the first two images of the first round.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LOLA_SCHEDULE = [(5, 4), (6, 3), (8, 2), (9, 1)]      # levels.plan_levels on LoLa-MNIST, margin 8 bits (profiles/level_schedule_probe.txt)


class Form:
    def __init__(self, name, Factory, make_net, schedule, recorded, check):
        from cryptonets_amd import networks
        from cryptonets_amd.hewrapper import CapturedEvaluation
        self.name, self.env, self.check = name, Factory.AllocateComputationEnv(), check
        net = make_net()
        head = networks.with_levels(net, schedule) if schedule else net
        head.PrepareNetwork()
        self.layers = list(networks._chain(head))[::-1]
        self.reader, self.encrypt = self.layers[0], self.layers[1]
        self.levels = [lv for _, lv in schedule]
        self.times = []
        self.cap = self.first = None
        self.first = self.encrypted(np.zeros(784))
        r = self.evaluate(self.first, self.first)                 # warm-up / rehearsal, decrypted as well: the arenas take their size before
        r.GetColumn(0).DecryptFullPrecision(self.env)              # a recording holds them
        r.Dispose()
        if recorded:
            self.cap = CapturedEvaluation(self.env, lambda x: self.evaluate(x, self.first), [self.first], levels=self.levels)

    def encrypted(self, img):
        self.reader.Features = np.asarray(img) / 256.0
        return self.encrypt.Apply(self.reader.GetNext())

    def evaluate(self, x, keep):
        for L in self.layers[2:]:
            y = L.Apply(x)
            if y is not x and x is not keep:
                x.Dispose()
            x = y
        return x

    def sync(self):
        for e in self.env.Environments:
            e.ctx.sync()
            for lv in self.levels:
                e.Level(lv).ctx.sync()

    def one(self, img, checked):
        x = self.encrypted(img)
        self.sync()
        t0 = time.perf_counter()
        y = self.cap.run(x) if self.cap else self.evaluate(x, None)
        self.sync()
        self.times.append(1e3 * (time.perf_counter() - t0))
        if checked:
            got = [int(v) for v in y.GetColumn(0).DecryptFullPrecision(self.env)]
            assert got == self.check(img), "%s: the logits differ from the integer model" % self.name
        if self.cap:
            x.Dispose()
        else:
            y.Dispose()

    def close(self):
        if self.cap:
            self.cap.result.Dispose()
            self.cap.Dispose()
        self.first.Dispose()


def probe(title, Factory, make_net, schedule, int_logits, records, rounds):
    M = Factory.AllocateComputationEnv().bigFactor

    def check(img):
        return [((v % M) - M) if (v % M) * 2 > M else (v % M) for v in int_logits(img)]
    forms = [Form("unrecorded top level", Factory, make_net, [], False, check),
             Form("unrecorded scheduled", Factory, make_net, schedule, False, check),
             Form("recorded top level", Factory, make_net, [], True, check),
             Form("recorded scheduled", Factory, make_net, schedule, True, check)]
    rng = np.random.default_rng(11)
    imgs = [np.where(rng.random(784) < 0.81, 0, rng.integers(1, 256, size=784)).astype(float) for _ in range(records)]
    for r in range(rounds):
        for f in forms:
            for i, img in enumerate(imgs):
                f.one(img, checked=(r == 0 and i < 2))
    print("# %s, schedule %s: Prediction-Time per image, %d rounds x %d images per form, forms alternating by round" % (title, schedule, rounds, records))
    print("%-24s %10s %10s %10s" % ("form", "median ms", "min ms", "max ms"))
    for f in forms:
        t = np.array(f.times)
        print("%-24s %10.2f %10.2f %10.2f" % (f.name, np.median(t), t.min(), t.max()), flush=True)
    for f in forms:
        f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from test_lola import PRIMES, int_logits, lola
    from cryptonets_amd.hewrapper import EncryptedSealBfvFactory
    F = EncryptedSealBfvFactory(list(PRIMES), 8192, 10, 20, -1, galois=True, client_seed=1234)
    probe("LoLa-MNIST (N = 8192, 5 limbs, 4 plaintext primes)", F, lambda: lola(F, np.zeros(784)), LOLA_SCHEDULE, int_logits, a.records, a.rounds)


if __name__ == "__main__":
    main()
