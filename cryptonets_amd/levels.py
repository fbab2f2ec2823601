"""Modulus-switching schedules for the networks: where, after which layer, the ciphertexts can drop to fewer coefficient moduli.

A SEAL user reads noise budgets and inserts mod_switch_to_next calls by hand.  `plan_levels` does it from measurements: it runs the chain
on calibration records, reads the noise budget after every layer (the minimum CryptoTracker.TestVectorBudget reads: SEAL's integer invariant noise budget,
on the device through cn_noise_norm), and descends greedily boundary by boundary.  Key switching costs about k^2 in the number of limbs k,
so every limb dropped early makes the later layers cheaper; switching cannot create budget, it only spends what the later layers leave.

    plan = plan_levels(network, Factory, records=1)
    head = networks.with_levels(network, plan.schedule)
"""
from .cryptotracker import INT_MAX
from .hewrapper import _env_at
from .layers import EncryptLayer

MAX_BACKOFF = 4


class LevelPlan:
    """schedule: [(boundary, limbs)] for networks.with_levels.  top / scheduled: per layer (position, layer name, limbs, min budget bits) at
    the top level and as scheduled (the scheduled trail includes the switches, named ModSwitch).  tail_runs: evaluations of the rest of the
    chain the descent needed; probes: switches measured without a tail run; backoffs: validation steps that raised the last switch."""

    def __init__(self, schedule, top, scheduled, tail_runs, probes=0, backoffs=0, margin_bits=8):
        self.schedule, self.top, self.scheduled = list(schedule), list(top), list(scheduled)
        self.tail_runs, self.probes, self.backoffs, self.margin_bits = tail_runs, probes, backoffs, margin_bits

    @property
    def final_budget(self):
        return self.scheduled[-1][3]

    def __str__(self):
        out = ["schedule %s  (margin %d bits; %d tail runs, %d switch probes, %d validation back-offs)"
               % (self.schedule or "none: top level throughout", self.margin_bits, self.tail_runs, self.probes, self.backoffs),
               "%-4s %-26s %6s %9s | %-26s %6s %9s" % ("pos", "top level", "limbs", "min bits", "as scheduled", "limbs", "min bits")]
        top = {p: (n, l, b) for p, n, l, b in self.top}
        for p, n, l, b in self.scheduled:
            t = top.get(p) if n != "ModSwitch" else None
            left = "%-26s %6d %9.1f" % t if t else "%-26s %6s %9s" % ("", "", "")
            out.append("%-4d %s | %-26s %6d %9.1f" % (p, left, n, l, b))
        return "\n".join(out)


def descend(oracle, boundaries, margin_bits=8):
    """The planner's logic over an `oracle` (the device one below, or a model in the CPU tests):
      oracle.trail() -> [(position, name, limbs, budget)] at the top level (budgets after the EncryptLayer onwards);
      oracle.advance(b): run the current intermediate up to the output of layer b;  oracle.probe(L): budget right after switching a copy of it
      to L limbs;  oracle.tail(L): final budget after switching a copy to L and running the rest of the chain;  oracle.accept(L): switch it;
      oracle.run(schedule) -> the scheduled trail (validation from the records).
    Returns a LevelPlan whose schedule passed validation; raises when no schedule within the back-off bound does."""
    top = oracle.trail()
    final_top = top[-1][3]
    if final_top < margin_bits:
        raise Exception("plan_levels: the top level leaves %.1f bits, below the margin of %d: no schedule can help" % (final_top, margin_bits))
    budget_at = {p: b for p, _, _, b in top}
    last = top[-1][0]
    cur = top[0][2]
    schedule, tail_runs, probes = [], 0, 0
    for b in boundaries:
        if cur <= 1:
            break
        oracle.advance(b)
        rest = budget_at[b] - final_top                        # what the layers after b consumed in the top-level trail
        # cheap prefilter (switch and probe, no tail run): a level whose budget right after the switch is below that cannot pass.  The
        # budget does not increase as the level falls, so the candidates that survive are cur-1 down to some lo.
        lo = cur
        for L in range(cur - 1, 0, -1):
            probes += 1
            if oracle.probe(L) < rest + (margin_bits if b == last else 0):
                break
            lo = L
        if lo == cur:
            continue
        if b == last:                                          # the reply level: the probe is the final budget
            best = lo
        else:                                                  # bisection for the lowest passing level among lo .. cur-1
            best, hi_l, lo_l = None, cur - 1, lo
            while lo_l <= hi_l:
                mid = (lo_l + hi_l) // 2
                tail_runs += 1
                if oracle.tail(mid) >= margin_bits:
                    best, hi_l = mid, mid - 1
                else:
                    lo_l = mid + 1
            if best is None:
                continue
        oracle.accept(best)
        schedule.append((b, best))
        cur = best
    # validation: the whole scheduled chain once from the records; back off the last switch while it fails
    backoffs = 0
    while True:
        trail = oracle.run(schedule)
        if trail[-1][3] >= margin_bits:
            return LevelPlan(schedule, top, trail, tail_runs, probes, backoffs, margin_bits)
        if not schedule:
            raise Exception("plan_levels: the top-level chain leaves %.1f bits on validation, below the margin of %d" % (trail[-1][3], margin_bits))
        if backoffs == MAX_BACKOFF:
            raise Exception("plan_levels: no validated schedule after %d back-offs (last %s leaves %.1f bits)" % (backoffs, schedule, trail[-1][3]))
        backoffs += 1
        b, L = schedule[-1]
        above = schedule[-2][1] if len(schedule) > 1 else top[0][2]
        schedule = schedule[:-1] + ([(b, L + 1)] if L + 1 < above else [])


def min_budget(ms, Factory):
    """the lowest noise budget (bits) over every ciphertext and plaintext prime of the matrices `ms`, each measured at its own level - what
    CryptoTracker.TestVectorBudget reads column by column, but with one device probe (cn_noise_norm) per contiguous range of one handle per
    plaintext prime instead of one per column; host-side clients are probed ciphertext by ciphertext (the tracker's watermark is untouched)"""
    best, columns = INT_MAX, 0
    for m in ms:
        env = _env_at(Factory.AllocateComputationEnv(), m.Limbs)
        ranges = {}                                                    # prime -> (environment, [(handle, first, count)])
        for col in m.leVectors:
            columns += 1
            for p, (atom, e) in enumerate(zip(col.eVectors, env.Environments)):
                d = atom.encData
                if d is None:
                    continue
                if hasattr(e.client, "noise_budget"):
                    ranges.setdefault(p, (e, []))[1].append((d.h, d.first, d.count))
                elif hasattr(e.client, "noise_budget_words"):
                    best = min([best] + [int(e.client.noise_budget_words(w)) for w in e.ctx.ct_download(d.h, d.first, d.count)])
        for e, rs in ranges.values():
            for h, first, count in _contiguous(rs):
                best = min([best] + [int(b) for b in e.client.noise_budget(h, first, count)])
    if not columns:
        raise ValueError("min_budget of no ciphertexts")
    return float(best)


def _contiguous(ranges):
    """(handle, first, count) ranges merged where they touch or overlap within one handle"""
    out = []
    for h, first, count in sorted(ranges, key=lambda r: (r[0], r[1])):
        if out and out[-1][0] == h and first <= out[-1][1] + out[-1][2]:
            h0, f0, c0 = out[-1]
            out[-1] = (h0, f0, max(c0, first + count - f0))
        else:
            out.append((h, first, count))
    return out


class _DeviceOracle:
    """descend()'s oracle on a real chain: the calibration records are encrypted once (one matrix per record) and every run starts from
    copies of them; layers are applied directly (Apply), so nothing of the chain is rewired and every intermediate is disposed here."""

    def __init__(self, network, Factory, records):
        from .networks import _chain
        layers = list(_chain(network))[::-1]
        k = next(i for i, p in enumerate(layers) if isinstance(p, EncryptLayer))
        self.layers, self.k, self.Factory = layers, k, Factory
        for p in layers:
            p.Factory = Factory
        network.PrepareNetwork()
        self.inputs = []
        for _ in range(int(records)):
            m = layers[k].GetNext()
            if m is None:
                break
            self.inputs.append(m)
        if not self.inputs:
            raise Exception("plan_levels: the reader gave no calibration record")
        self.state, self.pos = None, k

    def _env(self, m):
        return _env_at(self.Factory.AllocateComputationEnv(), m.Limbs)

    def budget(self, ms):
        return min_budget(ms, self.Factory)

    def _copy(self, m):
        from .hewrapper import EncryptedSealBfvMatrix, EncryptedSealBfvVector
        env = self._env(m)
        r = EncryptedSealBfvMatrix(Format=m.Format)
        r.leVectors = [EncryptedSealBfvVector.Copy(c, env) for c in m.leVectors]
        return r

    def _apply(self, ms, start, stop, schedule=(), trail=None):
        """run layers start+1 .. stop on the matrices `ms` (consumed), switching where `schedule` says; returns the outputs"""
        sw = dict(schedule)
        for p in range(start + 1, stop + 1):
            L = self.layers[p]
            ms = [self._step(L, m) for m in ms]
            if trail is not None:
                trail.append((p, type(L).__name__, ms[0].Limbs, self.budget(ms)))
            if p in sw:
                ms = [self._switch(m, sw[p]) for m in ms]
                if trail is not None:
                    trail.append((p, "ModSwitch", sw[p], self.budget(ms)))
        return ms

    @staticmethod
    def _step(L, m):
        y = L.Apply(m)
        if y is not m:
            m.Dispose()
        return y

    def _switch(self, m, limbs):
        y = m.ModSwitchTo(limbs, self._env(m))
        m.Dispose()
        return y

    def _dispose(self, ms):
        for m in ms or ():
            m.Dispose()

    def trail(self):
        k = self.k
        top = [(k, "EncryptLayer", self.inputs[0].Limbs, self.budget(self.inputs))]
        self._dispose(self._apply([self._copy(m) for m in self.inputs], k, len(self.layers) - 1, trail=top))
        self.state, self.pos = [self._copy(m) for m in self.inputs], k
        return top

    def advance(self, b):
        self.state = self._apply(self.state, self.pos, b)
        self.pos = b

    def probe(self, L):
        ms = [self._switch(self._copy(m), L) for m in self.state]
        try:
            return self.budget(ms)
        finally:
            self._dispose(ms)

    def tail(self, L):
        ms = self._apply([self._switch(self._copy(m), L) for m in self.state], self.pos, len(self.layers) - 1)
        try:
            return self.budget(ms)
        finally:
            self._dispose(ms)

    def accept(self, L):
        self.state = [self._switch(m, L) for m in self.state]

    def run(self, schedule):
        k = self.k
        trail = [(k, "EncryptLayer", self.inputs[0].Limbs, self.budget(self.inputs))]
        ms = [self._copy(m) for m in self.inputs]
        if k in dict(schedule):
            ms = [self._switch(m, dict(schedule)[k]) for m in ms]
            trail.append((k, "ModSwitch", dict(schedule)[k], self.budget(ms)))
        self._dispose(self._apply(ms, k, len(self.layers) - 1, schedule, trail))
        return trail

    def close(self):
        self._dispose(self.state)
        self._dispose(self.inputs)
        self.state = self.inputs = None


def plan_levels(network, Factory, records, margin_bits=8, boundaries=None):
    """Plan a modulus-switching schedule for the chain ending in `network` from `records` calibration records read through its reader
    (CryptoTracker budgets need a factory whose clients measure them: the device client or a host client).  `boundaries`: the positions
    (in networks._chain order, reader = 0) after which a switch may go - default every layer from the EncryptLayer on, the last one
    included (the reply level).  The descent is greedy, boundary by boundary, lowest passing level by bisection (the final budget does not
    increase as the level falls), with a cheap probe that skips levels whose budget right after the switch is already below what the rest of
    the chain consumes; the result is validated by one run of the whole scheduled chain (final budget >= margin_bits), backing off the last
    switch a bounded number of times.  Changes no option, key or layer wiring; frees every ciphertext it allocates (the layers keep their
    per-level plaintext weights and GEMM plans, made once per level, as they keep the top level's)."""
    oracle = _DeviceOracle(network, Factory, records)
    try:
        if boundaries is None:
            boundaries = range(oracle.k, len(oracle.layers))
        boundaries = sorted(int(b) for b in boundaries)
        if any(not oracle.k <= b < len(oracle.layers) for b in boundaries):
            raise ValueError("plan_levels: boundaries must lie in %d..%d" % (oracle.k, len(oracle.layers) - 1))
        return descend(oracle, boundaries, margin_bits)
    finally:
        oracle.close()
