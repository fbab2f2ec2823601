"""Modulus-switching schedules on the CPU: the exact-FP64 switch kernel in the gfx950 code object, networks.with_levels rewiring a chain,
and the planner's descent (levels.descend) over a model of the noise budget - no device."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "cryptonets_amd", "lib", "obj")


# ------------------------------------------------------------------ the FP64 switch kernel
# k_mod_switch_f64<KS, KD>: two coefficients x KS limbs as doubles; at <= 64 VGPRs a SIMD holds 8 waves (measured 36, 34, 50, 68, 60 VGPRs)
MS_F64_BUDGETS = [(5, 4, 64), (5, 2, 64), (8, 1, 64), (9, 6, 96), (9, 1, 64)]


def _resources(obj):
    from cryptonets_amd import _native
    _native.build()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    return kernel_resources, kernel_resources.resources(os.path.join(OBJ, obj))


@pytest.mark.parametrize("ks,kd,budget", MS_F64_BUDGETS)
def test_fp64_mod_switch_kernel_in_code_object_within_budget(ks, kd, budget):
    _, res = _resources("cn_l_modswitch_f64.o")
    cand = [k for k in res if k.startswith("void k_mod_switch_f64<%d, %d>" % (ks, kd))]
    assert cand, "k_mod_switch_f64<%d, %d> not in the gfx950 code object" % (ks, kd)
    r = res[cand[0]]
    assert r["vgpr_spill"] == 0 and r["scratch"] == 0, r
    assert r["vgpr"] + r["agpr"] <= budget, (cand[0], r)


def test_fp64_mod_switch_kernel_covers_every_pair():
    _, res = _resources("cn_l_modswitch_f64.o")
    pairs = {tuple(int(x) for x in re.match(r"void k_mod_switch_f64<(\d+), (\d+)>", k).groups()) for k in res if k.startswith("void k_mod_switch_f64<")}
    assert pairs == {(ks, kd) for ks in range(2, 13) for kd in range(1, ks)}


def test_fp64_mod_switch_kernel_uses_global_not_flat_memory_instructions():
    kr, _ = _resources("cn_l_modswitch_f64.o")
    assert not kr.flat_instructions(os.path.join(OBJ, "cn_l_modswitch_f64.o"))


def test_fp64_mod_switch_diagnostic_is_documented_and_read_only():
    src = open(os.path.join(ROOT, "cryptonets_amd", "csrc", "cn_api.hip")).read()
    rows = [line for line in src.split("\n") if '{"mod_switch_f64",' in line]
    assert len(rows) == 1 and "nullptr}," in rows[0]        # a row of cn_get_option's table of values, without a setter
    assert '"mod_switch_f64"' not in open(os.path.join(ROOT, "cryptonets_amd", "csrc", "cn_options.h")).read()      # not a tunable of the option table
    assert '"mod_switch_f64"' in open(os.path.join(ROOT, "include", "cnhip.h")).read()


# ------------------------------------------------------------------ with_levels
def _stub_chain(n_after=4):
    """reader -> EncryptLayer -> n_after pass-through layers (InputLayer-style stubs: nothing runs)"""
    from cryptonets_amd.layers import BaseLayer, EncryptLayer, InputLayer
    reader = InputLayer([[1.0]])
    enc = EncryptLayer(Source=reader)
    layers, src = [reader, enc], enc
    for _ in range(n_after):
        src = BaseLayer(Source=src)
        layers.append(src)
    return layers


def _names(head):
    from cryptonets_amd.networks import _chain
    return [(type(p).__name__, getattr(p, "Limbs", None) if type(p).__name__ == "ModSwitchLayer" else None) for p in _chain(head)][::-1]


def test_with_levels_inserts_switches_after_the_named_layers():
    from cryptonets_amd.layers import ModSwitchLayer
    from cryptonets_amd.networks import with_levels
    layers = _stub_chain(4)
    head = with_levels(layers[-1], [(2, 4), (4, 2)])
    assert head is layers[-1]
    assert _names(head) == [("InputLayer", None), ("EncryptLayer", None), ("BaseLayer", None), ("ModSwitchLayer", 4), ("BaseLayer", None),
                            ("BaseLayer", None), ("ModSwitchLayer", 2), ("BaseLayer", None)]
    assert isinstance(layers[3].Source, ModSwitchLayer) and layers[3].Source.Source is layers[2]      # rewired, not copied
    assert isinstance(layers[5].Source, ModSwitchLayer) and layers[5].Source.Source is layers[4]


def test_with_levels_switch_after_the_last_layer_is_the_reply_level():
    from cryptonets_amd.layers import ModSwitchLayer
    from cryptonets_amd.networks import with_levels
    layers = _stub_chain(3)
    head = with_levels(layers[-1], [(1, 3), (4, 1)])
    assert isinstance(head, ModSwitchLayer) and head.Limbs == 1 and head.Source is layers[-1]
    assert _names(head)[2] == ("ModSwitchLayer", 3)
    chain = _stub_chain(2)
    assert with_levels(chain[-1], []) is chain[-1]


@pytest.mark.parametrize("schedule", [[(2, 3), (3, 3)], [(2, 3), (3, 4)], [(3, 2), (2, 1)], [(2, 3), (2, 2)], [(6, 2)], [(0, 2)], [(2, 0)]])
def test_with_levels_refuses_bad_schedules(schedule):
    from cryptonets_amd.networks import with_levels
    layers = _stub_chain(4)
    before = [p.Source for p in layers]
    with pytest.raises(ValueError):
        with_levels(layers[-1], schedule)
    assert [p.Source for p in layers] == before                  # nothing rewired


def test_modswitch_layer_refuses_a_level_not_below_the_input():
    from types import SimpleNamespace
    from cryptonets_amd.layers import ModSwitchLayer
    L = ModSwitchLayer(Source=None, Factory=SimpleNamespace(AllocateComputationEnv=lambda: None), Limbs=3)
    for limbs in (3, 2):
        with pytest.raises(Exception, match="not below"):
            L.Apply(SimpleNamespace(Limbs=limbs))
    with pytest.raises(Exception, match="not encrypted"):
        L.Apply(SimpleNamespace(Limbs=None))


def test_recorded_evaluation_refuses_a_scheduled_chain_before_anything_runs():
    from cryptonets_amd.networks import evaluate_single_recorded, with_levels
    layers = _stub_chain(3)
    head = with_levels(layers[-1], [(3, 2)])
    with pytest.raises(Exception, match="ModSwitchLayer"):
        evaluate_single_recorded(head, Factory=None, records=2)       # the Factory is never touched


# ------------------------------------------------------------------ the planner's descent on a budget model
class ModelOracle:
    """Top level `top` limbs; layer p consumes cost[p] bits; a level L holds at most L * per_limb - floor bits, so switching to L leaves
    min(budget, L * per_limb - floor).  Counts what the planner asks for.  `lie`: bits the validation run finds fewer than the tail runs did."""

    def __init__(self, costs, top=9, per_limb=49.0, floor=40.0, fresh=None, lie=0.0, lie_runs=99):
        self.costs, self.top, self.per_limb, self.floor, self.lie, self.lie_runs = costs, top, per_limb, floor, lie, lie_runs
        self.fresh = 361.0 if fresh is None else fresh          # the measured fresh budget at 9 limbs
        self.last = len(costs)                     # positions 0 (EncryptLayer) .. last
        self.tails = self.probes = self.runs = 0
        self.validated = []

    def cap(self, L):
        return L * self.per_limb - self.floor

    def _forward(self, b0, budget, start, stop, schedule):
        out = []
        sw = dict(schedule)
        for p in range(start + 1, stop + 1):
            budget -= self.costs[p - 1]
            if p in sw:
                budget = min(budget, self.cap(sw[p]))
            out.append(budget)
        return budget, out

    def trail(self):
        b, out, tr = self.fresh, [], [(0, "EncryptLayer", self.top, self.fresh)]
        for p in range(1, self.last + 1):
            b -= self.costs[p - 1]
            tr.append((p, "L%d" % p, self.top, b))
        self.state, self.pos, self.level = self.fresh, 0, self.top
        return tr

    def advance(self, b):
        self.state, _ = self._forward(None, self.state, self.pos, b, ())
        self.pos = b

    def probe(self, L):
        self.probes += 1
        return min(self.state, self.cap(L))

    def tail(self, L):
        self.tails += 1
        b, _ = self._forward(None, min(self.state, self.cap(L)), self.pos, self.last, ())
        return b

    def accept(self, L):
        self.state, self.level = min(self.state, self.cap(L)), L

    def run(self, schedule):
        self.runs += 1
        sw = dict(schedule)
        b = self.fresh if 0 not in sw else min(self.fresh, self.cap(sw[0]))
        tr, lvl = [(0, "EncryptLayer", self.top, b)], self.top
        for p in range(1, self.last + 1):
            b -= self.costs[p - 1]
            tr.append((p, "L%d" % p, lvl, b))
            if p in sw:
                lvl = sw[p]
                b = min(b, self.cap(lvl))
                tr.append((p, "ModSwitch", lvl, b))
        if self.runs <= self.lie_runs:
            b -= self.lie
            tr[-1] = tr[-1][:3] + (b,)
        self.validated.append((list(schedule), b))
        return tr


def test_descent_finds_the_lowest_passing_level_by_bisection():
    from cryptonets_amd.levels import descend
    costs = [9, 61, 53, 104, 53, 58]                   # the measured LoLa-CIFAR trail at 9 limbs
    o = ModelOracle(costs, top=9)
    plan = descend(o, [3], margin_bits=8)              # after the first square only
    # rest after the square = 104 + 53 + 58 = 215; lowest L with L * 49 - 40 - 215 >= 8: L = 6 (254 - 215 = 39); L = 5 leaves -10
    assert plan.schedule == [(3, 6)]
    assert plan.final_budget >= 8
    assert o.tails <= 3                                # bisection over the survivors of the probe, not a scan
    # the same answer a full scan of the tails gives
    scan = [L for L in range(1, 9) if min(o.fresh - sum(costs[:3]), o.cap(L)) - sum(costs[3:]) >= 8]
    assert min(scan) == 6


def test_descent_prefilter_skips_tails_of_levels_that_cannot_hold_the_rest():
    from cryptonets_amd.levels import descend
    costs = [9, 61, 53, 104, 53, 58]
    o = ModelOracle(costs, top=9)
    descend(o, [3], margin_bits=8)
    # level 5 holds 205 bits, below the 215 the rest consumed: probed out, and the probe loop stops there (levels 1..4 hold even less)
    assert o.probes == 4                              # 8, 7, 6 pass the probe; 5 fails and ends it
    assert o.tails <= 3
    o2 = ModelOracle(costs, top=9, per_limb=20.0)      # nothing below the top holds the rest: no tail run at all
    plan = descend(o2, [3], margin_bits=8)
    assert o2.tails == 0 and plan.schedule == []


def test_descent_greedy_over_several_boundaries_and_the_reply_level():
    from cryptonets_amd.levels import descend
    costs = [9, 61, 53, 104, 53, 58]
    o = ModelOracle(costs, top=9)
    plan = descend(o, range(0, 7), margin_bits=8)
    levels = [L for _, L in plan.schedule]
    assert levels == sorted(levels, reverse=True) and len(set(levels)) == len(levels)
    assert plan.final_budget >= 8
    assert o.validated[-1] == (plan.schedule, plan.final_budget)     # the returned plan is the one validation passed


def test_descent_validation_backs_off_the_last_switch():
    from cryptonets_amd.levels import descend
    costs = [9, 61, 53, 104, 53, 58]
    o = ModelOracle(costs, top=9, lie=40.0, lie_runs=1)   # the first validation finds 40 bits fewer than the tails promised
    plan = descend(o, [3], margin_bits=8)
    assert plan.backoffs == 1 and plan.schedule == [(3, 7)]
    assert [s for s, _ in o.validated] == [[(3, 6)], [(3, 7)]]
    assert o.validated[-1][1] >= 8 and plan.final_budget == o.validated[-1][1]


def test_descent_raises_after_its_bound_and_never_returns_an_unvalidated_plan():
    from cryptonets_amd import levels
    costs = [9, 61, 53, 104, 53, 58]
    o = ModelOracle(costs, top=9, per_limb=60.0, lie=1000.0)   # validation always fails
    with pytest.raises(Exception, match="back-off|margin"):
        levels.descend(o, [3, 4, 5], margin_bits=8)
    assert o.runs <= levels.MAX_BACKOFF + 1


def test_descent_refuses_a_chain_without_budget_at_the_top():
    from cryptonets_amd.levels import descend
    o = ModelOracle([9, 61, 53, 104, 53, 58, 100], top=9)
    with pytest.raises(Exception, match="top level"):
        descend(o, [3], margin_bits=8)


def test_level_plan_prints_its_trail():
    from cryptonets_amd.levels import descend
    o = ModelOracle([9, 61, 53, 104, 53, 58], top=9)
    text = str(descend(o, [3], margin_bits=8))
    assert "schedule [(3, 6)]" in text and "ModSwitch" in text and "EncryptLayer" in text
