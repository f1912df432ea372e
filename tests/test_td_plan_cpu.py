"""No-GPU checks of TD learners inside step plans: the learn-then-reset oracle (tests/td_plan_oracle.py) by hand, the two new
entry points of the C ABI (riab_td_learn_step, riab_plan_set_learner) and their argument errors — the library loads
without a GPU and every error below comes back before anything is launched —, and the behaviour the rest of the package
relies on: `_population()` of a learning learner still refuses, `bind_reward` refuses what a step could not read."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import td_oracle as tdo
from tests import td_plan_oracle as tpo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


# ---- the oracle --------------------------------------------------------------------------------------------------
def test_batch_with_resets_is_single_lanes_restarted_at_the_masked_steps():
    """B = 3, masks that hit one lane, two lanes, nobody and everybody: every lane's V, dV/dt, td and trace equal those of
    a single-agent oracle that carries the batch's weights and is RESTARTED (fresh state) after each step its lane was
    masked in; the weights equal the by-hand mean of the three lanes' outer products, masked lanes included."""
    rng = np.random.RandomState(11)
    n, n_in, B, T = 2, 5, 3, 6
    w0 = rng.normal(size=(n, n_in)) * 0.3
    kw = dict(dt=0.05, tau=1.5, tau_e=0.4, eta=0.02, L2=0.003, activation="relu", gain=1.0, threshold=0.02)
    masks = [None, [True, False, False], [False, True, True], [False, False, False], [True, True, True], None]
    batch = tpo.PlanOracle([w0], B=B, **kw)
    V = [np.zeros((n, 1)) for _ in range(B)]              # what each single lane carries between steps
    E = [np.zeros((n_in, 1)) for _ in range(B)]
    for t in range(T):
        phi, r = rng.uniform(size=(n_in, B)), rng.normal(size=(n, B))
        w_before = batch.o.ws[0].copy()
        seen = batch.step([phi], r, masks[t])
        outer = []
        for b in range(B):
            s = tdo.TDOracle([w_before], B=1, **kw)
            s.V, s.traces = V[b].copy(), [E[b].copy()]
            s.update([phi[:, b]])
            s.update_weights(r[:, b])
            np.testing.assert_allclose(seen["V"][:, b], s.V[:, 0], rtol=1e-13)
            np.testing.assert_allclose(seen["dVdt"][:, b], s.dVdt[:, 0], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(seen["td"][:, b], s.td[:, 0], rtol=1e-12, atol=1e-13)
            outer.append(np.outer(s.td[:, 0] * s.prime[:, 0], s.traces[0][:, 0]))
            hit = masks[t] is not None and masks[t][b]
            V[b], E[b] = (np.zeros((n, 1)), np.zeros((n_in, 1))) if hit else (s.V.copy(), s.traces[0].copy())
            np.testing.assert_allclose(batch.o.traces[0][:, b], E[b][:, 0], rtol=1e-13)
            np.testing.assert_array_equal(batch.o.V[:, b], V[b][:, 0]) if hit else None
            if hit:
                assert not batch.o.td[:, b].any() and not batch.o.dVdt[:, b].any()
        by_hand = w_before + kw["dt"] * kw["eta"] * (outer[0] + outer[1] + outer[2]) / 3 - kw["eta"] * kw["dt"] * kw["L2"] * w_before
        np.testing.assert_allclose(batch.o.ws[0], by_hand, rtol=1e-12, atol=1e-15)
    # after the step that reset everybody the state is a fresh learner's with the weights learned so far
    fresh = tpo.PlanOracle([batch.o.ws[0]], B=B, **kw)
    again = tpo.PlanOracle([w0], B=B, **kw)
    rng = np.random.RandomState(11)
    for t in range(5):
        again.step([rng.uniform(size=(n_in, B))], rng.normal(size=(n, B)), masks[t])
    assert not again.o.V.any() and not again.o.traces[0].any() and fresh.o.ws[0].shape == again.o.ws[0].shape


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_prototyped_and_declared(L):
    src = open(HEADER).read()
    for s in ("riab_td_learn_step", "riab_plan_set_learner"):
        assert hasattr(L.lib, s) and s in L.PROTOTYPES, s
        assert re.search(r"^int " + s + r"\(", src, re.M), s
    assert len(L.PROTOTYPES["riab_td_learn_step"][1]) == 17 and len(L.PROTOTYPES["riab_plan_set_learner"][1]) == 15
    kinds = re.search(r"RIAB_REWARD_NONE = (\d).*?RIAB_REWARD_TASK = (\d).*?RIAB_REWARD_POINTER = (\d).*?RIAB_REWARD_POPULATION = (\d)",
                      src, re.S).groups()
    assert [int(k) for k in kinds] == [L.REWARD_NONE, L.REWARD_TASK, L.REWARD_POINTER, L.REWARD_POPULATION]
    # the step order of a plan with a learner is stated where riab_plan_set_task states today's
    doc = src[src.index("/* Attach a task (riab_task_*) to the plan"):src.index("int riab_plan_set_task(")]
    assert "LEARNS, THEN RESETS" in doc and "riab_td_learn_step" in doc


def _learner(L, **over):
    p = L.RiabTDParams()
    p.dt, p.tau, p.tau_e, p.eta, p.L2, p.B, p.Bp, p.n, p.Mp = 0.05, 1.0, 0.25, 0.01, 0.001, 5, 8, 2, 32
    for k, v in over.items():
        setattr(p, k, v)
    lay = (L.RiabTDLayer * 1)()
    lay[0].rates = lay[0].trace = lay[0].wt = 16
    lay[0].n_in = 8
    return p, lay


def test_learn_step_argument_errors_before_launch(L):
    ok = C.c_void_p(16)
    p, lay = _learner(L)
    need = L.lib.riab_td_workspace(p, lay, 1)

    def step(p, lay, n_layers=1, reward=ok, v=ok, v_last=ok, dvdt=ok, prime=ok, td=ok, ws=ok, floats=1 << 30, ld=(0, 0), f64=0):
        return L.lib.riab_td_learn_step(p, lay, n_layers, reward, f64, ld[0], ld[1], v, v_last, dvdt, prime, td, None, 1, ws,
                                        floats, None)

    assert step(None, lay) == L.EINVAL and step(p, None) == L.EINVAL
    assert step(_learner(L, Bp=6)[0], lay) == L.EALIGN
    assert step(_learner(L, tau_e=-0.1)[0], lay) == L.EINVAL and step(_learner(L, n=40)[0], lay) == L.EINVAL
    assert step(p, lay, 9) == L.ETOOBIG
    bad = _learner(L)[1]
    bad[0].trace = 20
    assert step(p, bad) == L.EALIGN
    for name in ("reward", "v", "v_last", "dvdt", "prime", "td", "ws"):
        assert step(p, lay, **{name: None}) == L.EINVAL, name
    for name in ("v", "v_last", "dvdt", "prime", "td", "ws"):
        assert step(p, lay, **{name: C.c_void_p(24)}) == L.EALIGN, name
    assert step(p, lay, reward=C.c_void_p(20), f64=1) == L.EALIGN and step(p, lay, reward=C.c_void_p(18), f64=0) == L.EALIGN
    assert step(p, lay, floats=need - 1) == L.EINVAL
    assert step(p, lay, ld=(-1, 0)) == L.EINVAL


class _Plan:
    """A native plan over made-up (aligned, never dereferenced) pointers: PlaceCells n = 8 (index 0), PlaceCells n = 2
    (index 1), a feed-forward layer n = 2 over population 0 (index 2)."""

    def __init__(self, L, ff_n=2):
        self.L = L
        env, motion = L.RiabEnv(), L.RiabMotion()
        env.extent[1] = env.extent[3] = env.scale = 1.0
        motion.dt = 0.05
        self.keep = (env, motion)
        self.h = C.c_void_p(L.lib.riab_plan_create(env, motion, 16, 8, 0, 1, 0, 16, 16))
        assert self.h
        for n in (8, 2):
            pop = L.RiabPopulation()
            pop.kind, pop.n, pop.table = L.POP_KINDS["place"], n, 16
            assert L.lib.riab_plan_add(self.h, pop) >= 0
        ff = L.RiabPopulation()
        ff.kind, ff.n, ff.n_inputs, ff.bias, ff.rates_prime = L.POP_KINDS["ff"], ff_n, 1, 16, 16
        ff.input_index[0], ff.input_wt[0] = 0, 16
        assert L.lib.riab_plan_add(self.h, ff) == 2

    def set(self, index=2, p=None, traces=(16,), v_last=16, dvdt=16, td=16, ws=16, floats=1 << 30, kind=None, reward=None, f64=0,
            ld=(0, 0), ridx=-1):
        L = self.L
        p = _learner(L)[0] if p is None else p
        kind = L.REWARD_NONE if kind is None else kind
        tr = (C.c_void_p * 8)(*traces)
        return L.lib.riab_plan_set_learner(self.h, index, p, tr, v_last, dvdt, td, ws, floats, kind, reward, f64, ld[0], ld[1], ridx)

    def __del__(self):
        self.L.lib.riab_plan_destroy(self.h)


def test_plan_set_learner_argument_errors_before_launch(L):
    P = _Plan(L)
    p, lay = _learner(L)
    need = L.lib.riab_td_workspace(p, lay, 1)
    assert P.set(index=0) == L.EINVAL and P.set(index=3) == L.EINVAL and P.set(index=-1) == L.EINVAL     # not an FF population
    assert P.set(kind=L.REWARD_POPULATION, ridx=2) == L.EINVAL and P.set(kind=L.REWARD_POPULATION, ridx=5) == L.EINVAL
    assert P.set(kind=L.REWARD_POPULATION, ridx=0) == L.EINVAL                                          # n = 8 against n = 2
    assert P.set(p=_learner(L, n=3)[0]) == L.EINVAL and P.set(p=_learner(L, Bp=12, B=9)[0]) == L.EINVAL  # not the plan's shapes
    for name in ("v_last", "dvdt", "td", "ws"):
        assert P.set(**{name: 24}) == L.EALIGN and P.set(**{name: None}) == L.EINVAL, name
    assert P.set(traces=(24,)) == L.EALIGN and P.set(traces=(None,)) == L.EINVAL
    assert P.set(kind=L.REWARD_POINTER, reward=20, f64=1) == L.EALIGN and P.set(kind=L.REWARD_POINTER) == L.EINVAL
    assert P.set(floats=need - 1) == L.EINVAL and P.set(kind=7) == L.EINVAL
    assert P.set(p=_learner(L, tau=0.0)[0]) == L.EINVAL
    wide = _Plan(L, ff_n=70000)
    assert wide.set(p=_learner(L, n=70000, Mp=70016)[0]) == L.ETOOBIG
    # nothing above left a learner behind: the split entry points still get past the learner check (to their own errors)
    assert L.lib.riab_plan_step_population(P.h, 7, None) == L.EINVAL
    assert P.set(kind=L.REWARD_POPULATION, ridx=1) == 0 and P.set(kind=L.REWARD_POINTER, reward=16, f64=1, ld=(0, 1)) == 0


def test_split_entry_points_and_unbound_rewards_are_refused(L):
    P = _Plan(L)
    assert P.set() == 0                                                         # a learner without a reward yet
    assert L.lib.riab_plan_step_agent(P.h, None) == L.EUNSUPPORTED
    assert L.lib.riab_plan_step_population(P.h, 0, None) == L.EUNSUPPORTED
    assert L.lib.riab_plan_step(P.h, 1, None) == L.EINVAL                       # no reward bound: before anything is launched
    assert P.set(kind=L.REWARD_TASK) == 0
    assert L.lib.riab_plan_step(P.h, 1, None) == L.EINVAL                       # the task's reward, and no task


# ---- the classes ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_world():
    import ratinabox_amd as riab
    from ratinabox_amd.contribs.ValueNeuron import ValueNeuron
    np.random.seed(0)
    ag = riab.Agent(riab.Environment({}), {"n_agents": 3, "device": "cpu"})
    pcs = riab.PlaceCells(ag, {"n": 16})
    return riab, ag, pcs, ValueNeuron(ag, {"input_layers": [pcs], "n": 2})


def test_learning_learner_still_refuses_population_and_offers_a_record(cpu_world, L):
    riab, ag, pcs, vn = cpu_world
    from ratinabox_amd.contribs.SuccessorFeatures import SuccessorFeatures
    assert vn.learning
    with pytest.raises(NotImplementedError, match="step plan"):    # what the AutoStepper relies on to stay eager
        vn._population({pcs: 0})
    pop, block = vn._learner_record({pcs: 0})
    assert pop.kind == L.POP_KINDS["ff"] and pop.n == 2 and pop.n_inputs == 1 and pop.input_index[0] == 0
    assert pop.input_wt[0] == vn.inputs[pcs.name].wt.data_ptr()                 # the master weights, not a copy
    assert block["traces"][0] == vn.inputs[pcs.name].trace.data_ptr() and block["reward"] == (L.REWARD_NONE, -1)
    assert block["params"].n == 2 and block["params"].Bp == ag._Bp and vn._workspace is not None
    feats = riab.PlaceCells(ag, {"n": 6})
    sf = SuccessorFeatures(ag, {"input_layers": [pcs], "features": feats})
    assert sf._learner_record({pcs: 0, feats: 1})[1]["reward"] == (L.REWARD_POPULATION, 1)
    with pytest.raises(NotImplementedError, match="before"):
        sf._learner_record({pcs: 0})
    from ratinabox_amd import plan
    assert plan.StepPlan.holds_learners and not plan.AutoStepper.holds_learners


def test_bind_reward_rejects_wrong_shapes_and_dtypes(cpu_world, L):
    riab, ag, pcs, vn = cpu_world
    from ratinabox_amd import plan
    n, B, Bp = 2, 3, ag._Bp
    ok = [torch.zeros((), dtype=torch.float64), torch.zeros(n), torch.zeros(B, dtype=torch.float64), torch.zeros(Bp),
          torch.zeros((n, B)), torch.zeros((n, Bp), dtype=torch.float64)]
    assert [plan._reward_binding(r, n, B, Bp) for r in ok] == [(1, 0, 0), (0, 1, 0), (1, 0, 1), (0, 0, 1), (0, B, 1), (1, Bp, 1)]
    bad = [torch.zeros(B + 2), torch.zeros((n + 1, B)), torch.zeros((B, n)), torch.zeros((n, B, 1)), torch.zeros(B, dtype=torch.float16),
           torch.zeros(B, dtype=torch.int64), np.zeros(B), 0.5]
    for r in bad:
        with pytest.raises(ValueError):
            plan._reward_binding(r, n, B, Bp)
    with pytest.raises(ValueError, match="live on"):
        plan._reward_binding(torch.zeros(B), n, B, Bp, torch.device("meta"))
    stub = plan.StepPlan.__new__(plan.StepPlan)                     # bind_reward's own checks come before any native call
    stub._h, stub._learners = None, {vn: [2, {"reward": (L.REWARD_NONE, -1)}, L.REWARD_NONE, None]}
    for r in bad:
        with pytest.raises(ValueError):
            stub.bind_reward(vn, r)
    with pytest.raises(ValueError, match="not a learning learner"):
        stub.bind_reward(pcs, torch.zeros(B))
    assert stub._learners[vn][2] == L.REWARD_NONE
