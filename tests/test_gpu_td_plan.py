"""TD learners inside step plans, on the GPU (run with `-m gpu`).

1. Kernel level, integer-exact (tests/td_shapes.py): torch.ops.riab.td_learn_step — two launches — against the sequence it
   replaces, td_forward_tail(no trace) + td_update(fused trace) + riab_td_reset(mask), bit for bit on every array and every
   lane, and against the integer product.
2. A plan that holds a learning ValueNeuron / SuccessorFeatures against the eager loop it stands for ("learn, then reset"),
   bit for bit: task plans over replicas and over one world, plans without a task, bound rewards.
3. What must not have moved: a frozen learner in a plan, Agent.simulate() with a learning one.
4. The operator's registration."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import td_shapes as sh
from tests.test_gpu_td_shapes import _Step, _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    from ratinabox_amd import ops  # noqa: F401  (registers torch.ops.riab.*)
    return ratinabox_amd


# ---- 1. the two launches against the four they replace ---------------------------------------------------------------
class _LearnStep(_Step):
    def _views(self):
        v = lambda pairs: [p[0] for p in pairs]
        return v(self.phi), v(self.trace), v(self.wt)

    def run_sequence(self, mask):
        """td_forward_tail(with_trace=False), td_update(fuse_trace=True), riab_td_reset(mask) on v, v_last, dvdt, td."""
        from ratinabox_amd import _lib as L
        phi, trace, wt = self._views()
        torch.ops.riab.td_forward_tail(self.v[0], self.v_last[0], self.dvdt[0], phi, trace, wt, self.consts, self.B, False)
        torch.ops.riab.td_update(wt, trace, phi, self.reward[0], self.v[0], self.dvdt[0], self.prime[0], self.td[0], self.ws,
                                 self.consts, self.B, True)
        if mask is not None:
            p = L.RiabTDParams()
            p.dt, p.tau, p.tau_e, p.eta, p.L2 = self.consts
            p.B, p.Bp, p.n, p.Mp = self.B, self.Bp, self.n, self.Mp
            lay = (L.RiabTDLayer * len(self.layers))()
            for l, k in enumerate(self.layers):
                lay[l].rates, lay[l].trace, lay[l].wt, lay[l].n_in = phi[l].data_ptr(), trace[l].data_ptr(), wt[l].data_ptr(), k
            rows = (C.c_void_p * 4)(*[x[0].data_ptr() for x in (self.v, self.v_last, self.dvdt, self.td)])
            L.check(L.lib.riab_td_reset(p, lay, len(self.layers), rows, 4, L.ptr(mask), L.current_stream()), "riab_td_reset")
        torch.cuda.synchronize()
        return self

    def run_learn_step(self, mask, zero_v=True):
        phi, trace, wt = self._views()
        torch.ops.riab.td_learn_step(wt, trace, phi, self.reward[0], self.v[0], self.v_last[0], self.dvdt[0], self.prime[0],
                                     self.td[0], mask, zero_v, self.ws, self.consts, self.B)
        torch.cuda.synchronize()
        return self

    def everything(self):
        """Every array whole: all Bp lanes, the guard rows, W^T's padding columns."""
        return {"wt": [w[1].clone() for w in self.wt], "trace": [e[1].clone() for e in self.trace], "v": self.v[1].clone(),
                "v_last": self.v_last[1].clone(), "dvdt": self.dvdt[1].clone(), "td": self.td[1].clone()}


def _masks(B, Bp, dev):
    """None; all lanes; every third lane + lane B - 1 (a quad with exactly one masked lane among them).  The arrays are
    Bp long and name every padded lane too: those must not be touched."""
    third = np.zeros(Bp, dtype=np.uint8)
    third[:B:3] = 1
    third[B - 1] = 1
    quads = third[:(B + 3) // 4 * 4].copy()
    quads[B:] = 0
    assert (quads.reshape(-1, 4).sum(1) == 1).any()
    third[B:] = 1
    return {"none": None, "all": torch.ones(Bp, dtype=torch.uint8, device=dev), "third": torch.from_numpy(third).to(dev)}


LEARN_CASES = [(n, key, batch) for n in (1, 33, 129, 257) for key in ("ragged", "eight") for batch in ((1, 4), (33, 36), (1022, 1024))]


@pytest.mark.parametrize("n,key,batch", LEARN_CASES, ids=[f"n{n}-{k}-{b[0]}" for n, k, b in LEARN_CASES])
def test_learn_step_equals_the_sequence_it_replaces(riab, n, key, batch):
    """n = 1, 33, 129: MT 1, 2, 8 with the trace fused; n = 257: two row groups behind the stand-alone trace kernel.  All
    three reward forms and all three masks at every shape; every array compared whole (padded lanes, guard rows and
    W^T's columns >= n included), then the weights and the TD error against the integer product."""
    (B, Bp), layers = batch, sh.LAYER_SETS[key]
    dev = torch.device("cuda")
    assert (sh.launch_path(n, layers, Bp)["mt"], sh.launch_path(n, layers, Bp)["groups"]) == sh.ROWS[n]
    masks = _masks(B, Bp, dev)
    for form in sh.REWARD_FORMS:
        case = sh.Case("learn-step", n, layers, B, Bp, form)
        a = sh.integer_inputs(case)
        ref = sh.integer_reference(case, a)
        for name, mask in masks.items():
            old = _LearnStep(riab, n, layers, B, Bp, a, sh.INT_CONSTS).run_sequence(mask)
            new = _LearnStep(riab, n, layers, B, Bp, a, sh.INT_CONSTS).run_learn_step(mask)
            new.guards_intact()
            want, got = old.everything(), new.everything()
            for k in want:
                xs, ys = (want[k], got[k]) if isinstance(want[k], list) else ([want[k]], [got[k]])
                for l, (x, y) in enumerate(zip(xs, ys)):
                    assert torch.equal(_bits(x), _bits(y)), (form, name, k, l, int((_bits(x) != _bits(y)).sum()))
            hit = torch.zeros(B, dtype=torch.bool, device=dev) if mask is None else mask[:B].bool()
            td = torch.from_numpy(ref["td"].astype(np.float32)).to(dev)
            td[:, hit] = 0.0
            assert torch.equal(new.td[0][:, :B], td) and not new.td[0][:, B:].any(), (form, name)
            for l in range(len(layers)):
                assert torch.equal(new.wt[l][0][:, :n], torch.from_numpy(ref["wt"][l]).to(dev)), (form, name, l)
                assert not new.wt[l][0][:, n:].any()
                e = torch.from_numpy(ref["traces"][l].astype(np.float32)).to(dev)
                e[:, hit] = 0.0
                assert torch.equal(new.trace[l][0][:, :B], e), (form, name, l)
            v = torch.from_numpy(a["v"][:, :B]).to(dev)
            v[:, hit] = 0.0
            assert torch.equal(new.v_last[0][:, :B], v) and torch.equal(new.v[0][:, :B], v)
            if mask is not None:
                assert not new.dvdt[0][:, :B][:, hit].any()
    # the caller's v is a history row: it stays as recorded, everything else as above; NaN in the padded lanes and the
    # guard rows changes nothing in the real lanes
    kept = _LearnStep(riab, n, layers, B, Bp, a, sh.INT_CONSTS).run_learn_step(masks["third"], zero_v=False)
    assert torch.equal(kept.v[1], _LearnStep(riab, n, layers, B, Bp, a, sh.INT_CONSTS).v[1])
    for k in ("v_last", "dvdt", "td"):
        assert torch.equal(_bits(getattr(kept, k)[1]), _bits(got[k])), k
    nan = _LearnStep(riab, n, layers, B, Bp, a, sh.INT_CONSTS, poison=True).run_learn_step(masks["third"])
    nan.guards_intact()
    for k in ("v", "v_last", "dvdt", "td"):
        assert torch.equal(getattr(nan, k)[0][:, :B], getattr(new, k)[0][:, :B]), k
    for l in range(len(layers)):
        assert torch.equal(nan.wt[l][0], new.wt[l][0]) and torch.equal(nan.trace[l][0][:, :B], new.trace[l][0][:, :B])


# ---- 2. a plan with a learner against the eager loop -----------------------------------------------------------------
def _learner_state(VN):
    out = {"td_error": VN.td_error, "firingrate_deriv": VN.firingrate_deriv}
    for name, e in VN.inputs.items():
        out["w:" + name], out["trace:" + name] = e["w"], e["eligibility_trace"]
    return out


def _assert_same(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (label, k)


def _task_worlds(riab, act, history, lanes="replicas", B=257):
    """The build of test_task_step_plan_equals_eager_loop (tests/test_gpu_task.py) + a ValueNeuron of two value neurons."""
    from ratinabox_amd.contribs.TaskEnvironment import SpatialGoalEnvironment
    from ratinabox_amd.contribs.ValueNeuron import ValueNeuron
    np.random.seed(2)
    env = SpatialGoalEnvironment(params={"walls": [[[0.5, 0.3], [0.5, 0.7]]]},
                                 possible_goal_positions=[[0.2, 0.25], [0.8, 0.7], [0.5, 0.1]],
                                 goalcachekws=dict(reset_n_goals=2, goalorder="sequential"),
                                 episode_terminate_delay=0.03, teleport_on_reset=True, seed=11,
                                 **({} if lanes == "replicas" else {"lanes": lanes}))
    Ag = riab.Agent(env, {"dt": 0.01, "n_agents": B, "seed": 4})
    PCs = riab.PlaceCells(Ag, {"n": 40})
    env.add_agents(Ag)
    VN = ValueNeuron(Ag, {"input_layers": [PCs], "n": 2, "tau": 0.5, "eta": 0.05, "save_history": history,
                          "activation_function": {"activation": act}})
    if act == "relu":   # (a relu that starts at zero has no gradient)
        VN.inputs[PCs.name]["w"] = np.random.RandomState(3).uniform(0.0, 0.1, size=(2, 40))
    return env, Ag, PCs, VN


@pytest.mark.parametrize("act,history", [("relu", True), ("linear", True), ("relu", False)],
                         ids=["relu", "linear", "relu-no-history"])
def test_task_plan_with_a_learner_equals_the_eager_loop(riab, act, history):
    """`env.make_step_plan(auto_reset=True, scripted_speed=speed)` with a learning ValueNeuron == `a = goal direction;
    env.step(a); PCs.update(); VN.learn(reward); VN.reset(lanes=done); env.reset(mask=done)`: reward and terminal every
    step, then positions, histories, weights, traces, TD error, task state and episode tables, bit for bit.  Without a
    history the learner's one row is not a history row: its `firingrate` (zeroed in the reset lanes) is compared too."""
    B, T, speed = 257, 150, 11.0 * 0.08
    e1, A1, P1, V1 = _task_worlds(riab, act, history)
    e2, A2, P2, V2 = _task_worlds(riab, act, history)
    plan = e2.make_step_plan(auto_reset=True, scripted_speed=speed)
    terms = 0
    for k in range(T):
        a = e1._goal_vector(speed)
        obs, rew, term, trunc, info = e1.step(a)
        rew, term = rew.clone(), term.clone()
        P1.update()
        V1.learn(e1.get_reward())
        done = e1.terminal
        V1.reset(lanes=done)
        e1.reset(mask=done)
        plan.step(1)
        assert torch.equal(e2.get_reward(), rew) and torch.equal(e2.terminal, term), k
        terms += int(term.sum().item())
    assert plan.info()["fused_steps"] == 0
    assert np.array_equal(A1.pos, A2.pos)
    assert np.array_equal(A1.history["pos"], A2.history["pos"])
    assert np.array_equal(P1.history["firingrate"], P2.history["firingrate"])
    if history:
        assert np.array_equal(V1.history["firingrate"], V2.history["firingrate"]) and np.abs(V1.history["firingrate"]).max() > 0
    else:
        assert np.array_equal(V1.firingrate, V2.firingrate)
    _assert_same(_learner_state(V1), _learner_state(V2), act)
    assert not np.array_equal(V1.inputs[P1.name]["w"], V1.inputs[P1.name]["w_init"])
    assert torch.equal(e1.task_state, e2.task_state)
    assert e1.episodes == e2.episodes and len(e1.episodes["episode"]) > 5 and terms > 5
    assert e1.t == e2.t and e1.diagnostics == e2.diagnostics and e1._reset_counter == e2._reset_counter


def test_one_world_task_plan_with_a_learner_equals_the_eager_loop(riab):
    """lanes="agents": the world's reset moves behind the learner; the learner's reset mask is the world's terminal column.
    (The plan advances its reset counter every step, reset or not: the eager loop is given the same counter.)"""
    B, T, speed = 256, 100, 11.0 * 0.08
    e1, A1, P1, V1 = _task_worlds(riab, "linear", True, lanes="agents", B=B)
    e2, A2, P2, V2 = _task_worlds(riab, "linear", True, lanes="agents", B=B)
    plan = e2.make_step_plan(auto_reset=True, scripted_speed=speed)
    c0, resets = e1._reset_counter, 0
    for k in range(T):
        a = e1._goal_vector(speed)
        obs, rew, term, trunc, info = e1.step(a)
        rew, term = rew.clone(), term.clone()
        P1.update()
        V1.learn(e1.get_reward())
        done = e1.terminal
        V1.reset(lanes=done)
        if bool(done[0].item()):
            e1._reset_counter = c0 + k
            e1.reset()
            resets += 1
        plan.step(1)
        assert torch.equal(e2.get_reward(), rew) and torch.equal(e2.terminal, term), k
    assert plan.info()["fused_steps"] == 0 and resets > 0
    assert np.array_equal(A1.pos, A2.pos) and np.array_equal(A1.history["pos"], A2.history["pos"])
    assert np.array_equal(P1.history["firingrate"], P2.history["firingrate"])
    assert np.array_equal(V1.history["firingrate"], V2.history["firingrate"])
    _assert_same(_learner_state(V1), _learner_state(V2), "world")
    assert torch.equal(e1.task_state, e2.task_state) and torch.equal(e1._world, e2._world) and e1.episodes == e2.episodes


def test_task_plan_without_auto_reset_learns_and_leaves_the_resets_to_the_caller(riab):
    """auto_reset=False: the plan learns and resets nothing; the caller's `VN.reset(lanes=...)`, `env.reset(mask=...)`
    between the steps keep working (as in test_task_plan_with_manual_resets)."""
    B, T, speed = 257, 150, 11.0 * 0.08    # (the build and the run in which test_task_step_plan_equals_eager_loop ends > 5 episodes)
    e1, A1, P1, V1 = _task_worlds(riab, "linear", True, B=B)
    e2, A2, P2, V2 = _task_worlds(riab, "linear", True, B=B)
    plan = e2.make_step_plan(auto_reset=False)
    n_term = 0
    for k in range(T):
        _, r1, t1, _, _ = e1.step(e1._goal_vector(speed))
        P1.update()
        V1.learn(e1.get_reward())
        V1.reset(lanes=t1)
        e1.reset(mask=t1)
        plan.step(1, drift_velocity=e2._goal_vector(speed))
        assert torch.equal(e2.get_reward(), r1) and torch.equal(e2.terminal, t1), k
        V2.reset(lanes=e2.terminal)
        e2.reset(mask=e2.terminal)
        n_term += int(t1.sum().item())
    assert n_term > 5
    assert np.array_equal(A1.pos, A2.pos) and torch.equal(e1.task_state, e2.task_state)
    assert np.array_equal(A1.history["pos"], A2.history["pos"]) and e1.episodes == e2.episodes
    _assert_same(_learner_state(V1), _learner_state(V2), "manual resets")


@pytest.mark.parametrize("B", [33, 256])
def test_successor_features_in_a_plan_without_a_task(riab, B):
    """Basis PlaceCells n = 40, features PlaceCells n = 33: the reward is this step's row of the features, resolved from
    the cursor.  step(1) and step(7) mixed up to 30 steps == `Ag.update(); PCs.update(); Feat.update(); SF.learn()`.
    (B = 256: whole segments, where the one-launch agent step may carry the PlaceCells.)"""
    from ratinabox_amd.contribs.SuccessorFeatures import SuccessorFeatures

    def build():
        np.random.seed(5)
        Ag = riab.Agent(riab.Environment({}), {"dt": 0.02, "n_agents": B, "seed": 6})
        PCs = riab.PlaceCells(Ag, {"n": 40, "widths": 0.15})
        Feat = riab.PlaceCells(Ag, {"n": 33, "widths": 0.25})
        SF = SuccessorFeatures(Ag, {"input_layers": [PCs], "features": Feat, "tau": 0.5, "eta": 0.05})
        return Ag, PCs, Feat, SF

    A1, P1, F1, S1 = build()
    A2, P2, F2, S2 = build()
    for _ in range(30):
        A1.update()
        P1.update()
        F1.update()
        S1.learn()
    plan = A2.make_step_plan()
    for n in (1, 7, 1, 1, 7, 7, 1, 5):
        plan.step(n)
    assert sum((1, 7, 1, 1, 7, 7, 1, 5)) == 30 and plan.info()["launches"] > 0
    assert np.array_equal(A1.history["pos"], A2.history["pos"])
    for X, Y in ((P1, P2), (F1, F2), (S1, S2)):
        assert np.array_equal(X.history["firingrate"], Y.history["firingrate"])
    _assert_same(_learner_state(S1), _learner_state(S2), f"successor features, B = {B}")
    assert np.abs(S1.inputs[P1.name]["w"] - S1.inputs[P1.name]["w_init"]).max() > 0
    # the features must be recorded before the learner
    A3, P3, F3, S3 = build()
    with pytest.raises(NotImplementedError, match="before"):
        A3.make_step_plan(neurons=[P3, S3, F3])


def test_value_neuron_with_a_bound_reward(riab):
    """`plan.bind_reward(VN, tensor)`: a float32 (n, Bp) tensor rewritten between the steps, then a float64 (B,) tensor; no
    reward bound: ValueError before anything is launched."""
    from ratinabox_amd.contribs.ValueNeuron import ValueNeuron
    B, n = 30, 3

    def build():
        np.random.seed(8)
        Ag = riab.Agent(riab.Environment({}), {"dt": 0.05, "n_agents": B, "seed": 2})
        PCs = riab.PlaceCells(Ag, {"n": 20, "widths": 0.2})
        VN = ValueNeuron(Ag, {"input_layers": [PCs], "n": n, "activation_function": {"activation": "linear"}})
        return Ag, PCs, VN

    A1, P1, V1 = build()
    A2, P2, V2 = build()
    gen = torch.Generator(device="cpu").manual_seed(4)
    plan = A2.make_step_plan()
    launches = plan.info()["launches"]
    with pytest.raises(ValueError, match="no reward"):
        plan.step(1)
    assert plan.info()["launches"] == launches and A2._step_index == A1._step_index
    r32 = torch.zeros((n, A2._Bp), dtype=torch.float32, device="cuda")
    plan.bind_reward(V2, r32)
    for k in range(8):
        r = torch.randn((n, A2._Bp), generator=gen)
        r32.copy_(r)                                   # read in place: the plan sees what was written between the steps
        plan.step(1)
        A1.update()
        P1.update()
        V1.learn(r.to("cuda"))
    r64 = torch.randn((B,), generator=gen, dtype=torch.float64).to("cuda")
    plan.bind_reward(V2, r64)
    plan.step(4)
    for k in range(4):
        A1.update()
        P1.update()
        V1.learn(r64)
    assert np.array_equal(V1.history["firingrate"], V2.history["firingrate"])
    _assert_same(_learner_state(V1), _learner_state(V2), "bound reward")
    assert np.abs(V1.inputs[P1.name]["w"] - V1.inputs[P1.name]["w_init"]).max() > 0
    for bad in (torch.zeros(B + 1, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B), 1.0):
        with pytest.raises(ValueError):
            plan.bind_reward(V2, bad)
    with pytest.raises(ValueError, match="not a learning learner"):
        plan.bind_reward(P2, r64)


# ---- 3. what has not moved -------------------------------------------------------------------------------------------
def test_frozen_learner_in_a_plan_and_simulate_refusal_are_unchanged(riab):
    from ratinabox_amd.contribs.ValueNeuron import ValueNeuron
    B = 33

    def build(learning):
        np.random.seed(9)
        Ag = riab.Agent(riab.Environment({}), {"dt": 0.05, "n_agents": B, "seed": 3})
        PCs = riab.PlaceCells(Ag, {"n": 24, "widths": 0.2})
        VN = ValueNeuron(Ag, {"input_layers": [PCs], "n": 2, "learning": learning})
        return Ag, PCs, VN

    A1, P1, V1 = build(False)
    A2, P2, V2 = build(False)
    w = V2.inputs[P2.name]["w"]
    plan = A2.make_step_plan()
    assert not plan._learners
    for _ in range(12):
        A1.update()
        P1.update()
        V1.update()
    plan.step(5)
    plan.step(7)
    assert np.array_equal(V1.history["firingrate"], V2.history["firingrate"]) and np.abs(V1.history["firingrate"]).max() > 0
    assert np.array_equal(V2.inputs[P2.name]["w"], w)                 # a frozen learner's weights do not move
    V2.learning = True                                                # the plan keeps the mode it recorded
    plan.step(3)
    assert np.array_equal(V2.inputs[P2.name]["w"], w)
    A3, P3, V3 = build(True)
    with pytest.raises(NotImplementedError, match="learning"):
        A3.simulate(8, neurons=[P3, V3])


# ---- 4. the operator's registration -----------------------------------------------------------------------------------
def test_td_learn_step_passes_opcheck(riab):
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(9)
    B, Bp, n, n_in = 62, 64, 5, 48
    consts = [0.05, 1.0, 0.25, 0.01, 0.001]
    phi = torch.rand((n_in, Bp), generator=gen).to(dev)
    rew = torch.rand((n, Bp), generator=gen).to(dev)
    prime = torch.ones((n, Bp), device=dev)
    v = torch.rand((n, Bp), generator=gen).to(dev)
    wt = torch.zeros((n_in, 32))
    wt[:, :n] = torch.randn((n_in, n), generator=gen) * 0.1
    wt, trace = wt.to(dev), torch.zeros((n_in, Bp), device=dev)
    v_last, dvdt, td = (torch.zeros((n, Bp), device=dev) for _ in range(3))
    ws = torch.empty(riab.ops.td_workspace_floats(n, [n_in], Bp), dtype=torch.float32, device=dev)
    mask = (torch.rand(B, generator=gen) < 0.3).to(torch.uint8).to(dev)
    for m, zero_v in ((None, False), (mask, True)):
        torch.library.opcheck(torch.ops.riab.td_learn_step.default,
                              ([wt], [trace], [phi], rew, v, v_last, dvdt, prime, td, m, zero_v, ws, consts, B),
                              test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError, match="mask"):
        torch.ops.riab.td_learn_step([wt], [trace], [phi], rew, v, v_last, dvdt, prime, td, mask[:B - 1], True, ws, consts, B)
