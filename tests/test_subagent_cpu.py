"""No-GPU checks of contribs.SubAgent: the float64 restatement of the sweep (tests/subagent_oracle.py) is pinned to the
reference's record, the C ABI's new entry points are checked the way tests/test_abi_cpu.py checks the rest, and the class
surface is checked on the CPU device (constructors, constants, refusals: nothing is launched)."""
import ctypes as C
import math
import os
import re
import warnings

import numpy as np
import pytest

from oracle import riab_oracle as orc
from tests import golden_util as gu
from tests import subagent_oracle as sao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
THETA_RUNS = ["subagent_theta_solid_wall.npz", "subagent_theta_periodic.npz", "subagent_theta_params.npz"]


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def load(name):
    """(every array read once: an .npz decompresses an array on each access)"""
    with gu.load(name) as z:
        return {k: z[k] for k in z.files}


def oracle_of(g, B=1):
    env = orc.EnvSpec(boundary_conditions="periodic" if bool(g["periodic"]) else "solid", walls=g["user_walls"])
    fwd = {str(k): float(v) for k, v in zip(g["forward_keys"], g["forward_vals"])}
    return sao.ThetaSequenceOracle(env, B, float(g["dt"]), float(g["lead_average_speed"]), fwd, float(g["v_sequence"]),
                                   float(g["theta_freq"]), float(g["theta_frac"]))


def lead_of(g, t, rolls):
    """the lead's state of step t as the oracle takes it (velocity and rotational velocity are only read, and only
    recorded, on the steps of a rollout)"""
    lead = dict(pos=g["lead_pos"][t], distance_travelled=g["lead_dist"][t], velocity=np.full(2, np.nan),
                rotational_velocity=np.nan)
    if t in rolls:
        i = int(np.nonzero(g["roll_step"] == t)[0][0])
        lead.update(velocity=g["roll_lead_vel"][i], rotational_velocity=g["roll_lead_rot"][i])
    return lead


def rollouts_of(g):
    """step index -> (normals (count, 2), future distances (count + 1,), future positions (count + 1, 2))"""
    out, zi, fi = {}, 0, 0
    for step, n in zip(g["roll_step"], g["roll_count"]):
        n = int(n)
        out[int(step)] = (g["roll_z"][zi:zi + n], g["fut_dist"][fi:fi + n + 1], g["fut_pos"][fi:fi + n + 1])
        zi, fi = zi + n, fi + n + 1
    return out


# ---- C1: the oracle against the reference ------------------------------------------------------------------------
# oracle.agent_step is not the reference's arithmetic to the bit (it rounds a step's length and a few products in another
# order): over the 84 recorded rollouts its future arrays stay within 9.5e-16 of the reference's (distances 3.9e-16,
# positions 9.5e-16: a few ulp of values below 1; none of it feeds back into the motion beyond the positions).  The
# bound is that measured deviation with a margin of 4.  Everything else is exact: counts, where the NaNs are, and every
# look-behind position, which is pure interpolation of recorded data.
ROLLOUT_DEVIATION = 9.5e-16
ROLLOUT_TOL = 4 * ROLLOUT_DEVIATION


@pytest.mark.parametrize("name", THETA_RUNS)
def test_oracle_reproduces_the_reference(name):
    """Fed with the lead's recorded state and the rollouts' recorded normals, the restatement gives the reference's
    ThetaSequenceAgent position at every step — NaN in the same places; exactly on look-behind steps, within
    ROLLOUT_TOL on look-ahead steps — and per rollout its count (exactly) and future arrays (within ROLLOUT_TOL)."""
    g = load(name)
    o, rolls = oracle_of(g), rollouts_of(g)
    assert o.K == int(g["K"])
    n_interp, worst = 0, 0.0
    for t in range(len(g["lead_t"])):
        lead = lead_of(g, t, rolls)
        z = rolls[t][0][:, :, None] if t in rolls else None
        pos = o.step(lead, float(g["lead_t"][t]), rollout_z=z)[0]
        assert o.rolled_out == (t in rolls), t
        if t in rolls:
            d, p = o.future[0]
            assert len(d) - 1 == len(rolls[t][0]) <= o.K // 2
            worst = max(worst, np.abs(d - rolls[t][1]).max(), np.abs(p - rolls[t][2]).max())
            np.testing.assert_allclose(d, rolls[t][1], rtol=0, atol=ROLLOUT_TOL, err_msg=f"future distances, step {t}")
            np.testing.assert_allclose(p, rolls[t][2], rtol=0, atol=ROLLOUT_TOL, err_msg=f"future positions, step {t}")
        ref = g["sub_pos"][t]
        np.testing.assert_array_equal(np.isnan(pos), np.isnan(ref), err_msg=f"step {t}")
        if o.phase(float(g["lead_t"][t])) < 0.5:
            np.testing.assert_array_equal(pos, ref, err_msg=f"look-behind step {t}")
        else:
            np.testing.assert_allclose(pos, ref, rtol=0, atol=ROLLOUT_TOL, equal_nan=True, err_msg=f"look-ahead step {t}")
        n_interp += int(np.isfinite(pos[0]) and not np.array_equal(pos, g["lead_pos"][t]))
    print(f"[{name}] oracle rollouts against the reference's: worst deviation {worst:.3g} (bound {ROLLOUT_TOL:.3g})")
    assert o.raises["behind"] == o.raises["ahead"] == o.raises["saturated"] == 0
    assert o.raises["far"] == len(g["far_steps"]) and (name != "subagent_theta_periodic.npz" or o.raises["far"] >= 1)
    # both look-behind branches were met: the lead's own position while it has not covered d_half, interpolation after
    behind_early = [t for t in range(len(g["lead_t"])) if np.array_equal(g["sub_pos"][t], g["lead_pos"][t])]
    assert behind_early and n_interp > 100
    # the SubAgent's clock: the lead's, plus the dt its own Agent.update adds (SubAgent.py:35-36, Agent.py:196)
    # (the generator asserts it on every step and keeps the first 100)
    np.testing.assert_array_equal(g["sub_t_head"], g["lead_t"][:100] + float(g["dt"]))


def test_shift_oracle_reproduces_the_reference_bit_for_bit():
    g = load("subagent_shift.npz")
    np.testing.assert_array_equal(sao.shift_position(g["lead_pos"], g["lead_hd"], 0.03), g["pos_plus"])
    np.testing.assert_array_equal(sao.shift_position(g["lead_pos"], g["lead_hd"], -0.03), g["pos_minus"])
    assert len(g["lead_pos"]) == 200


def test_oracle_takes_a_ready_made_future_table():
    """The same positions whether the oracle rolls out itself or is handed that rollout as a [K+1][3][B] table."""
    g = load("subagent_theta_solid_wall.npz")
    a, b, rolls = oracle_of(g), oracle_of(g), rollouts_of(g)
    for t in range(400):
        lead = lead_of(g, t, rolls)
        pa = a.step(lead, float(g["lead_t"][t]), rollout_z=rolls[t][0][:, :, None] if t in rolls else None)
        fut = None
        if t in rolls:
            d, p = a.future[0]
            table = np.full((a.K + 1, 3, 1), np.nan)
            table[:len(d), 0, 0], table[:len(d), 1:, 0] = d, p
            fut = (table, np.array([len(d) - 1]))
        pb = b.step(lead, float(g["lead_t"][t]), future=fut)
        np.testing.assert_array_equal(pa, pb)
    assert len([t for t in rolls if t < 400]) >= 7


def test_interp1d_restatement_is_scipys():
    from scipy.interpolate import interp1d
    rng = np.random.RandomState(3)
    xs = np.cumsum(rng.uniform(1e-4, 1e-3, size=6)) + 1.0
    ys = rng.uniform(size=(6, 2))
    f = interp1d(xs, ys, axis=0)
    for x in list(rng.uniform(xs[0], xs[-1], size=50)) + list(xs):
        np.testing.assert_array_equal(sao.interp1d_linear(xs, ys, x), f(x))
    assert sao.interp1d_linear(xs, ys, xs[0] - 1e-9) is None and sao.interp1d_linear(xs, ys, xs[-1] + 1e-9) is None
    assert sao.interp1d_linear(xs[:1], ys[:1], xs[0]) is None and sao.interp1d_linear(xs[:0], ys[:0], 1.0) is None


# ---- C2: the C ABI -----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("riab_theta_sequence_step", "riab_theta_sequence_rollout", "riab_shift_agent_position")


def test_abi_11_and_new_symbols(L):
    src = open(HEADER).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION == L.lib.riab_abi_version() == 11
    for s in NEW_SYMBOLS:
        assert hasattr(L.lib, s) and s in L.PROTOTYPES and re.search(r"\b%s\(" % s, src), s
    for name, val in (("NONE", L.THETA_NONE), ("BEHIND", L.THETA_BEHIND), ("AHEAD", L.THETA_AHEAD),
                      ("DIAG_BEHIND", L.THETA_DIAG_BEHIND), ("DIAG_AHEAD", L.THETA_DIAG_AHEAD),
                      ("DIAG_ROLLOUT", L.THETA_DIAG_ROLLOUT), ("DIAG_FAR", L.THETA_DIAG_FAR)):
        assert int(re.search(r"RIAB_THETA_%s = (\d+)" % name, src).group(1)) == val, name
    # the prototypes carry as many arguments as the header declares
    for s in NEW_SYMBOLS:
        decl = re.search(r"\bint %s\((.*?)\);" % s, src, re.S).group(1)
        assert len(decl.split(",")) == len(L.PROTOTYPES[s][1]), s


def test_argument_errors_before_launch(L):
    """Negative codes come from validation only: no device needed."""
    env, m, ok = L.RiabEnv(), L.RiabMotion(), C.c_void_p(64)
    m.dt = 0.125
    step = L.lib.riab_theta_sequence_step

    def s(env=env, lead=ok, B=8, ring=ok, cap=100, look=100, n=0, branch=L.THETA_BEHIND, d_half=0.125, frac=0.5, fut=ok,
          count=ok, K=10, out=ok, nreal=None):
        return step(env, lead, B, min(B, 5) if nreal is None else nreal, ring, cap, look, n, branch, 0.3, d_half, frac, fut, count, K, out, None, None)

    assert s(env=None) == L.EINVAL and s(lead=None) == L.EINVAL and s(ring=None) == L.EINVAL and s(out=None) == L.EINVAL
    assert s(B=0) == L.EINVAL and s(B=6) == L.EALIGN and s(n=-1) == L.EINVAL
    assert s(nreal=9) == L.EINVAL and s(nreal=-1) == L.EINVAL
    assert s(cap=99, look=100) == L.EINVAL and s(look=0) == L.EINVAL and s(cap=0, look=0) == L.EINVAL
    assert s(branch=3) == L.EINVAL and s(branch=-1) == L.EINVAL
    assert s(d_half=0.0) == L.EINVAL and s(frac=0.0) == L.EINVAL and s(d_half=float("nan")) == L.EINVAL
    assert s(branch=L.THETA_AHEAD, K=0) == L.EINVAL and s(branch=L.THETA_AHEAD, fut=None) == L.EINVAL
    assert s(branch=L.THETA_AHEAD, count=None) == L.EINVAL

    roll = L.lib.riab_theta_sequence_rollout

    def r(env=env, m=m, lead=ok, fwd=ok, B=8, K=10, dist=0.3, fut=ok, count=ok, nreal=None):
        return roll(env, m, lead, fwd, B, min(B, 5) if nreal is None else nreal, 0, None, None, 1, 0, K, dist, fut, count, None, None, None)

    assert r(env=None) == L.EINVAL and r(m=None) == L.EINVAL and r(lead=None) == L.EINVAL and r(fwd=None) == L.EINVAL
    assert r(fut=None) == L.EINVAL and r(count=None) == L.EINVAL
    assert r(K=0) == L.EINVAL and r(K=-3) == L.EINVAL and r(dist=0.0) == L.EINVAL and r(B=0) == L.EINVAL and r(B=6) == L.EALIGN
    assert r(nreal=9) == L.EINVAL and r(nreal=-1) == L.EINVAL
    drift = L.RiabMotion()
    drift.dt, drift.has_drift = 0.125, 1
    assert r(m=drift) == L.EINVAL

    shift = L.lib.riab_shift_agent_position
    assert shift(None, 8, 0.01, ok, None) == L.EINVAL and shift(ok, 8, 0.01, None, None) == L.EINVAL
    assert shift(ok, 0, 0.01, ok, None) == L.EINVAL and shift(ok, 6, 0.01, ok, None) == L.EALIGN


# ---- C3: the classes, device-free --------------------------------------------------------------------------------
@pytest.fixture()
def lead():
    import ratinabox_amd as riab
    np.random.seed(0)
    return riab, riab.Agent(riab.Environment({}), {"n_agents": 3, "device": "cpu", "dt": 0.002})


def test_defaults_and_params_protocol(lead):
    riab, Lead = lead
    from ratinabox_amd import contribs  # noqa: F401
    from ratinabox_amd.contribs.SubAgent import ShiftAgent, SubAgent, ThetaSequenceAgent, UnrelatedAgent
    assert SubAgent.default_params == {} and UnrelatedAgent.default_params == {}
    assert ThetaSequenceAgent.default_params == {"v_sequence": 5.0, "theta_freq": 10.0, "theta_frac": 0.5}
    assert ShiftAgent.default_params == {"shift_m": 0.01}
    allp = ThetaSequenceAgent.get_all_default_params()
    assert allp["v_sequence"] == 5.0 and allp["speed_mean"] == 0.08 and allp["dt"] == 0.05
    TS = ThetaSequenceAgent(Lead)
    assert isinstance(TS, riab.Agent) and TS.LeadAgent is Lead and TS.Environment is Lead.Environment
    assert TS in Lead.Environment.Agents and TS.ForwardSequenceAgent in Lead.Environment.Agents
    assert (TS.dt, TS.n_agents, TS._Bp, TS.device) == (Lead.dt, 3, 4, "cpu")
    assert (TS.v_sequence, TS.theta_freq, TS.theta_frac) == (5.0, 10.0, 0.5)
    np.testing.assert_array_equal(TS.pos, Lead.pos)
    np.testing.assert_array_equal(TS.velocity, Lead.velocity)
    assert not TS._auto_enabled
    fwd = TS.ForwardSequenceAgent
    assert type(fwd) is riab.Agent and (fwd.n_agents, fwd.device, fwd.dt) == (3, "cpu", Lead.dt)
    assert not hasattr(fwd, "v_sequence") and fwd.rng_seed != Lead.rng_seed
    S = ShiftAgent(Lead, {"shift_m": -0.03})
    assert S.shift_m == -0.03 and ShiftAgent(Lead).shift_m == 0.01
    U = UnrelatedAgent(Lead)
    assert U.LeadAgent is Lead and not U._auto_enabled


def test_constants_for_the_defaults_at_2ms(lead):
    _riab, Lead = lead
    from ratinabox_amd.contribs.SubAgent import ThetaSequenceAgent
    Lead.distance_travelled = np.array([0.5, 0.6, 0.7])
    n_hist = len(Lead.history["t"])
    TS = ThetaSequenceAgent(Lead)
    assert TS.T_theta == 0.1 and abs(TS.d_half - 0.125) < 1e-15 and abs(TS.forward_distance - 0.325) < 1e-15
    assert TS.lookback == 3906 and abs(TS.dt_forward - 0.125) < 1e-15
    assert TS.rollout_steps_max == math.ceil(4 * 0.325 / (0.002 * 5.0)) + 8 == 138
    assert TS._ring.shape == (3906, 3, 4) and TS._future.shape == (139, 3, 4) and TS._count.shape == (4,)
    assert TS._ring.dtype == TS._future.dtype == __import__("torch").float64
    # the constructor zeroes the lead's distance travelled and leaves its history lists alone
    np.testing.assert_array_equal(Lead.distance_travelled, np.zeros(3))
    assert len(Lead.history["t"]) == len(Lead.history["distance_travelled"]) == n_hist
    assert TS.theta_phase() == 0.0


def test_forward_agent_takes_the_subagents_parameters(lead):
    riab, _ = lead
    from ratinabox_amd.contribs.SubAgent import ThetaSequenceAgent
    Lead = riab.Agent(riab.Environment({}), {"device": "cpu", "dt": 0.001, "speed_mean": 0.05, "thigmotaxis": 0.2})
    TS = ThetaSequenceAgent(Lead, {"speed_mean": 0.12, "theta_freq": 8.0, "theta_frac": 0.6, "v_sequence": 3.0})
    fwd = TS.ForwardSequenceAgent
    assert fwd.speed_mean == 0.12 and fwd.thigmotaxis == 0.5          # what was passed to the SubAgent, or the defaults
    assert abs(TS.d_half - 0.1125) < 1e-15 and TS.lookback == int(5 * TS.d_half / (0.001 * 0.08))
    assert abs(TS.dt_forward - 0.001 * 3.0 / 0.08) < 1e-18            # the LEAD's average measured speed


def test_constructor_asserts_and_dt_warning(lead):
    riab, Lead = lead
    from ratinabox_amd.contribs.SubAgent import ShiftAgent, ThetaSequenceAgent
    with pytest.raises(AssertionError, match="too large"):
        ThetaSequenceAgent(riab.Agent(Lead.Environment, {"device": "cpu", "dt": 0.011}))
    ThetaSequenceAgent(riab.Agent(Lead.Environment, {"device": "cpu", "dt": 0.01}))
    with pytest.raises(AssertionError, match="too small"):
        ThetaSequenceAgent(Lead, {"v_sequence": 0.31})
    ThetaSequenceAgent(Lead, {"v_sequence": 0.32})
    with pytest.warns(UserWarning, match="overwritten to match dt of the LeadAgent"):
        S = ShiftAgent(Lead, {"dt": 0.5})
    assert S.dt == Lead.dt
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ShiftAgent(Lead)


def test_refusals(lead):
    riab, Lead = lead
    from ratinabox_amd.contribs.SubAgent import ShiftAgent, ThetaSequenceAgent
    from ratinabox_amd.contribs.TaskEnvironment import TaskEnvironment
    TS, S = ThetaSequenceAgent(Lead), ShiftAgent(Lead)
    for sub in (TS, S):
        with pytest.raises(NotImplementedError, match="open-loop"):
            sub.simulate(10)
        with pytest.raises(NotImplementedError, match="step plan"):
            sub.make_step_plan()
        with pytest.raises(NotImplementedError, match="plotting"):
            sub.plot_trajectory()
    shard = riab.Agent(Lead.Environment, {"device": "cpu", "dt": 0.002, "n_agents": 4, "agent_id0": 8})
    with pytest.raises(NotImplementedError, match="shard"):
        ThetaSequenceAgent(shard)
    env = TaskEnvironment(dt=0.002)
    task_lead = riab.Agent(env, {"device": "cpu", "dt": 0.002})
    with pytest.raises(NotImplementedError, match="SubAgent"):
        env.add_agents(ShiftAgent(task_lead))
