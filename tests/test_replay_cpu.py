"""No-GPU checks of contribs.SubAgent's DumbAgent and ReplayAgent: the float64 restatement (tests/replay_oracle.py) is
pinned to the reference's record (tests/golden/dumb_*.npz, replay_*.npz, written by tests/golden/make_golden_replay.py),
the lazy form of a replay — the kernel's — is shown to give the eager form's positions, the C ABI's new entry points are
checked the way tests/test_subagent_cpu.py checks the theta ones, and the class surface is checked on the CPU device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from oracle import riab_oracle as orc
from tests import golden_util as gu
from tests import replay_oracle as rpo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
ROOMS = ["wall", "periodic", "poly"]


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def load(name):
    """(every array read once: an .npz decompresses an array on each access)"""
    with gu.load(name) as z:
        return {k: z[k] for k in z.files}


def env_of(g):
    boundary, holes = gu.shape_from(g)
    return orc.EnvSpec(boundary_conditions="periodic" if bool(g["periodic"]) else "solid", walls=g["user_walls"],
                       boundary=boundary, holes=holes)


# ---- C1: the DumbAgent's oracle against the reference ------------------------------------------------------------
@pytest.mark.parametrize("room", ROOMS)
def test_dumb_oracle_reproduces_the_reference_bit_for_bit(room):
    """Fed with the lead's recorded positions and the recorded normals, the restatement gives the reference's
    displacement, displacement velocity and position at every step, bit for bit (a dozen float64 operations in the
    reference's own order), and the spring is cut by a wall / the position wraps on the steps the reference did so."""
    g = load(f"dumb_{room}.npz")
    o = rpo.DumbAgentOracle(env_of(g), 1, float(g["dt"]), float(g["drift_distance"]), float(g["drift_timescale"]))
    for t in range(len(g["lead_pos"])):
        pos = o.step(g["lead_pos"][t], g["z"][t].reshape(2, 1))
        np.testing.assert_array_equal(o.displacement_velocity[0], g["vel"][t], err_msg=f"velocity, step {t}")
        np.testing.assert_array_equal(o.displacement[0], g["disp"][t], err_msg=f"displacement, step {t}")
        np.testing.assert_array_equal(pos[0], g["pos"][t], err_msg=f"position, step {t}")
        assert bool(o.cut[0]) == bool(g["cut"][t]) and bool(o.outside[0]) == bool(g["moved"][t]), t
    assert len(g["lead_pos"]) == 600
    if room == "periodic":
        assert o.n_boundary >= 1 and o.n_wall_cuts == 0
    else:
        assert o.n_wall_cuts >= 1


# ---- C2: the ReplayAgent's oracle ---------------------------------------------------------------------------------
# oracle.agent_step is not the reference's arithmetic to the bit (tests/test_subagent_cpu.py: it rounds a step's length
# and a few products in another order).  Over the 22 recorded replays (59 to 727 sham updates each, 5268 table entries)
# the eager oracle's tables stay within 5.55e-16 of the reference's (wall 5.55e-16, periodic 3.33e-16, poly 5.55e-16);
# the bound on replay positions is that measured deviation with a margin of 4 (the positions themselves come out within
# 6.66e-16; the lazy form within 7.91e-16 of the eager one).  Both figures are printed by the tests and recorded in
# docs/EXPERIMENTS.md.  Flags, counts and the positions outside replays are exact.
REPLAY_DEVIATION = 5.6e-16
REPLAY_TOL = 4 * REPLAY_DEVIATION
# The lazy form is given room for the fastest replays of the fixtures (speed draws of 2.1-2.5 m/s over a sham agent that
# crawls): with the class's default bound, 4 x the expected sham steps per update + 8 = 58, ten of the 291 replay steps
# of the three runs run out of steps; the equality below is about the design, not about that bound.
LAZY_STEPS_MAX = 1024


def replays_of(g):
    """start step -> (index, normals (count, 2))"""
    out, zi = {}, 0
    for i, (step, n) in enumerate(zip(g["start_step"], g["count"])):
        out[int(step)] = (i, g["roll_z"][zi:zi + int(n)])
        zi += int(n)
    return out


def replay_oracle_of(g, mode, steps_max=None):
    sham = {str(k): float(v) for k, v in zip(g["sham_keys"], g["sham_vals"])}
    return rpo.ReplayAgentOracle(env_of(g), 1, float(g["dt"]), mode, sham, float(g["replay_freq"]), float(g["replay_duration"]),
                                 float(g["replay_speed"]), steps_max=steps_max)


def run_replay_oracle(g, mode):
    """the oracle's positions and flags over the fixture's run; lazy: lane 0 consumes the replay's recorded normals in
    order, `K` per call at the most"""
    o, reps = replay_oracle_of(g, mode, LAZY_STEPS_MAX if mode == "lazy" else None), replays_of(g)
    pos, flag, cursor, zrep = [], [], 0, None
    for t in range(len(g["flag"])):
        draws = None
        if not np.isnan(g["u"][t]):
            draws = dict(u=np.array([g["u"][t]]))
            if t in reps:
                i, zrep = reps[t]
                cursor = 0
                draws.update(speed=g["speed"][i:i + 1], duration=g["duration"][i:i + 1], pos=g["start_pos"][i].reshape(2, 1),
                             direction=g["direction"][i:i + 1])
        if mode == "eager":
            z = [zrep] if t in reps else None
        else:
            z = np.zeros((o.K, 2, 1))
            if zrep is not None:
                chunk = zrep[cursor:cursor + o.K]
                z[:len(chunk), :, 0] = chunk
        pos.append(o.step(g["lead_pos"][t], float(g["t_entry"][t]), draws=draws, z=z)[0])
        flag.append(bool(o.flag[0]))
        if mode == "lazy":
            cursor += int(o.steps_taken[0])
    return o, np.array(pos), np.array(flag)


@pytest.fixture(scope="module", params=ROOMS)
def replay_runs(request):
    g = load(f"replay_{request.param}.npz")
    return request.param, g, run_replay_oracle(g, "eager"), run_replay_oracle(g, "lazy")


def test_replay_fixture_covers_both_endings(replay_runs):
    _room, g, _e, _l = replay_runs
    flag = g["flag"]
    ended = int((flag[:-1] & ~flag[1:]).sum())
    assert ended >= 5 and flag[-1] and len(g["start_step"]) == ended + 1, "replays that end inside the run and one it cuts off"
    assert not flag[0] and g["t_entry"][0] == 0.0
    np.testing.assert_array_equal(g["t_entry"][1:], g["lead_t"][1:])       # the clock a ReplayAgent compares with


def test_replay_eager_oracle_against_the_reference(replay_runs):
    room, g, (o, pos, flag), _l = replay_runs
    np.testing.assert_array_equal(flag, g["flag"])
    np.testing.assert_array_equal(pos[~g["flag"]], g["lead_pos"][~g["flag"]])
    np.testing.assert_array_equal(pos[~g["flag"]], g["pos"][~g["flag"]])
    np.testing.assert_array_equal(o.rollout_counts, g["count"])
    # the deviation of oracle.agent_step from the reference over these rollouts: every entry of every table
    ti, dev = 0, 0.0
    for (d, p), n in zip(o.rollout_tables, g["count"]):
        n = int(n) + 1
        dev = max(dev, np.abs(d - g["table_dist"][ti:ti + n]).max(), np.abs(p - g["table_pos"][ti:ti + n]).max())
        ti += n
    assert ti == len(g["table_dist"])
    worst = np.abs(pos - g["pos"])[g["flag"]].max()
    print(f"[{room}] oracle.agent_step against the reference over {len(g['count'])} rollouts ({ti} table entries): worst "
          f"deviation {dev:.3g} (recorded {REPLAY_DEVIATION:.3g}); replay positions over {int(g['flag'].sum())} steps "
          f"{worst:.3g} (bound {REPLAY_TOL:.3g})")
    assert dev <= REPLAY_DEVIATION, "the recorded deviation is the worst over the fixtures"
    assert worst <= REPLAY_TOL
    assert o.n_started == len(g["start_step"]) and o.n_ended == o.n_started - 1


def test_replay_lazy_equals_eager(replay_runs):
    """The kernel's design computes the reference's quantity: two records and just enough sham steps per update give the
    positions of the up-front table."""
    room, g, (_oe, pos_e, flag_e), (ol, pos_l, flag_l) = replay_runs
    np.testing.assert_array_equal(flag_l, flag_e)
    np.testing.assert_array_equal(pos_l[~flag_l], g["lead_pos"][~flag_l])
    worst = np.abs(pos_l - pos_e).max()
    print(f"[{room}] lazy against eager: worst deviation {worst:.3g} (bound {REPLAY_TOL:.3g}); most sham steps in one update "
          f"{ol.max_steps_in_a_call} (K = {ol.K})")
    assert worst <= REPLAY_TOL
    np.testing.assert_allclose(pos_l[flag_l], g["pos"][flag_l], rtol=0, atol=REPLAY_TOL)
    assert ol.saturations == 0 and ol.max_steps_in_a_call < ol.K


# ---- C3: the C ABI -----------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("riab_dumb_agent_step", "riab_replay_agent_step")


def test_abi_11_and_new_symbols(L):
    src = open(HEADER).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION == L.lib.riab_abi_version() == 11
    for s in NEW_SYMBOLS:
        assert hasattr(L.lib, s) and s in L.PROTOTYPES and re.search(r"\b%s\(" % s, src), s
        decl = re.search(r"\bint %s\((.*?)\);" % s, src, re.S).group(1)
        assert len(decl.split(",")) == len(L.PROTOTYPES[s][1]), s     # as many arguments as the header declares
    for prefix, names in (("RIAB_DUMB_DIAG_", ("WALL_CUTS", "BOUNDARY", "SATURATIONS")),
                          ("RIAB_REPLAY_DIAG_", ("STARTED", "ENDED", "SATURATIONS", "RESAMPLE")),
                          ("RIAB_RP_", ("SPEED", "T_START", "T_END", "D_START", "LO", "HI")),
                          ("RIAB_RD_", ("U", "SPEED", "DURATION", "POS_X", "POS_Y", "DIRECTION"))):
        for name in names:
            mine = getattr(L, prefix[len("RIAB_"):] + name)
            assert int(re.search(r"%s%s = (\d+)" % (prefix, name), src).group(1)) == mine, prefix + name
    assert int(re.search(r"RIAB_REPLAY_ROWS = (\d+)", src).group(1)) == L.REPLAY_ROWS == L.RP_HI + 3
    assert int(re.search(r"RIAB_REPLAY_DRAWS = (\d+)", src).group(1)) == L.REPLAY_DRAWS


def test_argument_errors_before_launch(L):
    """Negative codes come from validation only: no device needed."""
    env, m, ok = L.RiabEnv(), L.RiabMotion(), C.c_void_p(64)
    m.dt = 0.125
    dumb = L.lib.riab_dumb_agent_step

    def d(env=env, lead=ok, B=8, nreal=None, disp=ok, vel=ok, dt=0.01, out=ok):
        return dumb(env, lead, B, min(B, 5) if nreal is None else nreal, 0, disp, vel, dt, 0.5, 0.1, 1.0, None, None, 1, 0, out,
                    None, None)

    assert d(env=None) == L.EINVAL and d(lead=None) == L.EINVAL and d(disp=None) == L.EINVAL and d(vel=None) == L.EINVAL
    assert d(out=None) == L.EINVAL and d(B=0) == L.EINVAL and d(B=6) == L.EALIGN
    assert d(nreal=9) == L.EINVAL and d(nreal=-1) == L.EINVAL and d(dt=0.0) == L.EINVAL and d(dt=float("nan")) == L.EINVAL
    many = L.RiabEnv()
    many.n_walls, many.walls = L.MAX_WALLS + 1, 64
    assert d(env=many) == L.ETOOBIG

    replay = L.lib.riab_replay_agent_step

    def r(env=env, m=m, lead=ok, sham=ok, B=8, nreal=None, flag=ok, state=ok, K=10, out=ok, steps=ok):
        return replay(env, m, lead, sham, B, min(B, 5) if nreal is None else nreal, 0, flag, state, 0.0, 0.003, 1.0, 0.1, 0.08,
                      None, None, 1, 0, None, None, 2, 0, K, out, steps, None, None, None)

    assert r(env=None) == L.EINVAL and r(m=None) == L.EINVAL and r(lead=None) == L.EINVAL and r(sham=None) == L.EINVAL
    assert r(flag=None) == L.EINVAL and r(state=None) == L.EINVAL and r(out=None) == L.EINVAL and r(steps=None) == L.EINVAL
    assert r(K=0) == L.EINVAL and r(K=-3) == L.EINVAL and r(B=0) == L.EINVAL and r(B=6) == L.EALIGN
    assert r(nreal=9) == L.EINVAL and r(nreal=-1) == L.EINVAL
    drift = L.RiabMotion()
    drift.dt, drift.has_drift = 0.125, 1
    assert r(m=drift) == L.EINVAL


# ---- C4: the classes, device-free --------------------------------------------------------------------------------
@pytest.fixture()
def lead():
    import ratinabox_amd as riab
    np.random.seed(0)
    return riab, riab.Agent(riab.Environment({}), {"n_agents": 3, "device": "cpu", "dt": 0.01})


def test_dumb_agent_surface(lead):
    riab, Lead = lead
    from ratinabox_amd import contribs  # noqa: F401
    from ratinabox_amd.contribs.SubAgent import DumbAgent, SubAgent
    assert DumbAgent.default_params == {"drift_distance": 0.05, "drift_timescale": 3.0} and issubclass(DumbAgent, SubAgent)
    D = DumbAgent(Lead)
    assert isinstance(D, riab.Agent) and D.LeadAgent is Lead and (D.dt, D.n_agents, D._Bp, D.device) == (Lead.dt, 3, 4, "cpu")
    # the derived constants of the reference's constructor (SubAgent.py:147-149)
    assert D.tau_v == 1.5 and D.sigma == np.pi ** 2 * 0.05 / 9.0 and D.acceleration_scale == D.sigma / 0.05
    assert D.displacement.shape == D.displacement_velocity.shape == (3, 2) and not D.displacement.any()
    assert all(t.shape == (2, 4) and t.dtype == __import__("torch").float64 for t in D.displacement_tensors)
    np.testing.assert_array_equal(D.pos, Lead.pos)
    assert not D._auto_enabled
    D2 = DumbAgent(Lead, {"drift_distance": 0.2, "drift_timescale": 1.0})
    assert D2.tau_v == 0.5 and abs(D2.sigma - np.pi ** 2 * 0.2) < 1e-15 and abs(D2.acceleration_scale - np.pi ** 2) < 1e-14
    one = DumbAgent(riab.Agent(Lead.Environment, {"device": "cpu", "dt": 0.01}))
    assert one.displacement.shape == (2,)
    assert D.dumb_diagnostics == dict(wall_cuts=0, boundary_corrections=0, resample_saturations=0)


def test_replay_agent_surface(lead):
    riab, Lead = lead
    from ratinabox_amd.contribs.SubAgent import ReplayAgent, SubAgent
    assert ReplayAgent.default_params == {"replay_freq": 0.3, "replay_duration": 0.1, "replay_speed": 1.0}
    assert issubclass(ReplayAgent, SubAgent)
    R = ReplayAgent(Lead, {"speed_mean": 0.12, "thigmotaxis": 0.2, "replay_speed": 1.5})
    sham = R.ReplayAgent
    assert type(sham) is riab.Agent and (sham.n_agents, sham.device, sham.dt) == (3, "cpu", Lead.dt) and not sham._auto_enabled
    assert sham.speed_mean == 0.12 and sham.thigmotaxis == 0.2             # what was passed to the SubAgent
    assert not any(hasattr(sham, k) for k in ReplayAgent.default_params)    # ... without the three replay keys
    assert sham in Lead.Environment.Agents and sham.rng_seed not in (R.rng_seed, Lead.rng_seed)
    assert (R.mean_replay_speed, R.mean_replay_duration, R.replay_freq) == (1.5, 0.1, 0.3)
    assert R.replay_steps_max == math.ceil(4 * 1.5 / 0.12) + 8 == 58
    assert ReplayAgent(Lead).replay_steps_max == math.ceil(4 * 1.0 / 0.08) + 8 == 58
    assert ReplayAgent(Lead, replay_steps_max=200).replay_steps_max == 200
    assert R.replay_state.shape == (10, 4) and R.replay_draws.shape == (6, 4) and R.replay_normals.shape == (58, 2, 4)
    assert R.replay_steps_taken.shape == (4,) and R.replay_flags.shape == (4,)
    assert R.is_undergoing_replay.shape == (3,) and not R.is_undergoing_replay.any()
    assert "replay" in R.history and R.history["replay"].shape == (0, 3) and len(R.history["t"]) == 0
    assert R.replay_diagnostics == dict(started=0, ended=0, saturations=0, resample_saturations=0)
    one = ReplayAgent(riab.Agent(Lead.Environment, {"device": "cpu", "dt": 0.01}))
    assert np.ndim(one.is_undergoing_replay) == 0 and not one.is_undergoing_replay       # one agent: a scalar


def test_refusals(lead):
    riab, Lead = lead
    from ratinabox_amd.contribs.SubAgent import DumbAgent, ReplayAgent
    from ratinabox_amd.contribs.TaskEnvironment import TaskEnvironment
    for sub in (DumbAgent(Lead), ReplayAgent(Lead)):
        with pytest.raises(NotImplementedError, match="open-loop"):
            sub.simulate(10)
        with pytest.raises(NotImplementedError, match="step plan"):
            sub.make_step_plan()
        with pytest.raises(NotImplementedError, match="plotting"):
            sub.plot_trajectory()
    shard = riab.Agent(Lead.Environment, {"device": "cpu", "dt": 0.01, "n_agents": 4, "agent_id0": 8})
    for cls in (DumbAgent, ReplayAgent):
        with pytest.raises(NotImplementedError, match="shard"):
            cls(shard)
    env = TaskEnvironment(dt=0.01)
    task_lead = riab.Agent(env, {"device": "cpu", "dt": 0.01})
    with pytest.raises(NotImplementedError, match="SubAgent"):
        env.add_agents(DumbAgent(task_lead))
    with pytest.raises(NotImplementedError, match="SubAgent"):
        env.add_agents(ReplayAgent(task_lead))
