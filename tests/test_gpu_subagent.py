"""contribs.SubAgent on the device (csrc/riab_theta_seq.hip) against the float64 oracle tests/subagent_oracle.py, which
tests/test_subagent_cpu.py pins to the reference's record, and against the motion kernel itself.

Bounds.  Interpolation (the sweep given the kernel's own future tables): 1e-12 — a few ulp of values of order 1 through
slopes of order 1.  Look-ahead positions against an oracle that rolls the future out itself: 4 x the deviation, measured
in the same test over the same rollouts, of riab_agent_step (the motion kernel as it was before this file existed) from
oracle.agent_step, floor 1e-12; both figures are printed before they are asserted (docs/EXPERIMENTS.md records them).
Every counter of "the reference would have raised" and of the bounded rollout loop is 0 in every test.

The sweep runs start from distance travelled 0 and last until every lane of the lead has covered d_half, so both look-behind
branches are met without the reference's ValueError: a lead whose distance is pre-set (1 m, say) makes the interpolating
branch live at once, but its window of records does not reach d_half back yet — the reference raises there, the kernel
counts such steps, and the counters are asserted 0 here."""
import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests import golden_util as gu
from tests import subagent_oracle as sao

pytestmark = pytest.mark.gpu

WALL = [[0.5, 0.0], [0.5, 0.5]]
FLOOR = 1e-12


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def _classes():
    from ratinabox_amd.contribs import SubAgent as m
    return m


def _env(riab, kind):
    env = riab.Environment({"boundary_conditions": "periodic"} if kind == "periodic" else {})
    if kind == "wall":
        env.add_wall(np.array(WALL))
    return env


def _oracle_env(kind):
    return orc.EnvSpec(boundary_conditions="periodic" if kind == "periodic" else "solid", walls=[WALL] if kind == "wall" else [])


def _state(ag):
    """float64 state of an agent, (12, B) on the host"""
    ag._sync_plan()
    return ag.state_tensor[:, :ag._B].cpu().numpy()


def _lead_dict(s):
    from ratinabox_amd import _lib as L
    return dict(pos=s[L.S_POS_X:L.S_POS_Y + 1].T.copy(), velocity=s[L.S_VEL_X:L.S_VEL_Y + 1].T.copy(),
                rotational_velocity=s[L.S_ROT_VEL].copy(), distance_travelled=s[L.S_DIST].copy())


def _no_raises(TS):
    d = TS.theta_diagnostics
    assert d["look_behind_raises"] == d["look_ahead_raises"] == d["rollout_saturations"] == 0, d
    return d


def motion_kernel_steps(fwd, m, start, z, n):
    """`n` calls of riab_agent_step(T = 1) — the ForwardSequenceAgent's environment, motion struct `m`, normals z
    [K][2][Bp] (device) — from the state `start` [12][Bp] (device): the states after each call, (n + 1, 12, Bp)."""
    from ratinabox_amd import _lib as L
    env, _walls = fwd.Environment.device_tables(fwd._device)
    st = start.clone()
    out = [st.cpu().numpy()]
    for k in range(n):
        rc = L.lib.riab_agent_step(env, m, L.ptr(st), fwd._Bp, int(fwd.agent_id0), None, L.ptr(z[k]), None, None, None,
                                   int(fwd.rng_seed), 0, 1, None, None, L.current_stream())
        L.check(rc, "riab_agent_step")
        out.append(st.cpu().numpy())
    return np.stack(out)


def rollout_start(TS):
    """What the rollout kernel starts from: the ForwardSequenceAgent's state with the lead's position, velocity,
    rotational velocity and distance."""
    from ratinabox_amd import _lib as L
    start = TS.ForwardSequenceAgent.state_tensor.clone()
    lead = TS._lead_state()
    for r in (L.S_POS_X, L.S_POS_Y, L.S_VEL_X, L.S_VEL_Y, L.S_ROT_VEL, L.S_DIST):
        start[r] = lead[r]
    return start


# ---- G1 ------------------------------------------------------------------------------------------------------------
def test_shift_agent(riab):
    np.random.seed(3)
    env = _env(riab, "wall")
    Lead = riab.Agent(env, {"n_agents": 5, "dt": 0.01})
    plus, minus = _classes().ShiftAgent(Lead, {"shift_m": 0.03}), _classes().ShiftAgent(Lead, {"shift_m": -0.03})
    assert Lead._Bp == plus._Bp == 8
    for _ in range(20):
        Lead.update()
        plus.update()
        minus.update()
        pos, hd = np.asarray(Lead.pos), np.asarray(Lead.head_direction)
        for sub, shift in ((plus, 0.03), (minus, -0.03)):
            err = np.abs(np.asarray(sub.pos) - sao.shift_position(pos, hd, shift)).max()
            assert err <= 1e-15, err
        assert plus.t == minus.t == Lead.t + Lead.dt      # the SubAgent's own Agent.update adds a dt to the lead's clock
    assert np.asarray(plus.history["pos"]).shape == (20, 5, 2)
    assert not np.allclose(np.asarray(plus.pos), np.asarray(Lead.pos))


# ---- G2 ------------------------------------------------------------------------------------------------------------
def test_rollout_is_the_motion_kernel(riab):
    """Every entry of the future table, the counts and the state written back are, bit for bit, what riab_agent_step
    (T = 1 per call, the same normals, the motion struct of dt_forward) gives from the same copied state."""
    from ratinabox_amd import _lib as L
    np.random.seed(4)
    rng = np.random.RandomState(40)
    env = _env(riab, "wall")
    B = 68                                             # one full wave and a partial one
    Lead = riab.Agent(env, {"n_agents": B, "dt": 0.002})
    TS = _classes().ThetaSequenceAgent(Lead)
    for _ in range(50):
        Lead.update(noise=rng.standard_normal((2, B)))
    fwd, K = TS.ForwardSequenceAgent, TS.rollout_steps_max
    z = rng.standard_normal((K, 2, B))
    start = rollout_start(TS)
    m = fwd._motion(TS.dt_forward, False, 1, {})
    zt = fwd._noise_tensor(z, K)
    env_struct, _walls = env.device_tables(fwd._device)
    TS._rollout(TS._lead_state(), env_struct, L.current_stream(), {"noise": z})
    torch.cuda.synchronize()
    table, count = (t.cpu().numpy() for t in TS.future_table)
    final = fwd.state_tensor.cpu().numpy()
    assert fwd._step_index == K
    _no_raises(TS)
    count = count[:B]
    assert count.min() >= 1 and count.max() <= K // 2
    assert len(set(count[:64].tolist())) > 1, "the lanes of the full wave must finish at different steps"
    ref = motion_kernel_steps(fwd, m, start, zt, int(count.max()))
    target = ref[0, L.S_DIST] + TS.forward_distance
    for b in range(B):
        n = int(count[b])
        reached = np.nonzero(ref[:, L.S_DIST, b] >= target[b])[0]
        assert len(reached) and reached[0] == n, (b, n, reached[:1])       # the first entry that reaches the target
        for row, s in ((0, L.S_DIST), (1, L.S_POS_X), (2, L.S_POS_Y)):
            np.testing.assert_array_equal(table[:n + 1, row, b], ref[:n + 1, s, b], err_msg=f"lane {b} row {row}")
        np.testing.assert_array_equal(final[:, b], ref[n, :, b], err_msg=f"final state of lane {b}")
    # the normals the rollout recorded are the ones it was given
    zo = TS.rollout_normals.cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(zo[:count[b], :, b], z[:count[b], :, b])


# ---- G3 / G7: the sweep against the oracle ---------------------------------------------------------------------------
def run_sweep(TS, n_steps, lead_update, rollout_noise, oracle_a, oracle_b):
    """`n_steps` of lead_update(step); TS.update() with explicit rollout normals.  Returns the SubAgent's positions, the
    two oracles' (a: fed the kernel's own future tables; b: rolling out itself), the look-ahead mask and the deviation of
    riab_agent_step from oracle.agent_step over the rollouts."""
    from ratinabox_amd import _lib as L
    Lead, fwd, K, B = TS.LeadAgent, TS.ForwardSequenceAgent, TS.rollout_steps_max, TS._B
    m = fwd._motion(TS.dt_forward, False, 1, {})
    got, ref_a, ref_b, ahead, dev, n_roll, n_interp = [], [], [], [], 0.0, 0, 0
    for step in range(n_steps):
        lead_update(step)
        lead = _lead_dict(_state(Lead))
        phase = TS.theta_phase()
        rolls = phase >= 0.5 and phase < 0.5 + TS.theta_frac / 2 and TS.last_theta_phase < 0.5
        z = fut = None
        if rolls:
            z = rollout_noise(n_roll)
            start, zt = rollout_start(TS), fwd._noise_tensor(z, K)
            TS.update(forward_agent_update_kwargs={"noise": z})
            assert TS.n_rollouts == n_roll + 1
            table, count = (t.cpu().numpy() for t in TS.future_table)
            fut = (table[:, :, :B], count[:B])
        else:
            TS.update()
            assert TS.n_rollouts == n_roll
        got.append(np.asarray(TS.pos).reshape(B, 2))
        ref_a.append(oracle_a.step(lead, Lead.t, future=fut))
        ref_b.append(oracle_b.step(lead, Lead.t, rollout_z=z))
        ahead.append(phase >= 0.5)
        if phase < 0.5:   # look-behind positions that were interpolated from the ring, not the lead's own
            n_interp += int((np.isfinite(got[-1][:, 0]) & (lead["distance_travelled"] >= TS.d_half)).sum())
        assert TS.t == Lead.t + Lead.dt
        if rolls:
            n_roll += 1
            cnt_o = oracle_b.rollouts[-1]["count"]
            np.testing.assert_array_equal(fut[1], cnt_o, err_msg=f"rollout {n_roll}: steps per lane, kernel against oracle")
            steps = motion_kernel_steps(fwd, m, start, zt, int(cnt_o.max()))
            for b in range(B):
                d, p = oracle_b.future[b]
                n = len(d)
                dev = max(dev, np.abs(steps[:n, L.S_DIST, b] - d).max(), np.abs(steps[:n, L.S_POS_X, b] - p[:, 0]).max(),
                          np.abs(steps[:n, L.S_POS_Y, b] - p[:, 1]).max())
    return dict(got=np.array(got), a=np.array(ref_a), b=np.array(ref_b), ahead=np.array(ahead), dev=dev, rollouts=n_roll,
                interpolated=n_interp)


def check_sweep(tag, r, TS, oracle_a, oracle_b):
    got, a, b, ahead = r["got"], r["a"], r["b"], r["ahead"]
    nan = np.isnan(got)
    np.testing.assert_array_equal(nan, np.isnan(a))
    np.testing.assert_array_equal(nan, np.isnan(b))
    err_a = np.nanmax(np.abs(got - a))
    err_behind = np.nanmax(np.abs(got - b)[~ahead]) if (~ahead).any() else 0.0
    err_ahead = np.nanmax(np.abs(got - b)[ahead])
    bound = max(4 * r["dev"], FLOOR)
    d = _no_raises(TS)
    print(f"[{tag}] {r['rollouts']} rollouts; interpolation with the kernel's tables {err_a:.3g} (bound 1e-12); "
          f"riab_agent_step against oracle.agent_step over the rollouts {r['dev']:.3g}; look-ahead against the oracle's own "
          f"rollouts {err_ahead:.3g} (bound {bound:.3g}); look-behind {err_behind:.3g}; dropped by the d_half rule {d['dropped_far']}")
    assert oracle_a.raises["behind"] == oracle_a.raises["ahead"] == oracle_b.raises["saturated"] == 0
    assert d["dropped_far"] == oracle_a.raises["far"] == oracle_b.raises["far"]     # (padding lanes are not counted)
    return err_a, err_behind, err_ahead, bound


SWEEP_STEPS = 1600   # (the slowest of five lanes needs about 1200 steps of 2 ms to cover d_half = 12.5 cm)


@pytest.fixture(scope="module", params=["wall", "periodic"])
def sweep(request, riab):
    kind = request.param
    np.random.seed(7)
    rng = np.random.RandomState(70 + (kind == "periodic"))
    B, dt = 5, 0.002
    Lead = riab.Agent(_env(riab, kind), {"n_agents": B, "dt": dt})
    TS = _classes().ThetaSequenceAgent(Lead)
    oa, ob = (sao.ThetaSequenceOracle(_oracle_env(kind), B, dt, Lead.average_measured_speed) for _ in range(2))
    assert (oa.K, oa.lookback) == (TS.rollout_steps_max, TS.lookback)
    r = run_sweep(TS, SWEEP_STEPS, lambda step: Lead.update(noise=rng.standard_normal((2, B))),
                  lambda n: rng.standard_normal((TS.rollout_steps_max, 2, B)), oa, ob)
    return kind, r, TS, oa, ob


def test_sweep_interpolation_given_the_kernels_tables(sweep):
    kind, r, TS, oa, ob = sweep
    err_a, _behind, _ahead, _bound = check_sweep(kind, r, TS, oa, ob)
    assert err_a <= 1e-12
    # both look-behind branches and the look-ahead were met: every lane has covered d_half by the end
    lead_dist = _state(TS.LeadAgent)[10]
    print(f"[{kind}] lead distances {np.round(lead_dist, 3)}, interpolated look-behind lane-steps {r['interpolated']}")
    assert (lead_dist > TS.d_half).all() and r["rollouts"] == SWEEP_STEPS // 50
    finite_behind = np.isfinite(r["got"][~r["ahead"]][:, :, 0]).sum(axis=0)
    assert (finite_behind >= 100).all() and np.isfinite(r["got"][r["ahead"]][:, :, 0]).sum() >= 1000
    assert r["interpolated"] >= 300
    if kind == "periodic":
        assert TS.Environment.boundary_conditions == "periodic"


def test_sweep_against_the_oracles_own_rollouts(sweep):
    kind, r, TS, oa, ob = sweep
    _a, err_behind, err_ahead, bound = check_sweep(kind, r, TS, oa, ob)
    assert err_behind <= 1e-12
    assert err_ahead <= bound


def test_fixture_replay_with_non_default_parameters(riab):
    """tests/golden/subagent_theta_params.npz on the device: the lead is put through the recorded states, the rollouts
    get the recorded normals.  theta_freq 8, theta_frac 0.6, v_sequence 3 and a speed_mean given to the
    ThetaSequenceAgent alone: the counts only come out if the forward agent moves with THAT speed_mean."""
    with gu.load("subagent_theta_params.npz") as zf:
        g = {k: zf[k] for k in zf.files}
    n_steps = 2400
    np.random.seed(9)
    dt = float(g["dt"])
    Lead = riab.Agent(_env(riab, "open"), {"n_agents": 1, "dt": dt})
    Lead.pos, Lead.velocity = g["pos0"], g["vel0"]
    params = {"theta_freq": float(g["theta_freq"]), "theta_frac": float(g["theta_frac"]), "v_sequence": float(g["v_sequence"])}
    fwd_params = {str(k): float(v) for k, v in zip(g["forward_keys"], g["forward_vals"])}
    params["speed_mean"] = fwd_params["speed_mean"]
    assert params["speed_mean"] != Lead.speed_mean
    TS = _classes().ThetaSequenceAgent(Lead, params)
    oa, ob = (sao.ThetaSequenceOracle(_oracle_env("open"), 1, dt, float(g["lead_average_speed"]), fwd_params,
                                      params["v_sequence"], params["theta_freq"], params["theta_frac"]) for _ in range(2))
    assert TS.rollout_steps_max == int(g["K"]) == oa.K
    K = TS.rollout_steps_max
    zi = np.concatenate(([0], np.cumsum(g["roll_count"])))

    roll_index = {int(s): i for i, s in enumerate(g["roll_step"])}

    def lead_update(step):
        Lead.update(forced_next_position=g["lead_pos"][step])
        if step in roll_index:     # (what a rollout copies besides the position; recorded on the rollouts' steps)
            Lead.velocity, Lead.rotational_velocity = g["roll_lead_vel"][roll_index[step]], g["roll_lead_rot"][roll_index[step]]
        Lead.distance_travelled, Lead.t = g["lead_dist"][step], float(g["lead_t"][step])

    def rollout_noise(n):
        z = np.zeros((K, 2, 1))
        z[:int(g["roll_count"][n]), :, 0] = g["roll_z"][zi[n]:zi[n + 1]]
        return z

    r = run_sweep(TS, n_steps, lead_update, rollout_noise, oa, ob)
    err_a, err_behind, err_ahead, bound = check_sweep("fixture params", r, TS, oa, ob)
    assert err_a <= 1e-12 and err_behind <= 1e-12 and err_ahead <= bound
    n_roll = int((g["roll_step"] < n_steps).sum())
    assert r["rollouts"] == n_roll >= 15
    np.testing.assert_array_equal([x["count"][0] for x in ob.rollouts], g["roll_count"][:n_roll])
    # ... and the reference's own record, which the oracle is within a few ulp of (tests/test_subagent_cpu.py)
    ref = g["sub_pos"][:n_steps]
    np.testing.assert_array_equal(np.isnan(r["got"][:, 0]), np.isnan(ref))
    assert np.nanmax(np.abs(r["got"][:, 0] - ref)) <= bound + 4e-15


# ---- G4 ------------------------------------------------------------------------------------------------------------
def _philox_run(riab, n_steps):
    np.random.seed(12)
    Lead = riab.Agent(_env(riab, "wall"), {"n_agents": 8, "dt": 0.002, "seed": 3})
    TS = _classes().ThetaSequenceAgent(Lead)
    zs = []
    for _ in range(n_steps):
        Lead.update()
        before = TS.n_rollouts
        TS.update()
        if TS.n_rollouts != before:
            torch.cuda.synchronize()
            zs.append((TS.rollout_normals.cpu().numpy().copy(), TS.future_table[1].cpu().numpy().copy()))
    return Lead, TS, zs


def test_philox_rollouts(riab):
    n_steps = 150                                      # three theta cycles
    _lead1, ts1, z1 = _philox_run(riab, n_steps)
    _lead2, ts2, z2 = _philox_run(riab, n_steps)
    p1, p2 = np.asarray(ts1.history["pos"]), np.asarray(ts2.history["pos"])
    assert p1.shape == (n_steps, 8, 2)
    np.testing.assert_array_equal(p1, p2)
    assert 0.3 < np.isnan(p1[:, :, 0]).mean() < 0.7 and np.isfinite(p1[-20:]).any()
    fwd, K = ts1.ForwardSequenceAgent, ts1.rollout_steps_max
    assert len(z1) == 3 and fwd._step_index == 3 * K and ts1.n_rollouts == 3
    assert fwd.rng_seed not in (ts1.rng_seed, ts1.LeadAgent.rng_seed)
    _no_raises(ts1)
    ids = np.arange(8)
    for r, (z, count) in enumerate(z1):
        np.testing.assert_array_equal(z, z2[r][0])
        for k in range(int(count[:8].max())):          # (one wave: every row up to its slowest lane's count is written)
            z_rot, z_spd, _z2, _z3 = orc.motion_normals(fwd.rng_seed, r * K + k, ids)
            # (the Philox words are bit-exact; log2 / sin / cos are the fp32 hardware approximations: the bound of
            # tests/test_gpu_parity.py for the motion kernel's own draws)
            np.testing.assert_allclose(z[k, 0, :8], z_rot, rtol=1e-5, atol=2e-5)
            np.testing.assert_allclose(z[k, 1, :8], z_spd, rtol=1e-5, atol=2e-5)


# ---- G5 ------------------------------------------------------------------------------------------------------------
def _plan_run(riab, auto):
    from ratinabox_amd.plan import AutoStepper
    np.random.seed(13)
    Lead = riab.Agent(_env(riab, "wall"), {"n_agents": 8, "dt": 0.002, "seed": 5})
    lead_pcs = riab.PlaceCells(Lead, {"n": 16, "wall_geometry": "euclidean"})
    TS = _classes().ThetaSequenceAgent(Lead)
    ts_pcs = riab.PlaceCells(TS, {"n": 16, "wall_geometry": "euclidean"})
    if not auto:
        Lead._auto_enabled = False
    engaged = 0
    for _ in range(150):
        Lead.update()
        lead_pcs.update()
        TS.update()
        ts_pcs.update()
        engaged += int(type(Lead._plan) is AutoStepper)
    assert TS._plan is None
    _no_raises(TS)
    return (engaged, np.asarray(TS.history["pos"]), np.asarray(TS.history["t"]), np.asarray(lead_pcs.history["firingrate"]),
            np.asarray(ts_pcs.history["firingrate"]), np.asarray(Lead.history["pos"]))


def test_lead_under_the_automatic_plan(riab):
    on, off = _plan_run(riab, True), _plan_run(riab, False)
    assert on[0] >= 100 and off[0] == 0, "the lead's loop must have been served by the automatic step plan"
    for a, b, what in zip(on[1:], off[1:], ("SubAgent pos", "SubAgent t", "lead rates", "SubAgent rates", "lead pos")):
        assert a.shape == b.shape and a.shape[0] == 150, what
        np.testing.assert_array_equal(a, b, err_msg=what)
    assert np.isfinite(on[1]).any() and np.isnan(on[1]).any()


# ---- G6 ------------------------------------------------------------------------------------------------------------
def test_neurons_on_the_sweep(riab):
    np.random.seed(14)
    Lead = riab.Agent(_env(riab, "wall"), {"n_agents": 8, "dt": 0.002})
    TS = _classes().ThetaSequenceAgent(Lead)
    PCs = riab.PlaceCells(TS, {"n": 16, "wall_geometry": "euclidean", "widths": 0.15})
    n_nan = n_fin = 0
    for _ in range(120):
        Lead.update()
        TS.update()
        PCs.update()
        pos, fr = np.asarray(TS.pos), np.asarray(PCs.firingrate)
        nan = np.isnan(pos[:, 0])
        assert fr.shape == (16, 8)
        assert not fr[:, nan].any(), "zero rates while the position is NaN"
        if (~nan).any():
            again = PCs.get_state(evaluate_at=None, pos=pos[~nan])
            np.testing.assert_array_equal(fr[:, ~nan], again)
            assert fr[:, ~nan].max() > 0
        n_nan, n_fin = n_nan + int(nan.sum()), n_fin + int((~nan).sum())
    assert n_nan >= 300 and n_fin >= 300
    _no_raises(TS)
