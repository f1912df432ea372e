"""contribs.SubAgent's DumbAgent and ReplayAgent on the device (csrc/riab_subagent.hip) against the float64 oracle
tests/replay_oracle.py, which tests/test_replay_cpu.py pins to the reference's record, and against the motion kernel
itself.

Shapes: B = 5 (padded to 8: a partial wave with padding lanes) and B = 68 (a full wave and a partial one).

Bounds.  DumbAgent: 1e-12 per step, the oracle stepped from the device's own previous state (a handful of float64
operations on values <= 1).  Replay interpolation given the kernel's own records: 1e-12.  Replay positions against an
oracle that moves its own sham agent: 4 x the deviation, measured in the same run over the same steps, of
riab_agent_step (the motion kernel as it was before this file existed) from oracle.agent_step, floor 1e-12; both figures
are printed before they are asserted (docs/EXPERIMENTS.md records them).

The replay runs' seed, speeds and `replay_steps_max` were checked on the CPU with the lazy oracle before they were
committed: the most sham steps any lane needs in one update is 42 (wall), 34 (periodic), 25 (poly) < 64, so the counter of
lanes that ran out of steps stays 0 by the reference's own arithmetic."""
import numpy as np
import pytest
import torch

from oracle import riab_oracle as orc
from tests import replay_oracle as rpo

pytestmark = pytest.mark.gpu

WALL = [[0.5, 0.0], [0.5, 0.5]]
L_ROOM = [[0.0, 0.0], [1.0, 0.0], [1.0, 0.6], [0.6, 0.6], [0.6, 1.0], [0.0, 1.0]]
HOLE = [[0.15, 0.15], [0.3, 0.15], [0.3, 0.3], [0.15, 0.3]]
FLOOR = 1e-12
DT = 0.01
RTOL = 1e-5     # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


def _classes():
    from ratinabox_amd.contribs import SubAgent as m
    return m


def _env(riab, kind):
    if kind == "poly":
        return riab.Environment({"boundary": L_ROOM, "holes": [HOLE]})
    env = riab.Environment({"boundary_conditions": "periodic"} if kind == "periodic" else {})
    if kind == "wall":
        env.add_wall(np.array(WALL))
    return env


def _oracle_env(kind):
    if kind == "poly":
        return orc.EnvSpec(boundary=L_ROOM, holes=[HOLE])
    return orc.EnvSpec(boundary_conditions="periodic" if kind == "periodic" else "solid", walls=[WALL] if kind == "wall" else [])


def _state(ag):
    """float64 state of an agent, (12, B) on the host"""
    ag._sync_plan()
    return ag.state_tensor[:, :ag._B].cpu().numpy()


def assert_rates(got, ref, scale=1.0, floor=0.0):
    """|got-ref| <= RTOL*|ref| + floor*RTOL*scale (+ fp32 underflow): the check of tests/test_gpu_parity.py"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape
    tol = RTOL * np.abs(ref) + floor * RTOL * scale + 1e-37
    bad = np.abs(got - ref) > tol
    assert not bad.any(), f"{bad.sum()} / {bad.size} outside tolerance; worst abs err {np.max(np.abs(got - ref)):.3e}"


# ---- G1: the DumbAgent, step by step ----------------------------------------------------------------------------------
def lead_path(kind, B, n_steps, rng):
    """A lead that stays where the spring meets the room: beside the wall (both sides of it), or by the edges and corners
    of the periodic box.  (n_steps, B, 2), strictly inside the box."""
    t = np.arange(1, n_steps + 1)[:, None]
    phase = rng.uniform(0, 2 * np.pi, B)[None, :]
    if kind == "wall":
        side = np.where(np.arange(B) % 2 == 0, -1.0, 1.0)
        x0 = 0.5 + side * rng.uniform(0.012, 0.035, B)
        y0 = rng.uniform(0.08, 0.42, B)
        x = x0[None, :] + 0.008 * np.sin(2 * np.pi * t / 140 + phase)
        y = y0[None, :] + 0.05 * np.sin(2 * np.pi * t / 190 + phase)
    else:
        x0 = np.where(np.arange(B) % 2 == 0, rng.uniform(0.02, 0.04, B), rng.uniform(0.96, 0.98, B))
        y0 = np.where(np.arange(B) % 3 == 0, rng.uniform(0.96, 0.98, B), rng.uniform(0.1, 0.9, B))
        x = x0[None, :] + 0.015 * np.sin(2 * np.pi * t / 140 + phase)
        y = y0[None, :] + 0.015 * np.sin(2 * np.pi * t / 190 + phase)
    return np.stack((x, y), axis=-1)


DUMB_STEPS = 300


@pytest.mark.parametrize("kind,B,philox", [("wall", 68, False), ("periodic", 68, False), ("periodic", 5, False),
                                           ("periodic", 5, True)])
def test_dumb_agent_one_step_parity(riab, kind, B, philox):
    """After every step the displacement, its velocity and the position are the oracle's, stepped from the device's own
    previous state with the same normals, to 1e-12 — every lane, every step — and the kernel's counters are the
    oracle's over the real lanes (B = 5: the three padding lanes repeat lane 0's lead, which sits by the edge — with
    explicit normals they repeat lane 0, with the agent's own Philox stream, whose recorded normals feed the oracle, they
    wander by themselves — and are not counted)."""
    np.random.seed(21)
    rng = np.random.RandomState({("wall", 68): 279, ("periodic", 68): 278, ("periodic", 5): 216}[kind, B])
    Lead = riab.Agent(_env(riab, kind), {"n_agents": B, "dt": DT})
    Dumb = _classes().DumbAgent(Lead)
    o = rpo.DumbAgentOracle(_oracle_env(kind), B, DT)
    path = lead_path(kind, B, DUMB_STEPS, rng)
    worst = dict(disp=0.0, vel=0.0, pos=0.0)
    lane0_events = 0
    for t in range(DUMB_STEPS):
        Lead.update(forced_next_position=path[t])
        z = rng.standard_normal((2, B))
        if philox:
            Dumb.update()
            z = Dumb.step_normals[:, :B].cpu().numpy()
        else:
            Dumb.update(noise=torch.as_tensor(z))
        lead_pos = _state(Lead)[0:2].T
        np.testing.assert_array_equal(lead_pos, path[t])
        ref = o.step(lead_pos, z)
        disp, vel = (x[:, :B].cpu().numpy().T for x in Dumb.displacement_tensors)
        pos = _state(Dumb)[0:2].T
        worst["disp"] = max(worst["disp"], np.abs(disp - o.displacement).max())
        worst["vel"] = max(worst["vel"], np.abs(vel - o.displacement_velocity).max())
        worst["pos"] = max(worst["pos"], np.abs(pos - ref).max())
        lane0_events += int(o.cut[0]) + int(o.outside[0])
        o.displacement, o.displacement_velocity = disp.copy(), vel.copy()      # the next step starts from the device's state
        assert Dumb.t == Lead.t + Lead.dt
    d = Dumb.dumb_diagnostics
    print(f"[dumb {kind} B={B}{' philox' if philox else ''}] worst |delta| displacement {worst['disp']:.3g}, velocity "
          f"{worst['vel']:.3g}, position {worst['pos']:.3g} (bound 1e-12); cut by the wall {o.n_wall_cuts} lane-steps, moved by the boundary conditions "
          f"{o.n_boundary}; kernel counters {d}")
    assert max(worst.values()) <= 1e-12
    if kind == "wall":
        assert o.n_wall_cuts >= 1
    else:
        assert o.n_boundary >= 1
    assert (d["wall_cuts"], d["boundary_corrections"], d["resample_saturations"]) == (o.n_wall_cuts, o.n_boundary, 0)
    if B == 5:
        assert Dumb._Bp == 8
    if B == 5 and not philox:
        assert lane0_events >= 1, "the lane the padding repeats must have been counted once per event"
    assert np.asarray(Dumb.history["pos"]).shape == (DUMB_STEPS, B, 2)
    np.testing.assert_array_equal(np.asarray(Dumb.displacement), disp)


# ---- G2: the DumbAgent on its own Philox stream ------------------------------------------------------------------------
def _dumb_philox_run(riab, B, n_steps):
    np.random.seed(22)
    Lead = riab.Agent(_env(riab, "periodic"), {"n_agents": B, "dt": DT, "seed": 4})
    Dumb = _classes().DumbAgent(Lead, {"seed": 9})
    mags = []
    for _ in range(n_steps):
        Lead.update()
        Dumb.update()
        mags.append(torch.sqrt((Dumb.displacement_tensors[0][:, :B] ** 2).sum(dim=0)))
    return Dumb, torch.stack(mags).cpu().numpy()


def test_dumb_agent_philox_stream(riab):
    B, T = 68, DUMB_STEPS
    d1, m1 = _dumb_philox_run(riab, B, T)
    d2, m2 = _dumb_philox_run(riab, B, T)
    np.testing.assert_array_equal(np.asarray(d1.history["pos"]), np.asarray(d2.history["pos"]))
    np.testing.assert_array_equal(m1, m2)
    np.testing.assert_array_equal(d1.displacement_velocity, d2.displacement_velocity)
    z = d1.step_normals[:, :B].cpu().numpy()
    assert np.isfinite(z).all() and len(np.unique(z)) == 2 * B            # every lane its own normals
    # the oracle's own run of the same length on NumPy normals: its lanes are independent, so the spread of their time
    # averages gives the standard error of the mean over B x T
    rng = np.random.RandomState(220)
    o = rpo.DumbAgentOracle(_oracle_env("periodic"), B, DT)
    lead = np.full((B, 2), 0.5)
    mo = np.empty((T, B))
    for t in range(T):
        o.step(lead, rng.standard_normal((2, B)))
        mo[t] = np.sqrt((o.displacement ** 2).sum(axis=1))
    mean_o, se = mo.mean(), mo.mean(axis=0).std(ddof=1) / np.sqrt(B)
    print(f"[dumb philox] mean |displacement| over {B} x {T}: device {m1.mean():.5f}, oracle {mean_o:.5f}, standard error "
          f"{se:.5f} ({abs(m1.mean() - mean_o) / se:.2f} of them apart)")
    assert abs(m1.mean() - mean_o) <= 5 * se


# ---- G3 / G4: replays with explicit draws and normals -------------------------------------------------------------------
REPLAY_STEPS = 400
REPLAY_PARAMS = {"replay_freq": 5.0, "replay_speed": 0.15}
REPLAY_STEPS_MAX = 64


def make_draws(rng, oenv, B):
    """the outcomes of one update's five draws for every lane"""
    e = oenv.extent
    pos = np.stack((rng.uniform(e[0], e[1], B), rng.uniform(e[2], e[3], B)), axis=-1)
    out = ~orc.env_is_inside(oenv, pos)
    while out.any():       # (Environment.sample_positions: rejected until inside)
        pos[out] = np.stack((rng.uniform(e[0], e[1], out.sum()), rng.uniform(e[2], e[3], out.sum())), axis=-1)
        out = ~orc.env_is_inside(oenv, pos)
    return dict(u=rng.uniform(size=B), speed=rng.rayleigh(REPLAY_PARAMS["replay_speed"], B), duration=rng.rayleigh(0.1, B),
                pos=pos.T.copy(), direction=rng.uniform(0, 2 * np.pi, B))


def sham_state_dict(s):
    """rows of a state matrix (12, B) -> the oracle's state dict"""
    return dict(pos=s[0:2].T.copy(), velocity=s[2:4].T.copy(), rotational_velocity=s[4].copy(), measured_velocity=s[5:7].T.copy(),
                measured_rotational_velocity=s[7].copy(), head_direction=s[8:10].T.copy(), distance_travelled=s[10].copy(),
                distance_to_closest_wall=s[11].copy())


def motion_kernel_steps(sham, m, start, z, n):
    """`n` calls of riab_agent_step(T = 1) — the sham agent's environment, motion struct `m`, normals z [K][2][Bp]
    (device) — from the state `start` [12][Bp] (device): the states after each call, (n + 1, 12, Bp)."""
    from ratinabox_amd import _lib as L
    env, _walls = sham.Environment.device_tables(sham._device)
    st = start.clone()
    out = [st.cpu().numpy()]
    for k in range(n):
        rc = L.lib.riab_agent_step(env, m, L.ptr(st), sham._Bp, int(sham.agent_id0), None, L.ptr(z[k]), None, None, None,
                                   int(sham.rng_seed), 0, 1, None, None, L.current_stream())
        L.check(rc, "riab_agent_step")
        out.append(st.cpu().numpy())
    return np.stack(out)


@pytest.fixture(scope="module", params=["wall", "periodic", "poly"])
def replay_run(request, riab):
    """400 steps of `Lead.update(); Rep.update(draws, noise)`; per call the kernel's records and sham state are compared
    with riab_agent_step(T = 1) from the same start, and the lazy oracle is fed what the kernel used."""
    from ratinabox_amd import _lib as L
    kind = request.param
    B, K = 68, REPLAY_STEPS_MAX
    np.random.seed(31)
    rng = np.random.RandomState(310 + ["wall", "periodic", "poly"].index(kind))
    oenv = _oracle_env(kind)
    Lead = riab.Agent(_env(riab, kind), {"n_agents": B, "dt": DT})
    Rep = _classes().ReplayAgent(Lead, dict(REPLAY_PARAMS), replay_steps_max=K)
    sham = Rep.ReplayAgent
    o = rpo.ReplayAgentOracle(oenv, B, DT, "lazy", None, REPLAY_PARAMS["replay_freq"], 0.1, REPLAY_PARAMS["replay_speed"],
                              steps_max=K, sham_state=sham_state_dict(_state(sham)))
    m = sham._motion(DT, False, 1, {})
    r = dict(kind=kind, Rep=Rep, o=o, got=[], ref=[], lead=[], flag=[], flag_o=[], bits_checked=0, interp_err=0.0, dev=0.0,
             lanes_stepping=set(), max_steps=0)
    for step in range(REPLAY_STEPS):
        Lead.update(noise=rng.standard_normal((2, B)))
        draws = make_draws(rng, oenv, B)
        z = rng.standard_normal((K, 2, B))
        t_entry = float(Rep.t)
        start = sham.state_tensor.clone()
        before = Rep.replay_state.cpu().numpy()
        Rep.update(draws=draws, noise=z)
        assert Rep.t == Lead.t + Lead.dt and sham._step_index == (step + 1) * K
        n = Rep.replay_steps_taken[:B].cpu().numpy()
        after, flag = Rep.replay_state.cpu().numpy(), Rep.replay_flags[:B].cpu().numpy().astype(bool)
        used, zu = Rep.replay_draws[:, :B].cpu().numpy(), Rep.replay_normals[:, :, :B].cpu().numpy()
        pos, lead = _state(Rep)[0:2].T, _state(Lead)[0:2].T
        final = _state(sham)
        # ---- the records are the motion kernel's (G3)
        if n.max() > 0:
            steps = motion_kernel_steps(sham, m, start, sham._noise_tensor(z, K), int(n.max()))
            for b in np.nonzero(n)[0]:
                k = int(n[b])
                d0 = after[L.RP_D_START, b]
                hi = (steps[k, L.S_DIST, b] - d0, steps[k, L.S_POS_X, b], steps[k, L.S_POS_Y, b])
                lo = (steps[k - 1, L.S_DIST, b] - d0, steps[k - 1, L.S_POS_X, b], steps[k - 1, L.S_POS_Y, b]) if k > 1 else \
                    tuple(before[L.RP_HI:L.RP_HI + 3, b])
                np.testing.assert_array_equal(after[L.RP_HI:L.RP_HI + 3, b], hi, err_msg=f"step {step} lane {b}: newer record")
                np.testing.assert_array_equal(after[L.RP_LO:L.RP_LO + 3, b], lo, err_msg=f"step {step} lane {b}: older record")
                np.testing.assert_array_equal(final[:, b], steps[k, :, b], err_msg=f"step {step} lane {b}: sham state")
                np.testing.assert_array_equal(zu[:k, :, b], z[:k, :, b])
                r["bits_checked"] += 1
            r["lanes_stepping"].update(np.nonzero(n)[0].tolist())
        idle = (n == 0) & ~np.isfinite(used[L.RD_SPEED])                  # neither stepped nor started: the state is kept
        np.testing.assert_array_equal(final[:, idle], start[:, :B].cpu().numpy()[:, idle])
        # ---- pos_out is the interpolation of those records
        moving = flag & np.isnan(used[L.RD_U])                           # in a replay that goes on
        for b in np.nonzero(moving)[0]:
            q = after[L.RP_SPEED, b] * (t_entry - after[L.RP_T_START, b])
            lo, hi = after[L.RP_LO:L.RP_LO + 3, b], after[L.RP_HI:L.RP_HI + 3, b]
            assert lo[0] < q <= hi[0], (step, b, lo[0], q, hi[0])
            want = (hi[1:] - lo[1:]) / (hi[0] - lo[0]) * (q - lo[0]) + lo[1:]
            r["interp_err"] = max(r["interp_err"], np.abs(pos[b] - want).max())
        # ---- the oracle, fed what the kernel used (G4)
        np.testing.assert_array_equal(used[L.RD_U][~np.isnan(used[L.RD_U])], draws["u"][~np.isnan(used[L.RD_U])])
        fed = dict(u=np.where(np.isnan(used[L.RD_U]), 2.0, used[L.RD_U]), speed=used[L.RD_SPEED], duration=used[L.RD_DURATION],
                   pos=used[L.RD_POS_X:L.RD_POS_Y + 1], direction=used[L.RD_DIRECTION])
        ref = o.step(lead, t_entry, draws=fed, z=zu, n_steps=n)
        stepped = n > 0
        if stepped.any():   # riab_agent_step against oracle.agent_step over the same steps: the newest records
            r["dev"] = max(r["dev"], np.abs(after[L.RP_HI, :B][stepped] - o.hi_d[stepped]).max(),
                           np.abs(after[L.RP_HI + 1:L.RP_HI + 3, :B].T[stepped] - o.hi_p[stepped]).max())
        r["max_steps"] = max(r["max_steps"], int(n.max()))
        r["got"].append(pos)
        r["ref"].append(ref)
        r["lead"].append(lead)
        r["flag"].append(flag)
        r["flag_o"].append(o.flag.copy())
    for k in ("got", "ref", "lead", "flag", "flag_o"):
        r[k] = np.array(r[k])
    return r


def test_replay_is_the_motion_kernel(replay_run):
    r = replay_run
    Rep = r["Rep"]
    print(f"[replay {r['kind']}] {r['bits_checked']} (call, lane) pairs compared bit for bit with riab_agent_step(T = 1); pos_out "
          f"against the host's interpolation of the records {r['interp_err']:.3g} (bound 1e-12); most sham steps in one update "
          f"{r['max_steps']} (K = {Rep.replay_steps_max})")
    assert r["bits_checked"] >= 1000 and r["interp_err"] <= 1e-12
    assert len(r["lanes_stepping"]) == 68 and r["max_steps"] >= 8, "every lane of both waves has replayed"


def test_replay_against_the_oracle(replay_run):
    r = replay_run
    Rep, o = r["Rep"], r["o"]
    np.testing.assert_array_equal(r["flag"], r["flag_o"])
    np.testing.assert_array_equal(r["got"][~r["flag"]], r["lead"][~r["flag"]])
    np.testing.assert_array_equal(r["ref"][~r["flag"]], r["lead"][~r["flag"]])
    err = np.abs(r["got"] - r["ref"])[r["flag"]].max()
    bound = max(4 * r["dev"], FLOOR)
    d = Rep.replay_diagnostics
    print(f"[replay {r['kind']}] {int(r['flag'].sum())} lane-steps in replay of {r['flag'].size}; riab_agent_step against "
          f"oracle.agent_step over the replays {r['dev']:.3g}; positions against the oracle {err:.3g} (bound {bound:.3g}); "
          f"step counts the oracle would have chosen differently {o.steps_disagree}; {d}")
    assert err <= bound
    assert d["saturations"] == 0 and d["resample_saturations"] == 0 and o.saturations == 0 and o.steps_disagree == 0
    assert Rep.ReplayAgent.diagnostics["bounce_saturations"] == 0      # (the sham agent's bounce and resample loops)
    assert d["started"] == o.n_started >= 68 and d["ended"] == o.n_ended >= 68
    hist = np.asarray(Rep.history["replay"])
    assert hist.shape == (REPLAY_STEPS, 68) and hist.dtype == bool
    np.testing.assert_array_equal(hist, r["flag"])
    assert 0.2 < r["flag"].mean() < 0.6


# ---- G5: replays on the agents' own Philox streams ----------------------------------------------------------------------
def _replay_philox_run(riab, n_steps):
    np.random.seed(41)
    Lead = riab.Agent(_env(riab, "wall"), {"n_agents": 68, "dt": DT, "seed": 6})
    Rep = _classes().ReplayAgent(Lead, {"replay_freq": 5.0})     # (its key and the sham agent's: derived from their indices)
    outside = 0
    for _ in range(n_steps):
        outside += int((Rep.replay_flags[:68] == 0).sum())       # lanes that draw the trigger in this update
        Lead.update()
        Rep.update()
    return Lead, Rep, outside


def test_replay_philox_streams(riab):
    n_steps = 300
    _l1, r1, outside = _replay_philox_run(riab, n_steps)
    _l2, r2, _ = _replay_philox_run(riab, n_steps)
    p1, f1 = np.asarray(r1.history["pos"]), np.asarray(r1.history["replay"])
    np.testing.assert_array_equal(p1, np.asarray(r2.history["pos"]))
    np.testing.assert_array_equal(f1, np.asarray(r2.history["replay"]))
    assert p1.shape == (n_steps, 68, 2) and f1.shape == (n_steps, 68) and np.isfinite(p1).all()
    for b in range(4):                                              # the same lane of the two waves: its own draws
        assert not np.array_equal(f1[:, b], f1[:, b + 64]), b
    sham = r1.ReplayAgent
    assert sham._step_index == n_steps * r1.replay_steps_max and len({sham.rng_seed, r1.rng_seed, r1.LeadAgent.rng_seed}) == 3
    d = r1.replay_diagnostics
    p = r1.replay_freq * DT
    expect, sd = p * outside, np.sqrt(outside * p * (1 - p))
    print(f"[replay philox] {d['started']} replays started in {outside} lane-steps outside replay: expected {expect:.1f} +- "
          f"{sd:.1f}; {d}")
    assert abs(d["started"] - expect) <= 5 * sd
    starts = (f1[1:] & ~f1[:-1]).sum() + f1[0].sum()
    assert starts == d["started"] and d["resample_saturations"] == 0
    # every started replay ends: no new ones from here on
    r1.replay_freq = 0.0
    for _ in range(200):
        r1.LeadAgent.update()
        r1.update()
        if not r1.is_undergoing_replay.any():
            break
    d = r1.replay_diagnostics
    assert not r1.is_undergoing_replay.any() and d["started"] == d["ended"]


# ---- G6: neurons on a ReplayAgent whose lead runs under the automatic step plan -------------------------------------------
def test_place_cells_on_a_replay_agent(riab):
    from ratinabox_amd.plan import AutoStepper
    np.random.seed(51)
    B, T = 5, 150
    Lead = riab.Agent(_env(riab, "wall"), {"n_agents": B, "dt": DT, "seed": 5})
    lead_pcs = riab.PlaceCells(Lead, {"n": 16, "wall_geometry": "euclidean"})
    Rep = _classes().ReplayAgent(Lead, {"replay_freq": 5.0})
    pcs = riab.PlaceCells(Rep, {"n": 16, "wall_geometry": "euclidean", "widths": 0.2})
    engaged, n_replay = 0, 0
    oenv = _oracle_env("wall")
    for _ in range(T):
        Lead.update()
        lead_pcs.update()
        Rep.update()
        pcs.update()
        engaged += int(type(Lead._plan) is AutoStepper)
        flag = np.atleast_1d(Rep.is_undergoing_replay)
        if flag.any():
            pos = np.asarray(Rep.pos, dtype=np.float32).astype(np.float64).reshape(B, 2)   # (the rate kernels read fp32 rows)
            ref = orc.place_cells(oenv, pos[flag], pcs.place_cell_centres, 0.2)
            assert_rates(np.asarray(pcs.firingrate)[:, flag], ref)
            n_replay += int(flag.sum())
    assert engaged >= 100, "the lead's loop must have been served by the automatic step plan"
    assert Rep._plan is None and n_replay >= 50
    assert np.asarray(Rep.history["pos"]).shape == (T, B, 2)
    hist = np.asarray(Rep.history["replay"])
    assert hist.shape == (T, B) and hist.sum() == n_replay
    moved = np.abs(np.asarray(Rep.history["pos"]) - np.asarray(Lead.history["pos"])).max(axis=-1) > 0
    np.testing.assert_array_equal(moved & ~hist, np.zeros_like(hist))       # outside replays the position is the lead's
    d = Rep.replay_diagnostics
    assert d["started"] >= 5 and d["resample_saturations"] == 0
