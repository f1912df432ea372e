"""`SubAgent`, `ThetaSequenceAgent`, `DumbAgent`, `ReplayAgent`, `ShiftAgent`, `UnrelatedAgent` — Agents slaved to another
Agent, on the device (reference ratinabox/contribs/SubAgent.py).

A SubAgent is an `Agent` of its lead's Environment whose position is a function of the lead's state: lane b of the
SubAgent follows lane b of the lead (`n_agents`, `device` and `dt` are the lead's).  Its position is computed by a
kernel of csrc/riab_theta_seq.hip or csrc/riab_subagent.hip from the lead's float64 state matrix and handed — a device
tensor, nothing visits the host — to the forced-position step every Agent has (`riab_agent_step(forced_pos=...)`), so
history, measured velocity and any `Neurons` population built on the SubAgent work as on any other Agent through their
eager `update()`.

`ThetaSequenceAgent`: once per theta cycle (`theta_freq`) the position sweeps at `v_sequence` from `d_half` behind the
lead, along the lead's own past, to `d_half` ahead of it, along a future simulated by the motion model from the lead's
position and velocity; outside the sweep (`theta_frac` of the cycle) the position is NaN.  `PlaceCells` on it show
theta sweeps and phase precession (their rate is zero while the position is NaN).

    Lead = Agent(Env, {"dt": 0.002, "n_agents": 1024})
    TS = ThetaSequenceAgent(Lead)
    PCs = PlaceCells(TS, {"n": 64})
    for _ in range(5000):
        Lead.update(); TS.update(); PCs.update()

Device memory: the look-behind needs the lead's last `lookback = int(5 d_half / (dt * average_measured_speed))` records
of (distance, x, y) per lane: 24 bytes x lookback x agents (dt 2 ms, defaults: 3906 records, 384 MB at 4096 agents; dt
1 ms: 7812 records, 768 MB).  The future table is `[K + 1][3]` float64 per lane, K = ceil(4 forward_distance / (dt
v_sequence)) + 8 steps: the bound on the reference's unbounded rollout loop (`theta_diagnostics["rollout_saturations"]`).

`DumbAgent`: a wrong position on a spring round the lead (`drift_distance`, `drift_timescale`), cut short where a wall
stands between the two, one launch per step.

`ReplayAgent`: the lead's position, except while a lane "replays": it jumps to a random place, explores there at its
replay speed and snaps back; `history["replay"]` flags those steps.  One launch per step; the replayed path is produced
as it is consumed (two records per lane), not as the reference's up-front table.

Not built: 1D environments, plotting.  A SubAgent cannot run inside `Agent.simulate()`, a
step plan or a `TaskEnvironment`, nor follow a shard of a multi-GPU run (NotImplementedError)."""
import copy
import math
import warnings

import numpy as np
import torch

from .. import _lib as _L
from .._history import HistoryView
from ..Agent import Agent


class SubAgent(Agent):
    """An Agent "subservient" to `LeadAgent` (SubAgent.py:10-36).  Subclasses compute a position from the lead's state
    in `update()`; the base class moves like an ordinary Agent on the lead's clock."""

    default_params = {}
    _is_subagent = True

    def __init__(self, LeadAgent, params={}):
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        self.LeadAgent = LeadAgent
        if int(getattr(LeadAgent, "agent_id0", 0)) != 0:
            raise NotImplementedError("a SubAgent of a shard of the agents (parallel.py) is not supported: build it on an "
                                      "unsharded Agent")
        if "dt" in self.params:
            warnings.warn("You have passed 'dt as a parameter but this will be overwritten to match dt of the LeadAgent")
        self.params["dt"] = self.LeadAgent.dt
        self.params["n_agents"] = self.LeadAgent.n_agents   # lane b follows lane b of the lead
        self.params["device"] = self.LeadAgent.device
        self.Environment = self.LeadAgent.Environment
        super().__init__(self.Environment, self.params)
        self._auto_enabled = False   # (no automatic step plan: every update() depends on the lead's state of the moment)
        # position and velocity start as the lead's (SubAgent.py:29-31)
        lead = self.LeadAgent
        lead._sync_plan()
        self._state[_L.S_POS_X:_L.S_VEL_Y + 1] = lead._state[_L.S_POS_X:_L.S_VEL_Y + 1]
        self._pos_out = torch.empty((1, 2, self._Bp), dtype=torch.float64, device=self._device)

    # ---- stepping ------------------------------------------------------------------------------------------------
    def _lead_state(self):
        """The lead's float64 state matrix as of its last update(), a step plan's included."""
        lead = self.LeadAgent
        lead._sync_plan()
        return lead._state

    def _forced_step(self, pos):
        """Agent.update(forced_next_position=pos) with `pos` a device tensor [1][2][Bp] float64."""
        self._advance(1, None, None, 1, {}, forced=pos)

    def update(self, **kwargs):
        """`t = LeadAgent.t`, then `Agent.update(**kwargs)` (SubAgent.py:33-36): the lead must have been updated first.
        `forced_next_position` may be a device tensor `(2, B)` / `(B, 2)`, which stays on the device."""
        self.t = self.LeadAgent.t
        forced = kwargs.get("forced_next_position")
        if torch.is_tensor(forced):
            kwargs.pop("forced_next_position")
            kwargs.pop("drift_velocity", None)                      # (a forced position overrides the motion model)
            kwargs.pop("drift_to_random_strength_ratio", None)
            return self._advance(1, kwargs.pop("dt", None), None, 1, kwargs, forced=self._as_device_f64(forced, 2).unsqueeze(0))
        super().update(**kwargs)

    # ---- where a SubAgent cannot run -------------------------------------------------------------------------------
    def simulate(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} has no open-loop run: its position depends on the lead's state "
                                  "of every step.  Step it with update() after the lead's update()")

    def make_step_plan(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} cannot be recorded in a step plan: its position depends on the "
                                  "lead's state of every step.  Step it with update() after the lead's update()")

    def plot_trajectory(self, *args, **kwargs):
        raise NotImplementedError("plotting is outside the accelerated path; use the reference package for figures")


class ThetaSequenceAgent(SubAgent):
    """A position that sweeps from behind the lead to ahead of it once per theta cycle (SubAgent.py:182-350):

        |.......A.........|................B..............|.................C.............|........A'.......|
        0              1/2-frac/2                        1/2                           1/2+frac/2           1

    A, A': NaN.  B, look behind: along the lead's past trajectory, `d_half` behind it at the start, meeting it at phase
    1/2.  C, look ahead: along a trajectory the motion model simulates from the lead's position and velocity at the first
    step of C (the `ForwardSequenceAgent`, whose motion parameters are the ones passed to THIS agent), up to `d_half`
    ahead.  Distances are measured along the trajectories (distance travelled), at `v_sequence` relative to the lead.

    `update(forward_agent_update_kwargs={...})`: per-call motion overrides of the rollout, as in the reference, and
    `"noise"`: explicit standard normals `(K, 2, B)` for the rollout of this step (parity runs; ignored on steps without
    a rollout); otherwise the ForwardSequenceAgent's own Philox stream, advanced by K per rollout."""

    default_params = {
        "v_sequence": 5.0,   # speed of the sequence in the reference frame of the lead, m/s
        "theta_freq": 10.0,  # theta frequency, Hz
        "theta_frac": 0.5,   # fraction of the theta cycle the sweep takes
    }

    def __init__(self, LeadAgent, params={}):
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        # a sham Agent whose only use is the motion model of the forward sequences (SubAgent.py:222-225): built from THIS
        # agent's parameters — what was passed here, not the lead's — without the three theta keys
        fwd_params = copy.deepcopy(self.params)
        for key in __class__.default_params.keys():
            fwd_params.pop(key)
        super().__init__(LeadAgent, self.params)
        lead = self.LeadAgent
        lead.distance_travelled = 0   # (SubAgent.py:220; the lead's history lists are left alone: DESIGN.md 5)
        fwd_params.update(dt=lead.dt, n_agents=lead.n_agents, device=lead.device)
        self.ForwardSequenceAgent = Agent(self.Environment, fwd_params)
        self.ForwardSequenceAgent._auto_enabled = False

        self.T_theta = 1 / self.theta_freq
        self.d_half = (self.theta_frac / 2) * self.T_theta * self.v_sequence   # distance covered by half a sweep
        self.last_theta_phase = 0
        assert (lead.dt <= self.T_theta / 10), \
            f"params['dt'] for the LeadAgent is too large. It must be < 10% of theta time period., i.e. smaller than {self.T_theta/10:.5f}"
        assert (self.v_sequence >= 4 * lead.speed_mean), \
            f"params['v_sequence'] is too small. It must be > 4*LeadAgent.speed_mean, i.e. larger than {4*lead.speed_mean:.2f}"
        # Agent.average_measured_speed is a constant, so the rollout's time step and target distance are constants too
        speed = lead.average_measured_speed
        self.dt_forward = lead.dt * self.v_sequence / speed                                      # SubAgent.py:320-322
        self.forward_distance = self.d_half + 100 * speed * (self.theta_frac / 2) * self.T_theta  # SubAgent.py:315
        self.lookback = max(1, int(5 * self.d_half / (lead.dt * speed)))                          # SubAgent.py:283
        self.rollout_steps_max = int(math.ceil(4 * self.forward_distance / (lead.dt * self.v_sequence))) + 8
        Bp, dev, K = self._Bp, self._device, self.rollout_steps_max
        self._capacity = self.lookback
        self._ring = torch.zeros((self._capacity, 3, Bp), dtype=torch.float64, device=dev)
        self._n_records = 0
        self._future = torch.zeros((K + 1, 3, Bp), dtype=torch.float64, device=dev)
        self._count = torch.zeros(Bp, dtype=torch.int32, device=dev)
        self._rollout_z = torch.zeros((K, 2, Bp), dtype=torch.float64, device=dev)
        self._tdiag = torch.zeros(4, dtype=torch.int32, device=dev)
        self.n_rollouts = 0

    # ---- read-outs -----------------------------------------------------------------------------------------------
    @property
    def theta_diagnostics(self):
        """Counters of the sweep kernels: look-behind / look-ahead steps of a lane where the reference would have raised
        (the lane got NaN), rollouts that used all `rollout_steps_max` steps, positions dropped by the `d_half` rule."""
        d = self._tdiag.cpu().numpy()
        return dict(look_behind_raises=int(d[_L.THETA_DIAG_BEHIND]), look_ahead_raises=int(d[_L.THETA_DIAG_AHEAD]),
                    rollout_saturations=int(d[_L.THETA_DIAG_ROLLOUT]), dropped_far=int(d[_L.THETA_DIAG_FAR]))

    @property
    def future_table(self):
        """The last rollout on the device: (`[K + 1, 3, B_padded]` float64 rows (distance, x, y) per entry, `[B_padded]`
        int32 steps taken per lane); entries 0 .. count are valid."""
        return self._future, self._count

    @property
    def rollout_normals(self):
        """The standard normals the last rollout used: device float64 `[K, 2, B_padded]` (rows a lane's wave did not reach
        keep older values)."""
        return self._rollout_z

    def theta_phase(self):
        """The phase in [0, 1) of the lead's clock in the theta cycle (SubAgent.py:267)."""
        t = self.LeadAgent.t
        return (t % (1 / self.theta_freq)) / ((1 / self.theta_freq))

    # ---- one step ------------------------------------------------------------------------------------------------
    def _rollout(self, lead_state, env, stream, kwargs):
        fwd, K = self.ForwardSequenceAgent, self.rollout_steps_max
        kwargs = dict(kwargs)
        noise = kwargs.pop("noise", None)
        m = fwd._motion(self.dt_forward, False, 1, kwargs)
        z = fwd._noise_tensor(noise, K) if noise is not None else None
        rc = _L.lib.riab_theta_sequence_rollout(env, m, _L.ptr(lead_state), _L.ptr(fwd._state), self._Bp, self._B, int(fwd.agent_id0),
                                                _L.ptr(z), _L.ptr(self._rollout_z), int(fwd.rng_seed), int(fwd._step_index),
                                                K, float(self.forward_distance), _L.ptr(self._future), _L.ptr(self._count),
                                                _L.ptr(fwd._diag), _L.ptr(self._tdiag), stream)
        _L.check(rc, "riab_theta_sequence_rollout")
        fwd._step_index += K        # whatever the lanes used: a lane's noise does not depend on the other lanes
        fwd._last_row = None        # (its state was written on the device)
        self._keep_rollout = (z, m)
        self.n_rollouts += 1

    def update(self, dt=None, drift_velocity=None, drift_to_random_strength_ratio=1, forward_agent_update_kwargs={}):
        """The position along the theta sequence for the lead's newest state (SubAgent.py:245-350); `dt` and the drift
        arguments are accepted and unused, as in the reference."""
        lead = self.LeadAgent
        lead_state = self._lead_state()
        self.t = lead.t
        phase = self.theta_phase()
        half = self.theta_frac / 2
        if (phase >= (0.5 - half)) and (phase < 0.5):
            branch = _L.THETA_BEHIND
        elif (phase >= 0.5) and (phase < 0.5 + half):
            branch = _L.THETA_AHEAD
        else:
            branch = _L.THETA_NONE
        env, _walls = self.Environment.device_tables(self._device)
        stream = _L.current_stream()
        if branch == _L.THETA_AHEAD and self.last_theta_phase < 0.5:   # the first step of C in this cycle
            self._rollout(lead_state, env, stream, forward_agent_update_kwargs)
        rc = _L.lib.riab_theta_sequence_step(env, _L.ptr(lead_state), self._Bp, self._B, _L.ptr(self._ring), self._capacity,
                                             self.lookback, self._n_records, branch, float(phase), float(self.d_half),
                                             float(self.theta_frac), _L.ptr(self._future), _L.ptr(self._count),
                                             self.rollout_steps_max, _L.ptr(self._pos_out), _L.ptr(self._tdiag), stream)
        _L.check(rc, "riab_theta_sequence_step")
        self._n_records += 1
        self.last_theta_phase = phase
        self._forced_step(self._pos_out)


class DumbAgent(SubAgent):
    """A wrong position that wanders round the lead as if attached to it by a spring (SubAgent.py:118-179).  In the
    lead's frame the velocity of the displacement is an Ornstein-Uhlenbeck process of scale `sigma` and coherence time
    `tau_v`, and a spring of stiffness `acceleration_scale` pulls the displacement back:

        d = drift_distance    the typical distance between the two agents
        tau_s = drift_timescale    how long the wrong position takes to journey round the true one
        sigma = pi^2 d / tau_s^2,  tau_v = tau_s / 2,  acceleration_scale = sigma / d

    A displacement that would cross a wall is cut to 95 % of the way to it, and the position obeys the Environment's
    boundary conditions.  One kernel launch per step (csrc/riab_subagent.hip: riab_dumb_agent_step).

    `update(noise=...)`: explicit standard normals `(2, B)` for this step (parity runs); otherwise the agent's own
    Philox stream, a pure function of (its seed, its step index, the global agent id)."""

    default_params = {
        "drift_distance": 0.05,   # ~average distance between the two agents
        "drift_timescale": 3.0,   # ~timescale over which the wrong position journeys around the true position
    }

    def __init__(self, LeadAgent, params={}):
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        super().__init__(LeadAgent, self.params)
        self.tau_v = self.drift_timescale / 2
        self.sigma = math.pi ** 2 * self.drift_distance / (self.drift_timescale ** 2)
        self.acceleration_scale = self.sigma / self.drift_distance
        Bp, dev = self._Bp, self._device
        self._disp = torch.zeros((2, Bp), dtype=torch.float64, device=dev)
        self._dvel = torch.zeros((2, Bp), dtype=torch.float64, device=dev)
        self._dumb_z = torch.zeros((2, Bp), dtype=torch.float64, device=dev)
        self._ddiag = torch.zeros(4, dtype=torch.int32, device=dev)

    # ---- read-outs -----------------------------------------------------------------------------------------------
    def _lanes(self, t):
        return self._squeeze(t[:, :self._B].t().cpu().numpy())

    @property
    def displacement(self):
        """position - lead position, accounting for the environment: `(B, 2)`, or `(2,)` for one agent"""
        return self._lanes(self._disp)

    @property
    def displacement_velocity(self):
        return self._lanes(self._dvel)

    @property
    def displacement_tensors(self):
        """(displacement, displacement velocity) on the device: float64 `[2, B_padded]` each"""
        return self._disp, self._dvel

    @property
    def step_normals(self):
        """The standard normals the last update() used: device float64 `[2, B_padded]`."""
        return self._dumb_z

    @property
    def dumb_diagnostics(self):
        """Counters of the step kernel over the real lanes: springs cut by a wall, positions the boundary conditions
        changed, and of those the rejection sampler's saturations (polygonal rooms and holes)."""
        d = self._ddiag.cpu().numpy()
        return dict(wall_cuts=int(d[_L.DUMB_DIAG_WALL_CUTS]), boundary_corrections=int(d[_L.DUMB_DIAG_BOUNDARY]),
                    resample_saturations=int(d[_L.DUMB_DIAG_SATURATIONS]))

    # ---- one step ------------------------------------------------------------------------------------------------
    def update(self, noise=None):
        lead = self.LeadAgent
        lead_state = self._lead_state()
        dt = float(lead.dt)
        # utils.ornstein_uhlenbeck(dt, x, drift=0, noise_scale=sigma, coherence_time=tau_v) (utils.py:361-368)
        ou_sigma = math.sqrt((2 * self.sigma ** 2) / (self.tau_v * dt))
        ou_theta = 1 / self.tau_v
        z = self._as_device_f64(noise, 2) if noise is not None else None
        env, _walls = self.Environment.device_tables(self._device)
        rc = _L.lib.riab_dumb_agent_step(env, _L.ptr(lead_state), self._Bp, self._B, int(self.agent_id0), _L.ptr(self._disp),
                                         _L.ptr(self._dvel), dt, ou_theta, ou_sigma, float(self.acceleration_scale), _L.ptr(z),
                                         _L.ptr(self._dumb_z), int(self.rng_seed), int(self._step_index), _L.ptr(self._pos_out),
                                         _L.ptr(self._ddiag), _L.current_stream())
        _L.check(rc, "riab_dumb_agent_step")
        self._keep_dumb = (z, _walls)
        self.t = lead.t
        self._forced_step(self._pos_out)


class ReplayAgent(SubAgent):
    """The lead's position, except during "replays": at rate `replay_freq` a lane detaches from its lead, jumps to a
    random place, explores there with the motion model at a speed drawn round `replay_speed` for a time drawn round
    `replay_duration`, and snaps back (SubAgent.py:358-432).

    `self.ReplayAgent` is a sham Agent whose only use is the motion model of the replays; its motion parameters are the
    ones passed to THIS agent.  The reference simulates a replay's whole path when it starts and interpolates that table
    afterwards; here the path is produced as it is consumed: a lane keeps the two records that bracket its position and
    its sham agent advances only as far as each update needs (csrc/riab_subagent.hip: riab_replay_agent_step, one launch
    per update) — the same positions, since the distance along a replay only grows.  A lane's sham agent takes at most
    `replay_steps_max` steps per update (default: 4 x the expected `replay_speed / speed_mean`, + 8); a lane that runs
    out takes its newest record as its position and is counted in `replay_diagnostics["saturations"]`.

    `update(draws=..., noise=...)` (parity runs): `draws` a dict of per-lane outcomes `u` (the trigger uniform), `speed`,
    `duration`, `pos` (2, B), `direction` — read by the lanes that are outside a replay, the last four by those that
    start one —; `noise` the standard normals `(K, 2, B)`, K = replay_steps_max, of the sham agent's steps of this
    call.  Otherwise this agent's own Philox stream and the sham agent's."""

    default_params = {
        "replay_freq": 0.3,       # frequency of replay events, Hz
        "replay_duration": 0.1,   # mean duration of replay events, s
        "replay_speed": 1.0,      # mean speed of replay events, m/s
    }

    def __init__(self, LeadAgent, params={}, replay_steps_max=None):
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        # the sham Agent (SubAgent.py:375-378): THIS agent's parameters without the three replay keys
        sham_params = copy.deepcopy(self.params)
        for key in __class__.default_params.keys():
            sham_params.pop(key)
        super().__init__(LeadAgent, self.params)
        lead = self.LeadAgent
        self.mean_replay_speed = self.replay_speed
        self.mean_replay_duration = self.replay_duration
        sham_params.update(dt=lead.dt, n_agents=lead.n_agents, device=lead.device)
        self.ReplayAgent = Agent(self.Environment, sham_params)
        self.ReplayAgent._auto_enabled = False
        expected = self.mean_replay_speed / self.ReplayAgent.speed_mean   # sham steps per update: the dt cancels
        self.replay_steps_max = int(replay_steps_max) if replay_steps_max is not None else int(math.ceil(4 * expected)) + 8
        assert self.replay_steps_max >= 1
        Bp, dev, K = self._Bp, self._device, self.replay_steps_max
        self._flag = torch.zeros(Bp, dtype=torch.int32, device=dev)
        self._rstate = torch.zeros((_L.REPLAY_ROWS, Bp), dtype=torch.float64, device=dev)
        self._draws = torch.full((_L.REPLAY_DRAWS, Bp), float("nan"), dtype=torch.float64, device=dev)
        self._replay_z = torch.zeros((K, 2, Bp), dtype=torch.float64, device=dev)
        self._steps = torch.zeros(Bp, dtype=torch.int32, device=dev)
        self._rdiag = torch.zeros(4, dtype=torch.int32, device=dev)
        self._flag_rows = torch.zeros((256, Bp), dtype=torch.bool, device=dev)
        self._n_flag_rows = 0
        self.history = HistoryView(tuple(self.history.keys()) + ("replay",), self._materialise_history,
                                   lambda: (self._sync_plan(), self._hist.version)[1])

    # ---- read-outs -----------------------------------------------------------------------------------------------
    @property
    def is_undergoing_replay(self):
        """per lane: `(B,)` bool, or a bool for one agent (the device flags: `replay_flags`)"""
        return self._squeeze(self._flag[:self._B].cpu().numpy().astype(bool))

    @property
    def replay_flags(self):
        """device int32 `[B_padded]`: 1 in a replay"""
        return self._flag

    @property
    def replay_state(self):
        """device float64 `[10, B_padded]`: speed, start time, end time, the sham agent's distance at the start, and the
        two records (distance since the start, x, y) a lane interpolates between (riab_hip.h RIAB_RP_*)"""
        return self._rstate

    @property
    def replay_draws(self):
        """What the last update() drew: device float64 `[6, B_padded]` rows u, speed, duration, x, y, direction; NaN where
        a draw was not taken (u: lanes in a replay; the others: lanes that started none)."""
        return self._draws

    @property
    def replay_normals(self):
        """The standard normals of the sham agent's steps of the last update(): device float64 `[K, 2, B_padded]` (rows a
        lane's wave did not reach keep older values)."""
        return self._replay_z

    @property
    def replay_steps_taken(self):
        """sham steps per lane in the last update(): device int32 `[B_padded]`"""
        return self._steps

    @property
    def replay_diagnostics(self):
        """Counters over the real lanes: replays started and ended, lane-steps that ran out of `replay_steps_max` sham
        steps, start positions whose rejection sampler ran out of attempts."""
        d = self._rdiag.cpu().numpy()
        return dict(started=int(d[_L.REPLAY_DIAG_STARTED]), ended=int(d[_L.REPLAY_DIAG_ENDED]),
                    saturations=int(d[_L.REPLAY_DIAG_SATURATIONS]), resample_saturations=int(d[_L.REPLAY_DIAG_RESAMPLE]))

    def _materialise_history(self):
        out = super()._materialise_history()
        rows = self._flag_rows[:self._n_flag_rows, :self._B].cpu().numpy()
        out["replay"] = rows[:, 0] if self._B == 1 else rows
        return out

    def reset_history(self):
        super().reset_history()
        self._n_flag_rows = 0

    def _draws_tensor(self, draws):
        """dict of per-lane outcomes -> device float64 `[6, Bp]` (padding lanes shadow lane 0)"""
        B = self._B
        rows = np.full((_L.REPLAY_DRAWS, self._Bp), np.nan)

        def lane(x):
            return (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)).astype(np.float64)

        for key, row in (("u", _L.RD_U), ("speed", _L.RD_SPEED), ("duration", _L.RD_DURATION), ("direction", _L.RD_DIRECTION)):
            rows[row, :B] = np.broadcast_to(lane(draws[key]).reshape(-1), (B,))
        pos = lane(draws["pos"])
        pos = pos.T if pos.shape == (B, 2) and B != 2 else pos.reshape(2, -1)
        rows[_L.RD_POS_X:_L.RD_POS_Y + 1, :B] = np.broadcast_to(pos, (2, B))
        rows[:, B:] = rows[:, :1]
        return torch.from_numpy(rows).to(self._device)

    # ---- one step ------------------------------------------------------------------------------------------------
    def update(self, draws=None, noise=None):
        lead, sham, K = self.LeadAgent, self.ReplayAgent, self.replay_steps_max
        lead_state = self._lead_state()
        t_now = float(self.t)   # the clock the reference compares with replay_end_time: this agent's own, as it was left
        d_in = self._draws_tensor(draws) if draws is not None else None
        z = sham._noise_tensor(noise, K) if noise is not None else None
        m = sham._motion(float(lead.dt), False, 1, {})
        env, _walls = self.Environment.device_tables(self._device)
        rc = _L.lib.riab_replay_agent_step(env, m, _L.ptr(lead_state), _L.ptr(sham._state), self._Bp, self._B, int(sham.agent_id0),
                                           _L.ptr(self._flag), _L.ptr(self._rstate), t_now, float(self.replay_freq * lead.dt),
                                           float(self.mean_replay_speed), float(self.mean_replay_duration),
                                           float(sham.speed_mean), _L.ptr(d_in), _L.ptr(self._draws), int(self.rng_seed),
                                           int(self._step_index), _L.ptr(z), _L.ptr(self._replay_z), int(sham.rng_seed),
                                           int(sham._step_index), K, _L.ptr(self._pos_out), _L.ptr(self._steps),
                                           _L.ptr(sham._diag), _L.ptr(self._rdiag), _L.current_stream())
        _L.check(rc, "riab_replay_agent_step")
        sham._step_index += K       # whatever the lanes used: a lane's noise does not depend on the other lanes
        sham._last_row = None       # (its state was written on the device)
        self._keep_replay = (d_in, z, m, _walls)
        if self.save_history:
            if self._n_flag_rows == self._flag_rows.shape[0]:
                self._flag_rows = torch.cat((self._flag_rows, torch.zeros_like(self._flag_rows)))
            self._flag_rows[self._n_flag_rows] = self._flag != 0
            self._n_flag_rows += 1
        self.t = lead.t
        self._forced_step(self._pos_out)


class ShiftAgent(SubAgent):
    """The lead's position shifted by `shift_m` metres along its head direction, ahead (positive) or behind
    (SubAgent.py:466-478)."""

    default_params = {
        "shift_m": 0.01,
    }

    def __init__(self, LeadAgent, params={}):
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        super().__init__(LeadAgent, self.params)

    def update(self):
        lead_state = self._lead_state()
        _L.check(_L.lib.riab_shift_agent_position(_L.ptr(lead_state), self._Bp, float(self.shift_m), _L.ptr(self._pos_out),
                                                  _L.current_stream()), "riab_shift_agent_position")
        self.t = self.LeadAgent.t
        self._forced_step(self._pos_out)


class UnrelatedAgent(SubAgent):
    """A SubAgent that moves by itself (SubAgent.py:480-489)."""

    default_params = {}

    def __init__(self, LeadAgent, params={}):
        super().__init__(LeadAgent, params)

    def update(self):
        super().update()
