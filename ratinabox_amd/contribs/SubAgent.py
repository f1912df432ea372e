"""`SubAgent`, `ThetaSequenceAgent`, `ShiftAgent`, `UnrelatedAgent` — Agents slaved to another Agent, on the device
(reference ratinabox/contribs/SubAgent.py).

A SubAgent is an `Agent` of its lead's Environment whose position is a function of the lead's state: lane b of the
SubAgent follows lane b of the lead (`n_agents`, `device` and `dt` are the lead's).  Its position is computed by a
kernel of csrc/riab_theta_seq.hip from the lead's float64 state matrix and handed — a device tensor, nothing visits the
host — to the forced-position step every Agent has (`riab_agent_step(forced_pos=...)`), so history, measured velocity
and any `Neurons` population built on the SubAgent work as on any other Agent through their eager `update()`.

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

Not built: `DumbAgent`, `ReplayAgent`, 1D environments, plotting.  A SubAgent cannot run inside `Agent.simulate()`, a
step plan or a `TaskEnvironment`, nor follow a shard of a multi-GPU run (NotImplementedError)."""
import copy
import math
import warnings

import torch

from .. import _lib as _L
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
