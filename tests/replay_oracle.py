"""Float64 NumPy restatement of contribs.SubAgent's DumbAgent and ReplayAgent (reference contribs/SubAgent.py:118-180,
358-432) for B lanes, on top of oracle.riab_oracle — what the tests compare csrc/riab_subagent.hip with, itself pinned
to the reference's record (tests/test_replay_cpu.py).

`DumbAgentOracle.step(lead_pos, z)`: one `DumbAgent.update()` up to the forced step; `lead_pos (B, 2)`, `z (2, B)` the
two standard normals of the OU increment per lane.  Returns the position `(B, 2)`; `displacement` and
`displacement_velocity` `(B, 2)` are the state (assign to them to step from somebody else's state).

`ReplayAgentOracle(mode=...).step(lead_pos, t, draws, z, ...)`: one `ReplayAgent.update()` up to the forced step.  `t` is
the clock the reference compares with `replay_end_time`: the ReplayAgent's own `t` when `update()` is entered.
  mode "eager"  the reference's form: a replay's whole trajectory (1.1 x speed x duration of path) is simulated when it
                starts, into a table that later steps interpolate (`z[b]`: the normals `(n, 2)` of lane b's rollout).
  mode "lazy"   the kernel's form: a lane keeps the two records that bracket its query distance and advances its sham
                agent only as far as the query needs (`z (K, 2, B)`: the normals of this call's sham steps, lane b's
                k-th step of the call takes `z[k, :, b]`)."""
import numpy as np

from oracle import riab_oracle as orc
from tests.subagent_oracle import interp1d_linear

SHAM_KEYS = ("pos", "velocity", "rotational_velocity", "measured_velocity", "measured_rotational_velocity", "head_direction",
             "distance_travelled", "distance_to_closest_wall")


class DumbAgentOracle:
    def __init__(self, env, B, dt, drift_distance=0.05, drift_timescale=3.0):
        self.env, self.B, self.dt = env, int(B), float(dt)
        self.tau_v = drift_timescale / 2
        self.sigma = np.pi ** 2 * drift_distance / (drift_timescale ** 2)
        self.acceleration_scale = self.sigma / drift_distance
        self.displacement = np.zeros((self.B, 2))
        self.displacement_velocity = np.zeros((self.B, 2))
        self.n_wall_cuts = self.n_boundary = 0

    def step(self, lead_pos, z, resample_pos=None):
        B, dt = self.B, self.dt
        lead = np.asarray(lead_pos, dtype=np.float64).reshape(B, 2)
        z = np.asarray(z, dtype=np.float64).reshape(2, B).T
        disp, vel = self.displacement.copy(), self.displacement_velocity.copy()
        # SubAgent.py:154-163
        ou = orc.ou_increment(vel, dt, 0.0, self.sigma, self.tau_v, z)
        spring = -self.acceleration_scale * disp * dt
        vel = vel + (ou + spring)
        disp = disp + vel * dt
        # :167-173: the walls are list a, the segment lead -> lead + displacement list b
        self.cut = np.zeros(B, dtype=bool)
        if len(self.env.walls):
            for b in range(B):
                seg = np.array([lead[b], lead[b] + disp[b]])
                l_a, l_b = orc.segment_intercepts(self.env.walls, seg[None])
                hit = ((l_a > 0) & (l_a < 1) & (l_b > 0) & (l_b < 1))[:, 0]
                if hit.any():
                    disp[b] = disp[b] * (0.95 * np.min(l_b[hit, 0]))
                    self.cut[b] = True
        # :175-178
        pos = lead + disp
        self.outside = ~orc.env_is_inside(self.env, pos)
        if self.outside.any():
            pos = np.where(self.outside[:, None], orc.env_apply_boundary_conditions(self.env, pos, resample_pos), pos)
        disp = np.stack([orc.env_vectors_between(self.env, pos[b], lead[b])[0, 0] for b in range(B)])
        self.displacement, self.displacement_velocity = disp, vel
        self.n_wall_cuts += int(self.cut.sum())
        self.n_boundary += int(self.outside.sum())
        return pos


class ReplayAgentOracle:
    def __init__(self, env, B, dt, mode, sham_params=None, replay_freq=0.3, replay_duration=0.1, replay_speed=1.0,
                 steps_max=None, sham_state=None):
        assert mode in ("eager", "lazy")
        self.env, self.B, self.dt, self.mode = env, int(B), float(dt), mode
        self.sham_params = dict(sham_params or {})
        self.speed_mean = self.sham_params.get("speed_mean", orc.DEFAULT_MOTION["speed_mean"])
        self.replay_freq, self.mean_duration, self.mean_speed = replay_freq, replay_duration, replay_speed
        # the bound of the kernel's per-call loop: 4 x the expected sham steps per update + 8
        self.K = int(steps_max) if steps_max is not None else int(np.ceil(4 * replay_speed / self.speed_mean)) + 8
        B = self.B
        self.flag = np.zeros(B, dtype=bool)
        self.speed, self.t_start, self.t_end, self.d_start = (np.zeros(B) for _ in range(4))
        if sham_state is None:   # (everything but position, velocity and rotational velocity only ever feeds outputs)
            sham_state = dict(pos=np.full((B, 2), 0.5), velocity=np.tile([self.speed_mean, 0.0], (B, 1)),
                              rotational_velocity=np.zeros(B), measured_velocity=np.tile([self.speed_mean, 0.0], (B, 1)),
                              measured_rotational_velocity=np.zeros(B), head_direction=np.tile([1.0, 0.0], (B, 1)),
                              distance_travelled=np.zeros(B), distance_to_closest_wall=np.full(B, np.inf))
        self.sham = {k: np.array(sham_state[k], dtype=np.float64) for k in SHAM_KEYS}
        self.table = [None] * B                                    # eager: (distances (n,), positions (n, 2)) per lane
        self.lo_d, self.hi_d = np.zeros(B), np.zeros(B)            # lazy: the two records
        self.lo_p, self.hi_p = np.zeros((B, 2)), np.zeros((B, 2))
        self.saturations = 0
        self.steps_disagree = 0
        self.n_started = self.n_ended = 0
        self.max_steps_in_a_call = 0
        self.rollout_counts = []                                   # eager: sham updates per replay, in order of start
        self.rollout_tables = []                                   # ... and their (distances, positions)

    # ---- the sham agent ----------------------------------------------------------------------------------------------
    def _sham_step(self, lanes, z_rot, z_spd, resample_pos=None):
        """one Agent.update() of the sham agents of `lanes`"""
        st = {k: self.sham[k][lanes] for k in SHAM_KEYS}
        new = orc.agent_step(self.env, st, self.dt, z_rot, z_spd, params=self.sham_params, resample_pos=resample_pos)
        for k in SHAM_KEYS:
            self.sham[k][lanes] = new[k]

    def _start(self, b, t, draws):
        """SubAgent.py:396-407: the four draws after the trigger"""
        self.flag[b] = True
        self.speed[b] = draws["speed"][b]
        duration = max(draws["duration"][b], self.mean_duration / 2)
        self.t_start[b] = t
        self.t_end[b] = t + duration
        direction = draws["direction"][b]
        self.sham["pos"][b] = np.asarray(draws["pos"], dtype=np.float64).reshape(2, self.B)[:, b]
        self.sham["velocity"][b] = self.speed_mean * np.array([np.cos(direction), np.sin(direction)])
        self.sham["rotational_velocity"][b] = 0.0
        self.d_start[b] = self.sham["distance_travelled"][b]
        self.n_started += 1
        return duration

    # ---- one update ----------------------------------------------------------------------------------------------------
    def step(self, lead_pos, t, draws=None, z=None, n_steps=None, resample_pos=None):
        B = self.B
        lead = np.asarray(lead_pos, dtype=np.float64).reshape(B, 2)
        pos = lead.copy()
        query = np.zeros(B)
        moving = np.zeros(B, dtype=bool)
        self.started = np.zeros(B, dtype=bool)
        for b in range(B):
            if not self.flag[b]:
                if draws is None or draws["u"][b] > self.replay_freq * self.dt:
                    continue
                duration = self._start(b, t, draws)
                self.started[b] = True
                pos[b] = self.sham["pos"][b]
                if self.mode == "eager":
                    zb = np.asarray(z[b], dtype=np.float64).reshape(-1, 2)
                    d, p, n = [0.0], [self.sham["pos"][b].copy()], 0
                    while self.sham["distance_travelled"][b] < self.d_start[b] + 1.1 * self.speed[b] * duration:
                        assert n < len(zb), f"the replay needs more than the {len(zb)} pairs of normals given"
                        self._sham_step([b], zb[n, :1], zb[n, 1:],
                                        None if resample_pos is None else np.asarray(resample_pos[b][n]).reshape(1, 2))
                        d.append(self.sham["distance_travelled"][b] - self.d_start[b])
                        p.append(self.sham["pos"][b].copy())
                        n += 1
                    self.table[b] = (np.array(d), np.array(p))
                    self.rollout_counts.append(n)
                    self.rollout_tables.append(self.table[b])
                else:
                    self.lo_d[b] = self.hi_d[b] = 0.0
                    self.lo_p[b] = self.hi_p[b] = self.sham["pos"][b]
            elif t < self.t_end[b]:
                query[b] = self.speed[b] * (t - self.t_start[b])
                moving[b] = True
            else:
                self.flag[b] = False
                self.n_ended += 1
        self.steps_taken = np.zeros(B, dtype=np.int64)
        if self.mode == "lazy":
            # (`n_steps (B,)`: take exactly the steps somebody else took, the device for instance, and count disagreements)
            active = moving & ~(self.hi_d >= query) if n_steps is None else moving & (np.asarray(n_steps) > 0)
            k = 0
            while active.any() and k < self.K:
                lanes = np.nonzero(active)[0]
                zk = np.asarray(z[k], dtype=np.float64).reshape(2, -1)
                self._sham_step(lanes, zk[0, lanes], zk[1, lanes], None if resample_pos is None else resample_pos[k][lanes])
                self.lo_d[lanes], self.lo_p[lanes] = self.hi_d[lanes], self.hi_p[lanes]
                self.hi_d[lanes] = self.sham["distance_travelled"][lanes] - self.d_start[lanes]
                self.hi_p[lanes] = self.sham["pos"][lanes]
                self.steps_taken[lanes] += 1
                k += 1
                arrived = self.hi_d >= query
                if n_steps is None:
                    active = active & ~arrived
                else:
                    active = active & (self.steps_taken < np.asarray(n_steps))
            if n_steps is not None:
                # the lane took the number of steps it was told to: does its own criterion agree?
                own_more = moving & ~(self.hi_d >= query) & (self.steps_taken < self.K)
                own_less = moving & (self.steps_taken > 0) & (self.lo_d >= query)
                self.steps_disagree += int((own_more | own_less).sum())
            self.max_steps_in_a_call = max(self.max_steps_in_a_call, int(self.steps_taken.max(initial=0)))
        for b in np.nonzero(moving)[0]:
            if self.mode == "eager":
                got = interp1d_linear(self.table[b][0], self.table[b][1], query[b])
                assert got is not None, "the table always covers the query"
                pos[b] = got
            elif not (self.hi_d[b] >= query[b]):
                self.saturations += 1          # out of steps: the newest record
                pos[b] = self.hi_p[b]
            else:
                slope = (self.hi_p[b] - self.lo_p[b]) / (self.hi_d[b] - self.lo_d[b])
                pos[b] = slope * (query[b] - self.lo_d[b]) + self.lo_p[b]
        return pos
