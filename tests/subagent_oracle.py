"""Float64 NumPy restatement of contribs.SubAgent's device path (csrc/riab_theta_seq.hip) for B lanes — what the tests
compare the kernels with, itself pinned to the reference's record (tests/test_subagent_cpu.py: the interpolation bit for
bit, the rollouts to a few ulp, which is how close oracle.agent_step is to the reference's own step).

`ThetaSequenceOracle.step(lead, t, ...)` is one `ThetaSequenceAgent.update()` up to the forced step: it takes the lead's
state after its update (`pos (B, 2)`, `velocity (B, 2)`, `rotational_velocity (B,)`, `distance_travelled (B,)`) and the
lead's clock, and returns the SubAgent's position `(B, 2)`.  On the first look-ahead step of a theta cycle it rolls the
future out with `oracle.riab_oracle.agent_step` from the normals `rollout_z (n, 2, B)` — or takes a ready-made future
table `future=(table (K+1, 3, B), count (B,))` instead."""
import math

import numpy as np

from oracle import riab_oracle as orc


def interp1d_linear(xs, ys, x_new):
    """scipy.interpolate.interp1d(xs, ys, axis=0)(x_new) with default arguments, for non-decreasing xs `(n,)`, ys
    `(n, 2)` and a scalar x_new; None where it raises (fewer than two points, x_new out of bounds)."""
    n = len(xs)
    if n < 2 or x_new < xs[0] or x_new > xs[-1]:
        return None
    i = int(np.clip(np.searchsorted(xs, x_new), 1, n - 1))
    lo, hi = i - 1, i
    slope = (ys[hi] - ys[lo]) / (xs[hi] - xs[lo])
    return slope * (x_new - xs[lo]) + ys[lo]


def shift_position(pos, head_direction, shift_m):
    """ShiftAgent (SubAgent.py:476)."""
    return np.asarray(pos, dtype=np.float64) + np.asarray(head_direction, dtype=np.float64) * shift_m


class ThetaSequenceOracle:
    def __init__(self, env, B, dt, lead_average_speed, forward_params=None, v_sequence=5.0, theta_freq=10.0,
                 theta_frac=0.5):
        self.env, self.B, self.dt = env, int(B), float(dt)
        self.v_sequence, self.theta_freq, self.theta_frac = v_sequence, theta_freq, theta_frac
        self.forward_params = dict(forward_params or {})
        self.T_theta = 1 / theta_freq
        self.d_half = (theta_frac / 2) * self.T_theta * v_sequence
        self.dt_forward = dt * v_sequence / lead_average_speed
        self.forward_distance = self.d_half + 100 * lead_average_speed * (theta_frac / 2) * self.T_theta
        self.lookback = max(1, int(5 * self.d_half / (dt * lead_average_speed)))
        self.K = int(math.ceil(4 * self.forward_distance / (dt * v_sequence))) + 8
        self.last_phase = 0
        self.n_rec = 0                                 # the records of every lane, newest last
        self.rec_d = np.empty((1024, self.B))
        self.rec_p = np.empty((1024, self.B, 2))
        self.future = None                             # per lane (distances (n,), positions (n, 2))
        self.raises = dict(behind=0, ahead=0, far=0, saturated=0)
        self.rollouts = []                             # per rollout: dict(count (B,), future=[(d, p)] per lane)
        # the ForwardSequenceAgent's own output-only state (measured velocity, head direction): never feeds the motion
        self._fwd_tail = dict(measured_velocity=np.tile([1.0, 0.0], (self.B, 1)), measured_rotational_velocity=np.zeros(self.B),
                              head_direction=np.tile([1.0, 0.0], (self.B, 1)),
                              distance_to_closest_wall=np.full(self.B, np.inf))

    def phase(self, t):
        return (t % (1 / self.theta_freq)) / ((1 / self.theta_freq))

    # ---- the forward rollout (SubAgent.py:305-327) -----------------------------------------------------------------
    def rollout(self, lead, z):
        """`z (n, 2, B)`: [rotation OU, speed OU] normals of the rollout's steps."""
        B = self.B
        st = dict(self._fwd_tail)
        st.update(pos=np.array(lead["pos"], dtype=np.float64).reshape(B, 2),
                  velocity=np.array(lead["velocity"], dtype=np.float64).reshape(B, 2),
                  rotational_velocity=np.array(lead["rotational_velocity"], dtype=np.float64).reshape(B),
                  distance_travelled=np.array(lead["distance_travelled"], dtype=np.float64).reshape(B))
        target = st["distance_travelled"] + self.forward_distance
        fd = [[st["distance_travelled"][b]] for b in range(B)]
        fp = [[st["pos"][b].copy()] for b in range(B)]
        active = st["distance_travelled"] < target
        final = {k: np.array(v, copy=True) for k, v in st.items()}
        k = 0
        while active.any() and k < self.K:
            assert k < len(z), f"the rollout needs more than the {len(z)} normals given"
            new = orc.agent_step(self.env, st, self.dt_forward, np.asarray(z[k][0], dtype=np.float64).reshape(B),
                                 np.asarray(z[k][1], dtype=np.float64).reshape(B), params=self.forward_params)
            st = {key: new[key] for key in final}
            for b in np.nonzero(active)[0]:
                fd[b].append(st["distance_travelled"][b])
                fp[b].append(st["pos"][b].copy())
                for key in final:
                    final[key][b] = st[key][b]
            active = active & (st["distance_travelled"] < target)
            k += 1
        self.raises["saturated"] += int(active.sum())
        self._fwd_tail = {key: final[key] for key in self._fwd_tail}
        self.forward_final = final
        self.future = [(np.array(fd[b]), np.array(fp[b])) for b in range(B)]
        self.rollouts.append(dict(count=np.array([len(d) - 1 for d in fd]), future=self.future))

    def set_future(self, table, count):
        table, count = np.asarray(table, dtype=np.float64), np.asarray(count)
        self.future = [(table[:count[b] + 1, 0, b].copy(), table[:count[b] + 1, 1:3, b].copy()) for b in range(self.B)]

    # ---- one update ------------------------------------------------------------------------------------------------
    def step(self, lead, t, rollout_z=None, future=None):
        B = self.B
        lpos = np.asarray(lead["pos"], dtype=np.float64).reshape(B, 2)
        ldist = np.asarray(lead["distance_travelled"], dtype=np.float64).reshape(B)
        if self.n_rec == len(self.rec_d):
            self.rec_d = np.concatenate((self.rec_d, np.empty_like(self.rec_d)))
            self.rec_p = np.concatenate((self.rec_p, np.empty_like(self.rec_p)))
        self.rec_d[self.n_rec], self.rec_p[self.n_rec] = ldist, lpos
        self.n_rec += 1
        phase = self.phase(t)
        half = self.theta_frac / 2
        pos = np.full((B, 2), np.nan)
        self.rolled_out = False
        if (phase >= (0.5 - half)) and (phase < 0.5):
            for b in range(B):
                if ldist[b] < self.d_half:
                    pos[b] = lpos[b]
                    continue
                L = min(self.lookback, self.n_rec)              # the newest L records (SubAgent.py:283-286)
                d = self.rec_d[self.n_rec - L:self.n_rec, b]
                p = self.rec_p[self.n_rec - L:self.n_rec, b]
                c = self.d_half / self.theta_frac
                m = -2 * c
                x = d[-1] - (m * phase + c)
                idx = int(np.argmin(np.abs(d - x)))
                got = interp1d_linear(d[idx - 3: idx + 3], p[idx - 3: idx + 3], x)
                if got is None:
                    self.raises["behind"] += 1
                else:
                    pos[b] = got
        elif (phase >= 0.5) and (phase < 0.5 + half):
            if self.last_phase < 0.5:
                self.rolled_out = True
                if future is not None:
                    self.set_future(*future)
                else:
                    self.rollout(lead, rollout_z)
            c = -self.d_half / self.theta_frac
            m = -2 * c
            for b in range(B):
                x = ldist[b] + (m * phase + c)
                got = None if self.future is None else interp1d_linear(self.future[b][0], self.future[b][1], x)
                if got is None:
                    self.raises["ahead"] += 1
                else:
                    pos[b] = got
        # further than d_half from the lead, round a periodic box if there is one: no position (SubAgent.py:341-343)
        v = pos - lpos
        if self.env.periodic:
            flip = np.abs(v) > (self.env.scale / 2)
            with np.errstate(invalid="ignore"):
                v = np.where(flip, -np.sign(v) * (self.env.scale - np.abs(v)), v)
        with np.errstate(invalid="ignore"):
            far = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) > self.d_half
        self.raises["far"] += int(far.sum())
        pos[far] = np.nan
        self.last_phase = phase
        return pos
