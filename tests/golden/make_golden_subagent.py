"""Generate tests/golden/subagent_*.npz by IMPORTING THE REFERENCE's contribs/SubAgent.py, the way make_golden_theta.py
drives the phase-precessing place cells.

Runs only in the build container (needs /root/reference); the .npz files are data (inputs + the reference's outputs)
and are committed.  Nothing from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_subagent.py [--out DIR]

`np.random.normal` is wrapped as in make_golden.py: draws with scale 1e-6 / 1e-9 (the reference's geometric
anti-degeneracy jitter) return zeros, every other draw comes from a private stream and is recorded as a standard normal.

subagent_theta_<name>.npz — one run of `Lead.update(); TS.update()` of a ThetaSequenceAgent:
  per step     lead_pos, lead_dist, lead_t (the lead after its update), sub_pos (the ThetaSequenceAgent after its own);
               sub_t_head: the ThetaSequenceAgent's clock on the first 100 steps (the script asserts `sub_t == lead_t + dt`
               on every step)
  per rollout  roll_step (index of the step it happened on), roll_count (updates of the ForwardSequenceAgent),
               roll_lead_vel / roll_lead_rot (the lead's velocity and rotational velocity, which only a rollout reads), and,
               concatenated over the rollouts, roll_z (sum count, 2) the normals [rotation, speed] of every update,
               fut_dist (sum (count + 1),) / fut_pos (sum (count + 1), 2) the future arrays, start entry included
  far_steps    steps whose position the `d_half` rule turned into NaN
subagent_shift.npz — a ShiftAgent with shift_m +0.03 and one with -0.03 on the same lead, 200 steps: lead_pos, lead_hd,
  pos_plus, pos_minus."""
import math
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

from ratinabox.Environment import Environment  # noqa: E402
from ratinabox.Agent import Agent  # noqa: E402
from ratinabox.contribs.SubAgent import ShiftAgent, ThetaSequenceAgent  # noqa: E402

_real = np.random.RandomState(0)
_rec = []
_orig_normal = np.random.normal


def _patched_normal(loc=0.0, scale=1.0, size=None):
    if isinstance(scale, float) and scale in (1e-6, 1e-9):
        return np.zeros(size) + loc
    z = _real.standard_normal(size)
    _rec.append(np.array(z, dtype=np.float64))
    return loc + scale * z


np.random.normal = _patched_normal

WALL = [[0.5, 0.0], [0.5, 0.5]]

CONFIGS = [  # name, env params, wall?, dt, steps, ThetaSequenceAgent params, lead start (pos, velocity), seed
    ("solid_wall", {}, True, 0.002, 1500, {}, ([0.42, 0.30], [0.08, 0.0]), 11),
    ("periodic", {"boundary_conditions": "periodic"}, False, 0.002, 1500, {}, ([0.97, 0.52], [0.08, 0.01]), 12),
    ("params", {}, False, 0.001, 3000, {"theta_freq": 8.0, "theta_frac": 0.6, "v_sequence": 3.0, "speed_mean": 0.12},
     ([0.30, 0.70], [0.0, -0.08]), 13),
]


def make_theta(dest, cfg):
    name, env_params, wall, dt, n_steps, ts_params, (pos0, vel0), seed = cfg
    np.random.seed(seed)
    _real.seed(seed)
    Env = Environment(dict(env_params))
    if wall:
        Env.add_wall(np.array(WALL))
    Lead = Agent(Env, {"dt": dt})
    Lead.pos, Lead.velocity = np.array(pos0, dtype=float), np.array(vel0, dtype=float)
    TS = ThetaSequenceAgent(Lead, dict(ts_params))
    K = int(math.ceil(4 * (TS.d_half + 100 * Lead.average_measured_speed * (TS.theta_frac / 2) * TS.T_theta)
                      / (dt * TS.v_sequence))) + 8
    fwd = TS.ForwardSequenceAgent
    trace = []
    fwd_update = fwd.update

    def recording_update(*a, **k):
        fwd_update(*a, **k)
        trace.append((float(fwd.distance_travelled), np.array(fwd.pos, dtype=np.float64)))

    fwd.update = recording_update
    dists = []
    env_dist = Env.get_distances_between___accounting_for_environment

    def recording_dist(*a, **k):
        d = env_dist(*a, **k)
        dists.append(float(np.ravel(d)[0]))
        return d

    rec = {k: [] for k in ("lead_pos", "lead_dist", "lead_t", "sub_pos")}
    roll = {k: [] for k in ("roll_step", "roll_count", "roll_z", "fut_dist", "fut_pos", "roll_lead_vel", "roll_lead_rot")}
    sub_t_head = []
    far_steps = []
    for step in range(n_steps):
        Lead.update()
        start = (float(Lead.distance_travelled), np.array(Lead.pos, dtype=np.float64))
        del _rec[:], trace[:], dists[:]
        Env.get_distances_between___accounting_for_environment = recording_dist
        try:
            TS.update()   # (must not raise: the fixture pins the reference where it is defined)
        finally:
            del Env.get_distances_between___accounting_for_environment
        rec["lead_pos"].append(np.array(Lead.pos, dtype=np.float64))
        rec["lead_dist"].append(float(Lead.distance_travelled))
        rec["lead_t"].append(float(Lead.t))
        rec["sub_pos"].append(np.array(TS.pos, dtype=np.float64))
        assert float(TS.t) == float(Lead.t) + dt
        if step < 100:
            sub_t_head.append(float(TS.t))
        if len(dists) == 1 and dists[0] > TS.d_half:
            far_steps.append(step)
        if trace:
            z = [float(v) for v in _rec if np.shape(v) == ()]
            assert len(z) == 2 * len(trace), (len(z), len(trace))
            assert len(trace) <= K // 2, f"rollout of {len(trace)} steps, K = {K}"
            roll["roll_step"].append(step)
            roll["roll_count"].append(len(trace))
            roll["roll_lead_vel"].append(np.array(Lead.velocity, dtype=np.float64))
            roll["roll_lead_rot"].append(float(Lead.rotational_velocity))
            roll["roll_z"].extend(np.array(z).reshape(-1, 2))
            roll["fut_dist"].extend([start[0]] + [d for d, _ in trace])
            roll["fut_pos"].extend([start[1]] + [p for _, p in trace])
    out = {k: np.array(v, dtype=np.float64) for k, v in rec.items()}
    out.update({k: np.array(v, dtype=np.float64) for k, v in roll.items() if k not in ("roll_step", "roll_count")})
    out.update(roll_step=np.array(roll["roll_step"], dtype=np.int64), roll_count=np.array(roll["roll_count"], dtype=np.int64),
               far_steps=np.array(far_steps, dtype=np.int64), sub_t_head=np.array(sub_t_head, dtype=np.float64))
    moved = np.diff(np.concatenate(([0.0], out["lead_dist"])))
    assert (moved > 0).all(), "a zero-displacement step of the lead"
    assert out["lead_dist"][-1] > 1.5 * TS.d_half, "the run must reach the interpolating look-behind branch"
    if name == "periodic":
        assert len(far_steps) >= 1, "the periodic run must meet the d_half rule"
    forward = {k: float(getattr(fwd, k)) for k in ("speed_mean", "speed_std", "speed_coherence_time",
                                                    "rotational_velocity_std", "rotational_velocity_coherence_time",
                                                    "thigmotaxis", "wall_repel_distance", "wall_repel_strength",
                                                    "head_direction_smoothing_timescale")}
    out.update(dt=np.float64(dt), K=np.int64(K), periodic=np.bool_(Env.boundary_conditions == "periodic"),
               user_walls=np.array([WALL] if wall else np.zeros((0, 2, 2)), dtype=np.float64),
               pos0=np.array(pos0, dtype=np.float64), vel0=np.array(vel0, dtype=np.float64),
               theta_freq=np.float64(TS.theta_freq), theta_frac=np.float64(TS.theta_frac), v_sequence=np.float64(TS.v_sequence),
               lead_average_speed=np.float64(Lead.average_measured_speed), lead_speed_mean=np.float64(Lead.speed_mean),
               forward_keys=np.array(sorted(forward)), forward_vals=np.array([forward[k] for k in sorted(forward)]))
    np.savez_compressed(os.path.join(dest, f"subagent_theta_{name}.npz"), **out)
    nan = np.isnan(out["sub_pos"][:, 0]).mean()
    print(f"subagent_theta_{name}: {len(roll['roll_step'])} rollouts of {min(roll['roll_count'])}-{max(roll['roll_count'])} "
          f"steps (K = {K}), {100 * nan:.0f} % NaN steps, {len(far_steps)} by the d_half rule, lead distance "
          f"{out['lead_dist'][-1]:.3f} m")


def make_shift(dest):
    np.random.seed(21)
    _real.seed(21)
    Env = Environment()
    Env.add_wall(np.array(WALL))
    Lead = Agent(Env, {"dt": 0.01})
    plus, minus = ShiftAgent(Lead, {"shift_m": 0.03}), ShiftAgent(Lead, {"shift_m": -0.03})
    rec = {k: [] for k in ("lead_pos", "lead_hd", "pos_plus", "pos_minus")}
    for _ in range(200):
        Lead.update()
        plus.update()
        minus.update()
        rec["lead_pos"].append(np.array(Lead.pos, dtype=np.float64))
        rec["lead_hd"].append(np.array(Lead.head_direction, dtype=np.float64))
        rec["pos_plus"].append(np.array(plus.pos, dtype=np.float64))
        rec["pos_minus"].append(np.array(minus.pos, dtype=np.float64))
    np.savez_compressed(os.path.join(dest, "subagent_shift.npz"), **{k: np.array(v) for k, v in rec.items()})
    print("subagent_shift: 200 steps")


if __name__ == "__main__":
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    for cfg in CONFIGS:
        make_theta(dest, cfg)
    make_shift(dest)
    print("wrote subagent_theta_*.npz, subagent_shift.npz to", dest)
