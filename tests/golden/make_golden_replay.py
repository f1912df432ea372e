"""Generate tests/golden/dumb_*.npz and replay_*.npz by IMPORTING THE REFERENCE's contribs/SubAgent.py, the way
make_golden_subagent.py drives the ThetaSequenceAgent.

Runs only in the build container (needs /root/reference); the .npz files are data (inputs + the reference's outputs)
and are committed.  Nothing from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_replay.py [--out DIR]

`np.random.normal` is wrapped as in make_golden_subagent.py (draws with scale 1e-6 / 1e-9, the reference's geometric
jitter, return zeros; every other draw comes from a private stream and is recorded as a standard normal);
`np.random.uniform` and `np.random.rayleigh` are wrapped too and their outcomes recorded.

Three rooms: `wall` (a solid box with the wall [[0.5, 0], [0.5, 0.5]]), `periodic` (a periodic box), `poly` (an
L-shaped room with a square hole).

dumb_<room>.npz — `Lead.update(); Dumb.update()` of a DumbAgent, per step: lead_pos, z (the two normals of the OU
  increment), disp / vel / pos (displacement, displacement velocity and position after the update), cut (the spring
  crossed a wall), moved (the boundary conditions changed the position).
replay_<room>.npz — `Lead.update(); Rep.update()` of a ReplayAgent with a raised replay_freq, per step: lead_pos, lead_t,
  t_entry (the ReplayAgent's own clock when update() is entered: what it compares with replay_end_time), u (the trigger
  uniform; NaN on steps inside a replay), pos, flag (history["replay"]).  Per replay: start_step, speed / duration (the
  Rayleigh outcomes, the duration before its floor), start_pos, direction, count (updates of the sham agent) and,
  concatenated over the replays, roll_z (sum count, 2) the normals [rotation, speed] of every update and table_dist
  (sum (count + 1),) / table_pos (sum (count + 1), 2) the interpolation table, start entry included.  The run ends
  inside a replay, after at least 5 that ended."""
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

import ratinabox  # noqa: E402
from ratinabox.Environment import Environment  # noqa: E402
from ratinabox.Agent import Agent  # noqa: E402
from ratinabox.contribs.SubAgent import DumbAgent, ReplayAgent  # noqa: E402

_real = np.random.RandomState(0)
_rec, _uni, _ray = [], [], []


def _patched_normal(loc=0.0, scale=1.0, size=None):
    if isinstance(scale, float) and scale in (1e-6, 1e-9):
        return np.zeros(size) + loc
    z = _real.standard_normal(size)
    _rec.append(np.array(z, dtype=np.float64))
    return loc + scale * z


def _patched_uniform(low=0.0, high=1.0, size=None):
    u = _real.uniform(low, high, size)
    _uni.append(np.array(u, dtype=np.float64))
    return u


def _patched_rayleigh(scale=1.0, size=None):
    r = _real.rayleigh(scale, size)
    _ray.append(float(r))
    return r


np.random.normal = _patched_normal
np.random.uniform = _patched_uniform
np.random.rayleigh = _patched_rayleigh

WALL = [[0.5, 0.0], [0.5, 0.5]]
L_ROOM = [[0.0, 0.0], [1.0, 0.0], [1.0, 0.6], [0.6, 0.6], [0.6, 1.0], [0.0, 1.0]]
HOLE = [[0.15, 0.15], [0.3, 0.15], [0.3, 0.3], [0.15, 0.3]]
DT = 0.01

ROOMS = {  # name: (env params, user wall?, lead start (pos, velocity), seed)
    "wall": ({}, True, ([0.46, 0.30], [0.0, 0.05]), 31),
    "periodic": ({"boundary_conditions": "periodic"}, False, ([0.985, 0.52], [0.08, 0.01]), 32),
    "poly": ({"boundary": L_ROOM, "holes": [HOLE]}, False, ([0.34, 0.22], [0.0, 0.05]), 33),
}


def make_env(name):
    env_params, wall, start, seed = ROOMS[name]
    np.random.seed(seed)
    _real.seed(seed)
    Env = Environment(dict(env_params))
    if wall:
        Env.add_wall(np.array(WALL))
    Lead = Agent(Env, {"dt": DT})
    Lead.pos, Lead.velocity = np.array(start[0], dtype=float), np.array(start[1], dtype=float)
    return Env, Lead


def env_record(name):
    env_params, wall, start, _seed = ROOMS[name]
    return dict(dt=np.float64(DT), periodic=np.bool_(env_params.get("boundary_conditions") == "periodic"),
                user_walls=np.array([WALL] if wall else np.zeros((0, 2, 2)), dtype=np.float64),
                env_boundary=np.array(env_params.get("boundary", np.zeros((0, 2))), dtype=np.float64),
                env_holes=np.array(sum(env_params.get("holes", []), []), dtype=np.float64).reshape(-1, 2),
                env_hole_sizes=np.array([len(h) for h in env_params.get("holes", [])], dtype=np.int64),
                pos0=np.array(start[0], dtype=np.float64), vel0=np.array(start[1], dtype=np.float64))


# (the poly room's lead keeps away from the hole: a longer, quicker spring reaches across its walls)
DUMB_PARAMS = {"wall": {}, "periodic": {}, "poly": {"drift_distance": 0.15, "drift_timescale": 2.0}}


def make_dumb(dest, name, n_steps=600):
    Env, Lead = make_env(name)
    Dumb = DumbAgent(Lead, dict(DUMB_PARAMS[name]))
    hits = []
    intercepts = ratinabox.utils.vector_intercepts

    def recording_intercepts(a, b, return_collisions=False):
        out = intercepts(a, b, return_collisions=return_collisions)
        if return_collisions == "as_well":
            hits.append(bool(np.any(out[1])))
        return out

    rec = {k: [] for k in ("lead_pos", "z", "disp", "vel", "pos", "cut", "moved")}
    for _ in range(n_steps):
        Lead.update()
        del _rec[:], _uni[:], hits[:]
        ratinabox.utils.vector_intercepts = recording_intercepts
        try:
            Dumb.update()
        finally:
            ratinabox.utils.vector_intercepts = intercepts
        z = [v for v in _rec if np.shape(v) == (2,)]
        assert len(z) == 1 and len(hits) == 1 and not _uni, (len(z), len(hits), len(_uni))   # (no position was resampled)
        rec["lead_pos"].append(np.array(Lead.pos, dtype=np.float64))
        rec["z"].append(z[0])
        rec["disp"].append(np.array(Dumb.displacement, dtype=np.float64))
        rec["vel"].append(np.array(Dumb.displacement_velocity, dtype=np.float64))
        rec["pos"].append(np.array(Dumb.pos, dtype=np.float64))
        rec["cut"].append(hits[0])
        # (the displacement kept is the environment-aware vector: it differs from pos - lead where the position wrapped)
        rec["moved"].append(not np.allclose(Dumb.pos, Lead.pos + rec["disp"][-1], atol=1e-9, rtol=0))
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(env_record(name))
    out.update(drift_distance=np.float64(Dumb.drift_distance), drift_timescale=np.float64(Dumb.drift_timescale))
    n_cut, n_moved = int(out["cut"].sum()), int(out["moved"].sum())
    if name != "periodic":
        assert n_cut >= 1, "the spring must be cut by a wall within the run"
    else:
        assert n_moved >= 1, "the position must wrap round the periodic box within the run"
    np.savez_compressed(os.path.join(dest, f"dumb_{name}.npz"), **out)
    print(f"dumb_{name}: {n_steps} steps, {n_cut} cut by a wall, {n_moved} moved by the boundary conditions, "
          f"mean |displacement| {np.linalg.norm(out['disp'], axis=1).mean():.4f}")


def make_replay(dest, name, replay_freq=4.0, min_steps=300, max_steps=1500):
    Env, Lead = make_env(name)
    Rep = ReplayAgent(Lead, {"replay_freq": replay_freq})
    sham = Rep.ReplayAgent
    n_updates, trace = [0], []
    sham_update = sham.update

    def counting_update(*a, **k):
        n_before = len(_uni)
        sham_update(*a, **k)
        assert len(_uni) == n_before, "the sham agent resampled its position: not recorded"
        n_updates[0] += 1
        trace.append((float(sham.distance_travelled), np.array(sham.pos, dtype=np.float64)))

    sham.update = counting_update
    started_at = []
    sham_init = sham.initialise_position_and_velocity

    def recording_init():
        sham_init()
        started_at.append((np.array(sham.pos, dtype=np.float64), np.array(sham.velocity, dtype=np.float64),
                           float(sham.distance_travelled)))

    sham.initialise_position_and_velocity = recording_init
    rec = {k: [] for k in ("lead_pos", "lead_t", "t_entry", "u", "pos", "flag")}
    rep = {k: [] for k in ("start_step", "speed", "duration", "start_pos", "direction", "count", "roll_z", "table_dist", "table_pos")}
    n_ended = 0
    for step in range(max_steps):
        Lead.update()
        del _rec[:], _uni[:], _ray[:], started_at[:], trace[:]
        n_updates[0] = 0
        was, t_entry = Rep.is_undergoing_replay, float(Rep.t)
        Rep.update()
        rec["lead_pos"].append(np.array(Lead.pos, dtype=np.float64))
        rec["lead_t"].append(float(Lead.t))
        rec["t_entry"].append(t_entry)
        rec["pos"].append(np.array(Rep.pos, dtype=np.float64))
        rec["flag"].append(bool(Rep.history["replay"][-1]))
        assert rec["flag"][-1] == bool(Rep.is_undergoing_replay)
        rec["u"].append(float(_uni[0]) if not was else np.nan)
        if not was and Rep.is_undergoing_replay:
            pos, vel, dist0 = started_at[0]
            z = [float(v) for v in _rec if np.shape(v) == ()]
            assert len(_ray) == 2 and len(z) == 2 * n_updates[0] and len(started_at) == 1
            direction = float(_uni[-1])
            assert np.array_equal(vel, sham.speed_mean * np.array([np.cos(direction), np.sin(direction)]))
            assert np.array_equal(pos, rec["pos"][-1]) and Rep.replay_speed == _ray[0]
            rep["start_step"].append(step)
            rep["speed"].append(_ray[0])
            rep["duration"].append(_ray[1])
            rep["start_pos"].append(pos)
            rep["direction"].append(direction)
            rep["count"].append(n_updates[0])
            rep["roll_z"].extend(np.array(z).reshape(-1, 2))
            rep["table_dist"].extend(np.array([dist0] + [d for d, _ in trace]) - dist0)
            rep["table_pos"].extend([pos] + [p for _, p in trace])
        else:
            assert n_updates[0] == 0 and not _ray and len(_uni) == (0 if was else 1)
        n_ended += int(was and not Rep.is_undergoing_replay)
        if step + 1 >= min_steps and n_ended >= 5 and Rep.is_undergoing_replay and rep["start_step"][-1] < step:
            break
    else:
        raise AssertionError("no stopping point: 5 ended replays and a run that ends inside one")
    t_entry, lead_t = np.array(rec["t_entry"]), np.array(rec["lead_t"])
    assert t_entry[0] == 0.0 and np.array_equal(t_entry[1:], lead_t[1:]), "the clock a ReplayAgent compares with"
    out = {k: np.array(v) for k, v in rec.items()}
    out.update({k: np.array(v, dtype=np.float64) for k, v in rep.items() if k not in ("start_step", "count")})
    out.update(start_step=np.array(rep["start_step"], dtype=np.int64), count=np.array(rep["count"], dtype=np.int64))
    out.update(env_record(name))
    sham_p = {k: float(getattr(sham, k)) for k in ("speed_mean", "speed_std", "speed_coherence_time",
                                                   "rotational_velocity_std", "rotational_velocity_coherence_time",
                                                   "thigmotaxis", "wall_repel_distance", "wall_repel_strength",
                                                   "head_direction_smoothing_timescale")}
    out.update(replay_freq=np.float64(replay_freq), replay_duration=np.float64(Rep.mean_replay_duration),
               replay_speed=np.float64(Rep.mean_replay_speed), sham_keys=np.array(sorted(sham_p)),
               sham_vals=np.array([sham_p[k] for k in sorted(sham_p)]))
    np.savez_compressed(os.path.join(dest, f"replay_{name}.npz"), **out)
    print(f"replay_{name}: {len(out['flag'])} steps, {len(rep['start_step'])} replays ({n_ended} ended) of "
          f"{min(rep['count'])}-{max(rep['count'])} sham updates, {100 * out['flag'].mean():.0f} % of the steps in replay")


if __name__ == "__main__":
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    for room in ROOMS:
        make_dumb(dest, room)
    for room in ROOMS:
        make_replay(dest, room)
    print("wrote dumb_*.npz, replay_*.npz to", dest)
