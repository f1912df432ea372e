"""Generate tests/golden/theta_*.npz by IMPORTING THE REFERENCE's contribs/PhasePrecessingPlaceCells.py, the way
make_golden_td.py drives the TD learners.

Runs only in the build container (needs /root/reference); the .npz files are data (inputs + the reference's outputs)
and are committed.  Nothing from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_theta.py [--out DIR]

theta_set_<name>.npz — set-state samples of one configuration (the four descriptions, solid and periodic rooms,
min_fr != 0, kappa 1 / 2 / 4): N_T time stamps (pairs straddling a multiple of 1 / theta_freq among them) x N_P
(pos, velocity) pairs (points within 2 cm of a wall, resting and almost resting agents among them).  Each sample is set on
ONE reference agent (`Ag.pos`, `Ag.velocity`, `Ag.t`) before `get_state()`; `fr[k, j]` = its rates at stamp k, pair j.

theta_rollout.npz — one natural run of T_ROLL reference steps at dt 1 ms (`Ag.update(); PPPCs.update()`), started
2 cm from a wall and heading into it: per step pos, velocity (Agent.velocity), measured velocity, t and firingrate.  Pins
that update() reads Agent.velocity and the clock after the agent's update."""
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
from ratinabox.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells  # noqa: E402

N_CELLS, N_T, N_P, T_ROLL, N_ROLL = 8, 16, 256, 2000, 24

CONFIGS = [  # name, description, periodic, kappa, theta_freq, precess_fraction, widths, min_fr, max_fr
    ("gaussian_solid", "gaussian", False, 1.0, 10.0, 0.5, 0.20, 0.5, 10.0),
    ("threshold_periodic", "gaussian_threshold", True, 2.0, 10.0, 0.5, 0.25, 0.2, 1.0),
    ("dog_solid", "diff_of_gaussians", False, 4.0, 8.0, 0.75, 0.15, 0.0, 5.0),
    ("tophat_periodic", "top_hat", True, 1.0, 10.0, 0.5, 0.30, 0.3, 2.0),
    ("gaussian_periodic", "gaussian", True, 4.0, 5.0, 1.0, 0.30, 0.1, 10.0),
    ("threshold_solid", "gaussian_threshold", False, 2.0, 6.0, 0.25, 0.20, 0.0, 1.0),
]


def stamps(theta_freq):
    p = 1.0 / theta_freq
    t = [0.0, 0.013, 1 * p - 1e-7, 1 * p + 1e-7, 0.25, 3 * p, 1.0, 1.2345, 30 * p - 1e-9, 30 * p + 1e-9, 7.77, 12.5,
         600 * p - 1e-6, 600 * p + 1e-6, 123.456, 600.05]
    assert len(t) == N_T
    return np.array(t, dtype=np.float64)


def pairs(rng):
    pos = rng.uniform(0.0, 1.0, size=(N_P, 2))
    near = rng.uniform(1e-3, 0.02, size=32)            # points beside a wall, all four walls
    for j in range(32):
        pos[j, j % 2] = near[j] if (j // 2) % 2 == 0 else 1.0 - near[j]
    ang = rng.uniform(0, 2 * np.pi, size=N_P)
    speed = rng.rayleigh(0.08, size=N_P)
    speed[32:40] = 0.0                                  # at rest: dir = 0, preferred phase pi
    speed[40:44] = 1e-7                                 # almost at rest: the 1e-8 of the normalisation shows
    speed[44:48] = 1e-8
    vel = speed[:, None] * np.stack((np.cos(ang), np.sin(ang)), axis=-1)
    return pos, vel


def make_set(dest, k, cfg):
    name, desc, periodic, kappa, tf, pf, widths, min_fr, max_fr = cfg
    np.random.seed(100 + k)
    rng = np.random.RandomState(200 + k)
    Env = Environment({"boundary_conditions": "periodic" if periodic else "solid"})
    Ag = Agent(Env)
    N = PhasePrecessingPlaceCells(Ag, {"n": N_CELLS, "description": desc, "kappa": kappa, "theta_freq": tf,
                                       "precess_fraction": pf, "widths": widths, "min_fr": min_fr, "max_fr": max_fr,
                                       "wall_geometry": "euclidean"})
    ts = stamps(tf)
    pos, vel = pairs(rng)
    fr = np.empty((N_T, N_P, N_CELLS), dtype=np.float64)
    for i, t in enumerate(ts):
        for j in range(N_P):
            Ag.pos, Ag.velocity, Ag.t = pos[j].copy(), vel[j].copy(), float(t)
            fr[i, j] = N.get_state().reshape(-1)
    out = dict(t=ts, pos=pos, vel=vel, fr=fr, centres=N.place_cell_centres.copy(),
               widths=np.asarray(N.place_cell_widths, dtype=np.float64).copy(), widths_scalar=np.float64(N.widths),
               description=np.array(desc), theta_freq=np.float64(tf), kappa=np.float64(kappa), precess_fraction=np.float64(pf),
               min_fr=np.float64(min_fr), max_fr=np.float64(max_fr), periodic=np.bool_(periodic),
               extent=np.array([Env.extent[1] - Env.extent[0], Env.extent[3] - Env.extent[2]], dtype=np.float64))
    np.savez_compressed(os.path.join(dest, f"theta_set_{name}.npz"), **out)
    print(f"theta_set_{name}: fr in [{fr.min():.3g}, {fr.max():.3g}]")


def make_rollout(dest):
    np.random.seed(42)
    Env = Environment()
    Ag = Agent(Env, {"dt": 0.001})
    Ag.pos = np.array([0.02, 0.4])
    Ag.velocity = np.array([-0.08, 0.03])
    kappa, tf, pf, widths, min_fr, max_fr = 2.0, 10.0, 0.5, 0.2, 0.25, 5.0
    N = PhasePrecessingPlaceCells(Ag, {"n": N_ROLL, "description": "gaussian", "kappa": kappa, "theta_freq": tf,
                                       "precess_fraction": pf, "widths": widths, "min_fr": min_fr, "max_fr": max_fr,
                                       "wall_geometry": "euclidean"})
    out = dict(pos0=Ag.pos.copy(), vel0=Ag.velocity.copy())
    rec = {k: [] for k in ("pos", "vel", "mvel", "t", "fr")}
    for _ in range(T_ROLL):
        Ag.update()
        N.update()
        rec["pos"].append(Ag.pos.copy())
        rec["vel"].append(Ag.velocity.copy())
        rec["mvel"].append(Ag.measured_velocity.copy())
        rec["t"].append(Ag.t)
        rec["fr"].append(N.firingrate.copy())
    out.update({k: np.array(v, dtype=np.float64) for k, v in rec.items()})
    gap = np.abs(out["vel"] - out["mvel"]).max()
    print(f"theta_rollout: max |Agent.velocity - measured velocity| = {gap:.3g}")
    assert gap > 1e-6, "the rollout must meet a wall: Agent.velocity and the measured velocity have to differ somewhere"
    out.update(centres=N.place_cell_centres.copy(), widths=np.asarray(N.place_cell_widths, dtype=np.float64).copy(),
               widths_scalar=np.float64(N.widths), description=np.array("gaussian"), theta_freq=np.float64(tf),
               kappa=np.float64(kappa), precess_fraction=np.float64(pf), min_fr=np.float64(min_fr), max_fr=np.float64(max_fr),
               periodic=np.bool_(False), extent=np.array([1.0, 1.0]), dt=np.float64(0.001))
    np.savez_compressed(os.path.join(dest, "theta_rollout.npz"), **out)


if __name__ == "__main__":
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    for k, cfg in enumerate(CONFIGS):
        make_set(dest, k, cfg)
    make_rollout(dest)
    print("wrote theta_set_*.npz, theta_rollout.npz to", dest)
