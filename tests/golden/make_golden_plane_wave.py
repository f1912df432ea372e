"""Generate tests/golden/plane_wave_*.npz by IMPORTING THE REFERENCE's contribs/PlaneWaveNeurons.py, the way
make_golden_theta.py drives the phase-precessing place cells.

Runs only in the build container (needs /root/reference); the .npz files are data (the drawn or assigned arrays, the
positions and the reference's get_state output) and are committed.  Nothing from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_plane_wave.py [--out DIR]

plane_wave_defaults.npz   default parameters; np.random.seed(SEED) directly in front of the constructor (the seed is
                          stored: the product's constructor must draw the same arrays)
plane_wave_periodic.npz   periodic room, wavescale 0.05, min_fr 0.5, max_fr 10
plane_wave_assigned.npz   hand-assigned arrays in a 2 x 1 m room (aspect 2): axis-aligned and diagonal w, wavelengths from
                          0.02 to 5 (longer than the room), offsets outside [0, lambda) and negative

Each: N_P positions — the four corners, points on each wall and the room's centre first, uniform draws behind them —
and `fr` (n, N_P) = PlaneWaveNeurons.get_state(evaluate_at=None, pos=pos)."""
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
from ratinabox.contribs.PlaneWaveNeurons import PlaneWaveNeurons  # noqa: E402

N_CELLS, N_P = 12, 256


def positions(rng, width, height):
    edge = [(0.0, 0.0), (width, 0.0), (0.0, height), (width, height), (width / 2, height / 2)]
    for f in (0.125, 0.5, 0.8125):
        edge += [(f * width, 0.0), (f * width, height), (0.0, f * height), (width, f * height)]
    pos = rng.uniform(0.0, 1.0, size=(N_P, 2)) * np.array([width, height])
    pos[:len(edge)] = np.array(edge)
    return pos


def save(dest, name, N, Env, pos, seed, periodic):
    fr = N.get_state(evaluate_at=None, pos=pos)
    assert fr.shape == (N.n, len(pos))
    out = dict(seed=np.int64(seed), n=np.int64(N.n), wavescale=np.float64(N.wavescale), min_fr=np.float64(N.min_fr),
               max_fr=np.float64(N.max_fr), periodic=np.bool_(periodic), aspect=np.float64(Env.aspect),
               scale=np.float64(Env.scale), extent=np.asarray(Env.extent, dtype=np.float64),
               phase_offsets=np.asarray(N.phase_offsets, dtype=np.float64).copy(), w=np.asarray(N.w, dtype=np.float64).copy(),
               wavescales=np.asarray(N.wavescales, dtype=np.float64).copy(), pos=pos, fr=np.asarray(fr, dtype=np.float64))
    np.savez_compressed(os.path.join(dest, f"plane_wave_{name}.npz"), **out)
    print(f"plane_wave_{name}: fr in [{fr.min():.3g}, {fr.max():.3g}], wavescales in [{N.wavescales.min():.3g}, "
          f"{N.wavescales.max():.3g}]")


def make_defaults(dest, seed=1234):
    Env = Environment()
    Ag = Agent(Env)
    np.random.seed(seed)               # (the population's draws start here, whatever the agent drew)
    N = PlaneWaveNeurons(Ag)           # (defaults: n = 10)
    save(dest, "defaults", N, Env, positions(np.random.RandomState(300), 1.0, 1.0), seed, False)


def make_periodic(dest, seed=4321):
    Env = Environment({"boundary_conditions": "periodic"})
    Ag = Agent(Env)
    np.random.seed(seed)               # (the population's draws start here, whatever the agent drew)
    N = PlaneWaveNeurons(Ag, {"n": N_CELLS, "wavescale": 0.05, "min_fr": 0.5, "max_fr": 10})
    save(dest, "periodic", N, Env, positions(np.random.RandomState(301), 1.0, 1.0), seed, True)


def make_assigned(dest, seed=99):
    Env = Environment({"aspect": 2, "scale": 1})
    Ag = Agent(Env)
    np.random.seed(seed)               # (the population's draws start here, whatever the agent drew)
    N = PlaneWaveNeurons(Ag, {"n": N_CELLS, "min_fr": 0.0, "max_fr": 1.0})
    s = np.sqrt(0.5)
    N.w = np.array([[1, 0], [0, 1], [-1, 0], [0, -1], [s, s], [s, -s], [-s, s], [-s, -s], [0.6, 0.8], [-0.8, 0.6], [1, 0], [0, 1]],
                   dtype=np.float64)
    N.wavescales = np.array([0.02, 0.02, 0.05, 0.1, 0.02, 0.3, 0.7, 1.0, 2.0, 5.0, 5.0, 0.035], dtype=np.float64)
    N.phase_offsets = np.array([[0.0, 0.0], [0.3, -0.4], [-1.5, 2.5], [0.01, 0.02], [7.0, -3.0], [0.31, 0.29], [-0.2, -0.9],
                                [1.0, 1.0], [-4.0, 0.5], [12.5, -12.5], [0.0, 100.0], [0.0175, 0.0525]], dtype=np.float64)
    save(dest, "assigned", N, Env, positions(np.random.RandomState(302), 2.0, 1.0), seed, False)


if __name__ == "__main__":
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    make_defaults(dest)
    make_periodic(dest)
    make_assigned(dest)
    print("wrote plane_wave_*.npz to", dest)
