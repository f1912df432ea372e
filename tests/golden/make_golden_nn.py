"""Generate tests/golden/nn_*.npz by IMPORTING THE REFERENCE's contribs/NeuralNetworkNeurons.py, the way
make_golden_plane_wave.py drives the plane waves.

Runs only in the build container (needs /root/reference); the .npz files are data (the input populations' parameters, the
positions, the reference's input rates, the module's parameters and the reference's outputs) and are committed.  Nothing
from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_nn.py [--out DIR]

nn_default_mlp.npz   only `n` given: the reference's default MultiLayerPerceptron(n_in, n, [20, 20])
nn_sequential.npz    tests/nn_modules.py mixed_sequential (Tanh, Sigmoid, Softplus, Identity; one Linear without bias)
nn_custom.npz        tests/nn_modules.py ResidualBlock (LayerNorm + skip: not a plain perceptron)

torch.manual_seed(seed) directly in front of each module's constructor.  Each file: PlaceCells (30) and GridCells (20)
parameters as feedforward.npz stores them; `pos` — corners, wall points and the centre first, uniform draws behind them
—; `inputs` (n_in, N_P), the reference's concatenated input rates at `pos`; every parameter of the module as
"p::<state_dict key>"; `fr` (n, N_P) = get_state(evaluate_at=None, pos=pos); `agent_pos`, `last_inputs` (n_in,) and `last`
(n,) = one update() row."""
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

warnings.filterwarnings("ignore")

from ratinabox.Environment import Environment  # noqa: E402
from ratinabox.Agent import Agent  # noqa: E402
from ratinabox.Neurons import PlaceCells, GridCells  # noqa: E402
from ratinabox.contribs.NeuralNetworkNeurons import NeuralNetworkNeurons  # noqa: E402

from tests import nn_modules  # noqa: E402

N_P, N_PC, N_GC, N_OUT = 256, 30, 20, 16


def f32exact(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def positions(rng):
    edge = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.5, 0.5)]
    for f in (0.125, 0.5, 0.8125):
        edge += [(f, 0.0), (f, 1.0), (0.0, f), (1.0, f)]
    pos = f32exact(rng.uniform(0.0, 1.0, size=(N_P, 2)))
    pos[:len(edge)] = np.array(edge)
    return pos


def make(dest, name, seed, build):
    np.random.seed(seed)
    Env = Environment()
    Ag = Agent(Env, {"dt": 0.05})
    PCs = PlaceCells(Ag, {"n": N_PC, "name": "PCs"})
    PCs.place_cell_centres = f32exact(PCs.place_cell_centres)
    GCs = GridCells(Ag, {"n": N_GC, "name": "GCs"})
    torch.manual_seed(seed)            # (the module's draws start here)
    N = NeuralNetworkNeurons(Ag, build(N_PC + N_GC, [PCs, GCs]))
    pos = positions(np.random.RandomState(seed + 1))
    inputs = np.concatenate([PCs.get_state(evaluate_at=None, pos=pos), GCs.get_state(evaluate_at=None, pos=pos)])
    fr = N.get_state(evaluate_at=None, pos=pos)
    assert fr.shape == (N.n, N_P) and inputs.shape == (N_PC + N_GC, N_P)
    Ag.pos = f32exact(np.array([0.37, 0.61]))
    PCs.update()
    GCs.update()
    N.update()
    out = dict(seed=np.int64(seed), n=np.int64(N.n), pc_centres=PCs.place_cell_centres, gc_gridscales=GCs.gridscales,
               gc_phase=GCs.phase_offsets, gc_orient=GCs.orientations, pos=pos, inputs=inputs,
               fr=np.asarray(fr, dtype=np.float64), agent_pos=np.array(Ag.pos),
               last_inputs=np.concatenate([PCs.firingrate, GCs.firingrate]).astype(np.float64),
               last=np.asarray(N.firingrate, dtype=np.float64).reshape(-1))
    out.update(nn_modules.state_arrays(N.NeuralNetworkModule))
    np.savez_compressed(os.path.join(dest, f"nn_{name}.npz"), **out)
    print(f"nn_{name}: n = {N.n}, fr in [{fr.min():.3g}, {fr.max():.3g}]")


if __name__ == "__main__":
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    make(dest, "default_mlp", 1201, lambda n_in, layers: {"n": N_OUT, "input_layers": layers})
    make(dest, "sequential", 1202, lambda n_in, layers: {"input_layers": layers,
                                                          "NeuralNetworkModule": nn_modules.mixed_sequential(n_in, N_OUT)})
    make(dest, "custom", 1203, lambda n_in, layers: {"input_layers": layers,
                                                      "NeuralNetworkModule": nn_modules.ResidualBlock(n_in, N_OUT)})
    print("wrote nn_*.npz to", dest)
