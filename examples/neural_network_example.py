"""contribs.NeuralNetworkNeurons on the device: first the reference's own usage (contribs/NeuralNetworkNeurons.py, the class
docstring) — one agent, PlaceCells and GridCells into the default multi-layer perceptron — then the batched form: 1024
agents training a perceptron to read the agent's x coordinate out of its PlaceCells, with `firingrate_torch` and
`torch.optim.Adam`.  The fused kernel reads the weights where the optimiser leaves them: no refresh call anywhere.

    python examples/neural_network_example.py [steps]
"""
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.NeuralNetworkNeurons import NeuralNetworkNeurons, MultiLayerPerceptron  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
np.random.seed(0)
torch.manual_seed(0)

# ---- the reference's usage ----------------------------------------------------------------------------------------------
Env = riab.Environment()
Ag = riab.Agent(Env)
PCs = riab.PlaceCells(Ag)
GCs = riab.GridCells(Ag)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")          # (the reference's notice that a default MLP is used)
    NNNs = NeuralNetworkNeurons(Ag, params={"n": 5, "input_layers": [PCs, GCs]})
for _ in range(20):
    Ag.update()
    PCs.update()
    GCs.update()
    NNNs.update()
print(f"{NNNs.n_in} inputs -> {NNNs.n} units on the {NNNs.engine} engine; firingrate {np.round(NNNs.firingrate, 4)}; "
      f"history {NNNs.history['firingrate'].shape}; firingrate_torch {tuple(NNNs.firingrate_torch.shape)} "
      f"(attached: {NNNs.firingrate_torch.requires_grad})")
assert NNNs.engine == "fused" and NNNs.history["firingrate"].shape == (20, 5)

# ---- the batched form: 1024 agents learn to read out x ----------------------------------------------------------------------
B = 1024
Ag = riab.Agent(riab.Environment(), {"n_agents": B, "dt": 0.05, "save_history": False})
PCs = riab.PlaceCells(Ag, {"n": 100, "widths": 0.15, "save_history": False})
net = MultiLayerPerceptron(n_in=100, n_out=1, n_hidden=[32, 32])
opt = torch.optim.Adam(net.parameters(), lr=3e-3)        # (built first: the constructor's .to(device) keeps the Parameters)
N = NeuralNetworkNeurons(Ag, {"input_layers": [PCs], "NeuralNetworkModule": net, "save_history": False})
first = last = None
for step in range(steps):
    Ag.update()
    PCs.update()
    N.update()                                            # one fused launch; the rates the rest of the package sees
    x = Ag.state_tensor[0, :B].to(torch.float32)          # the agents' x coordinates, on the device
    loss = ((N.firingrate_torch[:, 0] - x) ** 2).mean()  # autograd pass on the same inputs, read before they change
    opt.zero_grad()
    loss.backward()
    opt.step()
    if step % 100 == 0 or step == steps - 1:
        print(f"step {step:5d}  loss {loss.item():.5f}")
    first = loss.item() if first is None else first
    last = loss.item()
Ag.update()
PCs.update()
N.update()
err = np.abs(N.firingrate[0] - np.asarray(Ag.pos)[:, 0])
print(f"read-out of x by the fused kernel with the trained weights: mean |error| {err.mean():.4f} m over {B} agents "
      f"(engine {N.engine})")
assert N.engine == "fused" and (steps < 500 or (last < 0.1 * first and err.mean() < 0.1))
