"""Decoding position from the population, fitted on the device.

First the reference's scenario (its decoding_position_example demo and tests/test_advanced.py::test_decoding_position)
for ONE agent: a room with a wall, PlaceCells and GridCells, a ridge decoder fitted on every 5th row of the first part of
the run and tested on the rest.  Then 1024 agents: the decoding error of PlaceCells, GridCells and
BoundaryVectorCells fitted on every (step, agent) sample of the recorded history — nothing is copied to the host —
and the PlaceCell decoder handed back as a live FeedForwardLayer whose firing rate IS the decoded position.

    python examples/decoding_example.py [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 3000
np.random.seed(0)

# ---- one agent: the reference's scenario ------------------------------------------------------------------------
Env = riab.Environment()
Env.add_wall(np.array([[0.4, 0], [0.4, 0.4]]))
Ag = riab.Agent(Env, {"dt": 0.05})
PCs = riab.PlaceCells(Ag, {"n": 20, "description": "gaussian_threshold", "widths": 0.4})
GCs = riab.GridCells(Ag, {"n": 20})
Ag.simulate(steps)
t = Ag.history["t"]
t_split = t[int(0.8 * steps)]
for pops in ([PCs], [GCs], [PCs, GCs]):
    dec = riab.fit_linear_decoder(pops, target="pos", t_end=t_split, stride=5, alpha=0.01)
    err = float(dec.error(t_start=t_split).mean())
    print(f"one agent, {' + '.join(p.name for p in pops)}: fitted on {dec.n_samples} samples, "
          f"decoding error on the last {steps - int(0.8 * steps)} rows {100 * err:.1f} cm")

# ---- 1024 agents --------------------------------------------------------------------------------------------------
steps_b = max(50, steps // 15)
Ag = riab.Agent(Env, {"n_agents": 1024, "dt": 0.05})
pops = {"PlaceCells": riab.PlaceCells(Ag, {"n": 64, "description": "gaussian_threshold", "widths": 0.4}),
        "GridCells": riab.GridCells(Ag, {"n": 64}),
        "BoundaryVectorCells": riab.BoundaryVectorCells(Ag, {"n": 64})}
Ag.simulate(steps_b)
torch.cuda.synchronize()
t = Ag.history["t"]
t_split = t[int(0.8 * steps_b)]
decoders = {}
for name, N in pops.items():
    t0 = time.perf_counter()
    dec = decoders[name] = N.fit_decoder(t_end=t_split, alpha=0.01)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    err = dec.error(t_start=t_split)                                   # per agent, on the device
    print(f"1024 agents, {name}: {dec.n_samples} samples fitted in {1e3 * dt:.1f} ms; held-out decoding error "
          f"{100 * float(err.mean()):.2f} cm (worst agent {100 * float(err.max()):.2f} cm)")

# ---- the decoder as a population ------------------------------------------------------------------------------------
layer = decoders["PlaceCells"].as_layer({"name": "DecodedPosition"})
for _ in range(20):
    Ag.update()
    pops["PlaceCells"].update()
    layer.update()
gap = np.linalg.norm(layer.firingrate.T - Ag.pos, axis=1)
print(f"DecodedPosition (a FeedForwardLayer, n = {layer.n}): after 20 live steps its firing rate is "
      f"{100 * gap.mean():.2f} cm from the agents' positions on average")
assert gap.mean() < 0.1
