"""Theta phase precession on the device (George et al. 2023): first the reference's own example of
contribs.PhasePrecessingPlaceCells — one agent, ten seconds, the per-object loop unchanged — then the batched form the
model was written for: 1024 agents whose phase-precessing place cells feed ONE SuccessorFeatures learner.

    python examples/theta_precession_example.py [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.PhasePrecessingPlaceCells import PhasePrecessingPlaceCells  # noqa: E402
from ratinabox_amd.contribs.SuccessorFeatures import SuccessorFeatures  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
np.random.seed(0)

# ---- the reference's example (contribs/PhasePrecessingPlaceCells.py, __main__) ------------------------------------
Env = riab.Environment()
Ag = riab.Agent(Env)
Ag.speed_mean = 0.3
PPPCs = PhasePrecessingPlaceCells(Ag, params={"widths": 0.3, "theta_freq": 5, "precess_fraction": 1, "kappa": 2, "max_fr": 10.0,
                                              "description": "gaussian"})
while Ag.t < 10:
    Ag.update()
    PPPCs.update()
fr, t = PPPCs.history["firingrate"], PPPCs.history["t"]
best = int(fr.max(axis=0).argmax())
phase = PPPCs.theta_freq * (t % (1 / PPPCs.theta_freq))
active = fr[:, best] > 0.5 * fr[:, best].max()
print(f"one agent, {len(t)} steps: cell {best} peaks at {fr[:, best].max():.2f} Hz (max_fr 10, modulated up to "
      f"{10 * np.exp(2) / np.i0(2):.2f}); while it fires above half of that the theta phase spans "
      f"{phase[active].min():.2f}..{phase[active].max():.2f} of a cycle")
rate_map = PPPCs.get_state(evaluate_at="all")      # (no velocity away from the agent: the plain place fields, as in the reference)
assert rate_map.shape[0] == PPPCs.n and fr.shape == (len(t), PPPCs.n)

# ---- the batched form: phase-precessing cells as the basis of a successor-feature learner ---------------------------
B = 1024
Ag = riab.Agent(riab.Environment(), {"n_agents": B, "dt": 0.01, "speed_mean": 0.2, "save_history": False})
basis = PhasePrecessingPlaceCells(Ag, {"n": 256, "widths": 0.15, "kappa": 1, "theta_freq": 10, "description": "gaussian",
                                       "wall_geometry": "euclidean", "save_history": False})
features = riab.PlaceCells(Ag, {"n": 16, "widths": 0.2, "wall_geometry": "euclidean", "save_history": False})
SF = SuccessorFeatures(Ag, {"input_layers": [basis], "features": features, "tau": 1.0, "eta": 0.01, "save_history": False})
w0 = SF.inputs[basis.name]["w"].copy()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    Ag.update()
    basis.update()        # its own kernel: Agent.velocity and Agent.t are read where they live (float64 state, host clock)
    features.update()
    SF.update()
    SF.update_weights()   # the features are the reward
torch.cuda.synchronize()
dt = time.perf_counter() - t0
dw = np.abs(SF.inputs[basis.name]["w"] - w0).max()
print(f"{steps} steps x {B} agents x {basis.n} phase-precessing cells -> {SF.n} successor features in {dt:.2f} s "
      f"({dt / steps * 1e6:.0f} us per step); largest weight change {dw:.3g}; mean |TD error| {np.abs(SF.td_error).mean():.3g}")
assert dw > 0 and np.isfinite(SF.firingrate).all()
