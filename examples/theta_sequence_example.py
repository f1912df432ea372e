"""Theta sweeps on the device: the reference's usage of contribs.SubAgent.ThetaSequenceAgent — a lead Agent, a
ThetaSequenceAgent slaved to it, PlaceCells on the sweeping position — for one agent, then 1024 agents at once.

    python examples/theta_sequence_example.py [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.SubAgent import ThetaSequenceAgent  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
np.random.seed(0)

# ---- one agent: the sweep starts behind the lead and ends ahead of it ------------------------------------------------
Env = riab.Environment()
Lead = riab.Agent(Env, {"dt": 0.002})
TS = ThetaSequenceAgent(Lead)
PCs = riab.PlaceCells(TS, {"n": 32, "widths": 0.1, "wall_geometry": "euclidean"})
along = []                                   # the sweep's offset from the lead along the lead's direction of travel
while Lead.t < 4.0:
    Lead.update()
    TS.update()
    PCs.update()
    heading = Lead.velocity / np.linalg.norm(Lead.velocity)
    along.append((TS.theta_phase(), float((TS.pos - Lead.pos) @ heading)))
along = np.array(along)
late = along[len(along) * 3 // 4:]           # (the lead has covered d_half by then: the look-behind interpolates)
start = late[(late[:, 0] >= 0.25) & (late[:, 0] < 0.30), 1]
end = late[(late[:, 0] >= 0.70) & (late[:, 0] < 0.75), 1]
fr = PCs.history["firingrate"]
nan = np.isnan(TS.history["pos"][:, 0])
print(f"one agent, {len(along)} steps, {TS.n_rollouts} theta cycles: the sweep starts {-np.nanmean(start) * 100:.1f} cm behind the "
      f"lead and ends {np.nanmean(end) * 100:.1f} cm ahead of it (d_half {TS.d_half * 100:.1f} cm); no position on "
      f"{100 * nan.mean():.0f} % of the steps, where the place cells are silent (max rate {fr[nan].max():.1f}); {TS.theta_diagnostics}")
assert np.nanmean(start) < 0 < np.nanmean(end) and not fr[nan].any() and fr[~nan].max() > 0

# ---- 1024 agents ---------------------------------------------------------------------------------------------------
B = 1024
Lead = riab.Agent(riab.Environment(), {"n_agents": B, "dt": 0.002, "save_history": False})
TS = ThetaSequenceAgent(Lead, {"save_history": False})
PCs = riab.PlaceCells(TS, {"n": 256, "widths": 0.1, "wall_geometry": "euclidean", "save_history": False})
for _ in range(10):
    Lead.update(); TS.update(); PCs.update()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    Lead.update()
    TS.update()
    PCs.update()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
pos = TS.pos
print(f"{steps} steps x {B} agents x {PCs.n} place cells on the sweep in {dt:.2f} s ({dt / steps * 1e6:.0f} us per step, "
      f"{TS.n_rollouts} rollouts of at most {TS.rollout_steps_max} steps); ring of {TS.lookback} records = "
      f"{TS._ring.numel() * 8 / 1e6:.0f} MB; {TS.theta_diagnostics}")
assert pos.shape == (B, 2) and TS.theta_diagnostics["rollout_saturations"] == 0
