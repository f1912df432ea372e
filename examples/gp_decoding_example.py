"""Decoding position with a Gaussian process, beside the ridge decoder, fitted and run on the device.

The reference's comparison (its decoding_position_example demo and tests/test_advanced.py::test_decoding_position): one
agent in a room with a wall, thresholded PlaceCells and GridCells, both decoders fitted on every 5th row of the first part of
the run — GaussianProcessRegressor(alpha=0.01, RBF(sqrt(n / 20))) and Ridge(alpha=0.01) — and tested on the rest.  Then 1024
agents: the GP's training set is chosen from the (row, agent) samples of the recorded history by a deterministic rule, and
every held-out sample is decoded by one fused kernel; nothing is copied to the host.  A closing section asks for the
predictive standard deviation beside the mean (`return_std=True`) and prints how the decoded error compares with it.

    python examples/gp_decoding_example.py [steps]
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
    gp = riab.fit_gp_decoder(pops, target="pos", t_end=t_split, stride=5, alpha=0.01)
    ridge = riab.fit_linear_decoder(pops, target="pos", t_end=t_split, stride=5, alpha=0.01)
    print(f"one agent, {' + '.join(p.name for p in pops)}: {gp.n_samples} training samples, length scale "
          f"{gp.length_scale:.2f}; decoding error on the last {steps - int(0.8 * steps)} rows: GP "
          f"{100 * float(gp.error(t_start=t_split).mean()):.1f} cm, Ridge {100 * float(ridge.error(t_start=t_split).mean()):.1f} cm")

# ---- 1024 agents --------------------------------------------------------------------------------------------------
steps_b = max(50, steps // 15)
Ag = riab.Agent(Env, {"n_agents": 1024, "dt": 0.05})
pops = {"PlaceCells": riab.PlaceCells(Ag, {"n": 64, "description": "gaussian_threshold", "widths": 0.4}),
        "GridCells": riab.GridCells(Ag, {"n": 64})}
Ag.simulate(steps_b)
torch.cuda.synchronize()
t = Ag.history["t"]
t_split = t[int(0.8 * steps_b)]
held_out = (steps_b - int(0.8 * steps_b)) * 1024
for name, N in pops.items():
    t0 = time.perf_counter()
    gp = N.fit_gp_decoder(t_end=t_split, alpha=0.01, max_samples=2048)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    err = gp.error(t_start=t_split)                                    # per agent, on the device
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    ridge = N.fit_decoder(t_end=t_split, alpha=0.01)
    print(f"1024 agents, {name}: GP on {gp.n_samples} of {int(0.8 * steps_b) * 1024} samples fitted in {1e3 * (t1 - t0):.0f} ms, "
          f"{held_out} held-out samples decoded in {1e3 * (t2 - t1):.0f} ms: error {100 * float(err.mean()):.2f} cm "
          f"(worst agent {100 * float(err.max()):.2f} cm); Ridge on every sample {100 * float(ridge.error(t_start=t_split).mean()):.2f} cm")


# ---- the predictive standard deviation: one agent, then 1024 --------------------------------------------------------
def confidence(label, gp, agent, t_split):
    """decoded error, mean predicted std and the share of held-out samples whose error lies within two predicted std (the
    std is the GP's, of each target column: an uncalibrated number, printed as it comes)"""
    mean, std = gp.decode_tensor(t_start=t_split, return_std=True)                  # (T, 2, Bp), (T, Bp) on the device
    B = agent._B
    pos = gp._target_tensor(t_split, None)[:, :, :B]
    err = torch.sqrt(((mean[:, :, :B] - pos) ** 2).sum(dim=1))                      # (T, B)
    ok = torch.isfinite(err) & torch.isfinite(std[:, :B])
    err, sd = err[ok], std[:, :B][ok]
    print(f"{label}: log marginal likelihood {gp.log_marginal_likelihood_:.1f}; decoded error {100 * float(err.mean()):.2f} cm, "
          f"mean predicted std {100 * float(sd.mean()):.2f} cm, {100 * float((err <= 2 * sd).float().mean()):.1f} % of "
          f"{int(ok.sum())} samples within two predicted std")


np.random.seed(0)
Ag1 = riab.Agent(Env, {"dt": 0.05})
PC1 = riab.PlaceCells(Ag1, {"n": 20, "description": "gaussian_threshold", "widths": 0.4})
Ag1.simulate(steps)
t1 = Ag1.history["t"]
confidence("one agent, PlaceCells", riab.fit_gp_decoder([PC1], t_end=t1[int(0.8 * steps)], stride=5), Ag1, t1[int(0.8 * steps)])
for name, N in pops.items():
    confidence(f"1024 agents, {name}", N.fit_gp_decoder(t_end=t_split, alpha=0.01, max_samples=2048), Ag, t_split)
