"""Decoding position from SPIKES with a Bayesian (Poisson maximum-likelihood) decoder, fitted and run on the device.

The decoder of the place-cell literature: the spike counts of a short time window are set against the cells' tuning curves,
and the posterior over position bins gives an estimate (its mean, or its most probable bin) and a measure of confidence.
Here the tuning curves are the rate maps of the first part of a run, binned from the recorded spikes; the rest of the run is
decoded window by window from its spikes, by one fused kernel, and set against the ridge decoder — which reads the RATES an
experiment never has.  First one agent, then 1024; nothing is copied to the host.

    python examples/bayesian_decoding_example.py [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 6000
np.random.seed(0)
CELLS = {"n": 80, "widths": 0.15, "max_fr": 10.0, "save_spikes": True}

# ---- one agent ------------------------------------------------------------------------------------------------------
Env = riab.Environment()
Ag = riab.Agent(Env, {"dt": 0.05})
PCs = riab.PlaceCells(Ag, CELLS)
Ag.simulate(steps)
t = Ag.history["t"]
t_split = t[int(0.8 * steps)]
ridge = PCs.fit_decoder(t_end=t_split, alpha=0.01)
print(f"one agent, {PCs.n} place cells of {CELLS['max_fr']:.0f} Hz, tuning curves from the spikes of {int(0.8 * steps)} rows; "
      f"decoding the last {steps - int(0.8 * steps)} rows (Ridge on the rates: {100 * float(ridge.error(t_start=t_split).mean()):.1f} cm)")
for window in (1, 5, 20):
    dec = PCs.fit_bayesian_decoder(tuning="history", bin_size=0.05, t_end=t_split, spikes=True, window=window)
    out = dec.decode_all_tensor(t_start=t_split)                      # (windows, 6, 4): mean, MAP, log evidence, MAP probability
    print(f"  windows of {window:2d} rows ({1e3 * window * Ag.dt:.0f} ms): {out.shape[0]} windows on {dec.n_bins} bins, error of the "
          f"posterior mean {100 * float(dec.error(t_start=t_split).mean()):.1f} cm, MAP probability {float(out[:, 5, 0].mean()):.2f} on average")

# ---- 1024 agents --------------------------------------------------------------------------------------------------------
steps_b = max(100, steps // 20)
Ag = riab.Agent(Env, {"n_agents": 1024, "dt": 0.05})
PCs = riab.PlaceCells(Ag, CELLS)
Ag.simulate(steps_b)
torch.cuda.synchronize()
t = Ag.history["t"]
t_split = t[int(0.8 * steps_b)]
held_out = steps_b - int(0.8 * steps_b)
ridge = PCs.fit_decoder(t_end=t_split, alpha=0.01)
for prior in ("uniform", "occupancy"):
    t0 = time.perf_counter()
    dec = PCs.fit_bayesian_decoder(tuning="history", t_end=t_split, spikes=True, prior=prior, window=5)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    err = dec.error(t_start=t_split)                                  # per agent, on the device
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"1024 agents, {prior} prior: tables of {dec.n_bins} bins from {int(0.8 * steps_b) * 1024} samples in {1e3 * (t1 - t0):.1f} ms, "
          f"{(held_out // 5) * 1024} windows of 5 rows decoded from spikes in {1e3 * (t2 - t1):.1f} ms: error "
          f"{100 * float(err.mean()):.2f} cm (worst agent {100 * float(err.max()):.2f} cm); Ridge on the rates "
          f"{100 * float(ridge.error(t_start=t_split).mean()):.2f} cm")
