"""Decoding position from spikes of a RECORDED run: the Bayesian decoder's forward filter followed by a backward smoother.

`decoder.with_continuity()` decodes window t from the windows up to t.  But the history it reads is a finished run: the whole
of it is in device memory, so window t can be decoded from every window of the run, before AND after it, the forward-backward
(smoothed) posterior p(x_t | k_1..k_T) of offline place-cell decoding.  `filt.smoothed()` runs the filter with the log
posterior of every window kept, then one more sequential scan from the last window to the first (two kernels per window, all
issued by one native call); the decoded positions never leave the device.  24 place cells of 10 Hz, windows of 50 ms: first
one agent, then 64.

    python examples/bayesian_smoother_example.py [steps]
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
CELLS = {"n": 24, "widths": 0.15, "max_fr": 10.0, "save_spikes": True}


def compare(PCs, label):
    dec = PCs.fit_bayesian_decoder(tuning="groundtruth", window=1)
    filt = dec.with_continuity()                                         # sigma: speed_mean x window x dt, at least half a bin
    sm = filt.smoothed()                                                 # max_state_bytes=2**31: what may stay on the device
    timed = []
    for d in (dec, filt, sm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e = float(d.error().mean())
        torch.cuda.synchronize()
        timed.append((e, time.perf_counter() - t0))
    (e_dec, t_dec), (e_filt, t_filt), (e_sm, t_sm) = timed
    print(f"  {label}, windows of {1e3 * PCs.Agent.dt:.0f} ms, {dec.n_bins} bins, step of {filt.radius} bins: memoryless {100 * e_dec:.1f} cm "
          f"in {1e3 * t_dec:.1f} ms, filtered {100 * e_filt:.1f} cm in {1e3 * t_filt:.1f} ms, smoothed {100 * e_sm:.1f} cm in {1e3 * t_sm:.1f} ms")
    return filt, sm


# ---- one agent ------------------------------------------------------------------------------------------------------
Env = riab.Environment({"dx": 0.05})
Ag = riab.Agent(Env, {"dt": 0.05})
PCs = riab.PlaceCells(Ag, CELLS)
Ag.simulate(steps)
print(f"one agent, {PCs.n} place cells of {CELLS['max_fr']:.0f} Hz, {steps} rows of 50 ms, ground-truth tuning curves:")
filt, sm = compare(PCs, "1 agent")
f, s = filt.decode_all_tensor(), sm.decode_all_tensor()
print(f"  the run's log evidence (the sum of row 4, the same in both): {float(s[:, 4, 0].sum()):.1f}; mean MAP probability: filtered "
      f"{float(f[:, 5, 0].mean()):.3f}, smoothed {float(s[:, 5, 0].mean()):.3f}")

# ---- 64 agents ----------------------------------------------------------------------------------------------------------
steps_b = max(100, steps // 10)
Ag = riab.Agent(Env, {"n_agents": 64, "dt": 0.05})
PCs = riab.PlaceCells(Ag, CELLS)
Ag.simulate(steps_b)
torch.cuda.synchronize()
print(f"64 agents, {steps_b} rows each:")
compare(PCs, "64 agents")
