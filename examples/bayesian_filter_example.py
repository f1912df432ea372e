"""Decoding position from spikes with a continuity prior: the Bayesian decoder run as a forward filter on the device.

`fit_bayesian_decoder` decodes every window from the fitted prior alone, so a 50 ms window with a few dozen cells jumps
across the room whenever it holds few spikes.  `decoder.with_continuity()` carries the posterior of one window to the next
through a Gaussian step over the admissible bins (the animal cannot have moved far: the two-step reconstruction of Zhang et
al. 1998), mixed with a small share of the prior.  The likelihood of a batch of windows is one GEMM, the scan over the
windows two kernels per window, all issued by one native call; the decoded positions never leave the device.  First one
agent, then 1024, at windows of 1, 2 and 5 rows of 50 ms.

    python examples/bayesian_filter_example.py [steps]
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
    for window in (1, 2, 5):
        dec = PCs.fit_bayesian_decoder(tuning="groundtruth", window=window)
        filt = dec.with_continuity()                                     # sigma: speed_mean x window x dt, at least half a bin
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e_dec = float(dec.error().mean())
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        e_filt = float(filt.error().mean())
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(f"  {label}, windows of {window} rows ({1e3 * window * PCs.Agent.dt:.0f} ms), {dec.n_bins} bins, step of {filt.radius} bins "
              f"(sigma {100 * filt.sigma:.1f} cm): memoryless {100 * e_dec:.1f} cm in {1e3 * (t1 - t0):.1f} ms, filtered {100 * e_filt:.1f} cm "
              f"in {1e3 * (t2 - t1):.1f} ms")


# ---- one agent ------------------------------------------------------------------------------------------------------
Env = riab.Environment({"dx": 0.05})
Ag = riab.Agent(Env, {"dt": 0.05})
PCs = riab.PlaceCells(Ag, CELLS)
Ag.simulate(steps)
print(f"one agent, {PCs.n} place cells of {CELLS['max_fr']:.0f} Hz, {steps} rows of 50 ms, ground-truth tuning curves:")
compare(PCs, "1 agent")
out = PCs.fit_bayesian_decoder(tuning="groundtruth").with_continuity().decode_all_tensor()
print(f"  predictive log likelihood log p(k_t | k_<t), mean over the windows: {float(out[:, 4, 0].mean()):.3f}")

# ---- 1024 agents --------------------------------------------------------------------------------------------------------
steps_b = max(100, steps // 20)
Ag = riab.Agent(Env, {"n_agents": 1024, "dt": 0.05})
PCs = riab.PlaceCells(Ag, CELLS)
Ag.simulate(steps_b)
torch.cuda.synchronize()
print(f"1024 agents, {steps_b} rows each:")
compare(PCs, "1024 agents")
