"""contribs.PlaneWaveNeurons on the device: first the reference's own example (contribs/PlaneWaveNeurons.py, __main__) in
numbers — the ground-truth rate map of ten plane waves at wavescale 0.01, minimum and maximum printed where the reference draws
a figure — then the batched form: 1024 agents whose plane waves are the Fourier-feature basis of a FeedForwardLayer.

    python examples/plane_wave_example.py [steps]
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ratinabox_amd as riab  # noqa: E402
from ratinabox_amd.contribs.PlaneWaveNeurons import PlaneWaveNeurons  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
np.random.seed(0)

# ---- the reference's example ------------------------------------------------------------------------------------------
Env = riab.Environment()
Ag = riab.Agent(Env)
PWNs = PlaneWaveNeurons(Ag, params={"wavescale": 0.01})
maps, zero_bins = PWNs.get_rate_map(method="groundtruth")          # what plot_rate_map draws
print(f"{PWNs.n} plane waves, wavelengths {PWNs.wavescales.min():.4f}..{PWNs.wavescales.max():.4f} m: rate maps "
      f"{maps.shape[1]} x {maps.shape[2]}, rates {maps.min():.4f}..{maps.max():.4f} (min_fr {PWNs.min_fr}, max_fr {PWNs.max_fr})")
assert maps.shape[0] == PWNs.n and not zero_bins.any() and maps.min() >= 0 and maps.max() <= 1
# the three arrays are the user's to overwrite: one wave along x with a 25 cm wavelength and its crest at x = 0.5
PWNs.w[0], PWNs.wavescales[0], PWNs.phase_offsets[0] = [1.0, 0.0], 0.25, [0.5, 0.0]
line = PWNs.get_state(evaluate_at=None, pos=np.array([[0.5, 0.3], [0.625, 0.3], [0.75, 0.9]]))[0]
print(f"cell 0 after the edit: crest {line[0]:.4f}, trough {line[1]:.4f}, next crest {line[2]:.4f}")
assert abs(line[0] - 1) < 1e-4 and abs(line[1]) < 1e-4 and abs(line[2] - 1) < 1e-4

# ---- the batched form: plane waves under a FeedForwardLayer --------------------------------------------------------------
B = 1024
Ag = riab.Agent(riab.Environment(), {"n_agents": B, "dt": 0.01, "save_history": False})
basis = PlaneWaveNeurons(Ag, {"n": 256, "wavescale": 0.2, "save_history": False})
layer = riab.FeedForwardLayer(Ag, {"n": 32, "input_layers": [basis], "activation_function": {"activation": "tanh"},
                                   "save_history": False})
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    Ag.update()
    basis.update()
    layer.update()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
want = np.tanh(layer.inputs[basis.name]["w"] @ basis.firingrate)
err = np.abs(layer.firingrate - want).max()
print(f"{steps} steps x {B} agents x {basis.n} plane waves -> {layer.n} units in {dt:.2f} s ({dt / steps * 1e6:.0f} us per step); "
      f"largest |layer - tanh(W @ rates)| {err:.2e}")
assert layer.firingrate.shape == (32, B) and err < 1e-4
