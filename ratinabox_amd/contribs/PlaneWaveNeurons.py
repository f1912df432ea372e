"""`PlaneWaveNeurons` — a Fourier-feature basis over position, on the device
(reference ratinabox/contribs/PlaneWaveNeurons.py).

    phi_i  = (2 pi / wavescales_i) * ((phase_offsets_i - pos) . w_i)
    rate_i = (cos(phi_i) + 1) / 2, scaled to [min_fr, max_fr]

`n` plane waves with random unit directions `w`, wavelengths `wavescales` (Rayleigh around `wavescale`) and offsets
`phase_offsets`; the three arrays are attributes a user may overwrite or edit in place, as the reference invites (the device
table is keyed on their content).  A pure function of position: `update()`, `get_state()`, step plans and every form of
`Agent.simulate()` — the row-following rate kernel included, a PlaneWaveNeurons population can lead it — go through one
functor (csrc/riab_rate_cells.h: PlaneWaveCell, one fraction and one `v_cos_f32` per rate), spikes, OU noise, histories, rate
maps and use as an input layer through the base class.

The phase is fp32 revolutions: its error grows with (room size) / wavelength, and a Rayleigh draw can make a wavelength
arbitrarily small."""
import copy

import numpy as np
import torch

from .. import _lib
from ..Neurons import Neurons

_L = _lib


class PlaneWaveNeurons(Neurons):
    default_params = {
        "n": 10,
        "wavescale": 0.2,  # metres
        "min_fr": 0,
        "max_fr": 1,
        "name": "PlaneWaveNeurons",
    }

    _stream_kind = "plane_wave"

    def __init__(self, Agent, params={}):
        self.Agent = Agent
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        super().__init__(Agent, self.params)
        assert self.Agent.Environment.dimensionality == "2D", "PlaneWaveNeurons only available in 2D"
        if self.Agent.Environment.boundary_conditions == "periodic":
            print("PlaneWaveNeurons not optimized for periodic environments, you may notice some discontinuities")
        # (the reference's draw order)
        self.phase_offsets = np.random.uniform(0, self.wavescale, size=(self.n, 2))
        self.w = np.random.normal(size=(self.n, 2))
        self.w = self.w / np.expand_dims(np.linalg.norm(self.w, axis=1), axis=1)
        self.wavescales = np.random.rayleigh(scale=self.wavescale, size=self.n)

    def _call(self, io, stream):
        n = int(self.n)
        ph = np.asarray(self.phase_offsets, dtype=np.float64).reshape(n, 2)
        w = np.asarray(self.w, dtype=np.float64).reshape(n, 2)
        ws = np.asarray(self.wavescales, dtype=np.float64).reshape(n)

        def build():
            # phi / 2pi = ((offset - p) . w) / lambda = a - (x bx + y by), in revolutions like a term of GridCells' table
            tab = np.empty((n, 3), dtype=np.float64)
            a = (ph[:, 0] * w[:, 0] + ph[:, 1] * w[:, 1]) / ws
            tab[:, 0] = a - np.floor(a)
            tab[:, 1] = w[:, 0] / ws
            tab[:, 2] = w[:, 1] / ws
            tab32 = tab.astype(np.float32)
            tab32[:, 0][tab32[:, 0] >= 1.0] = 0.0   # (a fraction that rounds up to 1.0f: the same phase)
            return torch.from_numpy(tab32).to(self._device)

        tab = self._tables((ph, w, ws), build)
        if io is None:
            return dict(kind=_L.POP_KINDS[self._stream_kind], table=tab)
        _L.check(_L.lib.riab_plane_wave_neurons(io, _L.ptr(tab), n, stream), "riab_plane_wave_neurons")

    def _state_op(self, d):
        from .. import ops  # noqa: F401  (registers torch.ops.riab.*)
        return torch.ops.riab.plane_wave_neurons(d[0:2], self._call(None, None)["table"], float(self.min_fr), float(self.max_fr))
