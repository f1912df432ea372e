"""`PhasePrecessingPlaceCells` — place cells whose rate is modulated by the theta phase, on the device
(reference ratinabox/contribs/PhasePrecessingPlaceCells.py; George et al. 2023, "Rapid learning of predictive maps with
STDP and theta phase precession").

    rate = PlaceCells rate (scaled to [min_fr, max_fr]) * von Mises(theta phase - preferred phase) * 2 pi

The preferred phase of a cell falls from late to early in the theta cycle as the agent crosses the field: it depends on
the position along the DIRECTION OF MOTION, `Agent.velocity` — the velocity of the motion model, which differs from the
measured velocity the history keeps whenever a wall intervenes — and on the clock `Agent.t`.  Both live on the host /
in the float64 agent state only, the situation `VelocityCells` is in: `update()`, `get_state()` and step plans read the
velocity rows of the state (csrc/riab_rate_cells.h: ThetaPlaceCell, its own kernel after the step kernel in a plan), and
`Agent.simulate()` advances such a population through a native step plan, whose float64 clock is advanced by the same
`t += dt` as `Agent.t`.  Away from the agent (`evaluate_at="all"` / `pos=`) there is no velocity: the plain place-cell
rate is returned and a notice printed, as in the reference.

Parameters besides those of PlaceCells: `theta_freq` (Hz, default 10), `kappa` (von Mises concentration, default 1),
`precess_fraction` (fraction of the theta cycle the preferred phase sweeps across the field, default 0.5).  The field
boundary is `widths` (twice that for gaussian cells), so `one_hot` cells are refused.  Wall geometry: euclidean (solid or
periodic rooms); line_of_sight and geodesic raise."""
import copy

import numpy as np

from .. import _lib
from ..Neurons import LOG2E, Neurons, PlaceCells

_L = _lib


class PhasePrecessingPlaceCells(PlaceCells):
    default_params = {
        "n": 10,
        "min_fr": 0,
        "max_fr": 1,
        "theta_freq": 10,
        "kappa": 1,
        "precess_fraction": 0.5,
        "description": "gaussian_threshold",
        "name": "PhasePrecessingPlaceCell",
    }

    _stream_kind = None        # reads the float64 velocity state and the clock, not the history rows
    _state_op = None           # (its own kernel entry: riab_phase_precessing_place_cells)
    _reads_agent_state = True  # Agent.simulate() runs such populations through a native step plan
    _watch_arrays = ("place_cell_centres", "place_cell_widths")
    _watch_scalars = ("description", "wall_geometry", "widths", "theta_freq", "kappa", "precess_fraction")

    def __init__(self, Agent, params={}):
        self.Agent = Agent
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        self._modulated = False
        super().__init__(Agent, self.params)
        self.sigma = np.sqrt(1 / self.kappa)
        assert self.description in ["gaussian", "diff_of_gaussians", "gaussian_threshold", "top_hat"]

    # ---- the reference's surface ---------------------------------------------------------------------------------
    def theta_modulation_factors(self):
        """How much each cell's rate is modulated at the agent's position, velocity and clock: `(n,)`, or `(n, B)` with
        several agents (host float64, the reference's formula per agent)."""
        pos = np.asarray(self.Agent.pos, dtype=np.float64).reshape(-1, 2)
        vel = np.asarray(self.Agent.velocity, dtype=np.float64).reshape(-1, 2)
        direction = vel / (1e-8 + np.linalg.norm(vel, axis=-1, keepdims=True))
        theta_phase = self.theta_freq * (self.Agent.t % (1 / self.theta_freq)) * 2 * np.pi
        sigma = np.asarray(self.place_cell_widths, dtype=np.float64) * np.ones(int(self.n))
        if self.description == "gaussian":
            sigma = sigma * 2  # gaussian place cell boundary taken at 2 sigma
        centres = np.asarray(self.place_cell_centres, dtype=np.float64).reshape(-1, 2)
        to_cells = pos[None, :, :] - centres[:, None, :]
        sigmas_to_midline = (to_cells * direction[None, :, :]).sum(-1) / sigma[:, None]
        phase_diff = np.pi - sigmas_to_midline * self.precess_fraction * np.pi - theta_phase
        kappa = float(self.kappa)
        out = np.exp(kappa * (np.cos(phase_diff) - 1)) * (np.exp(kappa) / np.i0(kappa))
        return out[:, 0] if self._B == 1 else out

    def update(self, **kwargs):
        self._modulated = True
        try:
            super().update(**kwargs)
        finally:
            self._modulated = False

    def get_state_tensor(self, evaluate_at="agent", **kwargs):
        if evaluate_at == "agent":
            self._modulated = True
            try:
                return Neurons.get_state_tensor(self, "agent")
            finally:
                self._modulated = False
        print("Since you are not evaluating the firing rate using the current state of the agent no phase precession "
              "modulation has been applied (since this requires a velocity). Ignore this if you are plotting receptive field.")
        return Neurons.get_state_tensor(self, evaluate_at, **kwargs)

    def get_state(self, evaluate_at="agent", **kwargs):
        t = self.get_state_tensor(evaluate_at, **kwargs)
        return t[:, :self._last_P].cpu().numpy().astype(np.float64)

    def _rates_from_trajectory(self, traj, out, t0, tc, step0, dt, stream):
        raise NotImplementedError("PhasePrecessingPlaceCells read Agent.velocity and Agent.t, which the history rows do "
                                  "not keep (Agent.simulate() advances them through a step plan instead)")

    # ---- device tables and the launch ------------------------------------------------------------------------------
    def _theta_table(self):
        n = int(self.n)
        centres = np.asarray(self.place_cell_centres, dtype=np.float64).reshape(-1, 2)
        widths = np.asarray(self.place_cell_widths, dtype=np.float64)
        if widths.shape != (n,):
            widths = widths * np.ones(n)
        desc, pf = self.description, float(self.precess_fraction)

        def build():
            import torch
            tab = np.empty((n, 4), dtype=np.float64)
            tab[:, 0], tab[:, 1] = centres[:, 0], centres[:, 1]
            tab[:, 2] = -LOG2E / (2 * widths ** 2)
            tab[:, 3] = pf / (2 * widths * (2 if desc == "gaussian" else 1))
            return torch.from_numpy(tab.astype(np.float32)).to(self._device)

        hit = self._table_cache.get("theta")   # (keyed on content, beside the plain PlaceCells table of `_tables`)
        key = (centres.tobytes(), widths.tobytes(), desc, pf)
        if hit is None or hit[0] != key:
            hit = self._table_cache["theta"] = (key, build())
        return hit[1]

    def _call(self, io, stream):
        if io is not None and not self._modulated:
            return super()._call(io, stream)   # away from the agent: the plain place-cell rate
        if self.description not in _L.PC_DESCRIPTIONS or self.description == "one_hot":
            raise ValueError(f"PhasePrecessingPlaceCells: description {self.description!r} has no field width")
        geom = self.wall_geometry
        if geom == "geodesic" and len(self.Agent.Environment.walls) <= 4:
            geom = "euclidean"  # Environment.py:741-742
        if geom != "euclidean":
            raise NotImplementedError(f"PhasePrecessingPlaceCells on the device take the euclidean wall geometry, not {geom!r}")
        tab = self._theta_table()
        thw = float(np.asarray(self.widths, dtype=float).reshape(-1)[0])
        theta_freq, kappa = float(self.theta_freq), float(self.kappa)
        if io is None:  # descriptor for a step plan (whose clock gives the phase of each step)
            return dict(kind=_L.POP_KINDS["theta_place"], table=tab, description=_L.PC_DESCRIPTIONS[self.description],
                        geometry=_L.GEOMETRIES[geom], top_hat_width=thw, theta_freq=theta_freq, kappa=kappa)
        env, _w = self.Agent.Environment.device_tables(self._device)
        st = self.Agent._state
        theta_rev = theta_freq * (float(self.Agent.t) % (1 / theta_freq))
        rc = _L.lib.riab_phase_precessing_place_cells(env, io, _L.ptr(tab), int(self.n), _L.PC_DESCRIPTIONS[self.description],
                                                      _L.GEOMETRIES[geom], thw, kappa, theta_rev, _L.ptr(st[_L.S_VEL_X]),
                                                      _L.ptr(st[_L.S_VEL_Y]), stream)
        _L.check(rc, "riab_phase_precessing_place_cells")
