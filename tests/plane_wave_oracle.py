"""Float64 restatement of the reference's contribs/PlaneWaveNeurons.py: one cosine per cell,

    phi_i  = (2 pi / wavescales_i) * ((phase_offsets_i - p) . w_i)
    rate_i = (0.5 * (cos(phi_i) + 1)) * (max_fr - min_fr) + min_fr

tests/test_plane_wave_cpu.py pins it to the reference's record (tests/golden/plane_wave_*.npz); the device tests compare
against it where the reference has no record (positions the device itself produced).

`table` is the device's parameterisation of the same thing — the phase in REVOLUTIONS, a - (x bx + y by), one term of the
GridCells table — in float64; rounded to float32 it is what the kernel is handed.  `tolerance` is the allowance of the
device tests: the fp32 phase bound derived in DESIGN.md 5 turned into a rate error, plus the hardware cosine's."""
import numpy as np


def rates(pos, phase_offsets, w, wavescales, min_fr=0.0, max_fr=1.0):
    """PlaneWaveNeurons.get_state(evaluate_at=None, pos=pos) -> (n, P), float64."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    o = np.asarray(phase_offsets, dtype=np.float64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64).reshape(-1, 2)
    lam = np.asarray(wavescales, dtype=np.float64).reshape(-1)
    vecs = o[:, None, :] - pos[None, :, :]
    phi = (2 * np.pi / lam)[:, None] * (vecs * w[:, None, :]).sum(axis=-1)
    return (0.5 * (np.cos(phi) + 1)) * (float(max_fr) - float(min_fr)) + float(min_fr)


def table(phase_offsets, w, wavescales):
    """(n, 3) float64 = (a, bx, by): a = frac((o . w) / lambda), (bx, by) = w / lambda."""
    o = np.asarray(phase_offsets, dtype=np.float64).reshape(-1, 2)
    w = np.asarray(w, dtype=np.float64).reshape(-1, 2)
    lam = np.asarray(wavescales, dtype=np.float64).reshape(-1)
    a = (o[:, 0] * w[:, 0] + o[:, 1] * w[:, 1]) / lam
    return np.stack((a - np.floor(a), w[:, 0] / lam, w[:, 1] / lam), axis=-1)


def table32(phase_offsets, w, wavescales):
    """... rounded to float32 once; a fraction that rounds up to 1.0f is the phase 0."""
    t = table(phase_offsets, w, wavescales).astype(np.float32)
    t[t[:, 0] >= 1.0, 0] = 0.0
    return t


def phase_magnitude(tab, pos):
    """M_i = max_p (|x bx_i| + |y by_i|) over the given positions -> (n,)."""
    tab = np.asarray(tab, dtype=np.float64)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 2)
    return (np.abs(pos[None, :, 0] * tab[:, None, 1]) + np.abs(pos[None, :, 1] * tab[:, None, 2])).max(axis=1)


def tolerance(tab, pos, fr_range, e_cos):
    """Per-cell allowance (n,) of a device rate: (max_fr - min_fr) * (pi * 2 * (4 M_i + 3) * 2^-24 + e_cos).
    |d rev| <= (4 M + 3) 2^-24 (the fp32 roundings of a, b, the position and the two arithmetic steps); the rate's slope in
    the phase is at most pi per revolution; 2 is margin; e_cos the absolute allowance for the hardware cosine."""
    return float(fr_range) * (np.pi * 2 * (4 * phase_magnitude(tab, pos) + 3) * 2.0 ** -24 + float(e_cos))
