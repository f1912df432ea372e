"""Float64 restatement of the reference's contribs/PhasePrecessingPlaceCells.py (George et al. 2023): place cells whose
rate is multiplied by a von Mises of the theta phase, the preferred phase precessing with the position along the
direction of motion.  tests/test_theta_cpu.py pins it to the reference's record (tests/golden/theta_*.npz).

    base  = PlaceCells.get_state(pos)                    # already scaled to [min_fr, max_fr]
    dir   = velocity / (1e-8 + |velocity|)               # Agent.velocity: the motion model's, not the measured one
    sig_b = widths * (2 if description == "gaussian" else 1)
    s     = ((pos - centre) . dir) / sig_b               # plain subtraction, no periodic wrap
    theta = theta_freq * (t % (1 / theta_freq))          # revolutions
    D/2pi = 0.5 - s * precess_fraction / 2 - theta
    rate  = base * exp(kappa (cos D - 1)) * exp(kappa) / I0(kappa)

`dtype=np.float32` runs the same text in single precision: what plain fp32 arithmetic costs on the same inputs, the
yardstick the device kernel's allowance is derived from (tests/test_gpu_theta.py).  Two numbers reach the kernel by value
— theta of the row and exp(kappa) / I0(kappa) — worked out on the host in float64 and rounded once; the float32 run takes
them the same way."""
import numpy as np

DESCRIPTIONS = ("gaussian", "gaussian_threshold", "diff_of_gaussians", "top_hat")
RTOL = 1e-5   # the project's bound on device firing rates against the reference


def theta_rev(t, theta_freq):
    """Theta phase in revolutions at time t (float64, as Agent.t is)."""
    return float(theta_freq) * (float(t) % (1 / float(theta_freq)))


def von_mises_peak(kappa):
    """exp(kappa) / I0(kappa): the peak of the normalised von Mises times 2 pi."""
    return float(np.exp(float(kappa)) / np.i0(float(kappa)))


def place_rates(pos, centres, widths, description, min_fr, max_fr, periodic=False, extent=(1.0, 1.0), widths_scalar=None,
                dtype=np.float64):
    """PlaceCells.get_state with the euclidean wall geometry (Neurons.py:936-981) -> (n, P)."""
    f = dtype
    pos = np.asarray(pos, dtype=f).reshape(-1, 2)
    centres = np.asarray(centres, dtype=f).reshape(-1, 2)
    w = (np.asarray(widths, dtype=f) * np.ones(len(centres), dtype=f))[:, None]
    vec = centres[:, None, :] - pos[None, :, :]
    if periodic:   # Environment.py:670-674: the short way round
        ext = np.asarray(extent, dtype=f)
        flip = np.abs(vec) > ext / f(2)
        vec = np.where(flip, -np.sign(vec) * (ext - np.abs(vec)), vec)
    dist = np.sqrt(vec[..., 0] ** 2 + vec[..., 1] ** 2)
    g = np.exp(-(dist ** 2) / (f(2) * w ** 2))
    if description == "gaussian":
        fr = g
    elif description == "gaussian_threshold":
        fr = np.maximum(g - np.exp(f(-0.5)), f(0)) / (f(1) - np.exp(f(-0.5)))
    elif description == "diff_of_gaussians":
        ratio = f(1.5)
        fr = g - (f(1) / ratio ** 2) * np.exp(-(dist ** 2) / (f(2) * (ratio * w) ** 2))
        fr = fr * (ratio ** 2 / (ratio ** 2 - f(1)))
    elif description == "top_hat":
        ws = w[0, 0] if widths_scalar is None else f(widths_scalar)   # Neurons.py:976 uses the scalar `widths`
        fr = (dist < ws).astype(f)
    else:
        raise ValueError(description)
    return (fr * (f(max_fr) - f(min_fr)) + f(min_fr)).astype(f)


def modulation(pos, vel, t, centres, widths, description, theta_freq, kappa, precess_fraction, dtype=np.float64):
    """theta_modulation_factors (contribs/PhasePrecessingPlaceCells.py:94-119) for P (pos, velocity) pairs that share
    the clock t -> (n, P); every pair is an agent of its own (its own |velocity|)."""
    f = dtype
    pos = np.asarray(pos, dtype=f).reshape(-1, 2)
    vel = np.asarray(vel, dtype=f).reshape(-1, 2)
    centres = np.asarray(centres, dtype=f).reshape(-1, 2)
    sig_b = np.asarray(widths, dtype=f) * np.ones(len(centres), dtype=f)
    if description == "gaussian":
        sig_b = sig_b * f(2)
    speed = np.sqrt(vel[:, 0] ** 2 + vel[:, 1] ** 2)
    d = vel / (f(1e-8) + speed)[:, None]
    vec = pos[None, :, :] - centres[:, None, :]
    s = (vec[..., 0] * d[None, :, 0] + vec[..., 1] * d[None, :, 1]) / sig_b[:, None]
    th = f(theta_rev(t, theta_freq))
    delta = f(2 * np.pi) * (f(0.5) - s * f(precess_fraction) / f(2) - th)
    k = f(kappa)
    return (np.exp(k * (np.cos(delta) - f(1))) * f(von_mises_peak(kappa))).astype(f)


def rates(pos, vel, t, centres, widths, description, theta_freq, kappa, precess_fraction, min_fr=0.0, max_fr=1.0,
          periodic=False, extent=(1.0, 1.0), widths_scalar=None, dtype=np.float64):
    """PhasePrecessingPlaceCells.get_state(evaluate_at="agent") -> (n, P): the modulation AFTER the affine map."""
    base = place_rates(pos, centres, widths, description, min_fr, max_fr, periodic, extent, widths_scalar, dtype)
    return base * modulation(pos, vel, t, centres, widths, description, theta_freq, kappa, precess_fraction, dtype)


def config_of(g, prefix=""):
    """Keyword arguments of `rates` stored in a theta_*.npz fixture."""
    p = prefix
    return dict(centres=g[p + "centres"], widths=g[p + "widths"], description=str(g[p + "description"]),
                theta_freq=float(g[p + "theta_freq"]), kappa=float(g[p + "kappa"]),
                precess_fraction=float(g[p + "precess_fraction"]), min_fr=float(g[p + "min_fr"]), max_fr=float(g[p + "max_fr"]),
                periodic=bool(g[p + "periodic"]), extent=(float(g[p + "extent"][0]), float(g[p + "extent"][1])),
                widths_scalar=float(g[p + "widths_scalar"]))


def ratio(got, ref, fr_range):
    """Worst |got - ref| / (1e-5 (|ref| + range)): the `c` of the project's criterion |err| <= c 1e-5 (|ref| + range)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref) / (RTOL * (np.abs(ref) + fr_range))).max())
