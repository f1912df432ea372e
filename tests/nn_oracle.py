"""Float64 NumPy forward of a lowered multi-layer perceptron, with the error bound of an fp32 evaluation.

    h_0 = inputs (n_in, P);   h_l = act_l(W_l @ h_{l-1} + b_l)

The bound propagates the coefficients of test_randomised_feedforward_shapes_vs_oracle (tests/test_gpu_parity.py: an fp32
contraction is within 2e-6 * (|W| @ |x| + |b|) of the float64 product, and an activated value within 1e-6 of its own size)
through the layers: the error that enters a layer is carried through |W| and the activation's Lipschitz constant,

    tol_l = lip_l * (2e-6 * (|W_l| @ |h_{l-1}| + |b_l|) + |W_l| @ tol_{l-1}) + 1e-6 * |h_l|,      tol_0 given (default 0).
"""
import numpy as np

LIP = {"linear": 1.0, "relu": 1.0, "tanh": 1.0, "softplus": 1.0, "sigmoid": 0.25}


def activate(name, x):
    if name == "linear":
        return x
    if name == "relu":
        return np.maximum(x, 0.0)
    if name == "tanh":
        return np.tanh(x)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if name == "softplus":
        return np.logaddexp(0.0, x)
    raise ValueError(name)


def forward(layers, h0, tol0=0.0):
    """layers: [(W (n_out, n_in), b (n_out,) or None, activation name)]; h0 (n_in, P).  Returns (h_L, tol_L), both
    float64 (n_out, P)."""
    h = np.asarray(h0, dtype=np.float64)
    if h.ndim == 1:
        h = h[:, None]
    tol = np.zeros_like(h) + tol0
    for W, b, act in layers:
        W = np.asarray(W, dtype=np.float64)
        bb = np.zeros(W.shape[0]) if b is None else np.asarray(b, dtype=np.float64)
        x = W @ h + bb[:, None]
        cond = np.abs(W) @ np.abs(h) + np.abs(bb)[:, None]
        h_new = activate(act, x)
        tol = LIP[act] * (2e-6 * cond + np.abs(W) @ tol) + 1e-6 * np.abs(h_new)
        h = h_new
    return h, tol
