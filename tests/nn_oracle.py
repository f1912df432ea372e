"""Float64 NumPy forward of a lowered multi-layer perceptron, with the error bound of an fp32 evaluation.

    h_0 = inputs (n_in, P);   h_l = act_l(W_l @ h_{l-1} + b_l)

The bound propagates the coefficients of test_randomised_feedforward_shapes_vs_oracle (tests/test_gpu_parity.py: an fp32
contraction is within 2e-6 * (|W| @ |x| + |b|) of the float64 product, and an activated value within 1e-6 of its own size)
through the layers: the error that enters a layer is carried through |W| and the activation's Lipschitz constant,

    tol_l = lip_l * (2e-6 * (|W_l| @ |h_{l-1}| + |b_l|) + |W_l| @ tol_{l-1}) + 1e-6 * |h_l|,      tol_0 given (default 0).

An activation is a name (the torch leaves' defaults) or the kernel's own description (code, p0, p1, p2, p3): RIAB_ACT_* and
the four parameters of csrc/riab_act.h.  Their Lipschitz constants, from the formulas there (z = x - p1):

    linear    x                                       1        (the parameters are ignored)
    sigmoid   (p0 - p1) s(p3 (x - p2)) + p1           |p0 - p1| |p3| / 4      (s' = s (1 - s) <= 1/4, at x = p2)
    relu      p0 max(0, z)                            |p0|     (slope p0 or 0)
    tanh      p0 tanh(z)                              |p0|     (1 - tanh^2 <= 1, at z = 0)
    retanh    p0 max(0, tanh(z))                      |p0|     (tanh's slope where z > 0, 0 elsewhere; the supremum at z -> 0+)
    softplus  p0 log(1 + exp(z))                      |p0|     (slope p0 s(z) < p0, the supremum at z -> infinity; the kernel's
                                                               switch to p0 z above z = 20 has slope p0 as well)

tests/test_nn_cpu.py checks each against float64 finite differences.  The 2e-6 and 1e-6 coefficients are the same for every
parameter set.
"""
import numpy as np

LIP = {"linear": 1.0, "relu": 1.0, "tanh": 1.0, "softplus": 1.0, "sigmoid": 0.25}
LINEAR, SIGMOID, RELU, TANH, RETANH, SOFTPLUS = range(6)     # RIAB_ACT_* (include/riab_hip.h; SOFTPLUS is RIAB_ACT_SOFTMAX)


def lipschitz(act):
    """the constant of a name or of (code, p0, p1, p2, p3): the table of the module's docstring"""
    if isinstance(act, str):
        return LIP[act]
    code, p0, p1, _p2, p3 = act
    if code == LINEAR:
        return 1.0
    if code == SIGMOID:
        return abs(p0 - p1) * abs(p3) / 4.0
    if code in (RELU, TANH, RETANH, SOFTPLUS):
        return abs(p0)
    raise ValueError(act)


def activate(name, x):
    if not isinstance(name, str):
        code, p0, p1, p2, p3 = name
        if code == LINEAR:
            return x
        if code == SIGMOID:
            return (p0 - p1) / (1.0 + np.exp(-p3 * (x - p2))) + p1
        if code == RELU:
            return p0 * np.maximum(x - p1, 0.0)
        if code == TANH:
            return p0 * np.tanh(x - p1)
        if code == RETANH:
            return p0 * np.maximum(np.tanh(x - p1), 0.0)
        if code == SOFTPLUS:
            return p0 * np.logaddexp(0.0, x - p1)
        raise ValueError(name)
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
    """layers: [(W (n_out, n_in), b (n_out,) or None, activation name or (code, p0, p1, p2, p3))]; h0 (n_in, P).  Returns (h_L, tol_L), both
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
        tol = lipschitz(act) * (2e-6 * cond + np.abs(W) @ tol) + 1e-6 * np.abs(h_new)
        h = h_new
    return h, tol
