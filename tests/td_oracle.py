"""A NumPy restatement of the TD(lambda) rule of contribs.ValueNeuron / SuccessorFeatures (reference
contribs/ValueNeuron.py:59-113), batched: test infrastructure only (the frozen oracle/ package predates the learners).

In float64 and with one lane it reproduces the reference bit for bit (tests/test_td_cpu.py pins it on the fixtures
tests/golden/td_*.npz); with B lanes the weight change is the mean over the lanes of the per-lane outer products, the
batched semantics of the product.  Run in `dtype=np.float32` it measures what plain fp32 arithmetic costs on a given
run: the GPU tests derive their allowance from that figure (`check`).  `one_step` is the same rule for ONE step on arrays
handed in as the kernels get them (V and act' given): tests/test_gpu_td_shapes.py drives the operators against it."""
import numpy as np

FACTOR = 4.0     # kernel allowance over the fp32 NumPy run


def check(label, got, ref, err32, scale, keys):
    """|got - ref| <= FACTOR * (fp32 NumPy error) * scale per quantity; prints the measured ratio first."""
    lines, bad = [], []
    for k in keys:
        e = float(np.abs(np.asarray(got[k], float) - ref[k]).max()) / scale[k]
        lines.append(f"{k}: kernel {e:.2e}, fp32 NumPy {err32[k]:.2e}, ratio {e / max(err32[k], 1e-300):.2f}")
        if not e <= FACTOR * err32[k]:
            bad.append(k)
    print(f"[{label}] " + "; ".join(lines))
    assert not bad, (label, bad, lines)


def trace_step(f, dt, tau_e, phi, e):
    """e <- dt * phi + (1 - dt / tau_e) * e in the arithmetic `f` (tau_e == 0: e <- phi)."""
    if tau_e == 0:
        return phi.copy()
    return dt * phi + (f(1) - dt / tau_e) * e


def weight_step(f, dt, eta, L2, B, w, g, e):
    """W <- W + dt * eta * (g e^T) / B - eta * dt * L2 * W in the arithmetic `f`; g (n, B), e (n_in, B), w (n, n_in)."""
    G = np.matmul(g, e.T) / f(B)
    dw = dt * eta * G - eta * dt * L2 * w
    return (w + dw).astype(f)


def one_step(ws, traces, phis, v, v_last, prime, reward, dt, tau, tau_e, eta, L2, dtype=np.float64):
    """ONE step of the rule on given arrays, the way the kernels are handed them (V and act' are inputs, not computed):
    td_forward_tail (dV/dt, the traces) followed by td_update (TD error, weights).  Every array holds the B real lanes
    only: ws[l] (n, n_in_l), traces[l] / phis[l] (n_in_l, B), v / v_last / prime (n, B), reward a scalar, (n,), (B,) or
    (n, B).  Returns dict(dvdt, td, traces, ws) in `dtype`; the inputs are left as they are."""
    f = dtype
    dt, tau, tau_e, eta, L2 = f(dt), f(tau), f(tau_e), f(eta), f(L2)
    v, v_last, prime = (np.asarray(a, dtype=f) for a in (v, v_last, prime))
    n, B = v.shape
    r = np.asarray(reward, dtype=f)
    if r.ndim == 1 and r.shape[0] == n:
        r = r[:, None]
    dvdt = (v - v_last) / dt
    new_traces = [trace_step(f, dt, tau_e, np.asarray(p, dtype=f), np.asarray(e, dtype=f)) for p, e in zip(phis, traces)]
    td = (r + dvdt - v / tau) * np.ones((n, B), dtype=f)
    g = td * prime
    new_ws = [weight_step(f, dt, eta, L2, B, np.asarray(w, dtype=f), g, e) for w, e in zip(ws, new_traces)]
    return {"dvdt": dvdt, "td": td, "traces": new_traces, "ws": new_ws}


class TDOracle:
    def __init__(self, ws, dt, tau, tau_e, eta, L2, activation="relu", gain=1.0, threshold=0.0, B=1, dtype=np.float64):
        f = self.f = dtype
        self.ws = [np.array(w, dtype=f) for w in ws]           # (n, n_in_l) each
        self.n, self.B = self.ws[0].shape[0], int(B)
        self.dt, self.tau, self.tau_e, self.eta, self.L2 = f(dt), f(tau), f(tau_e), f(eta), f(L2)
        self.activation, self.gain, self.threshold = activation, f(gain), f(threshold)
        self.traces = [np.zeros((w.shape[1], self.B), dtype=f) for w in self.ws]
        self.V = np.zeros((self.n, self.B), dtype=f)
        self.dVdt = np.zeros((self.n, self.B), dtype=f)
        self.td = np.zeros((self.n, self.B), dtype=f)
        self.prime = np.zeros((self.n, self.B), dtype=f)

    def _lanes(self, x, rows):
        x = np.asarray(x, dtype=self.f)
        return x.reshape(rows, -1) if x.ndim < 2 else x

    def update(self, phis):
        """phis: one array (n_in_l,) or (n_in_l, B) per input layer."""
        f = self.f
        phis = [self._lanes(p, w.shape[1]) for p, w in zip(phis, self.ws)]
        x = np.zeros((self.n, self.B), dtype=f)
        for w, p in zip(self.ws, phis):
            # (one lane: the reference's matrix-vector product, so that the same BLAS routine rounds the same way)
            x += np.matmul(w, p[:, 0])[:, None] if self.B == 1 else np.matmul(w, p)
        if self.activation == "relu":
            V = self.gain * np.maximum(0, x - self.threshold)
            self.prime = (self.gain * ((x - self.threshold) > 0)).astype(f)
        else:
            assert self.activation == "linear"
            V = x
            self.prime = np.ones_like(x)
        self.pre = x
        self.dVdt = (V - self.V) / self.dt
        self.V = V.astype(f)
        for l, p in enumerate(phis):
            self.traces[l] = trace_step(f, self.dt, self.tau_e, p, self.traces[l])

    def update_weights(self, reward):
        """reward: scalar, (n,) (one per neuron), (B,) (one per lane; for n == B read as one per neuron) or (n, B)."""
        r = np.asarray(reward, dtype=self.f)
        if r.ndim == 1 and r.shape[0] == self.n:
            r = r[:, None]
        self.td = (r + self.dVdt - self.V / self.tau) * np.ones((self.n, self.B), dtype=self.f)
        g = self.td * self.prime
        for l, w in enumerate(self.ws):
            self.ws[l] = weight_step(self.f, self.dt, self.eta, self.L2, self.B, w, g, self.traces[l])

    def reset(self, mask=None):
        m = np.ones(self.B, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        for e in self.traces:
            e[:, m] = 0
        for a in (self.V, self.dVdt, self.td):
            a[:, m] = 0


def replay(g, prefix="", activation="relu", threshold=0.0, dtype=np.float64):
    """Run the oracle over a fixture's recorded input rates and rewards (one lane).  Returns dict of per-step V, prime,
    td, trace and w after T/2 and T steps, as float64."""
    T = len(g["phi"])
    o = TDOracle([g["w0"]], g["dt"], g["tau"], g["tau_e"], g["eta"], g["L2"], activation, 1.0, threshold, 1, dtype)
    out = {k: [] for k in ("V", "prime", "td", "trace")}
    for t in range(T):
        o.update([g["phi"][t]])
        o.update_weights(g["r"][t])
        out["V"].append(o.V[:, 0])
        out["prime"].append(o.prime[:, 0])
        out["td"].append(o.td[:, 0])
        out["trace"].append(o.traces[0][:, 0])
        if t + 1 == T // 2:
            out["w_half"] = o.ws[0].astype(np.float64)
    out["w_T"] = o.ws[0].astype(np.float64)
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


def reference_of(g, prefix):
    """The reference's record of a fixture run: td_value.npz keeps two runs (`relu_`, `linear_`), td_successor.npz one."""
    keys = ("V", "prime", "td", "w_half", "w_T")
    ref = {k: g[prefix + k] for k in keys}
    ref["trace"] = g["trace"]
    return ref


def fp32_allowance(g, prefix, activation, threshold):
    """Worst error of the oracle run in np.float32 against the reference, per quantity, normalised by the quantity's
    largest magnitude in the run; and those magnitudes.  The kernels are allowed 4 x this figure: their summation order
    (MFMA k-chains, split-K partial sums) differs from NumPy's, so equality with the fp32 NumPy run is not expected."""
    ref = reference_of(g, prefix)
    low = replay(g, prefix, activation, threshold, np.float32)
    scale = {k: float(np.abs(ref[k]).max()) for k in ("V", "td", "trace", "w_T")}
    scale["w_half"] = scale["w_T"]
    err = {k: float(np.abs(low[k] - ref[k]).max()) / scale[k] for k in ("V", "td", "trace", "w_half", "w_T")}
    return err, scale
