"""No-GPU checks of the Gaussian-process decoder's predictive variance: the float64 oracle (tests/gp_variance_oracle.py) and
GPDecoder.std_float64 / log_marginal_likelihood_ on host tensors against scikit-learn's recorded predict(return_std=True)
(tests/golden/gp_variance_reference.npz), the fp32 budget the GPU tolerance (tests/test_gpu_gp_variance.py) is derived from,
the ABI of riab_gp_predict_var with every refusal produced by validation alone, and the host logic that cuts the work into
workspaces."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import gp_decoder_oracle as gp
from tests import gp_variance_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "riab_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gp_variance_reference.npz")
CASES = {"a": (70, 57, 2), "b": (33, 5, 1), "c": (1, 3, 1)}
PRED_ALLOWANCE = 1e-12   # as tests/test_gp_decoder_cpu.py: two float64 solutions of a well-conditioned system, means of size 1


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def case(G, c):
    return G[f"X_{c}"], G[f"y_{c}"], G[f"Xq_{c}"], float(G[f"length_scale_{c}"]), float(G["alpha"])


def place_cell_problem():
    """The larger case of the fp32 budget: N = 512 samples of 20 Gaussian place cells at scattered positions, alpha = 0.01,
    the default length scale sqrt(n / 20) (cond(K + alpha I) = 1.9e4); queries inside the room, outside it, and at training
    points."""
    rng = np.random.RandomState(2)
    n, N = 20, 512
    centres = rng.rand(n, 2)
    pos, posq = rng.rand(N, 2), np.concatenate([rng.rand(48, 2), 1.0 + rng.rand(16, 2)])
    rates = lambda p: np.exp(-((p[:, None, :] - centres[None]) ** 2).sum(-1) / (2 * 0.2 ** 2)).astype(np.float32).astype(np.float64)
    X = rates(pos)
    return X, np.concatenate([rates(posq), X[:16]]), float(np.sqrt(n / 20)), 0.01


def test_golden_exercises_the_variance(G):
    """The fixture cannot be matched by a constant: sklearn's y_std^2 spans at least [0.05, 0.9] in every case."""
    assert float(G["alpha"]) == 0.01
    for c, (N, n, D) in CASES.items():
        X, y, Xq, ell, alpha = case(G, c)
        assert X.shape == (N, n) and y.shape == (N, D) and Xq.shape[1] == n and int(G[f"widths_{c}"].sum()) == n
        assert G[f"y_mean_{c}"].shape == (len(Xq), D) and G[f"y_std_{c}"].shape == (len(Xq),)
        var = G[f"y_std_{c}"] ** 2
        assert var.min() <= 0.05 and var.max() >= 0.9, (c, var.min(), var.max())
        assert np.array_equal(X.astype(np.float32).astype(np.float64), X)          # what a float32 history can hold
        assert np.array_equal(Xq.astype(np.float32).astype(np.float64), Xq)
    assert list(G["widths_a"]) == [7, 50]


@pytest.mark.parametrize("c", list(CASES))
def test_float64_parity_with_sklearn(G, c):
    """The oracle and GPDecoder (host tensors) against sklearn: y_std within 64 cond 2^-53 max|y_std|, the mean within 1e-12,
    the log marginal likelihood within 1e-9 relative.  Measured here: std 2.8e-15 (a), 2.3e-15 (b), 2.8e-16 (c) against
    allowances of 5.2e-14, 5.7e-12, 7.1e-15; lml 2e-16, 1.5e-15, 0 relative."""
    import torch
    from ratinabox_amd import GPDecoder
    X, y, Xq, ell, alpha = case(G, c)
    want_std, want_lml = G[f"y_std_{c}"], float(G[f"lml_{c}"])
    cond = np.linalg.cond(gp.gram(X, ell, alpha))
    allow = 64.0 * cond * 2.0 ** -53 * np.abs(want_std).max()
    dec = GPDecoder.from_samples(torch.from_numpy(X), torch.from_numpy(y), ell, alpha)
    got = dec.std_float64(torch.from_numpy(Xq))
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(Xq),)
    err_o = np.abs(orc.std(Xq, X, ell, alpha) - want_std).max()
    err_p = np.abs(got.numpy() - want_std).max()
    err_m = np.abs(dec.mean_float64(torch.from_numpy(Xq)).numpy() - G[f"y_mean_{c}"]).max()
    lml_o = orc.log_marginal_likelihood(X, y, ell, alpha)
    assert isinstance(dec.log_marginal_likelihood_, float)
    rel_o, rel_p = abs(lml_o - want_lml) / abs(want_lml), abs(dec.log_marginal_likelihood_ - want_lml) / abs(want_lml)
    print(f"{c}: y_std oracle {err_o:.3g}, std_float64 {err_p:.3g} (allowance {allow:.3g}, cond {cond:.3g}); mean {err_m:.3g}; "
          f"lml relative: oracle {rel_o:.3g}, from_samples {rel_p:.3g}")
    assert err_o <= allow and err_p <= allow and err_m <= PRED_ALLOWANCE
    assert rel_o <= 1e-9 and rel_p <= 1e-9
    # the fit keeps no factor and builds no variance table; a decoder constructed directly has no likelihood
    assert dec._linv_t is None and not any(isinstance(v, torch.Tensor) and v.dim() == 2 and v.shape[0] == v.shape[1] > 4
                                            for v in vars(dec).values())
    assert GPDecoder(dec.X_train_, dec.alpha_, ell, alpha).log_marginal_likelihood_ is None
    # a NaN query stays NaN through the clamp, the others are not affected
    Xn = Xq[:3].copy()
    Xn[1, 0] = np.nan
    s = dec.std_float64(torch.from_numpy(Xn)).numpy()
    assert np.isnan(s[1]) and np.abs(s[[0, 2]] - want_std[[0, 2]]).max() <= allow


def test_fp32_budget(G):
    """max |emulated fp32 var - float64 var| over the golden cases and the N = 512 place-cell case: the number the GPU
    tolerance is 8 times of.  Measured here: 1.57e-6 (a), 9.4e-7 (b), 1.2e-7 (c), 9.2e-7 (N = 512).  orc.FP32_VAR_ERROR is
    asserted to be that maximum rounded up, and to stay below 1e-3, a tenth of the smallest variance alpha / (1 + alpha) the
    model can express at alpha = 0.01 (it is 600 times below)."""
    worst = 0.0
    problems = [(c,) + case(G, c)[:1] + case(G, c)[2:] for c in CASES] + [("N = 512",) + place_cell_problem()]
    for name, X, Xq, ell, alpha in problems:
        v64 = orc.variance(Xq, X, ell, alpha)
        err = float(np.abs(orc.emulate_fp32(Xq, X, ell, alpha).astype(np.float64) - v64).max())
        print(f"{name}: fp32 emulation, max |var - float64 var| = {err:.3g} (var in [{v64.min():.3g}, {v64.max():.3g}])")
        worst = max(worst, err)
    print(f"worst {worst:.3g}; FP32_VAR_ERROR {orc.FP32_VAR_ERROR:.3g}; GPU tolerance {orc.GPU_VAR_TOLERANCE:.3g}")
    assert worst <= orc.FP32_VAR_ERROR <= 2.0 * worst, "FP32_VAR_ERROR is the measured maximum, rounded up"
    assert orc.FP32_VAR_ERROR <= 1e-3 and orc.MARGIN == 8.0 and orc.GPU_VAR_TOLERANCE == 8.0 * orc.FP32_VAR_ERROR


def test_variance_table_on_the_host(G):
    """GPDecoder._variance_table: L^-1 transposed, float32, exactly zero above the diagonal and in the padding, cached."""
    import torch
    from ratinabox_amd import GPDecoder
    for c, (N, n, D) in CASES.items():
        X, y, Xq, ell, alpha = case(G, c)
        dec = GPDecoder.from_samples(torch.from_numpy(X), torch.from_numpy(y), ell, alpha)
        t = dec._variance_table("cpu")
        Np = (N + 31) // 32 * 32
        assert t.dtype == torch.float32 and tuple(t.shape) == (Np, Np) and t.is_contiguous() and dec._variance_table("cpu") is t
        want = orc.linv_t_table(X, ell, alpha)
        got = t.numpy()
        assert not got[N:].any() and not got[:, N:].any() and not np.tril(got, -1).any()        # rows are j: j > i is below
        cond = np.linalg.cond(gp.gram(X, ell, alpha))
        assert np.abs(got - want).max() <= (2.0 ** -24 + 64.0 * cond * 2.0 ** -53) * np.abs(want).max()   # one float32 rounding
        assert (np.diag(got)[:N] > 0).all()


def test_symbol_declared_exported_prototyped_documented(L):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\briab_gp_predict_var\s*\(([^)]*)\)\s*;", src)
    assert m, "riab_gp_predict_var is not declared in riab_hip.h"
    assert len(m.group(1).split(",")) == 14 == len(L.PROTOTYPES["riab_gp_predict_var"][1]) and hasattr(L.lib, "riab_gp_predict_var")
    raw = open(HEADER).read()
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", raw).group(1)) == 11 == L.ABI_VERSION == L.lib.riab_abi_version()
    assert L.lib.riab_abi_sizeof(5) == C.sizeof(L.RiabFFInput)          # (the struct the entry point reuses is unchanged)
    assert "riab_gp_predict_var" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the header states the contract of linv_t, the rows that are never read and the workspace size
    doc = re.search(r"/\*(?:(?!\*/).)*?\*/\s*int riab_gp_predict_var", raw, flags=re.S).group(0)
    for phrase in ("zero above the diagonal", "NEVER READ", "m0 + 32 MT", "[T][Np][B]", "4 T Np B bytes", "finite"):
        assert phrase in doc, phrase
    import ratinabox_amd.ops  # noqa: F401
    import torch
    assert hasattr(torch.ops.riab, "gp_predict_var")


def test_argument_errors_before_launch(L):
    """Every refusal of riab_gp_predict_var is produced by validation alone: no device needed."""
    p, q = 4096, 4096 + 4

    def call(rates=p, wt=p, n_in=3, n_inputs=1, sq=p, alpha=p, D=2, n_train=40, inv=0.5, linv=p, T=1, B=8, ws=p, var=p, mean=p,
             null_inputs=False):
        arr = (L.RiabFFInput * 9)()
        for a in arr:
            a.rates, a.wt, a.n_in = rates, wt, n_in
        return L.lib.riab_gp_predict_var(None if null_inputs else arr, n_inputs, sq, alpha, D, n_train, inv, linv, T, B, ws, var,
                                         mean, None)
    assert call(T=0) == 0 and call(T=0, mean=None) == 0                           # nothing to do, nothing launched
    for null in ("rates", "wt", "sq", "alpha", "linv", "ws", "var"):
        assert call(**{null: None}) == L.EINVAL, null
        assert call(**{null: None}, T=0) == L.EINVAL, null
    assert call(null_inputs=True) == L.EINVAL
    assert call(n_inputs=0) == L.EINVAL and call(n_inputs=9) == L.EINVAL and call(n_inputs=8, T=0) == 0
    assert call(n_in=0) == L.EINVAL and call(D=0) == L.EINVAL and call(D=5) == L.EINVAL and call(D=4, T=0) == 0
    assert call(n_train=0) == L.EINVAL and call(n_train=-1) == L.EINVAL
    assert call(n_train=L.GP_MAX_TRAIN + 1) == L.ETOOBIG and call(n_train=L.GP_MAX_TRAIN, T=0) == 0
    assert call(B=6) == L.EALIGN == -2 and call(B=0) == L.EINVAL and call(T=-1) == L.EINVAL
    for mis in ("rates", "wt", "sq", "alpha", "linv", "ws", "var", "mean"):
        assert call(**{mis: q}) == L.EALIGN, mis
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(inv=bad) == L.EINVAL, bad
    assert call(T=1 << 40) == L.ETOOBIG and call(T=1 << 62, B=512) == L.ETOOBIG


# ---- host logic: how the work is cut into workspaces ----------------------------------------------------------------------
def test_workspace_pieces():
    from ratinabox_amd._gp_decoder import workspace_pieces
    for T, B, Np, limit in ((16, 4096, 2048, 2 ** 28), (3, 132, 160, 4 * 160 * 132), (3, 132, 160, 4 * 160 * 132 - 1),
                            (5, 1024, 96, 4 * 96 * 300), (7, 8, 32, 4 * 32 * 8 * 3), (1, 388, 64, 4 * 64 * 128), (0, 8, 32, 1 << 20),
                            (4, 260, 32, 4 * 32 * 259)):
        pieces = workspace_pieces(T, B, Np, limit)
        seen = np.zeros((T, B), dtype=np.int64)
        for t0, t1, c0, c1 in pieces:
            assert 0 <= t0 < t1 <= T and 0 <= c0 < c1 <= B and 4 * Np * (t1 - t0) * (c1 - c0) <= limit
            assert c0 % 128 == 0 and (c1 == B or c1 % 128 == 0)
            assert (c0, c1) == (0, B) or t1 == t0 + 1                  # rows are cut first; only a single row is cut over columns
            seen[t0:t1, c0:c1] += 1
        assert (seen == 1).all()                                          # every (row, column) once
        assert pieces == sorted(pieces)                                   # in order
    assert workspace_pieces(16, 4096, 2048, 2 ** 28) == [(t, t + 8, 0, 4096) for t in (0, 8)]
    assert workspace_pieces(3, 132, 160, 4 * 160 * 132 - 1) == [(t, t + 1, c, d) for t in range(3) for c, d in ((0, 128), (128, 132))]
    assert workspace_pieces(1, 388, 64, 4 * 64 * 300) == [(0, 1, 0, 256), (0, 1, 256, 388)]
    for T, B, Np, limit in ((1, 128, 32, 4 * 32 * 128 - 1), (2, 4096, 2048, (1 << 20) - 1), (1, 8, 32, 4 * 32 * 8 - 1), (1, 8, 32, 0)):
        with pytest.raises(ValueError, match="max_workspace_bytes"):
            workspace_pieces(T, B, Np, limit)


class _Recorder:
    """stands in for torch.ops.riab.gp_predict / gp_predict_var on host tensors: records the calls, returns what marks them"""

    def __init__(self):
        self.mean_calls, self.var_calls = [], []

    def gp_predict(self, rates, wts, sq, al, n_train, inv):
        import torch
        self.mean_calls.append(tuple(rates[0].shape))
        return torch.zeros((rates[0].shape[0], al.shape[0], rates[0].shape[2]))

    def gp_predict_var(self, rates, wts, sq, al, linv_t, n_train, inv, ws, with_mean):
        import torch
        T, _, B = rates[0].shape
        assert all(x.is_contiguous() and tuple(x.shape[::2]) == (T, B) for x in rates) and with_mean
        assert ws.numel() >= T * sq.shape[0] * B and tuple(linv_t.shape) == (sq.shape[0],) * 2
        self.var_calls.append((T, B, float(rates[0][0, 0, 0])))
        tag = rates[0][:, 0, :].clone()          # var := the first cell's rate, mean := it and its double
        return tag, torch.stack([tag, 2 * tag][:al.shape[0]], dim=1)


def test_predict_tensor_host_logic(G, monkeypatch):
    """predict_tensor on host tensors with the two operators replaced: without return_std no variance table is built and
    the mean operator alone is called; with it the pieces are issued in order, contiguous, and put back where they belong;
    a cut that cannot fit raises."""
    import torch
    from ratinabox_amd import GPDecoder
    X, y, Xq, ell, alpha = case(G, "a")
    dec = GPDecoder.from_samples(torch.from_numpy(X), torch.from_numpy(y), ell, alpha, widths=[7, 50])
    rec = _Recorder()
    monkeypatch.setattr(torch.ops.riab, "gp_predict", rec.gp_predict, raising=False)
    monkeypatch.setattr(torch.ops.riab, "gp_predict_var", rec.gp_predict_var, raising=False)
    T, B, Np = 3, 260, 96
    rates = [torch.arange(T * 7 * B, dtype=torch.float32).reshape(T, 7, B), torch.zeros(T, 50, B)]
    built = []
    real = GPDecoder._variance_table
    monkeypatch.setattr(GPDecoder, "_variance_table", lambda self, dev: built.append(dev) or real(self, dev))
    out = dec.predict_tensor(rates)
    assert tuple(out.shape) == (T, 2, B) and rec.mean_calls == [(T, 7, B)] and not rec.var_calls
    assert dec.predict_tensor(rates, return_std=False, max_workspace_bytes=0).shape == out.shape    # (the limit is not looked at)
    assert not built and dec._linv_t is None
    want_var = rates[0][:, 0, :]
    for limit, calls in ((2 ** 28, [(3, 260)]), (4 * Np * B * 2, [(2, 260), (1, 260)]), (4 * Np * B, [(1, 260)] * 3),
                         (4 * Np * B - 1, [(1, 256), (1, 4)] * 3), (4 * Np * 128, [(1, 128), (1, 128), (1, 4)] * 3)):
        rec.var_calls.clear()
        mean, std = dec.predict_tensor(rates, return_std=True, max_workspace_bytes=limit)
        assert [c[:2] for c in rec.var_calls] == calls, (limit, rec.var_calls)
        assert tuple(mean.shape) == (T, 2, B) and tuple(std.shape) == (T, B)
        assert torch.equal(std, torch.sqrt(want_var)) and torch.equal(mean[:, 0], want_var) and torch.equal(mean[:, 1], 2 * want_var)
    assert len(built) == 5 and dec._linv_t is not None and not rec.mean_calls[2:]
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        dec.predict_tensor(rates, return_std=True, max_workspace_bytes=4 * Np * 128 - 1)
    with pytest.raises(ValueError, match="widths"):
        dec.predict_tensor(rates[:1], return_std=True)
