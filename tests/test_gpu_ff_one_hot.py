"""riab_feedforward's streamed GEMM loop (csrc/riab_mfma_slab.h under csrc/riab_ff.hip) at the smallest shapes at which it
can go wrong: two input populations of 5 and 19 cells (K < 16, and K = 16 + 3: a second, ragged slab), n_out of 7, 40, 70
and 160 (1, 2, 2 and 4 MFMA row tiles; 160 is two row blocks), B of 4 and 132 (one and two position tiles) with the last
lane a padding lane that holds NaN, T = 2.

With one-hot inputs and the linear activation every product but one is 0 and the k-ordered fmaf chain is exact: the output
is fp32(W[m][k] + bias[m]) BIT FOR BIT (bias[m] alone where the input is all zeros).  With random inputs the bound is the one
of tests/test_gpu_parity.py::test_randomised_feedforward_shapes_vs_oracle against the float64 product.

Why it exists beside the other feed-forward tests: none of them compares bits with the weights, and none runs these
shapes.  test_randomised_feedforward_shapes_vs_oracle draws widths from {1, 3, 15, 16, 17, 31, 64, 100, 257} and n_out from
{1, 5, 31, ..., 300} with one time row and no padding lane; test_gpu_guard_bands.py::test_feedforward_layer has B of 4 and
132 but n of 1 and 33 only; test_gpu_ops.py and test_gpu_td.py run one population of 40 or more cells."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = (5, 19)
T = 2
LINEAR = 0


def run_op(xs, ws, bias):
    """xs [(T, n_l, B)], ws [(n_out, n_l)], bias (n_out,), float32 host arrays -> (T, n_out, B)"""
    import ratinabox_amd.ops  # noqa: F401  (registers torch.ops.riab.*)
    n_out = bias.shape[0]
    wts = []
    for w in ws:
        wt = np.zeros((w.shape[1], (n_out + 31) // 32 * 32), dtype=np.float32)
        wt[:, :n_out] = w.T
        wts.append(torch.from_numpy(wt).to(DEV))
    out = torch.ops.riab.feedforward([torch.from_numpy(x).to(DEV) for x in xs], wts, torch.from_numpy(bias).to(DEV), LINEAR,
                                     [1.0, 0.0, 0.0, 0.0])
    torch.cuda.synchronize()
    return out.cpu().numpy()


def split(X):
    """(T, K, B) -> the operator's inputs [(T, n_l, B)]"""
    out, k = [], 0
    for w in WIDTHS:
        out.append(np.ascontiguousarray(X[:, k:k + w]))
        k += w
    return out


@pytest.mark.parametrize("B", [4, 132])
@pytest.mark.parametrize("n_out", [7, 40, 70, 160])
def test_one_hot_bit_for_bit_and_random_vs_float64(n_out, B):
    rng = np.random.RandomState(1000 * n_out + B)
    K, n_real = sum(WIDTHS), B - 1
    W = rng.normal(0, 1 / np.sqrt(K), (n_out, K)).astype(np.float32)
    bias = rng.normal(0, 0.3, n_out).astype(np.float32)
    ws = [W[:, :WIDTHS[0]], W[:, WIDTHS[0]:]]

    # one-hot: position (t, b) holds a 1 in cell which[t, b]; which == K is the all-zero input.  The first and the last cell
    # of both populations and of the second slab are always among them.
    which = rng.randint(0, K + 1, size=(T, B))
    forced = [0, 4, 5, 20, 21, 23] if n_real * T <= 6 else [0, 4, 5, 20, 21, 23, K]
    which.reshape(-1)[[i for i in range(T * B) if i % B < n_real][:len(forced)]] = forced
    X = np.zeros((T, K + 1, B), dtype=np.float32)
    np.put_along_axis(X, which[:, None, :], 1.0, axis=1)
    X = X[:, :K]
    X[:, :, n_real:] = np.nan
    got = run_op(split(X), ws, bias)
    assert got.shape == (T, n_out, B) and got.dtype == np.float32
    Wz = np.concatenate([W, np.zeros((n_out, 1), dtype=np.float32)], axis=1)
    want = (Wz[:, which] + bias[:, None, None]).transpose(1, 0, 2)   # fp32 + fp32, rounded once: (T, n_out, B)
    assert want.dtype == np.float32
    assert np.array_equal(got[:, :, :n_real].view(np.uint32), want[:, :, :n_real].view(np.uint32))

    # random inputs in [0, 1] against the float64 product
    X = rng.uniform(0, 1, (T, K, B)).astype(np.float32)
    X[:, :, n_real:] = np.nan
    got = run_op(split(X), ws, bias)
    ref = np.einsum("mk,tkb->tmb", W.astype(np.float64), X[:, :, :n_real].astype(np.float64)) + bias.astype(np.float64)[None, :, None]
    cond = np.abs(W.astype(np.float64)).sum(1) + np.abs(bias.astype(np.float64))
    tol = 2e-6 * cond[None, :, None] + 1e-6 * np.abs(ref)
    err = np.abs(got[:, :, :n_real] - ref)
    print(f"n_out {n_out}, B {B}: worst |error| / tolerance = {(err / tol).max():.3g}")
    assert np.isfinite(got[:, :, :n_real]).all() and (err <= tol).all()
