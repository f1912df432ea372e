"""Generate tests/golden/gp_variance_reference.npz: scikit-learn's GaussianProcessRegressor.predict(return_std=True) and its
log marginal likelihood on three small synthetic problems, set up as the reference sets its decoder up
(alpha = 0.01, RBF with a fixed length scale, normalize_y=False).  Needs scikit-learn and NumPy; reads nothing.

    python tests/golden/make_golden_gp_variance.py [--out DIR]

Cases (`<c>` = a, b, c):
  a   N = 70 samples of n = 57 cells in two populations (7 + 50), D = 2 target columns
  b   N = 33, n = 5, D = 1
  c   N = 1, n = 3, D = 1
Rates are cubes of uniform numbers rounded to float32 (what a rate history holds), widened to float64 for the fit.  The
queries are training points, midpoints of pairs of training points, random points of the same distribution and points far
outside the training set, so that the predictive variance runs from alpha / (1 + alpha) to 1; the generator asserts that
sklearn's y_std^2 over the queries of EVERY case spans at least [0.05, 0.9].

  X_<c> (N, n), y_<c> (N, D), Xq_<c> (Q, n) float64      training rates and targets, query rates
  widths_<c> int64                                        the populations' widths
  length_scale_<c>, alpha float64                         the hyper-parameters
  y_mean_<c> (Q, D), y_std_<c> (Q,) float64               predict(Xq, return_std=True) (sklearn repeats the std per column:
                                                          the columns are asserted equal and one is kept)
  lml_<c> float64                                         log_marginal_likelihood_value_"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALPHA = 0.01
CASES = {"a": ((7, 50), 70, 2, 1.2), "b": ((5,), 33, 1, 0.45), "c": ((3,), 1, 1, 0.5)}   # widths, N, D, length scale


def problem(seed, n, N, D, ell):
    rng = np.random.RandomState(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    X = f32(rng.rand(N, n) ** 3)
    y = rng.rand(N, D)
    at = X[rng.randint(0, N, size=6)]
    mid = f32(0.5 * (X[rng.randint(0, N, size=6)] + X[rng.randint(0, N, size=6)]))
    near = f32(X[rng.randint(0, N, size=6)] + 0.6 * ell * rng.randn(6, n) / np.sqrt(n))
    rand = f32(rng.rand(6, n) ** 3)
    far = f32(X[rng.randint(0, N, size=6)] + 4.0 * ell * np.sign(rng.randn(6, n)) / np.sqrt(n))
    return X, y, np.concatenate([at, mid, near, rand, far])


def main(dest):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF
    warnings.filterwarnings("ignore")
    out = dict(alpha=np.float64(ALPHA))
    for seed, (tag, (widths, N, D, ell)) in enumerate(CASES.items()):
        X, y, Xq = problem(11 + seed, sum(widths), N, D, ell)
        model = GaussianProcessRegressor(alpha=ALPHA, kernel=RBF(ell, length_scale_bounds="fixed"), normalize_y=False)
        model.fit(X, y)
        mean, std = model.predict(Xq, return_std=True)
        mean, std = np.asarray(mean, dtype=np.float64).reshape(len(Xq), D), np.asarray(std, dtype=np.float64)
        if std.ndim == 2:
            assert (std == std[:, :1]).all()
            std = std[:, 0]
        var = std ** 2
        print(f"{tag}: N {N}, n {sum(widths)}, D {D}, length scale {ell}: y_std^2 over {len(Xq)} queries spans "
              f"[{var.min():.4f}, {var.max():.4f}], lml {model.log_marginal_likelihood_value_:.6f}")
        assert var.min() <= 0.05 and var.max() >= 0.9, "the queries do not exercise the variance"
        out.update({f"X_{tag}": X, f"y_{tag}": y, f"Xq_{tag}": Xq, f"widths_{tag}": np.array(widths, dtype=np.int64),
                    f"length_scale_{tag}": np.float64(ell), f"y_mean_{tag}": mean, f"y_std_{tag}": std,
                    f"lml_{tag}": np.float64(model.log_marginal_likelihood_value_)})
    path = os.path.join(dest, "gp_variance_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE)
