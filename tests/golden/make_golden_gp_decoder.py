"""Generate tests/golden/gp_decoder_reference.npz: scikit-learn's GaussianProcessRegressor on the decoding scenario that
tests/golden/decoder_reference.npz already holds, set up the way the reference's tests/test_advanced.py::test_decoding_position
and its decoding demo set it up beside their Ridge:

    GaussianProcessRegressor(alpha=0.01, kernel=RBF(np.sqrt(n / 20), length_scale_bounds="fixed"))

Reads only decoder_reference.npz (`fr`, `pos`, `n_train`, `stride`: float32 rows of one agent, as a device history holds
them) and needs scikit-learn; nothing else.  The fit is done in float64 on the float32 values widened, on every `stride`-th
training row (the reference's `[::5]`), for the PlaceCells alone ("pc", columns 0..19 of fr), the GridCells alone ("gc",
columns 20..39) and both ("all").

    python tests/golden/make_golden_gp_decoder.py [--out DIR]

  alpha_<tag> (480, 2) float64          the fitted dual coefficients (GaussianProcessRegressor.alpha_)
  pred_<tag> (600, 2) float64           predict() on the test rows (rows n_train .. T-1)
  length_scale_<tag> float64            sqrt(n / 20)
  alpha float64                         the regulariser, 0.01"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
COLUMNS = {"pc": slice(0, 20), "gc": slice(20, 40), "all": slice(0, 40)}
ALPHA = 0.01


def main(dest):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF
    warnings.filterwarnings("ignore")
    G = np.load(os.path.join(HERE, "decoder_reference.npz"))
    n_train, stride = int(G["n_train"]), int(G["stride"])
    x64, y64 = G["fr"].astype(np.float64), G["pos"].astype(np.float64)
    out = dict(alpha=np.float64(ALPHA))
    for tag, cols in COLUMNS.items():
        n = cols.stop - cols.start
        model = GaussianProcessRegressor(alpha=ALPHA, kernel=RBF(np.sqrt(n / 20), length_scale_bounds="fixed"))
        model.fit(x64[:n_train:stride, cols], y64[:n_train:stride])
        pred = model.predict(x64[n_train:, cols])
        out[f"alpha_{tag}"] = np.array(model.alpha_, dtype=np.float64)
        out[f"pred_{tag}"] = np.array(pred, dtype=np.float64)
        out[f"length_scale_{tag}"] = np.float64(model.kernel_.length_scale)
        err = np.linalg.norm(pred - y64[n_train:], axis=1).mean()
        print(f"{tag}: alpha_ {out[f'alpha_{tag}'].shape}, mean decoding error on the test rows {1000 * err:.1f} mm")
    path = os.path.join(dest, "gp_decoder_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE)
