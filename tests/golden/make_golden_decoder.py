"""Generate tests/golden/decoder_reference.npz by IMPORTING THE REFERENCE and fitting sklearn's Ridge to its history,
the way the reference's own tests/test_advanced.py::test_decoding_position and its decoding_position_example demo do.

Runs only in the build container (needs /root/reference and scikit-learn); the .npz file is data (inputs + the fitted
results) and is committed.  Nothing from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_decoder.py [--out DIR]

The reference's decoding scenario, shortened: Environment() with the wall [[0.4, 0], [0.4, 0.4]], one agent at dt 50 ms,
20 gaussian_threshold PlaceCells of width 0.4 and 20 GridCells; N_TRAIN training steps and N_TEST test steps.  A device
history holds fp32 rows, so the recorded positions and rates are rounded to float32 HERE and everything is fitted on
those values widened back to float64: what is stored is exactly what a replay fits.
sklearn.linear_model.Ridge(alpha=0.01) is fitted in float64 on every STRIDE-th training row (the reference's `[::5]`)
for the PlaceCells alone ("pc", columns 0..19 of fr), the GridCells alone ("gc", columns 20..39) and both ("all").

  pos (T, 2) float32, fr (T, 40) float32, t (T,) float64, n_train, stride, alpha
  coef_<tag> (2, n) float64, intercept_<tag> (2,) float64      the fitted model
  pred_<tag> (N_TEST, 2) float64                               its predict() on the test rows (rows n_train .. T-1)"""
import os
import sys
import warnings

os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_shims"))
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

from sklearn.linear_model import Ridge  # noqa: E402

from ratinabox.Environment import Environment  # noqa: E402
from ratinabox.Agent import Agent  # noqa: E402
from ratinabox.Neurons import PlaceCells, GridCells  # noqa: E402

N_TRAIN, N_TEST, STRIDE, ALPHA = 2400, 600, 5, 0.01
COLUMNS = {"pc": slice(0, 20), "gc": slice(20, 40), "all": slice(0, 40)}


def main(dest):
    np.random.seed(11)
    Env = Environment()
    Env.add_wall(np.array([[0.4, 0], [0.4, 0.4]]))
    Ag = Agent(Env, {"dt": 0.05})
    PCs = PlaceCells(Ag, {"n": 20, "description": "gaussian_threshold", "widths": 0.4})
    GCs = GridCells(Ag, {"n": 20})
    for _ in range(N_TRAIN + N_TEST):
        Ag.update()
        PCs.update()
        GCs.update()
    pos = np.array(Ag.history["pos"], dtype=np.float64).astype(np.float32)
    fr = np.concatenate((np.array(PCs.history["firingrate"]), np.array(GCs.history["firingrate"])), axis=1).astype(np.float32)
    out = dict(pos=pos, fr=fr, t=np.array(Ag.history["t"], dtype=np.float64), n_train=np.int64(N_TRAIN),
               stride=np.int64(STRIDE), alpha=np.float64(ALPHA))
    x64, y64 = fr.astype(np.float64), pos.astype(np.float64)
    for tag, cols in COLUMNS.items():
        model = Ridge(alpha=ALPHA)
        model.fit(x64[:N_TRAIN:STRIDE, cols], y64[:N_TRAIN:STRIDE])
        pred = model.predict(x64[N_TRAIN:, cols])
        out[f"coef_{tag}"] = np.array(model.coef_, dtype=np.float64)
        out[f"intercept_{tag}"] = np.array(model.intercept_, dtype=np.float64)
        out[f"pred_{tag}"] = np.array(pred, dtype=np.float64)
        err = np.linalg.norm(pred - y64[N_TRAIN:], axis=1).mean()
        print(f"{tag}: coef {out[f'coef_{tag}'].shape}, mean decoding error on the test rows {1000 * err:.1f} mm")
    path = os.path.join(dest, "decoder_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE)
