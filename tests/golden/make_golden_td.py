"""Generate tests/golden/td_value.npz and td_successor.npz by IMPORTING THE REFERENCE's TD learners
(contribs/ValueNeuron.py, contribs/SuccessorFeatures.py), the way make_golden.py drives the rest of it.

Runs only in the build container (needs /root/reference); the .npz files are data (inputs + the reference's outputs)
and are committed.  Nothing from the reference's source travels.

    MPLBACKEND=Agg python tests/golden/make_golden_td.py [--out DIR]

td_value.npz: ONE reference agent (dt 0.05, speed_mean 0.2) explores for T steps; 48 PlaceCells (widths 0.15) feed a
ValueNeuron with n = 2, tau = 1, eta = 0.01 and start weights 0.5 * |w_init|; the reward is r = [R, R / 2], R the rate
of a gaussian_threshold PlaceCell at the room's centre.  Two runs from the same seed — `relu` (gain 1, threshold 0.15)
and `linear` — see the same trajectory, input rates, reward and traces (none of them depends on the activation; asserted),
so those are stored once.  Recorded per step: position, input rates phi_t, reward r_t, and per run V_t, firingrate_prime,
td_error_t; the trace; w at the start, after T/2 and after T steps.

The relu run must cross its kink and stay clear of it (asserted): min_t |pre-activation - threshold| >= 1e-4, and
between 1 % and 20 % of the (step, neuron) samples on the zero side — the fp32 drift of a device run is ~1e-5, so no
`firingrate_prime` decision can flip.

td_successor.npz: SuccessorFeatures of 8 PlaceCells (the features) over the same kind of 48-cell basis, default relu."""
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

from ratinabox.Environment import Environment  # noqa: E402
from ratinabox.Agent import Agent  # noqa: E402
from ratinabox.Neurons import PlaceCells  # noqa: E402
from ratinabox.contribs.ValueNeuron import ValueNeuron  # noqa: E402
from ratinabox.contribs.SuccessorFeatures import SuccessorFeatures  # noqa: E402

SEED = 3   # (48 cells x 1000 steps: seeds 3, 4, 7 and 11 satisfy the kink condition below, 0-2, 5, 6, 8-10, 12, 13 do not)
DT, TAU, ETA = 0.05, 1.0, 0.01
N_IN, T_VALUE, T_SUCCESSOR = 48, 1000, 600
THRESHOLD = 0.15


def value_run(act):
    np.random.seed(SEED)
    Env = Environment()
    Ag = Agent(Env, {"dt": DT, "speed_mean": 0.2})
    PCs = PlaceCells(Ag, {"n": N_IN, "widths": 0.15})
    R = PlaceCells(Ag, {"n": 1, "place_cell_centres": np.array([[0.5, 0.5]]), "description": "gaussian_threshold"})
    VN = ValueNeuron(Ag, {"input_layers": [PCs], "tau": TAU, "eta": ETA, "n": 2, "activation_function": act})
    e = list(VN.inputs.values())[0]
    e["w"] = 0.5 * np.abs(e["w"])
    out = {"w0": e["w"].copy(), "pos0": Ag.pos.copy(), "centres": PCs.place_cell_centres.copy(),
           "widths": np.asarray(PCs.place_cell_widths, dtype=np.float64).copy(),
           "reward_centre": R.place_cell_centres.copy(), "reward_width": np.asarray(R.place_cell_widths, dtype=np.float64).copy()}
    rec = {k: [] for k in ("pos", "phi", "r", "V", "prime", "td", "trace", "pre")}
    for t in range(T_VALUE):
        Ag.update()
        R.update()
        PCs.update()
        VN.update()
        r = np.array([R.firingrate[0], 0.5 * R.firingrate[0]])
        rec["pre"].append(e["w"] @ PCs.firingrate)
        VN.update_weights(r)
        rec["pos"].append(Ag.pos.copy())
        rec["phi"].append(PCs.firingrate.copy())
        rec["r"].append(r)
        rec["V"].append(VN.firingrate.copy())
        rec["prime"].append(np.asarray(VN.firingrate_prime, dtype=np.float64).copy())
        rec["td"].append(VN.td_error.copy())
        rec["trace"].append(e["eligibility_trace"].copy())
        if t + 1 == T_VALUE // 2:
            out["w_half"] = e["w"].copy()
    out["w_T"] = e["w"].copy()
    out.update({k: np.array(v, dtype=np.float64) for k, v in rec.items()})
    out["tau_e"] = np.float64(VN.tau_e)
    out["L2"] = np.float64(VN.L2)
    return out


def make_value(dest):
    relu = value_run({"activation": "relu", "gain": 1.0, "threshold": THRESHOLD})
    lin = value_run({"activation": "linear"})
    shared = ("pos", "phi", "r", "trace", "w0", "pos0", "centres", "widths", "reward_centre", "reward_width", "tau_e", "L2")
    for k in shared:
        assert np.array_equal(relu[k], lin[k]), f"{k} differs between the relu and the linear run"
    dist = np.abs(relu["pre"] - THRESHOLD)
    zero_share = float((relu["pre"] <= THRESHOLD).mean())
    print(f"td_value: relu min |pre-activation - threshold| = {dist.min():.3e}, share on the zero side = {zero_share:.3f}")
    assert dist.min() >= 1e-4, "the relu run comes too close to its kink: pick another seed"
    assert 0.01 <= zero_share <= 0.20, "the relu run must cross its kink in 1-20 % of the samples"
    assert np.array_equal(relu["prime"], (relu["pre"] > THRESHOLD).astype(np.float64))
    out = {k: relu[k] for k in shared}
    out.update(dt=np.float64(DT), tau=np.float64(TAU), eta=np.float64(ETA), threshold=np.float64(THRESHOLD))
    for name, run in (("relu", relu), ("linear", lin)):
        for k in ("V", "prime", "td", "w_half", "w_T"):
            out[f"{name}_{k}"] = run[k]
    np.savez_compressed(os.path.join(dest, "td_value.npz"), **out)


def make_successor(dest):
    np.random.seed(SEED)
    Env = Environment()
    Ag = Agent(Env, {"dt": DT, "speed_mean": 0.2})
    PCs = PlaceCells(Ag, {"n": N_IN, "widths": 0.15})
    Feat = PlaceCells(Ag, {"n": 8, "widths": 0.2})
    SF = SuccessorFeatures(Ag, {"input_layers": [PCs], "features": Feat, "tau": TAU, "eta": ETA})
    e = list(SF.inputs.values())[0]
    e["w"] = 0.5 * np.abs(e["w"])
    out = {"w0": e["w"].copy(), "pos0": Ag.pos.copy(), "centres": PCs.place_cell_centres.copy(),
           "widths": np.asarray(PCs.place_cell_widths, dtype=np.float64).copy(),
           "feature_centres": Feat.place_cell_centres.copy(),
           "feature_widths": np.asarray(Feat.place_cell_widths, dtype=np.float64).copy()}
    rec = {k: [] for k in ("pos", "phi", "r", "V", "prime", "td", "trace")}
    for t in range(T_SUCCESSOR):
        Ag.update()
        PCs.update()
        Feat.update()
        SF.update()
        SF.update_weights()
        rec["pos"].append(Ag.pos.copy())
        rec["phi"].append(PCs.firingrate.copy())
        rec["r"].append(Feat.firingrate.copy())
        rec["V"].append(SF.firingrate.copy())
        rec["prime"].append(np.asarray(SF.firingrate_prime, dtype=np.float64).copy())
        rec["td"].append(SF.td_error.copy())
        rec["trace"].append(e["eligibility_trace"].copy())
        if t + 1 == T_SUCCESSOR // 2:
            out["w_half"] = e["w"].copy()
    out["w_T"] = e["w"].copy()
    out.update({k: np.array(v, dtype=np.float64) for k, v in rec.items()})
    assert (out["V"] > 0).all(), "the default relu (threshold 0) must stay on its linear side"
    out.update(dt=np.float64(DT), tau=np.float64(TAU), eta=np.float64(ETA), tau_e=np.float64(SF.tau_e), L2=np.float64(SF.L2))
    np.savez_compressed(os.path.join(dest, "td_successor.npz"), **out)


if __name__ == "__main__":
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    make_value(dest)
    make_successor(dest)
    print("wrote td_value.npz, td_successor.npz to", dest)
