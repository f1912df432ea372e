"""The step of a plan that holds a learner, restated in float64 on top of tests/td_oracle.TDOracle: "learn, then reset"
with one mask per step.  Test infrastructure only, NumPy only (tests/test_td_plan_cpu.py checks it by hand).

    for every step:   update(phis); update_weights(reward); reset(mask)        # mask None: nothing is reset

A masked lane starts the next step from V = 0 and empty traces — what `VN.learn(r); VN.reset(lanes=done)` leaves — while
the weights, which all lanes share, keep what every lane (the masked ones included) taught them in this step."""
import numpy as np

from tests import td_oracle as tdo


class PlanOracle:
    def __init__(self, ws, B, **kw):
        self.o = tdo.TDOracle(ws, B=B, **kw)
        self.B = int(B)

    def step(self, phis, reward, mask=None):
        """One plan step on the input rates `phis` (one (n_in_l, B) array per layer); returns dict(V, dVdt, td) as they
        were BEFORE the reset (what the learner's history row and the weight update saw)."""
        o = self.o
        o.update(phis)
        o.update_weights(reward)
        seen = {"V": o.V.copy(), "dVdt": o.dVdt.copy(), "td": o.td.copy()}
        if mask is not None:
            m = np.asarray(mask, dtype=bool).reshape(-1)
            assert m.shape[0] == self.B, "one mask entry per lane"
            o.reset(m)
        return seen

    def run(self, phis_seq, rewards, masks):
        """Every step of a run; returns the list of `step`'s results."""
        return [self.step(p, r, m) for p, r, m in zip(phis_seq, rewards, masks)]
