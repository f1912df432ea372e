"""No-GPU checks of the host half of the step plans (ratinabox_amd/plan.py): StepPlan and AutoStepper built on a CPU
agent, their native step calls replaced by stubs that launch nothing.  What is pinned is the bookkeeping the two
classes share: which history rows are opened, when they are re-opened, and what sync() publishes."""
import numpy as np
import pytest

import ratinabox_amd as riab
import ratinabox_amd._lib as L
from ratinabox_amd.plan import AutoStepper, StepPlan


@pytest.fixture()
def world():
    np.random.seed(0)
    ag = riab.Agent(riab.Environment({}), {"n_agents": 8, "dt": 0.01, "device": "cpu"})
    pcs = riab.PlaceCells(ag, {"n": 16})
    gcs = riab.GridCells(ag, {"n": 8, "save_spikes": False})
    hdc = riab.HeadDirectionCells(ag, {"n": 4, "save_history": False})
    return ag, pcs, gcs, hdc


def _clocks(n, dt=0.01):
    t, out = 0.0, []
    for _ in range(n):
        t += dt
        out.append(t)
    return out


def test_step_plan_rows_and_publishing(world):
    ag, pcs, gcs, hdc = world
    plan = StepPlan(ag, capacity=5)
    assert ag._plan is plan and plan.neurons == [pcs, gcs, hdc] and plan.capacity == 5
    seen = []
    plan._step_fn = lambda h, k, s: seen.append(k) or 0
    plan._raw_stream = lambda _i: None
    ks = [1, 1, 2, 3, 1, 5]
    for k in ks:
        plan.step(k)
    plan.sync()
    assert seen == ks
    want = _clocks(13)
    assert ag._times == want and pcs._times == want and gcs._times == want and hdc._times == []
    assert ag.t == want[-1]
    # (5 rows open; 1+1+2 fit, 3 do not: a 1-row tail is left behind; 3+1 fit, 5 do not; 5)
    for h in (ag._hist, pcs._hist_fr, pcs._hist_sp, gcs._hist_fr):
        assert h.filled == [4, 4, 5]
    assert len(gcs._hist_sp) == 0 and len(hdc._hist_fr) == 0
    assert pcs._rates.data_ptr() == pcs._hist_fr.row(12).data_ptr() and pcs._rates.shape == (16, ag._Bp)
    assert pcs._spikes_last.data_ptr() == pcs._hist_sp.row(12).data_ptr()
    assert gcs._rates.data_ptr() == gcs._hist_fr.row(12).data_ptr() and gcs._spikes_last is None
    fr, sp = plan._pop_rows[2]
    assert sp is None and fr.shape == (1, 4, ag._Bp) and hdc._rates.data_ptr() == fr[0].data_ptr()
    assert ag._last_row.data_ptr() == ag._hist.row(12).data_ptr()
    with pytest.raises(ValueError):
        plan.step(6)
    plan.close()
    assert ag._plan is None and not plan._h
    plan.close()
    assert seen == ks and ag._times == want


class _Full:
    """A native step of one owner that launches nothing, counts its calls and answers RIAB_EFULL once each time the
    rows opened for that owner are used up (`rows()`: how many are open now)."""

    def __init__(self, rows):
        self.rows, self.used, self.calls, self.full = rows, 0, 0, 0

    def __call__(self):
        self.calls += 1
        if self.used == self.rows():
            self.used = 0
            self.full += 1
            return L.EFULL
        self.used += 1
        return 0


def _stub(st):
    agent = _Full(lambda: st._agent_rows.shape[0])
    pops = [_Full(lambda i=i: st._pop_rows[i][0].shape[0]) for i in range(len(st.neurons))]
    st._step_agent_fn = lambda h, s: agent()
    st._step_pop_fn = lambda h, i, s: pops[i]()
    st._raw_stream = lambda _i: None
    return agent, pops


def test_auto_stepper_rollover_per_owner(world, monkeypatch):
    ag, pcs, gcs, hdc = world
    monkeypatch.setattr(AutoStepper, "CAPACITY", 6)
    st = AutoStepper(ag)
    assert ag._plan is st and type(st).__name__ == "AutoStepper" and st.neurons == [pcs, gcs, hdc]
    agent, pops = _stub(st)
    assert st._agent_rows.shape[0] == 6 and st._pop_rows[0][0].shape[0] == 64 and st._pop_rows[1][0].shape[0] == 64
    ok, ptrs = [], []
    for _ in range(150):
        ok += [st.step_agent(), st.step_population(pcs), st.step_population(gcs)]
        ptrs.append((st._agent_rows.data_ptr(), st._pop_rows[0][0].data_ptr(), st._pop_rows[1][0].data_ptr()))
    assert all(ok) and len(ok) == 450
    st.sync()
    want = _clocks(150)
    assert ag._times == want and pcs._times == want and gcs._times == want and hdc._times == []
    for h in (ag._hist, pcs._hist_fr, pcs._hist_sp, gcs._hist_fr):
        assert sum(h.filled) == 150
    assert len(gcs._hist_sp) == 0
    # the rounds (0-based) in which each owner's rows were opened anew: the agent's 6-row chunks, the populations' 64-row ones
    moved = [[r for r in range(1, 150) if ptrs[r][k] != ptrs[r - 1][k]] for k in range(3)]
    assert moved[0] == list(range(6, 150, 6)) and len(moved[0]) == 24 and agent.full == 24
    assert moved[1] == [64, 128] and moved[2] == [64, 128] and pops[0].full == 2 and pops[1].full == 2 and pops[2].calls == 0
    assert not set(moved[0]) & set(moved[1])
    assert ag._hist.filled == [6] * 25 and pcs._hist_fr.filled == [64, 64, 22] and pcs._hist_sp.filled == [64, 64, 22]
    assert gcs._hist_fr.filled == [64, 64, 22]
    assert pcs._rates.data_ptr() == pcs._hist_fr.row(149).data_ptr()
    assert pcs._spikes_last.data_ptr() == pcs._hist_sp.row(149).data_ptr()
    assert gcs._rates.data_ptr() == gcs._hist_fr.row(149).data_ptr() and gcs._spikes_last is None
    assert ag._last_row.data_ptr() == ag._hist.row(149).data_ptr()
    # a population whose tables changed is not served
    pcs.place_cell_centres[0, 0] += 0.01
    assert st.step_population(pcs) is False and st.step_population(gcs) is True
    st.sync()
    assert len(pcs._times) == 150 and len(gcs._times) == 151
    ag._auto_after = 2 * ag.AUTO_AFTER
    st.close()                       # (served 150 steps: worth recording again right away)
    assert ag._plan is None and not st._h and ag._auto_after == ag.AUTO_AFTER and ag._auto_streak == 0
    st.close()
    # ... and one closed after fewer than AUTO_KEEP served steps doubles the wait for the next
    st = AutoStepper(ag)
    _stub(st)
    assert ag.AUTO_KEEP > 2
    ag._auto_streak = 7
    assert st.step_agent() and st.step_agent()
    st.close()
    assert ag._auto_after == 2 * ag.AUTO_AFTER and ag._auto_streak == 0 and len(ag._times) == 152
