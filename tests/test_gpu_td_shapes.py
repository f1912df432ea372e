"""csrc/riab_td.hip at the shapes of wide learners: every td_grad_kernel<MT, FUSE>, several row groups (where the fused
trace update falls back to the stand-alone kernel), up to eight ragged input layers, batches whose last chunk is short
or whose Bp is no multiple of 32.  torch.ops.riab.td_forward_tail / td_update are driven directly on tensors made here
(tests/td_shapes.py lists the cases and the path each is meant to take; tests/test_td_cpu.py checks those claims).

1. Integer inputs for which fp32 arithmetic is exact in any order (tests/td_shapes.py): weights, TD error and traces
   must equal the integer product bit for bit; fused == plain; NaN in every padded lane and guard row changes nothing.
2. Real-valued inputs against the float64 one-step oracle (tests/td_oracle.py one_step), allowance 4 x the same oracle in
   np.float32, every ratio printed (docs/EXPERIMENTS.md records them).
3. td_reset with a lane mask, and ValueNeuron / SuccessorFeatures at width against TDOracle, learn() == update() +
   update_weights() bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import td_oracle as tdo
from tests import td_shapes as sh

pytestmark = pytest.mark.gpu

CLEAN_GUARD = 5.0      # what guard rows hold in a clean run: an odd value, so that a stray read breaks the equality
CASES = sh.cases()


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    from ratinabox_amd import ops  # noqa: F401  (registers torch.ops.riab.*)
    return ratinabox_amd


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(x, alloc, guard, dev):
    """x (rows, cols) as the leading rows of a device array of `alloc` rows whose other rows hold `guard`: (view, whole)."""
    whole = torch.full((alloc, x.shape[1]), guard, dtype=torch.float32, device=dev)
    whole[:x.shape[0]] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    return whole[:x.shape[0]], whole


def _guard_intact(whole, rows, guard):
    g = whole[rows:]
    return bool(torch.isnan(g).all()) if guard != guard else bool((g == guard).all())


class _Step:
    """One learning step on device arrays with guard rows: layer arrays are padded to whole 128-row blocks, row arrays
    to whole row groups.  `poison`: NaN in every lane >= B of phi, trace, v, v_last (so dV/dt) and reward and in every
    guard row; otherwise those lanes hold ordinary values and the guard rows CLEAN_GUARD."""

    def __init__(self, riab, n, layers, B, Bp, a, consts, w0=None, poison=False):
        dev = torch.device("cuda")
        self.n, self.layers, self.B, self.Bp, self.consts = n, layers, B, Bp, consts
        self.guard = guard = float("nan") if poison else CLEAN_GUARD
        path = sh.launch_path(n, layers, Bp)
        row_alloc = path["groups"] * path["mt"] * 32
        self.Mp = Mp = (n + 31) // 32 * 32

        def lanes(x):
            x = np.array(x, dtype=np.float32)
            if poison:
                x[:, B:] = np.nan
            return x

        def block(k):
            return (k + 127) // 128 * 128

        self.phi, self.trace, self.wt = [], [], []
        for l, k in enumerate(layers):
            self.phi.append(_guarded(lanes(a["phi"][l]), block(k), guard, dev))
            self.trace.append(_guarded(lanes(a["trace"][l]), block(k), guard, dev))
            w = np.zeros((k, Mp), dtype=np.float32)
            if w0 is not None:
                w[:, :n] = w0[l].T
            self.wt.append(_guarded(w, block(k), guard, dev))
        self.v = _guarded(lanes(a["v"]), row_alloc, guard, dev)
        self.v_last = _guarded(lanes(a["v_last"]), row_alloc, guard, dev)
        self.prime = _guarded(a["prime"], row_alloc, guard, dev)
        self.dvdt = _guarded(np.full((n, Bp), 7.0), row_alloc, guard, dev)
        self.td = _guarded(np.full((n, Bp), 7.0), row_alloc, guard, dev)
        r = np.array(a["reward"])
        if r.ndim == 2:
            self.reward = _guarded(lanes(r), row_alloc, guard, dev)
        else:
            if poison and r.shape[0] == Bp:
                r[B:] = np.nan
            assert r.dtype == np.float64
            self.reward = (torch.from_numpy(r).to(dev),) * 2
        self.ws = torch.empty(riab.ops.td_workspace_floats(n, layers, Bp), dtype=torch.float32, device=dev)
        assert self.ws.numel() == path["n_chunks"] * n * sum(layers)

    def run(self, fuse):
        views = lambda pairs: [p[0] for p in pairs]
        args = (views(self.phi), views(self.trace), views(self.wt), self.consts, self.B)
        torch.ops.riab.td_forward_tail(self.v[0], self.v_last[0], self.dvdt[0], *args, not fuse)
        torch.ops.riab.td_update(views(self.wt), views(self.trace), views(self.phi), self.reward[0], self.v[0], self.dvdt[0],
                                 self.prime[0], self.td[0], self.ws, self.consts, self.B, fuse)
        torch.cuda.synchronize()
        return self

    def guards_intact(self):
        """No kernel wrote outside the rows it was given (and W^T's padding columns are still zero)."""
        n = self.n
        for l, k in enumerate(self.layers):
            for name, pair in (("phi", self.phi[l]), ("trace", self.trace[l]), ("wt", self.wt[l])):
                assert _guard_intact(pair[1], k, self.guard), (name, l)
            assert not self.wt[l][0][:, n:].any(), ("wt padding columns", l)
        for name in ("v", "v_last", "prime", "dvdt", "td"):
            assert _guard_intact(getattr(self, name)[1], n, self.guard), name

    def outputs(self):
        B = self.B
        return {"wt": [w[0].clone() for w in self.wt], "trace": [e[0][:, :B].clone() for e in self.trace],
                "trace_all": [e[0].clone() for e in self.trace], "td": self.td[0].clone(),
                "dvdt": self.dvdt[0][:, :B].clone(), "v_last": self.v_last[0][:, :B].clone()}


def _same_bits(a, b, keys, label):
    for k in keys:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for l, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(_bits(x), _bits(y)), (label, k, l)


# ---- 1. integers: bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_integer_inputs_bit_for_bit(riab, case):
    n, layers, B, Bp = case.n, case.layers, case.B, case.Bp
    path = sh.launch_path(n, layers, Bp)
    assert (path["mt"], path["groups"]) == sh.ROWS[n]                                  # the path it was written for
    assert riab.ops.td_workspace_floats(n, layers, Bp) // (n * sum(layers)) == path["n_chunks"]
    if layers == sh.LAYER_SETS[sh.MODEST_LAYERS]:
        assert (path["slabs"], path["n_chunks"], path["last"]) == sh.BATCHES[(B, Bp)]
    assert sh.exactness_bound(B) < 2 ** 24
    a = sh.integer_inputs(case)
    ref = sh.integer_reference(case, a)
    dev = torch.device("cuda")
    runs = {}
    for fuse in (True, False):
        for poison in (False, True):
            s = _Step(riab, n, layers, B, Bp, a, sh.INT_CONSTS, poison=poison).run(fuse)
            s.guards_intact()
            runs[fuse, poison] = s.outputs()
    got = runs[True, False]
    for l in range(len(layers)):
        want = torch.from_numpy(ref["wt"][l]).to(dev)
        assert torch.equal(got["wt"][l][:, :n], want), ("weights", l, int((got["wt"][l][:, :n] != want).sum()))
        assert not got["wt"][l][:, n:].any()
        assert torch.equal(got["trace"][l], torch.from_numpy(ref["traces"][l].astype(np.float32)).to(dev)), ("trace", l)
    assert any(w.any() for w in ref["wt"]) or B * n < 8
    assert torch.equal(got["td"][:, :B], torch.from_numpy(ref["td"].astype(np.float32)).to(dev))
    assert not got["td"][:, B:].any()
    assert torch.equal(got["dvdt"], torch.from_numpy(a["dvdt"][:, :B]).to(dev))
    assert torch.equal(got["v_last"], torch.from_numpy(a["v"][:, :B]).to(dev))
    # fused == plain (above 256 rows: the fall-back to the stand-alone trace kernel is one), on every lane of the trace
    _same_bits(got, runs[False, False], ("wt", "trace_all", "td", "dvdt", "v_last"), "fused vs plain")
    # NaN in the padded lanes and the guard rows changes nothing
    for fuse in (True, False):
        _same_bits(got, runs[fuse, True], ("wt", "trace", "td", "dvdt", "v_last"), f"poisoned, fuse={fuse}")


def test_nine_layers_are_refused_before_any_launch(riab):
    from ratinabox_amd import _lib as L
    dev = torch.device("cuda")
    n, k, B, Bp = 129, 4, 33, 36
    p = L.RiabTDParams()
    p.dt, p.tau, p.tau_e, p.eta, p.L2, p.B, p.Bp, p.n, p.Mp = 0.5, 1.0, 1.0, 1.0, 0.0, B, Bp, n, 160
    lay = (L.RiabTDLayer * 9)()
    phi, trace, wt = (torch.ones((9, k, m), device=dev) for m in (Bp, Bp, 160))
    for l in range(9):
        lay[l].rates, lay[l].trace, lay[l].wt, lay[l].n_in = phi[l].data_ptr(), trace[l].data_ptr(), wt[l].data_ptr(), k
    v, v_last, dvdt, prime, td, r = (torch.ones((n, Bp), device=dev) for _ in range(6))
    ws = torch.ones(64 * n * 9 * k, device=dev)
    assert L.lib.riab_td_workspace(p, lay, 9) == L.EINVAL
    assert L.lib.riab_td_forward_tail(p, lay, 9, L.ptr(v), L.ptr(v_last), L.ptr(dvdt), 1, L.current_stream()) == L.ETOOBIG
    assert L.lib.riab_td_update(p, lay, 9, L.ptr(r), 0, Bp, 1, L.ptr(v), L.ptr(dvdt), L.ptr(prime), L.ptr(td), 1, L.ptr(ws),
                                ws.numel(), L.current_stream()) == L.ETOOBIG
    rows = (C.c_void_p * 1)(td.data_ptr())
    assert L.lib.riab_td_reset(p, lay, 9, rows, 1, None, L.current_stream()) == L.ETOOBIG
    torch.cuda.synchronize()
    for t in (phi, trace, wt, v, v_last, dvdt, prime, td, r, ws):
        assert bool((t == 1).all())                                                    # nothing was launched
    with pytest.raises(ValueError, match="input layers"):
        torch.ops.riab.td_update(list(wt), list(trace), list(phi), r, v, dvdt, prime, td, ws, sh.INT_CONSTS, B, True)


# ---- 2. real numbers against the float64 one-step oracle -------------------------------------------------------------
REAL_CONSTS = [0.05, 1.0, 0.25, 2.0, 0.01]   # eta = 2: the step moves the weights by about their own size, L2 > 0
REAL = [("MT4", 128, "ragged", (1022, 1024)), ("MT8", 256, "three", (1022, 1024)), ("two-groups", 257, "ragged", (1022, 1024)),
        ("eight-layers", 129, "eight", (1022, 1024)), ("short-chunk", 129, "ragged", (4150, 4152)),
        ("short-chunk-two-groups", 257, "three", (4150, 4152))]


@pytest.fixture(scope="module")
def real_references():
    """Inputs, float64 oracle and float32 oracle of every real-valued case: computed once, shared by fused and plain."""
    out = {}
    for i, (name, n, key, (B, Bp)) in enumerate(REAL):
        rng = np.random.RandomState(100 + i)
        layers = sh.LAYER_SETS[key]
        a = {"phi": [rng.uniform(size=(k, Bp)).astype(np.float32) for k in layers],
             "trace": [rng.uniform(size=(k, Bp)).astype(np.float32) for k in layers]}
        for k in ("v", "v_last", "reward"):
            a[k] = rng.uniform(size=(n, Bp)).astype(np.float32)
        a["prime"] = (rng.uniform(size=(n, Bp)) > 0.3).astype(np.float32)
        w0 = [(rng.normal(size=(n, k)) * 0.1).astype(np.float32) for k in layers]
        real = lambda x: x[:, :B].astype(np.float64)
        args = (w0, [real(e) for e in a["trace"]], [real(p) for p in a["phi"]], real(a["v"]), real(a["v_last"]),
                real(a["prime"]), real(a["reward"])) + tuple(REAL_CONSTS)
        out[name] = (a, w0, tdo.one_step(*args), tdo.one_step(*args, dtype=np.float32))
    return out


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("name,n,key,batch", REAL, ids=[r[0] for r in REAL])
def test_real_inputs_vs_float64_one_step_oracle(riab, real_references, name, n, key, batch, fuse):
    """Measured on an MI355X (kernel error / fp32 NumPy error, worst over the layers; fused = plain): see
    docs/EXPERIMENTS.md, "TD learning on the device", the table of wide learners."""
    (B, Bp), layers = batch, sh.LAYER_SETS[key]
    a, w0, exact, low = real_references[name]
    s = _Step(riab, n, layers, B, Bp, a, REAL_CONSTS, w0=w0).run(fuse)
    s.guards_intact()
    o = s.outputs()
    got = {"dvdt": o["dvdt"], "td": o["td"][:, :B]}
    ref = {"dvdt": exact["dvdt"], "td": exact["td"]}
    l32 = {"dvdt": low["dvdt"], "td": low["td"]}
    for l in range(len(layers)):
        got[f"trace{l}"], ref[f"trace{l}"], l32[f"trace{l}"] = o["trace"][l], exact["traces"][l], low["traces"][l]
        got[f"w{l}"], ref[f"w{l}"], l32[f"w{l}"] = o["wt"][l][:, :n].t(), exact["ws"][l], low["ws"][l]
        assert not torch.equal(o["wt"][l][:, :n].t().cpu(), torch.from_numpy(w0[l]))
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
    scale = {k: float(np.abs(ref[k]).max()) for k in ref}
    err32 = {k: float(np.abs(l32[k].astype(np.float64) - ref[k]).max()) / scale[k] for k in ref}
    tdo.check(f"one step {name} n={n} layers={layers} B={B} {'fused' if fuse else 'plain'}", got, ref, err32, scale, tuple(ref))
    assert not o["td"][:, B:].any()


# ---- 3. td_reset and the classes at width ----------------------------------------------------------------------------
def test_td_reset_masked_lanes_at_width(riab):
    """Arrays of 5, 300 (layers) and 257 rows (V, V_last, dV/dt, td) in one launch sized by the tallest: the masked lanes
    < B are zero afterwards, every other element — padded lanes, which the mask also names, and guard rows — keeps its
    bits."""
    from ratinabox_amd import _lib as L
    dev = torch.device("cuda")
    n, layers, B, Bp = 257, [5, 300], 33, 36
    rng = np.random.RandomState(12)
    mask = rng.uniform(size=Bp) < 0.4
    mask[[0, B - 1]] = True
    mask[[1, B - 2]] = False
    mask[B:] = True
    assert 4 < mask[:B].sum() < B - 4

    def array(rows, alloc):
        x = rng.uniform(1.0, 2.0, size=(rows, Bp)).astype(np.float32)
        x[:, B:] = np.nan
        return _guarded(x, alloc, float("nan"), dev)

    traces = [array(k, 384) for k in layers]
    rows = [array(n, 288) for _ in range(4)]
    before = [t[1].clone() for t in traces + rows]
    p = L.RiabTDParams()
    p.dt, p.tau, p.tau_e, p.eta, p.L2, p.B, p.Bp, p.n, p.Mp = 0.05, 1.0, 0.25, 0.01, 0.001, B, Bp, n, 288
    lay = (L.RiabTDLayer * 2)()
    dummy = torch.zeros(16, device=dev)
    for l, k in enumerate(layers):
        lay[l].rates, lay[l].trace, lay[l].wt, lay[l].n_in = dummy.data_ptr(), traces[l][0].data_ptr(), dummy.data_ptr(), k
    ptrs = (C.c_void_p * 4)(*[r[0].data_ptr() for r in rows])
    m = torch.from_numpy(mask.astype(np.uint8)).to(dev)
    L.check(L.lib.riab_td_reset(p, lay, 2, ptrs, 4, L.ptr(m), L.current_stream()), "riab_td_reset")
    torch.cuda.synchronize()
    hit = torch.from_numpy(mask[:B]).to(dev)
    for (view, whole), old, height in zip(traces + rows, before, layers + [n] * 4):
        assert not view[:, :B][:, hit].any(), height
        want = old.clone()
        want[:height, :B][:, hit] = 0.0
        assert torch.equal(_bits(whole), _bits(want)), height
    assert not dummy.any()


def _world(riab, B, successor):
    from ratinabox_amd.contribs.SuccessorFeatures import SuccessorFeatures
    from ratinabox_amd.contribs.ValueNeuron import ValueNeuron
    np.random.seed(13)
    Ag = riab.Agent(riab.Environment({}), {"dt": 0.05, "n_agents": B, "seed": 17})
    if successor:
        PCs = riab.PlaceCells(Ag, {"n": 300, "widths": 0.15, "save_spikes": False})
        VN = SuccessorFeatures(Ag, {"input_layers": [PCs], "features": PCs, "tau": 1.0, "eta": 0.05, "save_spikes": False})
        return Ag, [PCs], [PCs], VN
    PCs = riab.PlaceCells(Ag, {"n": 130, "widths": 0.15, "save_spikes": False})
    HDC = riab.HeadDirectionCells(Ag, {"n": 12, "save_spikes": False})
    R = riab.PlaceCells(Ag, {"n": 1, "place_cell_centres": np.array([[0.5, 0.5]]), "description": "gaussian_threshold",
                             "save_spikes": False})
    VN = ValueNeuron(Ag, {"input_layers": [PCs, HDC], "n": 100, "tau": 1.0, "eta": 0.05, "save_spikes": False})
    return Ag, [PCs, HDC], [PCs, HDC, R], VN


@pytest.mark.parametrize("successor", [False, True], ids=["ValueNeuron-100", "SuccessorFeatures-300"])
def test_classes_at_width(riab, successor):
    """ValueNeuron (n = 100 over 130 PlaceCells + 12 HeadDirectionCells) and SuccessorFeatures over its own basis of 300
    PlaceCells (n = n_in = 300: two row groups), 130 agents, 40 steps of learn(): V, td, traces and weights against
    TDOracle fed with the device's own input rates, and a twin stepped by update(); update_weights() has the same bits."""
    B, T = 130, 40
    snaps = []
    for fused in (True, False):
        Ag, layers, populations, VN = _world(riab, B, successor)
        if fused:
            kw = dict(dt=VN.Agent.dt, tau=VN.tau, tau_e=VN.tau_e, eta=VN.eta, L2=VN.L2, activation="relu", B=B)
            ws = [VN.inputs[l.name]["w"] for l in layers]
            orc, o32 = tdo.TDOracle(ws, **kw), tdo.TDOracle(ws, dtype=np.float32, **kw)
        for t in range(T):
            Ag.update()
            for N in populations:
                N.update()
            reward = None if successor else populations[-1].firingrate_tensor[0]
            if fused:
                VN.learn() if successor else VN.learn(reward)
                phis = [l.firingrate for l in layers]
                r = phis[0] if successor else populations[-1].firingrate.reshape(1, B)
                for o in (orc, o32):
                    o.update(phis)
                    o.update_weights(r)
            else:
                VN.update()
                VN.update_weights() if successor else VN.update_weights(reward)
        snaps.append([VN._rates.clone(), VN._td.clone(), VN._dvdt.clone()] + [VN.inputs[l.name].wt.clone() for l in layers] +
                     [VN.inputs[l.name].trace.clone() for l in layers])
        if fused:
            got = {"V": VN.firingrate, "td": VN.td_error}
            ref, low = {"V": orc.V, "td": orc.td}, {"V": o32.V, "td": o32.td}
            for i, l in enumerate(layers):
                got[f"w{i}"], ref[f"w{i}"], low[f"w{i}"] = VN.inputs[l.name]["w"], orc.ws[i], o32.ws[i]
                got[f"trace{i}"], ref[f"trace{i}"], low[f"trace{i}"] = VN.inputs[l.name]["eligibility_trace"], orc.traces[i], o32.traces[i]
            moved = max(float(np.abs(orc.ws[i] - ws[i]).max() / np.abs(ws[i]).max()) for i in range(len(layers)))
    for x, y in zip(*snaps):
        assert torch.equal(_bits(x), _bits(y))
    assert snaps[0][3].abs().max() > 0
    scale = {k: float(np.abs(ref[k]).max()) for k in ref}
    err32 = {k: float(np.abs(low[k].astype(np.float64) - ref[k]).max()) / scale[k] for k in ref}
    label = "SuccessorFeatures n=300" if successor else "ValueNeuron n=100"
    print(f"[classes at width, {label}] weights moved by {moved:.2e} of their largest in {T} steps")
    tdo.check(f"classes at width, {label}, B={B}, {T} steps", got, ref, err32, scale, tuple(ref))
