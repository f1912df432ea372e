"""GPU tests of contribs.NeuralNetworkNeurons and its fused kernel (riab_mlp_forward, csrc/riab_mlp.hip): the reference's
goldens, random shapes against the float64 oracle (tests/nn_oracle.py: its docstring derives the bound), per-step ==
streamed, training through `firingrate_torch` with the weights read in place, use as an input layer, and the operator."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import riab_oracle as orc
from tests import golden_util as gu
from tests import nn_modules, nn_oracle

pytestmark = pytest.mark.gpu

ACT_LEAF = {"linear": None, "relu": nn.ReLU, "tanh": nn.Tanh, "sigmoid": nn.Sigmoid, "softplus": nn.Softplus}


@pytest.fixture(scope="module")
def riab():
    assert torch.cuda.is_available(), "these tests need the GPU"
    import ratinabox_amd
    return ratinabox_amd


@pytest.fixture(scope="module")
def NNN():
    from ratinabox_amd.contribs.NeuralNetworkNeurons import NeuralNetworkNeurons
    return NeuralNetworkNeurons


def _world(riab, g, n_agents=1):
    Ag = riab.Agent(riab.Environment({}), {"dt": 0.05, "n_agents": n_agents})
    PCs = riab.PlaceCells(Ag, {"place_cell_centres": g["pc_centres"], "name": "PCs", "wall_geometry": "euclidean"})
    GCs = riab.GridCells(Ag, {"gridscale": list(g["gc_gridscales"]), "orientation": list(g["gc_orient"]),
                              "phase_offset": g["gc_phase"], "name": "GCs"})
    return Ag, PCs, GCs


def _linears(module):
    return [m for m in module.modules() if type(m) is nn.Linear]


def _sequential(widths, acts, biases):
    """nn.Sequential of Linears widths[i] -> widths[i+1] with the named activation behind each."""
    mods = []
    for i, (act, bias) in enumerate(zip(acts, biases)):
        mods.append(nn.Linear(widths[i], widths[i + 1], bias=bias))
        if ACT_LEAF[act] is not None:
            mods.append(ACT_LEAF[act]())
    return nn.Sequential(*mods)


def _within(got, ref, tol, what=""):
    err = np.abs(np.asarray(got) - np.asarray(ref))
    print(f"{what}: max err {err.max():.3g}, max err / bound {(err / tol).max():.3g}")
    assert got.shape == ref.shape
    assert (err <= tol).all(), (what, err.max(), (err / tol).max())


# ------------------------------------------------------------------------------------------------------ goldens
def _golden_module(name, g):
    from ratinabox_amd.contribs.NeuralNetworkNeurons import MultiLayerPerceptron
    if name == "default_mlp":
        return nn_modules.load_arrays(MultiLayerPerceptron(50, 16, [20, 20]), g), nn_modules.DEFAULT_KEYS, nn_modules.DEFAULT_ACTS
    if name == "sequential":
        return nn_modules.load_arrays(nn_modules.mixed_sequential(50, 16), g), nn_modules.MIXED_KEYS, nn_modules.MIXED_ACTS
    return nn_modules.load_arrays(nn_modules.ResidualBlock(50, 16), g), None, None


def _custom_bound(g, x):
    """The bound for the module that is no layer list (x: (n_in, P) float64 inputs).  The torch engine evaluates the
    same fp32 module as the reference did, on inputs that differ by at most 1e-5 per rate: the input error goes through the
    module's float64 Jacobian |J| @ 1e-5, and each of the two fp32 evaluations is allowed 8 x the reference's own
    largest distance from the float64 evaluation of the module on the reference's inputs (stored in the golden file)."""
    m64 = nn_modules.load_arrays(nn_modules.ResidualBlock(50, 16), g).double()
    xt = torch.from_numpy(np.ascontiguousarray(x.T))
    J = torch.func.vmap(torch.func.jacrev(lambda v: m64(v[None])[0]))(xt).detach().abs().sum(-1).numpy().T      # (n, P)
    with torch.no_grad():
        e_ref = np.abs(m64(torch.from_numpy(np.ascontiguousarray(g["inputs"].T))).numpy().T - g["fr"]).max()
    return 1e-5 * J + 16 * e_ref


@pytest.mark.parametrize("name,engine", [("default_mlp", "fused"), ("sequential", "fused"), ("custom", "torch")])
def test_goldens_vs_reference(riab, NNN, name, engine):
    g = gu.load(f"nn_{name}.npz")
    module, keys, acts = _golden_module(name, g)
    Ag, PCs, GCs = _world(riab, g)
    N = NNN(Ag, {"input_layers": [PCs, GCs], "NeuralNetworkModule": module})
    assert N.engine == engine and N.n == 16 and N.n_in == 50
    got = N.get_state(evaluate_at=None, pos=g["pos"])
    if keys is not None:
        layers = nn_modules.linear_layers(g, keys, acts)
        tol = nn_oracle.forward(layers, g["inputs"], tol0=1e-5)[1]
        tol1 = nn_oracle.forward(layers, g["last_inputs"], tol0=1e-5)[1][:, 0]
    else:
        tol, tol1 = _custom_bound(g, g["inputs"]), _custom_bound(g, g["last_inputs"][:, None])[:, 0]
    _within(got, g["fr"], tol, f"{name} get_state")
    assert N.engine == engine
    Ag.pos = g["agent_pos"]
    PCs.update(); GCs.update(); N.update()
    _within(N.firingrate, g["last"], tol1, f"{name} update")
    assert N.history["firingrate"].shape == (1, 16) and N.history["spikes"].shape == (1, 16)
    # "last" is the default of get_state, (n, P) in the product's convention
    assert np.array_equal(N.get_state()[:, 0], N.firingrate) and N.get_state().shape == (16, 1)


# ------------------------------------------------------------------------------------------------------ random shapes
def _draw(rs):
    n_inputs = int(rs.randint(1, 4))
    in_widths = [int(rs.choice([1, 3, 15, 16, 17, 100, 257])) for _ in range(n_inputs)]
    depth = int(rs.choice([1, 2, 3, 8]))
    hidden = [int(rs.choice([1, 20, 31, 32, 33, 64, 65, 127, 128])) for _ in range(depth - 1)]
    n_out = int(rs.choice([1, 5, 33, 128, 129, 300]))
    P = int(rs.choice([1, 7, 127, 128, 129, 500]))
    acts = [str(rs.choice(["linear", "relu", "tanh", "sigmoid", "softplus"])) for _ in range(depth)]
    biases = [bool(rs.uniform() >= 0.25) for _ in range(depth)]
    return in_widths, hidden, n_out, P, acts, biases


def _random_case(riab, NNN, seed, in_widths, hidden, n_out, P, acts, biases, rs):
    np.random.seed(seed)
    torch.manual_seed(seed)
    Ag = riab.Agent(riab.Environment({}))
    layers = [(riab.PlaceCells if i % 2 == 0 else riab.GridCells)(Ag, {"n": w, "name": f"in{i}"})
              for i, w in enumerate(in_widths)]
    module = _sequential([sum(in_widths)] + hidden + [n_out], acts, biases)
    N = NNN(Ag, {"input_layers": layers, "NeuralNetworkModule": module})
    pos = rs.uniform(0, 1, (P, 2)).astype(np.float32).astype(np.float64)
    ins = np.concatenate([L_.get_state(evaluate_at=None, pos=pos) for L_ in layers])          # the kernels' own fp32 rates
    got = N.get_state(evaluate_at=None, pos=pos)
    ref, tol = nn_oracle.forward(nn_modules.module_layers(list(zip(_linears(module), acts))), ins)
    assert got.shape == (n_out, P)
    return N, got, ref, tol


@pytest.mark.parametrize("seed", range(8))
def test_randomised_shapes_vs_oracle(riab, NNN, seed):
    rs = np.random.RandomState(8770 + seed)     # (a base whose 8 draws cover every depth, hidden width and position count)
    case = _draw(rs)
    N, got, ref, tol = _random_case(riab, NNN, seed, *case, rs)
    assert N.engine == "fused", case
    _within(got, ref, tol, str(case))


def test_hidden_width_129_runs_on_torch_within_the_same_bound(riab, NNN):
    rs = np.random.RandomState(7200)
    N, got, ref, tol = _random_case(riab, NNN, 11, [17, 100], [129], 33, 129, ["tanh", "linear"], [True, True], rs)
    assert N.engine == "torch"
    _within(got, ref, tol, "hidden 129")


# ------------------------------------------------------------------------------------------------------ per-step == streamed
def _twin(riab, NNN, g, engine, **extra):
    np.random.seed(3)
    torch.manual_seed(5)
    Ag, PCs, GCs = _world(riab, g, n_agents=300)
    N = NNN(Ag, dict({"n": 16, "input_layers": [PCs, GCs], "engine": engine}, **extra))
    return Ag, PCs, GCs, N


@pytest.mark.parametrize("engine", ["auto", "torch"])
def test_per_step_and_streamed_agree(riab, NNN, engine):
    g = gu.load("nn_default_mlp.npz")
    with pytest.warns(UserWarning, match="default MLP"):
        Ag, PCs, GCs, N = _twin(riab, NNN, g, engine)
        Ag2, P2, G2, N2 = _twin(riab, NNN, g, engine)
    assert N.engine == N2.engine == ("fused" if engine == "auto" else "torch")
    for _ in range(9):
        Ag.update(); PCs.update(); GCs.update(); N.update()
    Ag2.simulate(9, chunk=4)
    torch.cuda.synchronize()
    assert Ag2.engine_runs["chunks"] == 1
    fr, fr2 = N.history["firingrate"], N2.history["firingrate"]
    assert fr.shape == fr2.shape == (9, 16, 300) and N2.history["spikes"].shape == (9, 16, 300)
    assert np.array_equal(PCs.history["firingrate"], P2.history["firingrate"])
    if engine == "auto":
        assert np.array_equal(fr2, fr)
        assert np.array_equal(N2.history["spikes"], N.history["spikes"])
    else:
        np.testing.assert_allclose(fr2, fr, rtol=2e-5, atol=2e-5)
    assert np.array_equal(N2.firingrate, fr2[-1]) and len(N2.history["t"]) == 9


def test_noise_advances_on_both_paths(riab, NNN):
    g = gu.load("nn_default_mlp.npz")
    with pytest.warns(UserWarning, match="default MLP"):
        Ag, PCs, GCs, N = _twin(riab, NNN, g, "auto", noise_std=0.1)
    for _ in range(3):
        Ag.update(); PCs.update(); GCs.update(); N.update()
    noise_a = N.noise.copy()
    assert np.isfinite(N.firingrate).all() and np.abs(noise_a).max() > 0
    Ag.simulate(5, chunk=4)
    torch.cuda.synchronize()
    assert N.history["firingrate"].shape == (8, 16, 300) and np.isfinite(N.history["firingrate"]).all()
    assert not np.array_equal(N.noise, noise_a)


# ------------------------------------------------------------------------------------------------------ training
def test_training_sees_through(riab, NNN):
    g = gu.load("nn_default_mlp.npz")
    np.random.seed(4)
    torch.manual_seed(6)
    Ag, PCs, GCs = _world(riab, g, n_agents=37)
    with pytest.warns(UserWarning, match="default MLP"):
        N = NNN(Ag, {"n": 16, "input_layers": [PCs, GCs]})
    module = N.NeuralNetworkModule
    lin = _linears(module)
    acts = nn_modules.DEFAULT_ACTS
    opt = torch.optim.Adam(module.parameters(), lr=1e-2)
    Ag.update(); PCs.update(); GCs.update(); N.update()
    assert N.engine == "fused"
    before = N.firingrate.copy()
    y = N.firingrate_torch
    assert tuple(y.shape) == (37, 16) and y.is_cuda and y.requires_grad
    np.testing.assert_allclose(y.detach().cpu().numpy().T, before, rtol=2e-5, atol=2e-5)
    opt.zero_grad()
    y.sum().backward()
    for q in module.parameters():
        assert q.grad is not None and float(q.grad.abs().max()) > 0
    opt.step()
    ins = np.concatenate([PCs.firingrate, GCs.firingrate])

    def check(what):
        N.update()                     # (no refresh call: the kernel reads the parameters where they are)
        ref, tol = nn_oracle.forward(nn_modules.module_layers(list(zip(lin, acts))), ins)
        _within(N.firingrate, ref, tol, what)
        return N.firingrate.copy()
    after = check("after the Adam step")
    assert not np.array_equal(after, before)
    with torch.no_grad():
        lin[0].weight[0].zero_()
        lin[0].bias[0] = 0.0
    dropped = check("row 0 zeroed")
    assert not np.array_equal(dropped, after)
    with torch.no_grad():              # unit 0 of the first layer is now exactly relu(0) = 0: what it feeds cannot matter
        lin[1].weight[:, 0] = 123.0
    assert np.array_equal(check("column 0 of the next layer"), dropped)
    # get_state(save_torch=True) stores the attached (P, n) result until the next update()
    pos = g["pos"][:10]
    fr = N.get_state(evaluate_at=None, pos=pos, save_torch=True)
    assert tuple(N.firingrate_torch.shape) == (10, 16) and N.firingrate_torch.requires_grad
    np.testing.assert_allclose(N.firingrate_torch.detach().cpu().numpy().T, fr, rtol=2e-5, atol=2e-5)
    N.update()
    assert tuple(N.firingrate_torch.shape) == (37, 16)


# ------------------------------------------------------------------------------------------------------ downstream
def test_as_an_input_of_a_feedforward_layer(riab, NNN):
    g = gu.load("nn_sequential.npz")
    module, _k, _a = _golden_module("sequential", g)
    np.random.seed(8)
    Ag, PCs, GCs = _world(riab, g, n_agents=5)
    N = NNN(Ag, {"input_layers": [PCs, GCs], "NeuralNetworkModule": module, "name": "NN"})
    F = riab.FeedForwardLayer(Ag, {"n": 7, "input_layers": [N], "activation_function": {"activation": "linear"}})
    for _ in range(2):
        Ag.update(); PCs.update(); GCs.update(); N.update(); F.update()
    w = F.inputs["NN"]["w"]
    ref, _ = orc.feedforward([N.firingrate], [w], F.biases, {"activation": "linear"})
    x = N.firingrate
    tol = 2e-6 * (np.abs(w) @ np.abs(x) + np.abs(np.asarray(F.biases))[:, None]) + 1e-6 * np.abs(ref)
    _within(F.firingrate, ref, tol, "FeedForwardLayer(NN)")


# ------------------------------------------------------------------------------------------------------ operator
def test_operator(riab):
    from ratinabox_amd import ops  # noqa: F401
    torch.manual_seed(9)
    dev = "cuda"
    seq = _sequential([19, 33, 20, 130], ["tanh", "softplus", "sigmoid"], [True, False, True]).to(dev)
    lin = _linears(seq)
    ws, bs = [m.weight.detach() for m in lin], [None if m.bias is None else m.bias.detach() for m in lin]
    acts = [3, 5, 1]
    pars = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    xs = [torch.rand(2, 3, 8, device=dev), torch.rand(2, 16, 8, device=dev)]
    torch.library.opcheck(torch.ops.riab.mlp_forward.default, (xs, ws, bs, acts, pars))
    # one direct call against nn.Sequential; T x ceil(B / 128) >= the chip's 256 compute units: the four-wave tile
    T, B = 96, 388
    xs = [torch.rand(T, 3, B, device=dev), torch.rand(T, 16, B, device=dev)]
    got = torch.ops.riab.mlp_forward(xs, ws, bs, acts, pars)
    assert tuple(got.shape) == (T, 130, B)
    x = torch.cat(xs, dim=1)
    with torch.no_grad():
        ref = seq(x.permute(0, 2, 1).reshape(T * B, 19)).reshape(T, B, 130).permute(0, 2, 1)
    h0 = x.permute(1, 0, 2).reshape(19, T * B).cpu().numpy().astype(np.float64)
    _o, tol = nn_oracle.forward(nn_modules.module_layers(list(zip(lin, ["tanh", "softplus", "sigmoid"]))), h0)
    tol = tol.reshape(130, T, B).transpose(1, 0, 2)
    _within(got.cpu().numpy(), ref.cpu().numpy(), tol, "operator vs nn.Sequential")
    # determinism: a row launched alone (one-wave tile) has the bits of the same row inside the many-row launch
    for t in (0, 41, T - 1):
        one = torch.ops.riab.mlp_forward([v[t:t + 1].contiguous() for v in xs], ws, bs, acts, pars)
        assert torch.equal(one[0], got[t])
    few = torch.ops.riab.mlp_forward([v[:, :, :132].contiguous() for v in xs], ws, bs, acts, pars)
    assert torch.equal(few, got[:, :, :132])
