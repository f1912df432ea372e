"""No-GPU checks of contribs.NeuralNetworkNeurons: the float64 oracle against the reference's goldens, the constructor's
semantics, the host-side lowering of a torch module to the fused kernel's layer list, and the C ABI of riab_mlp_forward."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch.nn as nn

from tests import golden_util as gu
from tests import nn_modules, nn_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = {"device": "cpu", "n_agents": 3}


@pytest.fixture(scope="module")
def riab():
    import ratinabox_amd
    return ratinabox_amd


@pytest.fixture(scope="module")
def nnn():
    from ratinabox_amd.contribs import NeuralNetworkNeurons as mod
    return mod


def _world(riab, widths=(30, 20)):
    Ag = riab.Agent(riab.Environment({}), dict(CPU))
    layers = [riab.PlaceCells(Ag, {"n": w, "name": f"in{i}"}) for i, w in enumerate(widths)]
    return Ag, layers


def _make(riab, nnn, module, widths=(30, 20), **extra):
    Ag, layers = _world(riab, widths)
    return nnn.NeuralNetworkNeurons(Ag, dict({"input_layers": layers, "NeuralNetworkModule": module}, **extra))


# ----------------------------------------------------------------------------------------------- oracle vs reference
@pytest.mark.parametrize("name,keys,acts", [("default_mlp", nn_modules.DEFAULT_KEYS, nn_modules.DEFAULT_ACTS),
                                            ("sequential", nn_modules.MIXED_KEYS, nn_modules.MIXED_ACTS)])
def test_oracle_matches_the_reference_within_the_bound(name, keys, acts):
    g = gu.load(f"nn_{name}.npz")
    layers = nn_modules.linear_layers(g, keys, acts)
    ref, tol = nn_oracle.forward(layers, g["inputs"])
    assert ref.shape == g["fr"].shape == (16, 256)
    err = np.abs(ref - g["fr"])
    assert (err <= tol).all(), (err / tol).max()
    ref1, tol1 = nn_oracle.forward(layers, g["last_inputs"])
    assert (np.abs(ref1[:, 0] - g["last"]) <= tol1[:, 0]).all()
    assert (tol > 0).all() and tol.max() < 1e-4        # (the bound is a few ulps of O(1) rates, not a free pass)


def test_oracle_sequential_has_a_bias_free_layer():
    g = gu.load("nn_sequential.npz")
    assert "p::2.weight" in g and "p::2.bias" not in g and "p::0.bias" in g


# (code, p0, p1, p2, p3) off the defaults: RIAB_ACT_* sigmoid, relu, tanh, retanh, softplus, and linear (which ignores them)
CODED = [(1, 2.0, -0.5, 0.3, 1.7), (1, -1.0, 2.0, -0.4, -3.0), (2, 1.5, 0.2, 0.0, 0.0), (2, -0.7, -0.3, 0.0, 0.0),
         (3, 0.8, -0.1, 0.0, 0.0), (4, 1.3, 0.15, 0.0, 0.0), (5, 0.6, -0.3, 0.0, 0.0), (5, -2.5, 0.4, 0.0, 0.0),
         (0, 3.0, 1.0, 0.5, 2.0)]


@pytest.mark.parametrize("act", CODED, ids=lambda a: "-".join(str(v) for v in a))
def test_lipschitz_constants_by_finite_differences(act):
    """nn_oracle.lipschitz for the kernel's (code, p0..p3): no float64 central difference on a fine grid exceeds it, and
    the largest comes within 1 % of it (the constant is the supremum, not merely a bound)."""
    lip = nn_oracle.lipschitz(act)
    x = np.linspace(-40.0, 40.0, 800001)          # 1e-4 apart: the retanh supremum sits just right of its threshold
    h = 1e-6
    slope = np.abs(nn_oracle.activate(act, x + h) - nn_oracle.activate(act, x - h)) / (2 * h)
    assert slope.max() <= lip * (1 + 1e-6), (slope.max(), lip)
    assert slope.max() >= 0.99 * lip, (slope.max(), lip)


def test_coded_activations_at_their_defaults_are_the_named_ones():
    x = np.linspace(-30.0, 30.0, 6001)
    for name, code, pars in (("linear", 0, (0.0, 0.0, 0.0, 0.0)), ("sigmoid", 1, (1.0, 0.0, 0.0, 1.0)), ("relu", 2, (1.0, 0.0, 0.0, 0.0)),
                             ("tanh", 3, (1.0, 0.0, 0.0, 0.0)), ("softplus", 5, (1.0, 0.0, 0.0, 0.0))):
        assert np.array_equal(nn_oracle.activate((code,) + pars, x), nn_oracle.activate(name, x)), name
        assert nn_oracle.lipschitz((code,) + pars) == nn_oracle.LIP[name]
    assert np.array_equal(nn_oracle.activate((4, 1.0, 0.0, 0.0, 0.0), x), np.maximum(np.tanh(x), 0.0))


# ----------------------------------------------------------------------------------------------- constructor
def test_n_from_the_module_and_n_in(riab, nnn):
    N = _make(riab, nnn, nn.Sequential(nn.Linear(50, 7)))
    assert N.n == 7 and N.n_in == 50 and N._rates.shape == (7, N._Bp)
    assert N.firingrate.shape == (7, 3) and N.Agent.Neurons[-1] is N


def test_default_mlp_and_its_warning(riab, nnn):
    Ag, layers = _world(riab)
    with pytest.warns(UserWarning, match="default MLP with 50 inputs, 16 outputs and 2 hidden ReLU layers of size 20"):
        N = nnn.NeuralNetworkNeurons(Ag, {"n": 16, "input_layers": layers})
    assert type(N.NeuralNetworkModule) is nnn.MultiLayerPerceptron
    shapes = [tuple(m.weight.shape) for m in N.NeuralNetworkModule.net if isinstance(m, nn.Linear)]
    assert shapes == [(20, 50), (20, 20), (16, 20)]
    assert [type(m) for m in N.NeuralNetworkModule.net] == [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear]
    assert N.n == 16 and N.engine == "fused"


def test_both_or_neither_is_a_value_error(riab, nnn):
    Ag, layers = _world(riab)
    before = len(Ag.Neurons)
    with pytest.raises(ValueError, match="both 'n' and `NeuralNetworkModule`"):
        nnn.NeuralNetworkNeurons(Ag, {"n": 4, "input_layers": layers, "NeuralNetworkModule": nn.Linear(50, 4)})
    with pytest.raises(ValueError, match="neither a 'NeuralNetworkModule' nor 'n'"):
        nnn.NeuralNetworkNeurons(Ag, {"input_layers": layers})
    assert len(Ag.Neurons) == before       # (nothing half-constructed was attached)


def test_wrong_input_size_is_a_value_error(riab, nnn):
    Ag, layers = _world(riab)
    with pytest.raises(ValueError, match=r"does not accept inputs of size \(1,50\)"):
        nnn.NeuralNetworkNeurons(Ag, {"input_layers": layers, "NeuralNetworkModule": nn.Linear(49, 4)})


def test_parameters_keep_their_identity(riab, nnn):
    m = nnn.MultiLayerPerceptron(50, 4)
    ids = [id(q) for q in m.parameters()]
    N = _make(riab, nnn, m)
    assert N.NeuralNetworkModule is m and [id(q) for q in m.parameters()] == ids


# ----------------------------------------------------------------------------------------------- lowering
RELU, TANH, SIGM, SOFTPLUS, LINEAR = 2, 3, 1, 5, 0


def test_lowering_accepts_plain_perceptrons(riab, nnn, L):
    assert (L.ACTIVATIONS["relu"], L.ACTIVATIONS["tanh"], L.ACTIVATIONS["sigmoid"], L.ACTIVATIONS["softmax"],
            L.ACTIVATIONS["linear"]) == (RELU, TANH, SIGM, SOFTPLUS, LINEAR)
    N = _make(riab, nnn, nnn.MultiLayerPerceptron(50, 16, [20, 20]))
    got = N.lowered_layers()
    assert N.engine == "fused"
    assert [(s, a, p) for s, a, p, _b in got] == [((20, 50), RELU, (1.0, 0.0, 0.0, 0.0)), ((20, 20), RELU, (1.0, 0.0, 0.0, 0.0)),
                                                   ((16, 20), LINEAR, (0.0, 0.0, 0.0, 0.0))]
    lin = [m for m in N.NeuralNetworkModule.net if isinstance(m, nn.Linear)]
    assert all(b is m.bias for (_s, _a, _p, b), m in zip(got, lin))

    N = _make(riab, nnn, nn_modules.mixed_sequential(50, 16))
    got = N.lowered_layers()
    assert N.engine == "fused"
    assert [(s, a, p) for s, a, p, _b in got] == [((24, 50), TANH, (1.0, 0.0, 0.0, 0.0)), ((33, 24), SIGM, (1.0, 0.0, 0.0, 1.0)),
                                                   ((16, 33), SOFTPLUS, (1.0, 0.0, 0.0, 0.0)), ((16, 16), LINEAR, (0.0, 0.0, 0.0, 0.0))]
    assert got[1][3] is None and got[0][3] is not None      # (the Linear without bias)

    nested = nn.Sequential(nn.Sequential(nn.Linear(50, 128), nn.ReLU()), nn.Sequential(nn.Sequential(nn.Linear(128, 9))),
                           nnn.MultiLayerPerceptron(9, 300, [5]))
    N = _make(riab, nnn, nested)
    assert N.engine == "fused" and N.n == 300
    assert [(s, a) for s, a, _p, _b in N.lowered_layers()] == [((128, 50), RELU), ((9, 128), LINEAR), ((5, 9), RELU),
                                                              ((300, 5), LINEAR)]


@pytest.fixture(scope="module")
def L():
    from ratinabox_amd import _lib
    return _lib


def _deep(n_linear):
    mods = [nn.Linear(50, 8)]
    for _ in range(n_linear - 1):
        mods += [nn.ReLU(), nn.Linear(8, 8)]
    return nn.Sequential(*mods)


@pytest.mark.parametrize("case", ["residual", "activation_first", "two_activations", "hidden_129", "nine_linears", "double",
                                  "softplus_beta", "engine_torch"])
def test_lowering_refuses(riab, nnn, case):
    extra = {}
    if case == "residual":
        m = nn_modules.ResidualBlock(50, 16)
    elif case == "activation_first":
        m = nn.Sequential(nn.Tanh(), nn.Linear(50, 4))
    elif case == "two_activations":
        m = nn.Sequential(nn.Linear(50, 4), nn.ReLU(), nn.Tanh())
    elif case == "hidden_129":
        m = nn.Sequential(nn.Linear(50, 129), nn.ReLU(), nn.Linear(129, 4))
    elif case == "nine_linears":
        m = _deep(9)
    elif case == "double":
        m = nnn.MultiLayerPerceptron(50, 4).double()
    elif case == "softplus_beta":
        m = nn.Sequential(nn.Linear(50, 4), nn.Softplus(beta=2))
    else:
        m, extra = nnn.MultiLayerPerceptron(50, 4), {"engine": "torch"}
    N = _make(riab, nnn, m, **extra)
    assert N.engine == "torch" and N.lowered_layers() is None
    assert N.n == {"residual": 16, "nine_linears": 8}.get(case, 4)


def test_lowering_limits_are_the_kernels(riab, nnn):
    assert _make(riab, nnn, _deep(8)).engine == "fused"                         # eight Linears: the limit itself
    N = _make(riab, nnn, nn.Sequential(nn.Linear(50, 128), nn.Linear(128, 129)))  # a wide LAST layer is fine
    assert N.engine == "fused" and N.n == 129
    N.NeuralNetworkModule.double()                                               # decided per call, not at construction
    assert N.engine == "torch"
    N.NeuralNetworkModule.float()
    assert N.engine == "fused"


def test_no_step_plan(riab, nnn):
    N = _make(riab, nnn, nn.Linear(50, 4))
    with pytest.raises(NotImplementedError):
        N._population()
    with pytest.raises(NotImplementedError):
        N.Agent.make_step_plan()


# ----------------------------------------------------------------------------------------------- ABI
def test_abi_symbol_header_binding_and_docs(L):
    header = open(os.path.join(ROOT, "include", "riab_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\briab_mlp_forward\s*\(", code) and "riab_mlp_forward" in L.PROTOTYPES
    assert hasattr(L.lib, "riab_mlp_forward")
    assert "riab_mlp_forward" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert L.ABI_VERSION == 11 and L.lib.riab_abi_version() == 11
    assert int(re.search(r"#define RIAB_ABI_VERSION (\d+)", header).group(1)) == 11
    assert L.RiabPopulation._fields_[-1][0] == "kappa"
    assert L.lib.riab_abi_sizeof(11) == C.sizeof(L.RiabMLPLayer) == 48
    assert int(re.search(r"#define RIAB_MLP_MAX_LAYERS (\d+)", header).group(1)) == L.MLP_MAX_LAYERS == 8
    assert int(re.search(r"#define RIAB_MLP_MAX_HIDDEN (\d+)", header).group(1)) == L.MLP_MAX_HIDDEN == 128


def _call(L, widths, layers, T=1, B=8, inputs=None, out=64, input_n=None, n_inputs=None, n_layers=None, null_layers=False):
    """riab_mlp_forward with dummy non-null device pointers: validation only.  layers: [(n_in, n_out, act)]."""
    n = len(widths)
    ptrs = (C.c_void_p * max(n, 1))(*(inputs if inputs is not None else [64 + 16 * i for i in range(n)]))
    wn = (C.c_int32 * max(n, 1))(*(input_n if input_n is not None else widths))
    arr = (L.RiabMLPLayer * max(len(layers), 1))()
    for q, (n_in, n_out, act) in zip(arr, layers):
        q.w, q.bias, q.n_in, q.n_out, q.activation = 64, None, n_in, n_out, act
    return L.lib.riab_mlp_forward(ptrs, wn, n if n_inputs is None else n_inputs, None if null_layers else arr,
                                  len(layers) if n_layers is None else n_layers, T, B, C.c_void_p(out) if out else None, None)


def test_abi_validation_before_any_launch(L):
    ok = [(10, 20, 2), (20, 4, 0)]
    EINVAL, EALIGN, ETOOBIG = L.EINVAL, L.EALIGN, L.ETOOBIG
    # null pointers, non-positive sizes
    assert L.lib.riab_mlp_forward(None, None, 1, None, 1, 1, 8, None, None) == EINVAL
    assert _call(L, [10], ok, out=0) == EINVAL and _call(L, [10], ok, null_layers=True) == EINVAL
    assert _call(L, [10], ok, inputs=[0]) == EINVAL
    assert _call(L, [10], ok, T=0) == EINVAL and _call(L, [10], ok, B=0) == EINVAL and _call(L, [10], ok, B=-4) == EINVAL
    assert _call(L, [10], ok, n_inputs=0) == EINVAL and _call(L, [10], ok, n_layers=0) == EINVAL
    assert _call(L, [4, 0, 6], ok) == EINVAL and _call(L, [10], [(10, 0, 0)]) == EINVAL
    # a broken width chain, inputs that do not add up to the first layer's n_in, an unknown activation
    assert _call(L, [10], [(10, 20, 2), (21, 4, 0)]) == EINVAL
    assert _call(L, [4, 5], ok) == EINVAL and _call(L, [11], ok) == EINVAL
    assert _call(L, [10], [(10, 20, 6)]) == EINVAL and _call(L, [10], [(10, 20, -1)]) == EINVAL
    # alignment
    assert _call(L, [10], ok, B=6) == EALIGN
    assert _call(L, [10], ok, inputs=[68]) == EALIGN and _call(L, [10], ok, out=72) == EALIGN
    # limits
    assert _call(L, [1] * 9, [(9, 4, 0)]) == ETOOBIG
    assert _call(L, [10], [(10, 8, 2)] + [(8, 8, 2)] * 8) == ETOOBIG
    assert _call(L, [10], [(10, 129, 2), (129, 4, 0)]) == ETOOBIG
    assert _call(L, [10], ok, T=65536) == ETOOBIG
