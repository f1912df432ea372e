"""Small torch modules shared by tests/golden/make_golden_nn.py (which runs them inside the reference) and the
NeuralNetworkNeurons tests (which rebuild them from the golden files' parameter arrays)."""
import numpy as np
import torch
import torch.nn as nn

# the activation behind each Linear of `mixed_sequential`, in the oracle's names (tests/nn_oracle.py)
MIXED_ACTS = ("tanh", "sigmoid", "softplus", "linear")
MIXED_WIDTHS = (24, 33, 16)


def mixed_sequential(n_in, n_out):
    """Tanh, Sigmoid, Softplus and Identity behind four Linears (the second without bias), one pair nested."""
    a, b, c = MIXED_WIDTHS
    return nn.Sequential(nn.Linear(n_in, a), nn.Tanh(),
                         nn.Linear(a, b, bias=False), nn.Sigmoid(),
                         nn.Sequential(nn.Linear(b, c), nn.Softplus()),
                         nn.Linear(c, n_out), nn.Identity())


class ResidualBlock(nn.Module):
    """Not a plain perceptron: LayerNorm and a skip connection (the torch engine's case)."""

    def __init__(self, n_in, n_out, width=32):
        super().__init__()
        self.inp = nn.Linear(n_in, width)
        self.norm = nn.LayerNorm(width)
        self.mid = nn.Linear(width, width)
        self.out = nn.Linear(width, n_out)

    def forward(self, x):
        h = torch.relu(self.inp(x))
        h = h + torch.tanh(self.mid(self.norm(h)))
        return self.out(h)


def state_arrays(module):
    """{"p::<state_dict key>": float64 array} of every parameter of a module."""
    return {"p::" + k: v.detach().cpu().numpy().astype(np.float64) for k, v in module.state_dict().items()}


def load_arrays(module, g):
    """The inverse: fill `module` (float32) from a golden file's arrays."""
    sd = {k: torch.from_numpy(np.asarray(g["p::" + k])).to(v.dtype) for k, v in module.state_dict().items()}
    module.load_state_dict(sd)
    return module


def linear_layers(g, keys, acts):
    """[(W float64, b float64 or None, activation name)] for the oracle, from a golden file's arrays: `keys` are the
    state_dict prefixes of the Linears in evaluation order."""
    out = []
    for k, act in zip(keys, acts):
        W = np.asarray(g[f"p::{k}.weight"], dtype=np.float64)
        b = np.asarray(g[f"p::{k}.bias"], dtype=np.float64) if f"p::{k}.bias" in g else None
        out.append((W, b, act))
    return out


DEFAULT_KEYS, DEFAULT_ACTS = ("net.0", "net.2", "net.4"), ("relu", "relu", "linear")
MIXED_KEYS = ("0", "2", "4.0", "5")


def module_layers(module_leaves):
    """[(W, b or None, name)] for the oracle from [(nn.Linear, oracle activation name)] pairs (the Linear's CURRENT
    float32 parameters, as float64)."""
    out = []
    for lin, act in module_leaves:
        W = lin.weight.detach().cpu().numpy().astype(np.float64)
        b = None if lin.bias is None else lin.bias.detach().cpu().numpy().astype(np.float64)
        out.append((W, b, act))
    return out
