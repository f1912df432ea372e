"""The networks and launch shapes that tests/test_gpu_mlp_paths.py runs through riab_mlp_forward, as data: the list that is
claimed to reach every form the host chooses (csrc/riab_mlp_logic.h) and every branch the kernel takes on it.  The claim
is checked by code: tests/test_mlp_logic_cpu.py::test_the_cases_reach_every_path feeds every (case, shape) below through
the decision and fails, naming it, for any combination that no case reaches.  Each case is the only one that reaches
something (its `why`): delete one and that test fails.

No torch at import time (the CPU test needs none); `draw` and `operator_args` make a case's arrays and tensors.
"""
import math
from collections import namedtuple

import numpy as np

LINEAR, SIGMOID, RELU, TANH, RETANH, SOFTPLUS = range(6)    # RIAB_ACT_* (SOFTPLUS: RIAB_ACT_SOFTMAX)
DEFAULT_PARAMS = {LINEAR: (0.0, 0.0, 0.0, 0.0), SIGMOID: (1.0, 0.0, 0.0, 1.0), RELU: (1.0, 0.0, 0.0, 0.0),
                  TANH: (1.0, 0.0, 0.0, 0.0), RETANH: (1.0, 0.0, 0.0, 0.0), SOFTPLUS: (1.0, 0.0, 0.0, 0.0)}

# a layer: rows, has a bias, RIAB_ACT_*, its four parameters (None: the defaults), and the element offset of its weight
# matrix in its allocation (1: the base is 4 mod 16 — a view into a flat parameter buffer — and forces 4-byte reads)
Layer = namedtuple("Layer", "n_out bias act params w_off", defaults=(True, LINEAR, None, 0))
Case = namedtuple("Case", "name inputs layers why")

CASES = [
    Case("one_7", (3, 17), [Layer(7)],
         "mlp_kernel<1>; 16-byte reads of a population with K < 4"),
    Case("one_40", (5, 19), [Layer(40, False, RETANH, (1.5, 0.1, 0.0, 0.0))],
         "mlp_first_layer<2> in mlp_kernel<2>; retanh"),
    Case("one_129", (16, 4), [Layer(129, True, SOFTPLUS, (0.7, -0.2, 0.0, 0.0))],
         "two passes, the last with one tile; 16-byte reads at K = 16"),
    Case("one_300", (5, 19, 108), [Layer(300, False)],
         "three passes, the last with two tiles; 16-byte reads at K > 16, ragged"),
    Case("one_228", (3, 17), [Layer(228, True, LINEAR, None, 1)],
         "two passes, the last with four tiles; 4-byte reads at K < 4"),
    Case("one_70_flat", (16, 4), [Layer(70, True, TANH, (2.0, 0.3, 0.0, 0.0), 1)],
         "4-byte reads at K = 16 and at 4 <= K < 16"),
    Case("deep_20_33_130", (3, 17), [Layer(20, True, RELU, (1.25, 0.05, 0.0, 0.0)), Layer(33, False, SOFTPLUS),
                                     Layer(130, True, SIGMOID, (2.0, -1.0, 0.25, 1.5))],
         "mlp_first_layer<1> in mlp_kernel<2>; 4-byte register layer of two tiles behind rows that hold act(0) != 0; bias on, off, on"),
    Case("deep_64_96_1", (5, 19), [Layer(64, False, SIGMOID), Layer(96, True, RELU), Layer(1, False)],
         "mlp_first_layer<2> in mlp_kernel<4>; 16-byte register layers of two and three tiles; bias off, on, off"),
    Case("deep_20_128_65_33", (16, 4), [Layer(20, True, RELU), Layer(128, True, TANH, None, 1), Layer(65, False, SOFTPLUS),
                                        Layer(33, True, LINEAR)],
         "mlp_first_layer<1> in mlp_kernel<4>; 4-byte register layer of one tile (flat) and of three; 16-byte of four"),
    Case("deep_128_300_flat", (5, 19, 108), [Layer(128, True, RELU), Layer(300, True, LINEAR, None, 1)],
         "4-byte register layer of four tiles"),
]

BATCHES = (4, 36, 132)       # less than one tile; a tile plus a quad at one wave; two four-wave tiles or five one-wave ones
T_ONE_WAVE = 2


def n_in(case):
    return sum(case.inputs)


def widths(case):
    """[(n_in, n_out)] per layer"""
    out, k = [], n_in(case)
    for L in case.layers:
        out.append((k, L.n_out))
        k = L.n_out
    return out


def params(layer):
    return tuple(float(p) for p in (layer.params if layer.params is not None else DEFAULT_PARAMS[layer.act]))


def expected_nw(T, B, cus):
    """the header comment of csrc/riab_mlp.hip: four waves iff ceil(B / 128) * T covers the chip's compute units"""
    return 4 if -(-B // 128) * T >= cus else 1


def launch_shapes(cus):
    """[(nw, T, B)]: every B at the one-wave block (T = 2) and at the four-wave block (the fewest rows that give it)"""
    out = []
    for B in BATCHES:
        out.append((1, T_ONE_WAVE, B))
        out.append((4, -(-cus // -(-B // 128)), B))
    for nw, T, B in out:
        assert expected_nw(T, B, cus) == nw, (nw, T, B, cus)
    return out


def facts_line(case, T, B, cus, flat=False):
    """the case as a line of facts for tests/native/mlp_logic_host.cpp (flat: every weight base 4 mod 16)"""
    words = [f"in={n}" for n in case.inputs]
    for (k, m), L in zip(widths(case), case.layers):
        words.append(f"layer={k}:{m}:{int(L.bias)}:{L.act}:{4 if (flat or L.w_off) else 0}")
    return " ".join(words + [f"T={T}", f"B={B}", f"cus={cus}"])


def place(w, off, device):
    """float32 array -> a contiguous device tensor of its shape whose first element lies `off` elements into a 256-byte
    aligned allocation"""
    import torch
    flat = torch.zeros(w.size + 8, dtype=torch.float32, device=device)
    assert flat.data_ptr() % 16 == 0
    v = flat[off:off + w.size].view(w.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(w)))
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def draw(case, seed):
    """weights and biases as nn.Linear draws them (float32 arrays): [(W, b or None)]"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    out = []
    for (k, m), L in zip(widths(case), case.layers):
        bound = 1.0 / math.sqrt(k)            # kaiming_uniform_(a = sqrt(5)) and the bias: both U(-1 / sqrt(n_in), 1 / sqrt(n_in))
        W = ((torch.rand(m, k, generator=gen) * 2 - 1) * bound).numpy()
        b = ((torch.rand(m, generator=gen) * 2 - 1) * bound).numpy() if L.bias else None
        out.append((W, b))
    return out


def operator_args(case, arrays, device, flat=False):
    """(weights, biases, activations, act_params) of torch.ops.riab.mlp_forward for the case's arrays"""
    import torch
    ws = [place(W, 1 if (flat or L.w_off) else 0, device) for (W, _b), L in zip(arrays, case.layers)]
    bs = [None if b is None else torch.from_numpy(b).to(device) for _W, b in arrays]
    acts = [L.act for L in case.layers]
    pars = [p for L in case.layers for p in params(L)]
    return ws, bs, acts, pars


def oracle_layers(case, arrays):
    """the case for tests/nn_oracle.forward"""
    return [(W.astype(np.float64), None if b is None else b.astype(np.float64), (L.act,) + params(L))
            for (W, b), L in zip(arrays, case.layers)]
