"""The fused MLP kernel (riab_mlp_forward, csrc/riab_mlp.hip) on every launch path, through torch.ops.riab.mlp_forward.

Which paths there are is csrc/riab_mlp_logic.h; that the networks of tests/mlp_path_cases.py reach all of them is checked
without a GPU by tests/test_mlp_logic_cpu.py.  Here they run:

 (a) one layer, one-hot inputs, linear: out == fp32(W[m][k] + bias[m]) on every bit (mlp_first_layer's fetch, stash, k
     mapping and passes; mlp_finish's bias row and store);
 (b) several layers whose hidden weights are 0/1 selection matrices: a one-hot input stays one-hot, and the last layer gives
     fp32(W_L[m][p] + bias_L[m]) on every bit (mlp_reg_tile's k mapping, for one to four tiles of the layer before);
 (c) every case with random inputs against the float64 oracle under its own bound (tests/nn_oracle.py: the 2e-6 and 1e-6
     coefficients as they were);
 (d) the six activations with parameters off their defaults, as a hidden and as the last activation;
 (e) bits that must not depend on the form: a row of a four-wave launch == the row launched alone at one wave; weights at a
     base that is 4 mod 16 (4-byte reads) == the aligned weights;
 (f) guard bands around the output of the four-wave block.

Shapes: B of 4, 36 and 132 with the last lane a padding lane that holds NaN (only lanes < B - 1 are compared); T = 2 at the
one-wave block; at the four-wave block the fewest rows that give it on this chip, T = ceil(CUs / ceil(B / 128)).  Every
launch first asserts that the block it is meant to test is the one the host's rule picks on this device."""
import functools

import numpy as np
import pytest
import torch

from tests import mlp_path_cases as mc
from tests import nn_oracle
from tests.guard_arena import CANARIES, GuardArena

pytestmark = pytest.mark.gpu

DEV = "cuda"
LINEAR, SIGMOID, RELU, TANH, RETANH, SOFTPLUS = range(6)
NO_PARAMS = [0.0, 0.0, 0.0, 0.0]


@functools.lru_cache(maxsize=None)
def compute_units():
    import ratinabox_amd.ops  # noqa: F401  (registers torch.ops.riab.*)
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def shapes():
    return mc.launch_shapes(compute_units())


def launch(xs, ws, bs, acts, pars, nw):
    """torch.ops.riab.mlp_forward, after checking that this launch takes the block of `nw` waves"""
    T, B = int(xs[0].shape[0]), int(xs[0].shape[2])
    assert mc.expected_nw(T, B, compute_units()) == nw, (T, B, compute_units(), nw)
    return torch.ops.riab.mlp_forward(xs, ws, bs, acts, pars)


def split(X, widths):
    """(T, K, B) host array -> the operator's inputs [(T, n_l, B)] on the device"""
    out, k = [], 0
    for w in widths:
        out.append(torch.from_numpy(np.ascontiguousarray(X[:, k:k + w])).to(DEV))
        k += w
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def edge_cells(widths):
    """the first and the last cell of every population and of every 16-slab inside one"""
    out, o = [], 0
    for K in widths:
        for s in range(0, K, 16):
            out += [o + s, o + min(s + 15, K - 1)]
        o += K
    return out


def one_hot(rng, widths, T, B, value=1.0):
    """-> (which (T, B), X (T, K, B) float32): position (t, b) holds `value` in cell which[t, b], which == K is the all-zero
    input; the compared positions take, in order, the edge cells, the all-zero input, every cell once more, random ones (as many
    as there are positions: six at B = 4, T = 2)."""
    K, n_real = sum(widths), B - 1
    order = edge_cells(widths) + [K] + list(rng.permutation(K + 1))
    which = rng.randint(0, K + 1, size=(T, B))
    real = [t * B + b for t in range(T) for b in range(n_real)]
    m = min(len(order), len(real))
    which.reshape(-1)[real[:m]] = order[:m]
    X = np.zeros((T, K + 1, B), dtype=np.float32)
    np.put_along_axis(X, which[:, None, :], np.float32(value), axis=1)
    X = np.ascontiguousarray(X[:, :K])
    X[:, :, n_real:] = np.nan
    return which, X


# ---------------------------------------------------------------------------------------------------------------------
# (a) one layer, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n_out", [7, 40, 70, 129, 228, 300])
def test_one_layer_one_hot_bit_for_bit(n_out, bias):
    """Exact: every product but one is 0 and the sum is rounded once.  n_out: one pass of 1, 2 and 4 tiles; two passes with a
    last one of 1 and of 4 tiles; three with a last one of 2.  Each with aligned weights (16-byte reads where koff % 4 == 0)
    and with the matrix at a base 4 mod 16 (4-byte reads), at both blocks.
    A second run puts +inf where the 1 was: the output is +-inf with the weight's sign.  A NaN there would mean that a rate row
    the stash should have zeroed (a row past its population's K, fetched from row K - 1) met a weight column outside the matrix."""
    for widths in ((3, 17), (5, 19), (16, 4), (5, 19, 108)):
        K = sum(widths)
        rng = np.random.RandomState(100000 + 1000 * n_out + 10 * K + bias)
        W = rng.uniform(-1, 1, (n_out, K)).astype(np.float32) / np.float32(np.sqrt(K))
        assert (W != 0).all()
        b = rng.uniform(-0.3, 0.3, n_out).astype(np.float32) if bias else None
        b_dev = torch.from_numpy(b).to(DEV) if bias else None
        Wz = np.concatenate([W, np.zeros((n_out, 1), dtype=np.float32)], axis=1)
        bcol = b[:, None, None] if bias else np.float32(0.0)
        for nw, T, B in shapes():
            which, X = one_hot(rng, widths, T, B)
            want = (Wz[:, which] + bcol).transpose(1, 0, 2)      # fp32 + fp32, rounded once: (T, n_out, B)
            sign = np.where(Wz[:, which] > 0, np.float32(np.inf), np.float32(-np.inf))
            want_inf = np.where(which[None] == K, np.zeros((), np.float32) + bcol, sign).astype(np.float32).transpose(1, 0, 2)
            assert want.dtype == np.float32 and want.shape == (T, n_out, B)
            xs, xs_inf = split(X, widths), split(np.where(X == 1, np.float32(np.inf), X), widths)
            for off in (0, 1):
                w_dev = mc.place(W, off, DEV)
                got = launch(xs, [w_dev], [b_dev], [LINEAR], NO_PARAMS, nw).cpu().numpy()
                bad = np.argwhere(bits(got[:, :, :B - 1]) != bits(want[:, :, :B - 1]))
                assert len(bad) == 0, (widths, nw, T, B, off, len(bad), bad[0], which[bad[0][0], bad[0][2]])
                got = launch(xs_inf, [w_dev], [b_dev], [LINEAR], NO_PARAMS, nw).cpu().numpy()
                bad = np.argwhere(bits(got[:, :, :B - 1]) != bits(want_inf[:, :, :B - 1]))
                assert len(bad) == 0, ("inf", widths, nw, T, B, off, len(bad), bad[0], which[bad[0][0], bad[0][2]])


# ---------------------------------------------------------------------------------------------------------------------
# (b) several layers, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def selection_chain(rng, n_in, hidden):
    """0/1 matrices (h_i, h_{i-1}), one 1 per column, every row hit -> (matrices, unit of the last width per input cell)"""
    mats, prev, comp = [], n_in, np.arange(n_in)
    for h in hidden:
        assert h <= prev
        sigma = np.concatenate([rng.permutation(h), rng.randint(0, h, size=prev - h)])
        rng.shuffle(sigma)
        M = np.zeros((h, prev), dtype=np.float32)
        M[sigma, np.arange(prev)] = 1.0
        assert (M.sum(0) == 1).all() and (M.sum(1) >= 1).all()
        mats.append(M)
        comp, prev = sigma[comp], h
    return mats, comp


CHAINS = [  # (input widths, hidden widths, n_out): depths 2, 3 and 8; last hidden widths 20, 33, 65, 96, 128
    ((3, 17), [20], 33), ((5, 19, 108), [33], 130), ((5, 19, 108), [65], 1), ((5, 19, 108), [96], 228), ((5, 19, 108), [128], 300),
    ((5, 19, 108), [33, 20], 130), ((5, 19, 108), [65, 33], 33), ((5, 19, 108), [96, 65], 1), ((5, 19, 108), [128, 96], 33),
    ((5, 19, 108), [128, 128], 130),
    ((5, 19, 108), [128, 128, 96, 96, 65, 33, 20], 130), ((5, 19, 108), [128, 96, 96, 65, 65, 64, 33], 33),
    ((5, 19, 108), [128, 128, 128, 96, 96, 65, 65], 1), ((5, 19, 108), [128, 128, 128, 128, 128, 96, 96], 33),
    ((5, 19, 108), [128] * 7, 300),
]


@pytest.mark.parametrize("chain", CHAINS, ids=lambda c: "-".join(str(h) for h in c[1]) + f"-{c[2]}")
def test_selection_layers_one_hot_bit_for_bit(chain):
    """mlp_reg_tile's k mapping: hidden layers are selection matrices (no bias; linear and relu alternate), so the one-hot
    input stays exactly one-hot, and the last layer (random weights, linear, with and without bias) must give
    fp32(W_L[m][p] + bias_L[m]) for the unit p the chain selects — bias_L[m] or +0.0 for the all-zero input.  Every matrix
    aligned and at a base 4 mod 16.  Every unit of the last hidden layer is the selected one at a compared position of every
    launch that has more positions than input cells, and (asserted) of the launches of a test taken together."""
    widths, hidden, n_out = chain
    K = sum(widths)
    rng = np.random.RandomState(7000 + 13 * len(hidden) + hidden[-1] + n_out)
    mats, comp = selection_chain(rng, K, hidden)
    WL = rng.uniform(-1, 1, (n_out, hidden[-1])).astype(np.float32) / np.float32(np.sqrt(hidden[-1]))
    bL = rng.uniform(-0.3, 0.3, n_out).astype(np.float32)
    acts = [(LINEAR, RELU)[i % 2] for i in range(len(hidden))] + [LINEAR]
    pars = [p for a in acts for p in mc.DEFAULT_PARAMS[a]]
    Wz = np.concatenate([WL, np.zeros((n_out, 1), dtype=np.float32)], axis=1)
    compz = np.concatenate([comp, [hidden[-1]]])        # the all-zero input selects no unit: the zero column
    placed = {off: [mc.place(M, off, DEV) for M in mats] + [mc.place(WL, off, DEV)] for off in (0, 1)}
    seen = set()
    for nw, T, B in shapes():
        which, X = one_hot(rng, widths, T, B)
        xs = split(X, widths)
        p = compz[which]
        units = set(p[:, :B - 1].reshape(-1).tolist()) - {hidden[-1]}
        if T * (B - 1) > K:
            assert units == set(range(hidden[-1])), (T, B)
        seen |= units
        for bias in (True, False):
            want = (Wz[:, p] + (bL[:, None, None] if bias else np.float32(0.0))).transpose(1, 0, 2)
            for off in (0, 1):
                bs = [None] * len(hidden) + [torch.from_numpy(bL).to(DEV) if bias else None]
                got = launch(xs, placed[off], bs, acts, pars, nw).cpu().numpy()
                bad = np.argwhere(bits(got[:, :, :B - 1]) != bits(want[:, :, :B - 1]))
                assert len(bad) == 0, (nw, T, B, bias, off, len(bad), bad[0], which[bad[0][0], bad[0][2]])
    assert seen == set(range(hidden[-1]))


# ---------------------------------------------------------------------------------------------------------------------
# (c), (e): every case of mlp_path_cases.py, run once per shape with its own weight placement and once all flat
# ---------------------------------------------------------------------------------------------------------------------
CASES = {c.name: c for c in mc.CASES}


@functools.lru_cache(maxsize=None)
def case_runs(name):
    """[(nw, T, B, xs (device), X (host), args (aligned as the case says), got, got_flat)] for every launch shape"""
    case = CASES[name]
    seed = 4200 + list(CASES).index(name)
    arrays = mc.draw(case, seed)
    rng = np.random.RandomState(seed)
    args, args_flat = mc.operator_args(case, arrays, DEV), mc.operator_args(case, arrays, DEV, flat=True)
    runs = []
    for nw, T, B in shapes():
        X = rng.uniform(0, 1, (T, mc.n_in(case), B)).astype(np.float32)
        X[:, :, B - 1:] = np.nan
        xs = split(X, case.inputs)
        runs.append((nw, T, B, xs, X, args, launch(xs, *args, nw), launch(xs, *args_flat, nw)))
    return arrays, runs


@pytest.mark.parametrize("name", list(CASES))
def test_case_random_inputs_vs_float64(name):
    """inputs uniform in [0, 1], weights as nn.Linear draws them; the reference and the bound are tests/nn_oracle.forward's"""
    case = CASES[name]
    arrays, runs = case_runs(name)
    layers = mc.oracle_layers(case, arrays)
    n_out = case.layers[-1].n_out
    for nw, T, B, _xs, X, _args, got, _flat in runs:
        h0 = X[:, :, :B - 1].transpose(1, 0, 2).reshape(mc.n_in(case), T * (B - 1)).astype(np.float64)
        ref, tol = nn_oracle.forward(layers, h0)
        ref, tol = (v.reshape(n_out, T, B - 1).transpose(1, 0, 2) for v in (ref, tol))
        g = got.cpu().numpy()[:, :, :B - 1]
        err = np.abs(g - ref)
        print(f"{name} nw {nw} T {T} B {B}: worst |error| {err.max():.3g}, worst |error| / bound {(err / tol).max():.3g}")
        assert g.shape == ref.shape and np.isfinite(g).all()
        assert (err <= tol).all(), (name, nw, T, B, err.max(), (err / tol).max())


@pytest.mark.parametrize("name", list(CASES))
def test_case_bits_do_not_depend_on_the_form(name):
    """rows 0, T / 2 and T - 1 of the four-wave launch == the same row launched alone (one wave); every weight matrix at a
    base 4 mod 16 (4-byte reads everywhere) == the case's own placement: the loads differ, the values and the chain do not"""
    _arrays, runs = case_runs(name)
    for nw, T, B, xs, _X, args, got, flat in runs:
        assert torch.equal(got[:, :, :B - 1].view(torch.int32), flat[:, :, :B - 1].view(torch.int32)), (name, nw, T, B, "flat")
        if nw == 4:
            for t in (0, T // 2, T - 1):
                one = launch([x[t:t + 1].contiguous() for x in xs], *args, 1)
                assert torch.equal(one[0, :, :B - 1].view(torch.int32), got[t, :, :B - 1].view(torch.int32)), (name, T, B, t)


# ---------------------------------------------------------------------------------------------------------------------
# (d) activations with parameters
# ---------------------------------------------------------------------------------------------------------------------
OFF_DEFAULT = {LINEAR: (3.0, 1.0, 0.5, 2.0),             # (ignored by the kernel and by the oracle)
               SIGMOID: (2.0, -0.5, 0.3, 1.7),           # max, min, mid, beta
               RELU: (1.5, 0.2, 0.0, 0.0),               # gain, threshold
               TANH: (0.8, -0.1, 0.0, 0.0),
               RETANH: (1.3, 0.15, 0.0, 0.0),
               SOFTPLUS: (0.6, -0.3, 0.0, 0.0)}


@pytest.mark.parametrize("where", ["hidden", "last"])
@pytest.mark.parametrize("code", range(6))
def test_activation_parameters(code, where):
    """(5, 19) -> 33 -> 7 with the activation under test behind the 33-wide layer (linear behind the last) or behind the
    last one (relu behind the hidden layer).  Weights are U(-3, 3) / sqrt(n_in), so that pre-activations lie on both sides of every threshold; the
    softplus layer's are scaled further, onto both sides of its z = 20 switch (both asserted)."""
    widths, outs = (5, 19), (33, 7)
    idx = 0 if where == "hidden" else 1
    rng = np.random.RandomState(900 + 10 * code + idx)
    acts = [(RELU,) + mc.DEFAULT_PARAMS[RELU], (LINEAR,) + mc.DEFAULT_PARAMS[LINEAR]]
    acts[idx] = (code,) + OFF_DEFAULT[code]
    layers, k = [], sum(widths)
    for i, m in enumerate(outs):
        scale = 60.0 if (i == idx and code == SOFTPLUS) else 3.0
        W = (rng.uniform(-1, 1, (m, k)) * scale / np.sqrt(k)).astype(np.float32)
        b = (rng.uniform(-1, 1, m) * scale / np.sqrt(k)).astype(np.float32)
        layers.append((W, b))
        k = m
    spec = [(W.astype(np.float64), b.astype(np.float64), a) for (W, b), a in zip(layers, acts)]
    ws = [torch.from_numpy(W).to(DEV) for W, _b in layers]
    bs = [torch.from_numpy(b).to(DEV) for _W, b in layers]
    pars = [float(p) for a in acts for p in a[1:]]
    for nw, T, B in shapes():
        X = rng.uniform(0, 1, (T, sum(widths), B)).astype(np.float32)
        X[:, :, B - 1:] = np.nan
        h0 = X[:, :, :B - 1].transpose(1, 0, 2).reshape(sum(widths), T * (B - 1)).astype(np.float64)
        # the pre-activations of the layer under test lie on both sides of the activation's threshold / midpoint
        z = nn_oracle.forward(spec[:idx], h0)[0] if idx else h0
        z = spec[idx][0] @ z + spec[idx][1][:, None] - (0.0 if code == LINEAR else OFF_DEFAULT[code][2 if code == SIGMOID else 1])
        assert (z > 0.1).any() and (z < -0.1).any()
        if code == SOFTPLUS:
            assert (z > 21).any() and ((z > 0) & (z < 19)).any()
        ref, tol = nn_oracle.forward(spec, h0)
        ref, tol = (v.reshape(outs[-1], T, B - 1).transpose(1, 0, 2) for v in (ref, tol))
        got = launch(split(X, widths), ws, bs, [a[0] for a in acts], pars, nw).cpu().numpy()[:, :, :B - 1]
        err = np.abs(got - ref)
        print(f"act {code} {where} nw {nw} T {T} B {B}: worst |error| {err.max():.3g}, worst |error| / bound {(err / tol).max():.3g}")
        assert np.isfinite(got).all() and (err <= tol).all(), (code, where, nw, T, B, err.max(), (err / tol).max())


# ---------------------------------------------------------------------------------------------------------------------
# (f) guard bands at the four-wave block
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("n_out", [1, 33, 130])
@pytest.mark.parametrize("B", [132, 4])
def test_guard_bands_four_wave_block(B, n_out, depth):
    """The operator allocates its own output, so this test calls the function it wraps (ratinabox_amd.ops.mlp_launch) on a
    view in the middle of a canary-filled arena: nothing outside the view is written, every element inside is, and the
    bits are the same for both canaries.  (3, 17) -> [20 relu -> 33 tanh ->] n_out; the values under the oracle's bound."""
    from ratinabox_amd import _lib, ops
    cus = compute_units()
    T = -(-cus // -(-B // 128))
    assert mc.expected_nw(T, B, cus) == 4
    case = mc.Case("guard", (3, 17), ([mc.Layer(20, True, RELU), mc.Layer(33, False, TANH)] if depth == 3 else [])
                   + [mc.Layer(n_out, True, LINEAR)], "")
    arrays = mc.draw(case, 600 + n_out + depth)
    ws, bs, acts, pars = mc.operator_args(case, arrays, DEV)
    rng = np.random.RandomState(B + n_out)
    X = rng.uniform(0, 1, (T, 20, B)).astype(np.float32)
    X[:, :, B - 1:] = np.nan
    xs = split(X, case.inputs)
    h0 = X[:, :, :B - 1].transpose(1, 0, 2).reshape(20, T * (B - 1)).astype(np.float64)
    ref, tol = (v.reshape(n_out, T, B - 1).transpose(1, 0, 2) for v in nn_oracle.forward(mc.oracle_layers(case, arrays), h0))
    first = None
    for canary in CANARIES:
        arena = GuardArena(canary)
        out = arena.view((T, n_out, B), torch.float32, DEV)
        ops.mlp_launch(xs, ws, bs, acts, [pars[4 * i:4 * i + 4] for i in range(len(ws))], out, _lib.current_stream())
        torch.cuda.synchronize()
        got = arena.check(out, other=first)
        first = got if first is None else first
        assert (np.abs(got[:, :, :B - 1] - ref) <= tol).all()
