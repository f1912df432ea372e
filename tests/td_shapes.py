"""The shapes at which tests/test_gpu_td_shapes.py drives csrc/riab_td.hip, the path each of them is meant to take, and the
integer inputs for which the kernels' fp32 arithmetic is exact: test infrastructure only, NumPy only (tests/test_td_cpu.py
checks the claims made here without a GPU).

The launcher's rule, restated (`launch_path`): the rows n are cut into 32-row tiles, MT in {1, 2, 4, 8} tiles ride in one
workgroup, more than 8 tiles take several row groups (and then the fused trace update is replaced by the stand-alone
kernel); every input layer is cut into 128-row blocks; the batch is cut into 32-lane slabs and those into at most 64
chunks so that about 512 workgroups exist.

The integer inputs (`integer_inputs`): dt = 0.5 and tau_e = 1 make both trace coefficients 0.5, tau = 1, L2 = 0, eta = 1,
weights start at zero; phi and the trace hold even integers in [0, 4], v, dV/dt and the reward integers in [-3, 3],
act' is 0 or 1.  Then td in [-9, 9], g = td * act' and the new trace in [0, 4] are small integers, every partial sum of
G[i][j] = sum_b g[i][b] e[j][b] is an integer of magnitude <= 36 B < 2^24 (`exactness_bound`), and fp32 addition of
such integers is exact in any order: the kernel must equal the integer product to the last bit."""
from collections import namedtuple

import numpy as np

INT_CONSTS = [0.5, 1.0, 1.0, 1.0, 0.0]     # dt, tau, tau_e, eta, L2
TD_MAX = 9                                 # |r + dV/dt - v / tau| <= 3 + 3 + 3
TRACE_MAX = 4
MAX_LAYERS = 8

Case = namedtuple("Case", "name n layers B Bp reward")
REWARD_FORMS = ("f32_nb", "f64_lane", "f64_neuron")   # float32 (n, Bp); float64 (Bp,); float64 (n,)

# n -> (MT, row groups) it is meant to reach
ROWS = {1: (1, 1), 33: (2, 1), 64: (2, 1), 65: (4, 1), 128: (4, 1), 129: (8, 1), 256: (8, 1), 257: (8, 2), 520: (8, 3)}
LAYER_SETS = {"one": [1], "ragged": [127, 129], "three": [300, 5, 128], "eight": [1, 31, 33, 64, 130, 7, 128, 257]}
# (B, Bp) -> (slabs per chunk, chunks, slabs of the last chunk) over the layer set "ragged" (3 blocks: 64 chunks wanted)
BATCHES = {(1, 4): (1, 1, 1), (30, 32): (1, 1, 1), (33, 36): (1, 2, 1), (1022, 1024): (1, 32, 1),
           (4150, 4152): (3, 44, 1), (16384, 16384): (8, 64, 8)}
MODEST_LAYERS, MODEST_BATCH = "ragged", (33, 36)
WIDE = (129, 257)                          # MT 8 in one group; two groups


def launch_path(n, layers, Bp):
    """dict(mt, groups, blocks, n_slabs, slabs, n_chunks, last) by riab_td_update's rule."""
    tiles = (n + 31) // 32
    mt = 1 if tiles <= 1 else 2 if tiles <= 2 else 4 if tiles <= 4 else 8
    blocks = sum((k + 127) // 128 for k in layers)
    n_slabs = (Bp + 31) // 32
    want = min(max(512 // blocks, 1), 64, n_slabs)
    slabs = (n_slabs + want - 1) // want
    n_chunks = (n_slabs + slabs - 1) // slabs
    return dict(mt=mt, groups=(tiles + mt - 1) // mt, blocks=blocks, n_slabs=n_slabs, slabs=slabs, n_chunks=n_chunks,
                last=n_slabs - (n_chunks - 1) * slabs)


def exactness_bound(B):
    """The largest magnitude a partial sum of G can reach on the integer inputs."""
    return B * TD_MAX * TRACE_MAX


def cases():
    """Every n against one modest layer set and batch; every layer set, batch and reward form against n = 129 and 257; a
    seeded draw of a dozen further combinations."""
    out = [Case(f"rows-{n}", n, LAYER_SETS[MODEST_LAYERS], *MODEST_BATCH, "f32_nb") for n in ROWS]
    for n in WIDE:
        out += [Case(f"layers-{k}-n{n}", n, v, *MODEST_BATCH, "f32_nb") for k, v in LAYER_SETS.items()]
        out += [Case(f"batch-{B}-{Bp}-n{n}", n, LAYER_SETS[MODEST_LAYERS], B, Bp, "f32_nb") for B, Bp in BATCHES]
        out += [Case(f"reward-{r}-n{n}", n, LAYER_SETS["three"], *MODEST_BATCH, r) for r in REWARD_FORMS]
    rng = np.random.RandomState(20)
    rows, sets, batches = list(ROWS), list(LAYER_SETS), list(BATCHES)
    for k in range(12):
        n, s = rows[rng.randint(len(rows))], sets[rng.randint(len(sets))]
        (B, Bp), r = batches[rng.randint(len(batches))], REWARD_FORMS[rng.randint(len(REWARD_FORMS))]
        out.append(Case(f"draw{k}-n{n}-{s}-{B}-{r}", n, LAYER_SETS[s], B, Bp, r))
    return out


def integer_inputs(case, seed=0):
    """The inputs of one step, float32 arrays over all Bp lanes (lanes >= B hold values of the same kind: they must not
    matter): phi[l], trace[l] (n_in_l, Bp); v, dvdt, prime (n, Bp); v_last = v - dt * dvdt, so that td_forward_tail
    reproduces dvdt exactly; reward in the case's form.  A different pattern for every layer and every case."""
    rng = np.random.RandomState([seed, case.n, case.B, len(case.layers)] + list(case.layers))
    n, Bp = case.n, case.Bp
    a = {"phi": [2.0 * rng.randint(0, 3, size=(k, Bp)) for k in case.layers],
         "trace": [2.0 * rng.randint(0, 3, size=(k, Bp)) for k in case.layers],
         "v": rng.randint(-3, 4, size=(n, Bp)), "dvdt": rng.randint(-3, 4, size=(n, Bp)),
         "prime": rng.randint(0, 2, size=(n, Bp))}
    shape = {"f32_nb": (n, Bp), "f64_lane": (Bp,), "f64_neuron": (n,)}[case.reward]
    r = rng.randint(-3, 4, size=shape)
    a["reward"] = r.astype(np.float32 if case.reward == "f32_nb" else np.float64)
    for k in ("phi", "trace"):
        a[k] = [x.astype(np.float32) for x in a[k]]
    for k in ("v", "dvdt", "prime"):
        a[k] = a[k].astype(np.float32)
    a["v_last"] = a["v"] - np.float32(INT_CONSTS[0]) * a["dvdt"]       # half-integers: exact
    return a


def integer_reference(case, a):
    """What one step must leave, in integers: dict(td (n, B) int64, traces [(n_in_l, B) int64], G [(n, n_in_l) int64],
    wt [(n_in_l, n) float32]).  The product is taken by the float64 BLAS — exact for integers whose partial sums stay
    below 2^53, and checked against NumPy's int64 product in tests/test_td_cpu.py — because NumPy's own integer matmul
    takes seconds at the widest cases."""
    n, B = case.n, case.B
    r = a["reward"].astype(np.int64)
    r = {"f32_nb": lambda: r[:, :B], "f64_lane": lambda: r[None, :B], "f64_neuron": lambda: r[:, None]}[case.reward]()
    v, dvdt, prime = (a[k][:, :B].astype(np.int64) for k in ("v", "dvdt", "prime"))
    td = (r + dvdt - v) * np.ones((n, B), dtype=np.int64)
    g = td * prime
    twice = [p[:, :B].astype(np.int64) + e[:, :B].astype(np.int64) for p, e in zip(a["phi"], a["trace"])]
    assert all(not (t & 1).any() for t in twice)
    traces = [t // 2 for t in twice]
    assert np.abs(td).max() <= TD_MAX and all(0 <= e.min() and e.max() <= TRACE_MAX for e in traces)
    G = [np.matmul(g.astype(np.float64), e.T.astype(np.float64)) for e in traces]
    assert all(np.abs(x).max() <= exactness_bound(B) for x in G)
    G = [x.astype(np.int64) for x in G]
    dt, eta = INT_CONSTS[0], INT_CONSTS[3]
    scale = np.float32(np.float64(np.float32(dt)) * np.float64(np.float32(eta)) / np.float64(B))   # as the host computes it
    wt = [np.ascontiguousarray((scale * x.astype(np.float32)).T) for x in G]                      # ONE fp32 multiply
    assert all(w.dtype == np.float32 for w in wt)
    return {"td": td, "traces": traces, "G": G, "wt": wt}
