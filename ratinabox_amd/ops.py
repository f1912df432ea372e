"""`torch.ops.riab.*` — the C ABI of libriab_hip.so (include/riab_hip.h) registered as PyTorch custom operators.

The reference's only PyTorch touch-point is a user network consuming firing rates
(ratinabox/contribs/NeuralNetworkNeurons.py:6-7); registering the kernels as operators is what lets such code —
and `torch.compile` / CUDA-graph capture around it — call the accelerated path directly on device tensors:

    rates = torch.ops.riab.place_cells(pos, table, None, [0, 1, 0, 1, 1.0], False, 0, 0, 0.2, 0.0, 1.0)   # (n, P)

Every operator is a thin wrapper: it checks shapes, fills the ABI's structs with `data_ptr()`s and enqueues the
kernel on the CURRENT stream; nothing is synchronised.  Each has a fake (meta) implementation, so the operators
trace under `torch.compile(fullgraph=True)` and FakeTensorMode.  Layouts are the ABI's: the position / agent axis
is the last (fastest) one and must be a multiple of 4 (pad; padding columns are computed like any other).

Functional operators (return a new tensor)
    place_cells, grid_cells, plane_wave_neurons, head_direction_cells, boundary_vector_cells   rates float32 (n, P)
    spikes                                                              uint8 (T, n, B) from rates (T, n, B)
    feedforward                                                         float32 (T, n_out, B)
    mlp_forward   a whole multi-layer perceptron in one launch (contribs.NeuralNetworkNeurons)   float32 (T, n_out, B)
    gp_predict    the predictive mean of an RBF Gaussian-process decoder over rate rows                 float32 (T, D, B)
    gp_predict_var  its predictive variance (and the mean) through a workspace of kernel values   float32 (T, B), (T, D, B)
    bayes_decode  Poisson maximum-likelihood position decoding of spike counts (or rates) over bins       float32 (T, 6, B)
In-place operators
    history_window_counts  spike rows of a history piece added into the uint8 counts of their time windows
    bayes_filter     the Bayesian decoder with a continuity prior: a forward filter over consecutive windows, state carried
    bayes_filter_keep  that filter with every window's log posterior kept; bayes_smooth: the backward pass over them, which
                     turns the filtered posteriors of a recorded run into the smoothed ones
    history_moments  the float64 moment matrix of [rates ; targets ; 1] over history rows: what a ridge decoder is solved from
    td_forward_tail  the tail of ValueNeuron.update(): dV/dt, V_last and (optionally) the eligibility traces
    td_update        ValueNeuron.update_weights(reward): TD error, batch-mean gradient on the matrix cores, W^T updated
    td_learn_step    ValueNeuron.learn(reward) behind the forward pass + reset(lanes=mask), in two launches
    agent_step_      T fused Agent.update() steps on the float64 state (12, B); writes the history rows
    simulate_        T x (Agent.update(); N.update() for N in populations) as ONE native call (riab_simulate): the state,
                     the trajectory rows and every population's rate / spike rows are written

`Neurons.get_state()`, `Agent.update()` and `Agent.simulate()` go through these operators (step plans call the ABI
directly: their launches are issued from C++)."""
from typing import List, Optional

import torch
from torch import Tensor

from . import _lib as _L

C = _L.C

# Schemas are DEFINED once (Library "DEF") and the implementations registered for the CUDA (= HIP) key directly:
# `torch.library.custom_op` wraps every call in ~15 us of Python (measured on the per-step path), this route costs
# the dispatcher's boxed call into the Python function and nothing else.
_ns = torch.library.Library("riab", "DEF")
_TAGS = (torch.Tag.pt2_compliant_tag,)


def _register(schema, fake):
    """decorator: define `riab::<schema>`, register the function for CUDA and `fake` as its meta implementation"""
    name = schema.split("(", 1)[0]

    def deco(fn):
        _ns.define(schema, tags=_TAGS)
        _ns.impl(name, fn, "CUDA")
        torch.library.register_fake("riab::" + name, fake, lib=_ns)
        return fn
    return deco


def _env_struct(walls: Optional[Tensor], env: List[float], periodic: bool):
    """RiabEnv from operator arguments: env = [left, right, bottom, top, scale] for a box, or
    [left, right, bottom, top, scale, polygon, n_boundary, hole_mask_low32, hole_mask_high32] (include/riab_hip.h:
    RiabEnv) when the boundary is a general polygon and / or the environment has holes.  (The 64-bit edge mask travels
    as two 32-bit halves: a float list holds each of them exactly, all 64 walls of the C ABI included.)"""
    if len(env) not in (5, 9):
        raise ValueError("env must be [left, right, bottom, top, scale] (+ [polygon, n_boundary, hole_mask_lo, hole_mask_hi])")
    e = _L.RiabEnv()
    for i in range(4):
        e.extent[i] = float(env[i])
    e.scale = float(env[4])
    e.periodic = 1 if periodic else 0
    if len(env) == 9:
        e.polygon, e.n_boundary, e.hole_mask = int(env[5]), int(env[6]), int(env[7]) | (int(env[8]) << 32)
    if walls is None:
        e.n_walls, e.walls = 0, None
    else:
        if walls.dtype != torch.float64 or walls.dim() != 2 or walls.shape[1] != 4 or not walls.is_contiguous():
            raise ValueError("walls must be a contiguous float64 tensor (n_walls, 4) = (ax, ay, bx, by)")
        e.n_walls, e.walls = int(walls.shape[0]), walls.data_ptr()
    return e


def _rows(t: Tensor, rows: int, what: str):
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != rows or not t.is_contiguous() or t.shape[1] % 4:
        raise ValueError(f"{what} must be a contiguous float32 tensor ({rows}, P) with P a multiple of 4, got "
                         f"{tuple(t.shape)} {t.dtype}")
    return int(t.shape[1])


def _io(pos: Optional[Tensor], hd: Optional[Tensor], P: int, out: Tensor, min_fr: float, max_fr: float):
    io = _L.RiabRateIO()
    if pos is not None:
        io.pos_x, io.pos_y = pos[0].data_ptr(), pos[1].data_ptr()
    if hd is not None:
        io.hd_x, io.hd_y = hd[0].data_ptr(), hd[1].data_ptr()
    io.pos_ld, io.T, io.B = P, 1, P
    io.rates = out.data_ptr()
    io.dt = 0.0
    io.min_fr, io.max_fr = float(min_fr), float(max_fr)
    return io


# ---- PlaceCells ------------------------------------------------------------------------------------------------
@_register("place_cells(Tensor pos, Tensor table, Tensor? walls, float[] env, bool periodic, int description, "
           "int geometry, float top_hat_width, float min_fr, float max_fr) -> Tensor",
           lambda pos, table, walls, env, periodic, description, geometry, top_hat_width, min_fr, max_fr:
           pos.new_empty((table.shape[0], pos.shape[1])))
def place_cells(pos: Tensor, table: Tensor, walls: Optional[Tensor], env: List[float], periodic: bool, description: int,
                geometry: int, top_hat_width: float, min_fr: float, max_fr: float) -> Tensor:
    """PlaceCells.get_state (riab_place_cells).  pos float32 (2, P); table float32 (n, 3) = (centre x, centre y,
    -log2(e)/(2 w^2)); walls float64 (n_walls, 4) in Environment.walls order or None; env = [l, r, b, t, scale];
    description RIAB_PC_*; geometry RIAB_GEOM_*.  Returns rates float32 (n, P)."""
    P = _rows(pos, 2, "pos")
    n = int(table.shape[0])
    out = torch.empty((n, P), dtype=torch.float32, device=pos.device)
    e = _env_struct(walls, env, periodic)
    io = _io(pos, None, P, out, min_fr, max_fr)
    _L.check(_L.lib.riab_place_cells(e, io, _L.ptr(table), n, int(description), int(geometry), float(top_hat_width),
                                     _L.current_stream()), "riab_place_cells")
    return out


# ---- GridCells -------------------------------------------------------------------------------------------------
@_register("grid_cells(Tensor pos, Tensor table, int description, float f0, float min_fr, float max_fr) -> Tensor",
           lambda pos, table, description, f0, min_fr, max_fr: pos.new_empty((table.shape[0], pos.shape[1])))
def grid_cells(pos: Tensor, table: Tensor, description: int, f0: float, min_fr: float, max_fr: float) -> Tensor:
    """GridCells.get_state (riab_grid_cells).  table float32 (n, 9), see include/riab_hip.h."""
    P = _rows(pos, 2, "pos")
    n = int(table.shape[0])
    out = torch.empty((n, P), dtype=torch.float32, device=pos.device)
    io = _io(pos, None, P, out, min_fr, max_fr)
    _L.check(_L.lib.riab_grid_cells(io, _L.ptr(table), n, int(description), float(f0), _L.current_stream()),
             "riab_grid_cells")
    return out


# ---- contribs.PlaneWaveNeurons -----------------------------------------------------------------------------------
@_register("plane_wave_neurons(Tensor pos, Tensor table, float min_fr, float max_fr) -> Tensor",
           lambda pos, table, min_fr, max_fr: pos.new_empty((table.shape[0], pos.shape[1])))
def plane_wave_neurons(pos: Tensor, table: Tensor, min_fr: float, max_fr: float) -> Tensor:
    """contribs.PlaneWaveNeurons.get_state (riab_plane_wave_neurons).  pos float32 (2, P); table float32 (n, 3) = (a, bx, by),
    the phase in revolutions a - (x bx + y by), see include/riab_hip.h.  Returns rates float32 (n, P)."""
    P = _rows(pos, 2, "pos")
    n = int(table.shape[0])
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != 3 or not table.is_contiguous():
        raise ValueError("table must be a contiguous float32 tensor (n, 3) = (a, bx, by)")
    out = torch.empty((n, P), dtype=torch.float32, device=pos.device)
    io = _io(pos, None, P, out, min_fr, max_fr)
    _L.check(_L.lib.riab_plane_wave_neurons(io, _L.ptr(table), n, _L.current_stream()), "riab_plane_wave_neurons")
    return out


# ---- HeadDirectionCells ----------------------------------------------------------------------------------------
@_register("head_direction_cells(Tensor head_direction, Tensor table, float min_fr, float max_fr) -> Tensor",
           lambda head_direction, table, min_fr, max_fr: head_direction.new_empty((table.shape[0], head_direction.shape[1])))
def head_direction_cells(head_direction: Tensor, table: Tensor, min_fr: float, max_fr: float) -> Tensor:
    """HeadDirectionCells.get_state (riab_head_direction_cells).  head_direction float32 (2, P); table float32 (n, 3)
    = (cos, sin of the preferred angle, log2(e)/sigma^2)."""
    P = _rows(head_direction, 2, "head_direction")
    n = int(table.shape[0])
    out = torch.empty((n, P), dtype=torch.float32, device=head_direction.device)
    io = _io(None, head_direction, P, out, min_fr, max_fr)
    _L.check(_L.lib.riab_head_direction_cells(io, _L.ptr(table), n, _L.current_stream()), "riab_head_direction_cells")
    return out


# ---- BoundaryVectorCells ---------------------------------------------------------------------------------------
@_register("boundary_vector_cells(Tensor pos, Tensor? head_direction, Tensor walls, float[] env, bool periodic, "
           "Tensor test_dirs, Tensor ray_rden, Tensor cells, Tensor vm_table, Tensor inv_norm, bool egocentric, "
           "Tensor? cell_rows, Tensor? windows, float min_fr, float max_fr) -> Tensor",
           lambda pos, head_direction, walls, env, periodic, test_dirs, ray_rden, cells, vm_table, inv_norm, egocentric,
           cell_rows, windows, min_fr, max_fr: pos.new_empty((cells.shape[1], pos.shape[1])))
def boundary_vector_cells(pos: Tensor, head_direction: Optional[Tensor], walls: Tensor, env: List[float], periodic: bool,
                          test_dirs: Tensor, ray_rden: Tensor, cells: Tensor, vm_table: Tensor, inv_norm: Tensor,
                          egocentric: bool, cell_rows: Optional[Tensor], windows: Optional[Tensor], min_fr: float,
                          max_fr: float) -> Tensor:
    """BoundaryVectorCells.get_state (riab_boundary_vector_cells_windowed).  Tables as documented in
    include/riab_hip.h (test_dirs float64 (K, 2), ray_rden float64 (K, n_walls), cells float32 (4, n), vm_table,
    inv_norm float32 (n,), optional direction windows)."""
    P = _rows(pos, 2, "pos")
    if egocentric:
        if head_direction is None or _rows(head_direction, 2, "head_direction") != P:
            raise ValueError("egocentric cells need head_direction (2, P)")
    n, K = int(cells.shape[1]), int(test_dirs.shape[0])
    out = torch.empty((n, P), dtype=torch.float32, device=pos.device)
    e = _env_struct(walls, env, periodic)
    io = _io(pos, head_direction if egocentric else None, P, out, min_fr, max_fr)
    _L.check(_L.lib.riab_boundary_vector_cells_windowed(e, io, _L.ptr(test_dirs), _L.ptr(ray_rden), K, _L.ptr(cells),
                                                        _L.ptr(vm_table), _L.ptr(inv_norm), n, 1 if egocentric else 0, None,
                                                        _L.ptr(cell_rows), _L.ptr(windows), _L.current_stream()),
             "riab_boundary_vector_cells")
    return out


# ---- Poisson spikes --------------------------------------------------------------------------------------------
@_register("spikes(Tensor rates, Tensor? uniforms, float dt, int seed, int step0, int pop_id, int agent_id0) -> Tensor",
           lambda rates, uniforms, dt, seed, step0, pop_id, agent_id0: rates.new_empty(rates.shape, dtype=torch.uint8))
def spikes(rates: Tensor, uniforms: Optional[Tensor], dt: float, seed: int, step0: int, pop_id: int,
           agent_id0: int) -> Tensor:
    """Neurons.save_to_history's spike rule `u < dt * rate` (riab_spikes) on rates float32 (T, n, B): with explicit
    `uniforms` (same shape) or, when None, the Philox uniforms keyed by (seed; step0 + t, cell, agent id, pop_id).
    Returns uint8 (T, n, B)."""
    if rates.dtype != torch.float32 or rates.dim() != 3 or not rates.is_contiguous() or rates.shape[2] % 4:
        raise ValueError("rates must be a contiguous float32 tensor (T, n, B) with B a multiple of 4")
    T, n, B = (int(x) for x in rates.shape)
    if uniforms is not None and (uniforms.shape != rates.shape or uniforms.dtype != torch.float32 or
                                 not uniforms.is_contiguous()):
        raise ValueError("uniforms must match rates (contiguous float32)")
    out = torch.empty((T, n, B), dtype=torch.uint8, device=rates.device)
    io = _L.RiabRateIO()
    io.pos_ld, io.T, io.B = B, T, B
    io.rates, io.spikes = rates.data_ptr(), out.data_ptr()
    io.u_in = uniforms.data_ptr() if uniforms is not None else None
    io.dt = float(dt)
    io.seed, io.step0, io.agent_id0, io.pop_id = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), int(agent_id0), int(pop_id)
    _L.check(_L.lib.riab_spikes(io, n, _L.current_stream()), "riab_spikes")
    return out


# ---- FeedForwardLayer ------------------------------------------------------------------------------------------
@_register("feedforward(Tensor[] inputs, Tensor[] weights_t, Tensor bias, int activation, float[] act_params) -> Tensor",
           lambda inputs, weights_t, bias, activation, act_params:
           inputs[0].new_empty((inputs[0].shape[0], bias.shape[0], inputs[0].shape[2])))
def feedforward(inputs: List[Tensor], weights_t: List[Tensor], bias: Tensor, activation: int,
                act_params: List[float]) -> Tensor:
    """FeedForwardLayer.get_state (riab_feedforward, fp32 matrix cores): out[t][m][b] = act(sum_l sum_k
    w_l[m][k] * inputs_l[t][k][b] + bias[m]).  inputs_l float32 (T, n_in_l, B); weights_t_l float32 (n_in_l, Mp) =
    the weight matrix TRANSPOSED, rows zero-padded to Mp = n_out rounded up to 32; bias float32 (n_out,);
    activation RIAB_ACT_*; act_params as in include/riab_hip.h.  Returns float32 (T, n_out, B)."""
    if not inputs or len(inputs) != len(weights_t) or len(inputs) > 8:
        raise ValueError("1..8 input layers, one transposed weight matrix each")
    T, _, B = (int(x) for x in inputs[0].shape)
    n_out = int(bias.shape[0])
    arr = (_L.RiabFFInput * len(inputs))()
    for l, (x, w) in enumerate(zip(inputs, weights_t)):
        if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous() or x.shape[0] != T or x.shape[2] != B:
            raise ValueError("inputs must be contiguous float32 (T, n_in, B) with equal T and B")
        if w.dtype != torch.float32 or not w.is_contiguous() or w.shape[0] != x.shape[1] or w.shape[1] % 32 or \
                w.shape[1] < n_out:
            raise ValueError("weights_t[l] must be contiguous float32 (n_in_l, Mp), Mp = n_out rounded up to 32")
        arr[l].rates, arr[l].wt, arr[l].n_in = x.data_ptr(), w.data_ptr(), int(x.shape[1])
    pars = (C.c_float * 4)(*[float(p) for p in (list(act_params) + [0.0] * 4)[:4]])
    out = torch.empty((T, n_out, B), dtype=torch.float32, device=inputs[0].device)
    _L.check(_L.lib.riab_feedforward(arr, len(inputs), _L.ptr(bias), n_out, T, B, int(activation), pars, _L.ptr(out), None,
                                     _L.current_stream()), "riab_feedforward")
    return out


# ---- contribs.NeuralNetworkNeurons: a whole multi-layer perceptron in one launch -----------------------------------
def mlp_launch(inputs, weights, biases, activations, act_params, out, stream):
    """riab_mlp_forward on device tensors, written into `out` float32 (T, n_out, B): inputs[l] contiguous float32
    (T, n_l, B); weights[i] float32 (n_out_i, n_in_i) = nn.Linear.weight, READ IN PLACE (their data_ptr()s are taken here,
    at every call); biases[i] float32 (n_out_i,) or None; activations[i] RIAB_ACT_*; act_params[i] 4 floats."""
    n_in, n_l = len(inputs), len(weights)
    if not n_in or not n_l or len(biases) != n_l or len(activations) != n_l or len(act_params) != n_l:
        raise ValueError("one weight, one bias entry, one activation and 4 activation parameters per layer; >= 1 input")
    T, _, B = (int(x) for x in inputs[0].shape)
    ptrs, widths = (C.c_void_p * n_in)(), (C.c_int32 * n_in)()
    for l, x in enumerate(inputs):
        if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous() or x.shape[0] != T or x.shape[2] != B:
            raise ValueError("inputs must be contiguous float32 (T, n_in, B) with equal T and B")
        ptrs[l], widths[l] = x.data_ptr(), int(x.shape[1])
    arr = (_L.RiabMLPLayer * n_l)()
    for i, (w, b) in enumerate(zip(weights, biases)):
        if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.device != inputs[0].device:
            raise ValueError("weights[i] must be a contiguous float32 tensor (n_out, n_in) on the inputs' device")
        if b is not None and (b.dtype != torch.float32 or tuple(b.shape) != (w.shape[0],) or not b.is_contiguous()
                              or b.device != w.device):
            raise ValueError("biases[i] must be None or a contiguous float32 tensor (n_out,) on the weights' device")
        q = arr[i]
        q.w, q.bias = w.data_ptr(), (b.data_ptr() if b is not None else None)
        q.n_out, q.n_in, q.activation = int(w.shape[0]), int(w.shape[1]), int(activations[i])
        for k in range(4):
            q.act_params[k] = float(act_params[i][k])
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != T * int(weights[-1].shape[0]) * B:
        raise ValueError("out must be a contiguous float32 tensor (T, n_out, B)")
    _L.check(_L.lib.riab_mlp_forward(ptrs, widths, n_in, arr, n_l, T, B, _L.ptr(out), stream), "riab_mlp_forward")


@_register("mlp_forward(Tensor[] inputs, Tensor[] weights, Tensor?[] biases, int[] activations, float[] act_params) -> Tensor",
           lambda inputs, weights, biases, activations, act_params:
           inputs[0].new_empty((inputs[0].shape[0], weights[-1].shape[0], inputs[0].shape[2])))
def mlp_forward(inputs: List[Tensor], weights: List[Tensor], biases: List[Optional[Tensor]], activations: List[int],
                act_params: List[float]) -> Tensor:
    """A multi-layer perceptron in ONE launch (riab_mlp_forward, csrc/riab_mlp.hip): h_0 = the inputs concatenated along
    the cell axis, h_i = act_i(weights_i @ h_{i-1} + biases_i), hidden activations kept in registers.  inputs_l float32
    (T, n_l, B), B % 4 == 0; weights_i float32 (n_out_i, n_in_i) — nn.Linear.weight as it is, read in place —; biases_i
    float32 (n_out_i,) or None; activations_i RIAB_ACT_*; act_params 4 floats per layer, flat.  At most 8 inputs and 8
    layers, hidden widths <= 128.  Forward only (no autograd formula).  Returns float32 (T, n_out, B)."""
    if len(act_params) != 4 * len(weights):
        raise ValueError("act_params holds 4 floats per layer")
    out = torch.empty((int(inputs[0].shape[0]), int(weights[-1].shape[0]), int(inputs[0].shape[2])), dtype=torch.float32,
                      device=inputs[0].device)
    mlp_launch(inputs, weights, biases, activations, [act_params[4 * i:4 * i + 4] for i in range(len(weights))], out,
               _L.current_stream())
    return out


# ---- TD learning: contribs.ValueNeuron / SuccessorFeatures -------------------------------------------------------
def _td_structs(n: int, B: int, Bp: int, consts: List[float], rates: List[Tensor], traces: List[Tensor],
                weights_t: List[Tensor]):
    """(RiabTDParams, RiabTDLayer array) from operator arguments; consts = [dt, tau, tau_e, eta, L2]."""
    if len(consts) != 5:
        raise ValueError("consts must be [dt, tau, tau_e, eta, L2]")
    if not rates or len(rates) != len(traces) or len(rates) != len(weights_t) or len(rates) > 8:
        raise ValueError("1..8 input layers: one rates, one trace and one transposed weight tensor each")
    p = _L.RiabTDParams()
    p.dt, p.tau, p.tau_e, p.eta, p.L2 = (float(c) for c in consts)
    p.B, p.Bp, p.n, p.Mp = int(B), int(Bp), int(n), (int(n) + 31) // 32 * 32
    arr = (_L.RiabTDLayer * len(rates))()
    for l, (x, e, w) in enumerate(zip(rates, traces, weights_t)):
        for name, t in (("rates", x), ("traces", e)):
            if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[1] != Bp:
                raise ValueError(f"{name}[{l}] must be a contiguous float32 tensor (n_in, Bp)")
        if e.shape[0] != x.shape[0]:
            raise ValueError("traces[l] must have the shape of rates[l]")
        if w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape) != (x.shape[0], p.Mp):
            raise ValueError("weights_t[l] must be contiguous float32 (n_in_l, Mp), Mp = n rounded up to 32")
        arr[l].rates, arr[l].trace, arr[l].wt, arr[l].n_in = x.data_ptr(), e.data_ptr(), w.data_ptr(), int(x.shape[0])
    return p, arr


def _td_rows(t: Tensor, n: int, Bp: int, what: str):
    if t.dtype != torch.float32 or tuple(t.shape) != (n, Bp) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 tensor ({n}, {Bp})")


def td_workspace_floats(n: int, n_ins: List[int], Bp: int) -> int:
    """Floats of workspace `td_update` needs for a learner of n neurons over input layers of n_ins cells and Bp lanes."""
    p = _L.RiabTDParams()
    p.n, p.Bp, p.B = int(n), int(Bp), int(Bp)
    arr = (_L.RiabTDLayer * len(n_ins))()
    for l, k in enumerate(n_ins):
        arr[l].n_in = int(k)
    need = int(_L.lib.riab_td_workspace(p, arr, len(n_ins)))
    if need < 0:
        raise _L.RiabError(f"riab_td_workspace failed with code {need}: {_L.strerror(need)}")
    return need


@_register("td_forward_tail(Tensor v, Tensor(a!) v_last, Tensor(b!) dvdt, Tensor[] rates, Tensor(c!)[] traces, "
           "Tensor[] weights_t, float[] consts, int B, bool with_trace) -> ()",
           lambda v, v_last, dvdt, rates, traces, weights_t, consts, B, with_trace: None)
def td_forward_tail(v: Tensor, v_last: Tensor, dvdt: Tensor, rates: List[Tensor], traces: List[Tensor],
                    weights_t: List[Tensor], consts: List[float], B: int, with_trace: bool) -> None:
    """The tail of ValueNeuron.update() (riab_td_forward_tail), in place: dvdt = (v - v_last) / dt; v_last = v; with
    `with_trace` traces_l = dt * rates_l + (1 - dt / tau_e) * traces_l.  v, v_last, dvdt float32 (n, Bp); rates_l,
    traces_l float32 (n_in_l, Bp); weights_t_l float32 (n_in_l, Mp) (not touched); consts = [dt, tau, tau_e, eta, L2];
    B the real lanes."""
    n, Bp = int(v.shape[0]), int(v.shape[1])
    for name, t in (("v", v), ("v_last", v_last), ("dvdt", dvdt)):
        _td_rows(t, n, Bp, name)
    p, arr = _td_structs(n, B, Bp, consts, rates, traces, weights_t)
    _L.check(_L.lib.riab_td_forward_tail(p, arr, len(rates), _L.ptr(v), _L.ptr(v_last), _L.ptr(dvdt),
                                         1 if with_trace else 0, _L.current_stream()), "riab_td_forward_tail")


def _reward_strides(reward: Tensor, n: int, B: int, Bp: int):
    """(stride over neurons, stride over lanes) in elements of a reward tensor: a scalar, (n,) one per neuron, (B..,) one
    per lane, (n, B..) one per neuron and lane (B.. = B or the padded Bp) — read in place, whatever its strides.  A 1-D reward of length n == B > 1
    is read the reference's way: one per neuron."""
    if reward.dtype not in (torch.float32, torch.float64):
        raise ValueError("reward must be float32 or float64")
    if reward.dim() == 0 or reward.numel() == 1:
        return 0, 0
    if reward.dim() == 1:
        if reward.shape[0] == n:
            return int(reward.stride(0)), 0
        if reward.shape[0] in (B, Bp):
            return 0, int(reward.stride(0))
    elif reward.dim() == 2 and reward.shape[0] == n and reward.shape[1] in (B, Bp):
        return int(reward.stride(0)), int(reward.stride(1))
    raise ValueError(f"reward must be a scalar, (n,) = ({n},), (B,) = ({B},) or (n, B), got {tuple(reward.shape)}")


@_register("td_update(Tensor(a!)[] weights_t, Tensor(b!)[] traces, Tensor[] rates, Tensor reward, Tensor v, Tensor dvdt, "
           "Tensor prime, Tensor(c!) td, Tensor(d!) workspace, float[] consts, int B, bool fuse_trace) -> ()",
           lambda weights_t, traces, rates, reward, v, dvdt, prime, td, workspace, consts, B, fuse_trace: None)
def td_update(weights_t: List[Tensor], traces: List[Tensor], rates: List[Tensor], reward: Tensor, v: Tensor, dvdt: Tensor,
              prime: Tensor, td: Tensor, workspace: Tensor, consts: List[float], B: int, fuse_trace: bool) -> None:
    """ValueNeuron.update_weights(reward) for the whole batch (riab_td_update), in place: td = reward + dvdt - v / tau;
    weights_t_l += dt * eta / B * sum_{b<B} (td * prime)[:, b] (x) traces_l[:, b] - eta * dt * L2 * weights_t_l (as W^T,
    float32 (n_in_l, Mp)).  With `fuse_trace` the trace update of `td_forward_tail` is applied on the fly.  reward:
    float32 / float64, a scalar, (n,), (B,) or (n, B) (see _reward_strides).  workspace: float32, at least
    `td_workspace_floats(n, [n_in_l], Bp)` elements.  Lanes b >= B contribute nothing."""
    n, Bp = int(v.shape[0]), int(v.shape[1])
    for name, t in (("v", v), ("dvdt", dvdt), ("prime", prime), ("td", td)):
        _td_rows(t, n, Bp, name)
    p, arr = _td_structs(n, B, Bp, consts, rates, traces, weights_t)
    if workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous float32 tensor")
    ld_n, ld_b = _reward_strides(reward, n, int(B), Bp)
    _L.check(_L.lib.riab_td_update(p, arr, len(rates), _L.ptr(reward), 1 if reward.dtype == torch.float64 else 0, ld_n, ld_b,
                                   _L.ptr(v), _L.ptr(dvdt), _L.ptr(prime), _L.ptr(td), 1 if fuse_trace else 0,
                                   _L.ptr(workspace), int(workspace.numel()), _L.current_stream()), "riab_td_update")


@_register("td_learn_step(Tensor(a!)[] weights_t, Tensor(b!)[] traces, Tensor[] rates, Tensor reward, Tensor(c!) v, "
           "Tensor(d!) v_last, Tensor(e!) dvdt, Tensor prime, Tensor(f!) td, Tensor? mask, bool zero_v, Tensor(g!) workspace, "
           "float[] consts, int B) -> ()",
           lambda weights_t, traces, rates, reward, v, v_last, dvdt, prime, td, mask, zero_v, workspace, consts, B: None)
def td_learn_step(weights_t: List[Tensor], traces: List[Tensor], rates: List[Tensor], reward: Tensor, v: Tensor,
                  v_last: Tensor, dvdt: Tensor, prime: Tensor, td: Tensor, mask: Optional[Tensor], zero_v: bool,
                  workspace: Tensor, consts: List[float], B: int) -> None:
    """`td_forward_tail(with_trace=False)`, `td_update(fuse_trace=True)` and ValueNeuron.reset(lanes=mask) in two launches
    (riab_td_learn_step), in place and with the same bits: dvdt = (v - v_last) / dt is worked out inside the gradient pass,
    the finish launch adds the partial sums, copies v to v_last and zeroes the columns b < B with mask[b] != 0 of the traces,
    v_last, dvdt, td and — `zero_v` only — v.  mask: uint8 / bool (>= B,) or None (no reset).  Other arguments as `td_update`."""
    n, Bp = int(v.shape[0]), int(v.shape[1])
    for name, t in (("v", v), ("v_last", v_last), ("dvdt", dvdt), ("prime", prime), ("td", td)):
        _td_rows(t, n, Bp, name)
    p, arr = _td_structs(n, B, Bp, consts, rates, traces, weights_t)
    if workspace.dtype != torch.float32 or not workspace.is_contiguous():
        raise ValueError("workspace must be a contiguous float32 tensor")
    if mask is not None and (mask.dtype not in (torch.uint8, torch.bool) or mask.dim() != 1 or not mask.is_contiguous()
                             or mask.shape[0] < int(B)):
        raise ValueError(f"mask must be a contiguous uint8 or bool tensor of at least B = {int(B)} lanes")
    ld_n, ld_b = _reward_strides(reward, n, int(B), Bp)
    _L.check(_L.lib.riab_td_learn_step(p, arr, len(rates), _L.ptr(reward), 1 if reward.dtype == torch.float64 else 0, ld_n,
                                       ld_b, _L.ptr(v), _L.ptr(v_last), _L.ptr(dvdt), _L.ptr(prime), _L.ptr(td), _L.ptr(mask),
                                       1 if zero_v else 0, _L.ptr(workspace), int(workspace.numel()), _L.current_stream()),
             "riab_td_learn_step")


# ---- Agent.update ----------------------------------------------------------------------------------------------
MOTION_FIELDS = ("dt", "rot_theta_kw", "rot_sigma_kw", "rot_drift_kw", "speed_theta_kw", "speed_sigma_kw", "speed_mean_kw",
                 "speed_mean", "speed_std_is_zero", "has_drift", "drift_theta", "wall_repel_strength_kw",
                 "wall_repel_distance_kw", "thigmotaxis_kw", "hd_tau")


def seed_arg(seed: int) -> int:
    """A uint64 Philox key as the int64 the operator schemas carry (two's complement; the operators undo it)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def motion_list(m) -> List[float]:
    """RiabMotion struct -> the flat list `agent_step_` takes (MOTION_FIELDS order)."""
    return [float(getattr(m, k)) for k in MOTION_FIELDS]


@_register("agent_step_(Tensor(a!) state, Tensor(b!)? hist, Tensor(c!)? diag, Tensor? walls, float[] env, bool periodic, "
           "float[] motion, Tensor? drift, Tensor? noise, Tensor(d!)? noise_out, Tensor? forced_pos, Tensor? resample_pos, "
           "int seed, int step0, int agent_id0, int T) -> ()",
           lambda state, hist, diag, walls, env, periodic, motion, drift, noise, noise_out, forced_pos, resample_pos, seed,
           step0, agent_id0, T: None)
def agent_step_(state: Tensor, hist: Optional[Tensor], diag: Optional[Tensor], walls: Optional[Tensor], env: List[float],
                periodic: bool, motion: List[float], drift: Optional[Tensor], noise: Optional[Tensor],
                noise_out: Optional[Tensor], forced_pos: Optional[Tensor], resample_pos: Optional[Tensor], seed: int,
                step0: int, agent_id0: int, T: int) -> None:
    """T fused Agent.update() steps (riab_agent_step), in place: state float64 (12, B) (rows RIAB_S_*), hist float32
    (T, 8, B) or None, diag int32 (4,) or None.  motion = the RiabMotion fields in MOTION_FIELDS order; drift float64
    (2, B); noise float64 (T, 2, B) explicit standard normals (None: Philox keyed by (seed; step0 + t, agent_id0 + b));
    noise_out records the normals used; forced_pos float64 (T, 2, B) moves the agents instead of the motion model;
    resample_pos float64 (T, 2, B): explicit replacement positions for agents that end a step in a hole / outside a
    polygonal boundary (None: Philox draws)."""
    if state.dtype != torch.float64 or state.dim() != 2 or state.shape[0] != _L.STATE_ROWS or not state.is_contiguous():
        raise ValueError("state must be a contiguous float64 tensor (12, B)")
    B = int(state.shape[1])
    if len(motion) != len(MOTION_FIELDS):
        raise ValueError(f"motion must hold the {len(MOTION_FIELDS)} RiabMotion fields")
    m = _L.RiabMotion()
    for k, v in zip(MOTION_FIELDS, motion):
        setattr(m, k, int(v) if k in ("speed_std_is_zero", "has_drift") else float(v))
    if hist is not None and (hist.dtype != torch.float32 or tuple(hist.shape) != (T, _L.HIST_ROWS, B) or
                             not hist.is_contiguous()):
        raise ValueError("hist must be a contiguous float32 tensor (T, 8, B)")
    for name, t in (("noise", noise), ("noise_out", noise_out), ("forced_pos", forced_pos), ("resample_pos", resample_pos)):
        if t is not None and (t.dtype != torch.float64 or tuple(t.shape) != (T, 2, B) or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float64 tensor (T, 2, B)")
    if drift is not None and (drift.dtype != torch.float64 or tuple(drift.shape) != (2, B) or not drift.is_contiguous()):
        raise ValueError("drift must be a contiguous float64 tensor (2, B)")
    e = _env_struct(walls, env, periodic)
    _L.check(_L.lib.riab_agent_step(e, m, _L.ptr(state), B, int(agent_id0), _L.ptr(drift), _L.ptr(noise), _L.ptr(noise_out),
                                    _L.ptr(forced_pos), _L.ptr(resample_pos), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0),
                                    int(T), _L.ptr(hist), _L.ptr(diag), _L.current_stream()),
             "riab_agent_step")


# ---- the open-loop run: riab_simulate ----------------------------------------------------------------------------
@_register("simulate_(Tensor(a!) state, Tensor(b!) hist, Tensor(c!)[] rates, Tensor(d!)[] spikes, Tensor(e!) ctrl, "
           "Tensor(f!)? diag, int streamer, int run, int hist_row, int[] rate_rows, int[] spike_rows) -> ()",
           lambda state, hist, rates, spikes, ctrl, diag, streamer, run, hist_row, rate_rows, spike_rows: None)
def simulate_(state: Tensor, hist: Tensor, rates: List[Tensor], spikes: List[Tensor], ctrl: Tensor, diag: Optional[Tensor],
              streamer: int, run: int, hist_row: int, rate_rows: List[int], spike_rows: List[int]) -> None:
    """One riab_simulate call (include/riab_hip.h).  `run` is the address of a RiabSimulate argument block — built by
    `Agent.simulate_args()` or by hand through `ratinabox_amd._lib.RiabSimulate`; the caller keeps it, its population
    array and the tables they point to alive — and `streamer` the RiabStreamer handle.  What the call WRITES is taken
    from the tensors given here, not from the block (a tracer may hand the operator other tensors than the ones the
    block was built from: functionalisation runs it on copies): state float64 (12, B); hist float32 (rows, 8, B), the
    T rows from `hist_row` on; rates[i] float32 (rows, n_i, B) from `rate_rows[i]` on, one tensor per population of the
    block; spikes uint8 likewise for the populations whose block entry has a spike buffer, in order; ctrl int32
    control words; diag int32 (4,) or None.  Enqueues on the current stream, synchronises nothing.  Raises `RiabError`
    on a non-zero return code of the ABI (its `.code` holds it: RIAB_EUNSUPPORTED = nothing was launched)."""
    r = C.cast(C.c_void_p(run), C.POINTER(_L.RiabSimulate)).contents
    B, T, npop = int(r.B), int(r.T), int(r.n_pops)
    if state.dtype != torch.float64 or tuple(state.shape) != (_L.STATE_ROWS, B) or not state.is_contiguous():
        raise ValueError("state must be a contiguous float64 tensor (12, B) with the block's B")
    if hist.dtype != torch.float32 or hist.dim() != 3 or tuple(hist.shape[1:]) != (_L.HIST_ROWS, B) or \
            hist_row < 0 or hist_row + T > hist.shape[0] or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous float32 tensor (rows, 8, B) holding rows hist_row .. hist_row + T")
    if len(rates) != npop or len(rate_rows) != npop:
        raise ValueError("one rates tensor and one first row per population of the block")
    r.state, r.hist, r.ctrl = state.data_ptr(), hist.data_ptr() + hist_row * _L.HIST_ROWS * B * 4, ctrl.data_ptr()
    r.diag = diag.data_ptr() if diag is not None else None
    j = 0
    for i in range(npop):
        q = r.pops[i]
        n, fr = int(q.n), rates[i]
        if fr.dtype != torch.float32 or fr.dim() != 3 or tuple(fr.shape[1:]) != (n, B) or not fr.is_contiguous() or \
                rate_rows[i] < 0 or rate_rows[i] + int(q.capacity_rows) > fr.shape[0]:
            raise ValueError(f"rates[{i}] must be a contiguous float32 tensor (rows, {n}, {B}) holding the block's rows")
        q.rates_base = fr.data_ptr() + rate_rows[i] * n * B * 4
        if q.spikes_base:
            sp = spikes[j]
            if sp.dtype != torch.uint8 or tuple(sp.shape[1:]) != (n, B) or not sp.is_contiguous() or \
                    spike_rows[j] < 0 or spike_rows[j] + int(q.capacity_rows) > sp.shape[0]:
                raise ValueError(f"spikes[{j}] must be a contiguous uint8 tensor (rows, {n}, {B}) holding the block's rows")
            q.spikes_base = sp.data_ptr() + spike_rows[j] * n * B
            j += 1
    rc = int(_L.lib.riab_simulate(C.c_void_p(streamer), C.byref(r), _L.current_stream()))
    if rc:
        e = _L.RiabError(f"riab_simulate failed with code {rc}: {_L.strerror(rc)}")
        e.code = rc
        raise e


# ---- rate maps and occupancy from the history: riab_history_* ------------------------------------------------------
_EDGE_CACHE = {}


def _edges(edges_x: Tensor, edges_y: Tensor, device):
    """(host x, host y, device copy [nx + 1 + ny + 1]) of the two edge tensors: the library checks the host values
    before it launches and the kernel reads the device copy (kept per content: a map is asked for again and again
    on the same grid)."""
    for e in (edges_x, edges_y):
        if e.device.type != "cpu" or e.dtype != torch.float64 or e.dim() != 1 or not e.is_contiguous():
            raise ValueError("edges must be contiguous float64 HOST tensors (np.arange(lo, hi + dx, dx))")
    key = (edges_x.numpy().tobytes(), edges_y.numpy().tobytes(), str(device))
    dev = _EDGE_CACHE.get(key)
    if dev is None:
        if len(_EDGE_CACHE) >= 16:
            _EDGE_CACHE.clear()
        dev = _EDGE_CACHE[key] = torch.cat((edges_x, edges_y)).to(device)
    return dev


@_register("history_bin_index(Tensor traj, Tensor edges_x, Tensor edges_y, int n_real, Tensor(a!) counts) -> Tensor",
           lambda traj, edges_x, edges_y, n_real, counts: traj.new_empty((traj.shape[0], traj.shape[2]), dtype=torch.int16))
def history_bin_index(traj: Tensor, edges_x: Tensor, edges_y: Tensor, n_real: int, counts: Tensor) -> Tensor:
    """Stage A of a rate map (riab_history_bin_index): the bin of every (step, agent) sample of trajectory rows `traj`
    float32 (T, 8, B) on the grid of the float64 HOST tensors edges_x (nx + 1,) / edges_y (ny + 1,) — np.histogram2d's
    rule — for the first `n_real` agents of a row.  Returns the ids, (T, B) int16 holding the ABI's uint16 bits:
    (ny - 1 - ky) * nx + kx, or -1 (= RIAB_RATEMAP_DROPPED) for a sample outside the grid, a NaN or a padding lane.
    counts: int64 (ny, nx), the occupancy, ADDED to."""
    if traj.dtype != torch.float32 or traj.dim() != 3 or traj.shape[1] != _L.HIST_ROWS or not traj.is_contiguous():
        raise ValueError("traj must be a contiguous float32 tensor (T, 8, B)")
    T, B = int(traj.shape[0]), int(traj.shape[2])
    nx, ny = int(edges_x.shape[0]) - 1, int(edges_y.shape[0]) - 1
    dev = _edges(edges_x, edges_y, traj.device)
    if counts.dtype != torch.int64 or counts.numel() != max(nx, 0) * max(ny, 0) or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int64 tensor (ny, nx)")
    ids = torch.empty((T, B), dtype=torch.int16, device=traj.device)
    _L.check(_L.lib.riab_history_bin_index(_L.ptr(traj), T, B, int(n_real), edges_x.data_ptr(), nx, edges_y.data_ptr(), ny,
                                           _L.ptr(dev), _L.ptr(ids), _L.ptr(counts), _L.current_stream()),
             "riab_history_bin_index")
    return ids


@_register("history_rate_map(Tensor rows, Tensor bin_ids, Tensor(a!) sums) -> ()", lambda rows, bin_ids, sums: None)
def history_rate_map(rows: Tensor, bin_ids: Tensor, sums: Tensor) -> None:
    """Stage B of a rate map (riab_history_rate_map), in place: sums[c].flat[id] += rows[t, c, b] for every sample whose
    bin id is not dropped.  rows: float32 rates or uint8 spikes (T, n, B); bin_ids: int16 (T, B) from
    `history_bin_index` on the same steps; sums: float64 (n, ny, nx), ADDED to (in float64 throughout; spike sums are
    exact)."""
    if rows.dtype not in (torch.float32, torch.uint8) or rows.dim() != 3 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous float32 (rates) or uint8 (spikes) tensor (T, n, B)")
    T, n, B = (int(x) for x in rows.shape)
    if bin_ids.dtype != torch.int16 or tuple(bin_ids.shape) != (T, B) or not bin_ids.is_contiguous():
        raise ValueError("bin_ids must be a contiguous int16 tensor (T, B) of the same steps")
    if sums.dtype != torch.float64 or sums.dim() < 2 or sums.shape[0] != n or not sums.is_contiguous():
        raise ValueError("sums must be a contiguous float64 tensor (n, ny, nx)")
    n_bins = int(sums.numel() // max(n, 1))
    if n == 0:
        return
    need = int(_L.lib.riab_history_rate_map_workspace(T, n, B, n_bins))
    if need < 0:
        raise _L.RiabError(f"riab_history_rate_map_workspace failed with code {need}: {_L.strerror(need)}")
    ws = torch.empty(max(need, 1), dtype=torch.float64, device=rows.device)
    _L.check(_L.lib.riab_history_rate_map(_L.ptr(rows), 1 if rows.dtype == torch.uint8 else 0, T, n, B, _L.ptr(bin_ids),
                                          n_bins, _L.ptr(sums), _L.ptr(ws), int(ws.numel()), _L.current_stream()),
             "riab_history_rate_map")


@_register("history_rate_map_finish(Tensor sums, Tensor counts, bool norm_by_bincount) -> (Tensor, Tensor)",
           lambda sums, counts, norm_by_bincount: (sums.new_empty(sums.shape), counts.new_empty(counts.shape, dtype=torch.bool)))
def history_rate_map_finish(sums: Tensor, counts: Tensor, norm_by_bincount: bool):
    """The end of a rate map (riab_history_rate_map_finish): (maps float64 like sums — sums / counts with empty bins'
    counts set to 1, or the sums —, zero_bins bool like counts: True where no sample fell)."""
    if sums.dtype != torch.float64 or not sums.is_contiguous() or counts.dtype != torch.int64 or not counts.is_contiguous():
        raise ValueError("sums must be contiguous float64 (n, ny, nx), counts contiguous int64 (ny, nx)")
    n_bins = int(counts.numel())
    n = int(sums.numel() // max(n_bins, 1))
    if n * n_bins != sums.numel():
        raise ValueError("sums must hold one map of counts' shape per cell")
    maps = torch.empty_like(sums)
    zero = torch.empty(counts.shape, dtype=torch.bool, device=counts.device)
    _L.check(_L.lib.riab_history_rate_map_finish(_L.ptr(sums), _L.ptr(counts), n, n_bins, 1 if norm_by_bincount else 0,
                                                 _L.ptr(maps), _L.ptr(zero), _L.current_stream()),
             "riab_history_rate_map_finish")
    return maps, zero


# ---- linear decoders from the history: riab_history_moments ----------------------------------------------------------
@_register("history_moments(Tensor[] inputs, Tensor traj, int[] target_rows, int t_step, int n_real, Tensor(a!) moments, "
           "Tensor(b!) n_dropped) -> ()", lambda inputs, traj, target_rows, t_step, n_real, moments, n_dropped: None)
def history_moments(inputs: List[Tensor], traj: Tensor, target_rows: List[int], t_step: int, n_real: int, moments: Tensor,
                    n_dropped: Tensor) -> None:
    """The moment matrix a ridge decoder is solved from (riab_history_moments, float64 matrix cores), in place:
    moments += sum of z z^T over the samples (t in 0, t_step, 2 t_step, ...; b < n_real) of z = [inputs_0[t, :, b] ; ... ;
    traj[t, target_rows, b] ; 1].  inputs_l: float32 (T, n_l, B) rate rows; traj: float32 (T, 8, B) of the same steps;
    moments: float64 (m, m), m = sum n_l + len(target_rows) + 1, ADDED to; n_dropped: int64 (1,), ADDED to: the samples
    left out because a target value was not finite (padding lanes b >= n_real are left out and not counted)."""
    if not inputs or len(inputs) > 8:
        raise ValueError("1..8 input histories")
    if traj.dtype != torch.float32 or traj.dim() != 3 or traj.shape[1] != _L.HIST_ROWS or not traj.is_contiguous():
        raise ValueError("traj must be a contiguous float32 tensor (T, 8, B)")
    T, B = int(traj.shape[0]), int(traj.shape[2])
    arr = (_L.RiabMomentInput * len(inputs))()
    m = len(target_rows) + 1
    for l, x in enumerate(inputs):
        if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous() or x.shape[0] != T or x.shape[2] != B or \
                x.device != traj.device:
            raise ValueError("inputs must be contiguous float32 (T, n_l, B) tensors of traj's steps, lanes and device")
        arr[l].rows, arr[l].n = x.data_ptr(), int(x.shape[1])
        m += int(x.shape[1])
    if moments.dtype != torch.float64 or tuple(moments.shape) != (m, m) or not moments.is_contiguous() or \
            moments.device != traj.device:
        raise ValueError(f"moments must be a contiguous float64 tensor ({m}, {m}) on traj's device")
    if n_dropped.dtype != torch.int64 or n_dropped.numel() != 1 or n_dropped.device != traj.device:
        raise ValueError("n_dropped must be an int64 tensor of one element on traj's device")
    need = int(_L.lib.riab_history_moments_workspace(T, int(t_step), m, B))
    if need < 0:
        raise _L.RiabError(f"riab_history_moments_workspace failed with code {need}: {_L.strerror(need)}")
    ws = torch.empty(max(need, 1), dtype=torch.float64, device=traj.device)
    rows = (C.c_int32 * len(target_rows))(*[int(r) for r in target_rows])
    _L.check(_L.lib.riab_history_moments(arr, len(inputs), _L.ptr(traj), rows, len(target_rows), T, int(t_step), B,
                                         int(n_real), _L.ptr(moments), _L.ptr(n_dropped), _L.ptr(ws), _L.current_stream()),
             "riab_history_moments")


# ---- Gaussian-process decoders over history rows: riab_gp_predict -----------------------------------------------------
def _gp_args(inputs, train_t, sq_train, alpha, n_train):
    """The checks gp_predict and gp_predict_var share -> (the RiabFFInput array, T, B, D, Np, device)"""
    if not inputs or len(inputs) != len(train_t) or len(inputs) > 8:
        raise ValueError("1..8 inputs, one transposed training matrix each")
    T, _, B = (int(x) for x in inputs[0].shape)
    Np = (int(n_train) + 31) // 32 * 32
    dev = inputs[0].device
    arr = (_L.RiabFFInput * len(inputs))()
    for l, (x, w) in enumerate(zip(inputs, train_t)):
        if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous() or x.shape[0] != T or x.shape[2] != B or \
                x.device != dev:
            raise ValueError("inputs must be contiguous float32 (T, n_l, B) with equal T, B and device")
        if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.shape[0] != x.shape[1] or \
                w.shape[1] != Np or w.device != dev:
            raise ValueError(f"train_t[l] must be contiguous float32 (n_l, {Np}) on the inputs' device")
        arr[l].rates, arr[l].wt, arr[l].n_in = x.data_ptr(), w.data_ptr(), int(x.shape[1])
    if sq_train.dtype != torch.float32 or tuple(sq_train.shape) != (Np,) or not sq_train.is_contiguous() or sq_train.device != dev:
        raise ValueError(f"sq_train must be a contiguous float32 tensor ({Np},) on the inputs' device")
    if alpha.dtype != torch.float32 or alpha.dim() != 2 or alpha.shape[1] != Np or not alpha.is_contiguous() or \
            alpha.device != dev:
        raise ValueError(f"alpha must be a contiguous float32 tensor (D, {Np}) on the inputs' device")
    return arr, T, B, int(alpha.shape[0]), Np, dev


@_register("gp_predict(Tensor[] inputs, Tensor[] train_t, Tensor sq_train, Tensor alpha, int n_train, float inv_two_ell2) "
           "-> Tensor", lambda inputs, train_t, sq_train, alpha, n_train, inv_two_ell2:
           inputs[0].new_empty((inputs[0].shape[0], alpha.shape[0], inputs[0].shape[2])))
def gp_predict(inputs: List[Tensor], train_t: List[Tensor], sq_train: Tensor, alpha: Tensor, n_train: int,
               inv_two_ell2: float) -> Tensor:
    """The predictive mean of an RBF Gaussian process over rate rows (riab_gp_predict: fp32 matrix cores, exponential and
    alpha contraction fused): out[t][d][b] = sum_{j < n_train} exp(-max(0, |x*|^2 + |x_j|^2 - 2 x*.x_j) inv_two_ell2)
    alpha[d][j], x* the concatenated inputs_l[t, :, b].  inputs_l float32 (T, n_l, B); train_t_l float32 (n_l, Np): the
    training matrix of input l TRANSPOSED, Np = n_train rounded up to 32, zero padded; sq_train float32 (Np,) = |x_j|^2;
    alpha float32 (D, Np), D = 1..4, zero padded.  Returns float32 (T, D, B)."""
    arr, T, B, D, _, dev = _gp_args(inputs, train_t, sq_train, alpha, n_train)
    out = torch.empty((T, D, B), dtype=torch.float32, device=dev)
    _L.check(_L.lib.riab_gp_predict(arr, len(inputs), _L.ptr(sq_train), _L.ptr(alpha), D, int(n_train), float(inv_two_ell2), T,
                                    B, _L.ptr(out), _L.current_stream()), "riab_gp_predict")
    return out


@_register("gp_predict_var(Tensor[] inputs, Tensor[] train_t, Tensor sq_train, Tensor alpha, Tensor linv_t, int n_train, "
           "float inv_two_ell2, Tensor(a!) workspace, bool with_mean=True) -> (Tensor, Tensor)",
           lambda inputs, train_t, sq_train, alpha, linv_t, n_train, inv_two_ell2, workspace, with_mean=True:
           (inputs[0].new_empty((inputs[0].shape[0], inputs[0].shape[2])),
            inputs[0].new_empty((inputs[0].shape[0], alpha.shape[0] if with_mean else 0, inputs[0].shape[2]))))
def gp_predict_var(inputs: List[Tensor], train_t: List[Tensor], sq_train: Tensor, alpha: Tensor, linv_t: Tensor, n_train: int,
                   inv_two_ell2: float, workspace: Tensor, with_mean: bool = True):
    """The predictive variance of an RBF Gaussian process over rate rows, in sklearn's formulation (riab_gp_predict_var, two
    launches): var[t][b] = max(0, 1 - |L^-1 k*|^2), k*_j the kernel value gp_predict sums.  Arguments as gp_predict, and
    linv_t float32 (Np, Np): linv_t[j][i] = (L^-1)[i][j] of K + alpha I = L L^T, zero above the diagonal of L^-1 and in the
    padding; workspace: a contiguous float32 tensor of at least T Np B elements, overwritten with k* as (T, Np, B).  Returns
    (var float32 (T, B), mean float32 (T, D, B) with gp_predict's bits, or (T, 0, B) with with_mean=False)."""
    arr, T, B, D, Np, dev = _gp_args(inputs, train_t, sq_train, alpha, n_train)
    if linv_t.dtype != torch.float32 or tuple(linv_t.shape) != (Np, Np) or not linv_t.is_contiguous() or linv_t.device != dev:
        raise ValueError(f"linv_t must be a contiguous float32 tensor ({Np}, {Np}) on the inputs' device")
    if workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != dev or \
            workspace.numel() < T * Np * B:
        raise ValueError(f"workspace must be a contiguous float32 tensor of at least T Np B = {T * Np * B} elements")
    var = torch.empty((T, B), dtype=torch.float32, device=dev)
    mean = torch.empty((T, D if with_mean else 0, B), dtype=torch.float32, device=dev)
    _L.check(_L.lib.riab_gp_predict_var(arr, len(inputs), _L.ptr(sq_train), _L.ptr(alpha), D, int(n_train), float(inv_two_ell2),
                                        _L.ptr(linv_t), T, B, _L.ptr(workspace), _L.ptr(var),
                                        _L.ptr(mean) if with_mean else None, _L.current_stream()), "riab_gp_predict_var")
    return var, mean


# ---- Bayesian decoding from spikes: riab_history_window_counts, riab_bayes_decode --------------------------------------
@_register("history_window_counts(Tensor rows, int row0, int window, Tensor(a!) counts) -> ()",
           lambda rows, row0, window, counts: None)
def history_window_counts(rows: Tensor, row0: int, window: int, counts: Tensor) -> None:
    """The spike counts of windows of `window` consecutive history rows (riab_history_window_counts), in place, piece by
    piece: counts[(row0 + r) // window] += rows[r].  rows: uint8 (T, n, B), one piece of a spike history whose first row
    is selected row `row0`; counts: uint8 (n_windows, n, B), ADDED to (rows of windows >= n_windows are ignored)."""
    if rows.dtype != torch.uint8 or rows.dim() != 3 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous uint8 tensor (T, n, B)")
    T, n, B = (int(x) for x in rows.shape)
    if counts.dtype != torch.uint8 or counts.dim() != 3 or tuple(counts.shape[1:]) != (n, B) or not counts.is_contiguous() \
            or counts.device != rows.device:
        raise ValueError(f"counts must be a contiguous uint8 tensor (n_windows, {n}, {B}) on the rows' device")
    _L.check(_L.lib.riab_history_window_counts(_L.ptr(rows), T, n, B, int(row0), int(window), int(counts.shape[0]),
                                               _L.ptr(counts), _L.current_stream()), "riab_history_window_counts")


@_register("bayes_decode(Tensor[] inputs, Tensor[] log_rates, Tensor bias, Tensor centres, int n_bins, float scale, "
           "int block_tiles=0) -> Tensor", lambda inputs, log_rates, bias, centres, n_bins, scale, block_tiles=0:
           bias.new_empty((inputs[0].shape[0], 6, inputs[0].shape[2])))
def bayes_decode(inputs: List[Tensor], log_rates: List[Tensor], bias: Tensor, centres: Tensor, n_bins: int, scale: float,
                 block_tiles: int = 0) -> Tensor:
    """Poisson maximum-likelihood decoding of every (window, lane) sample (riab_bayes_decode: fp32 matrix cores, bias and
    running softmax fused): l_j = sum_c k_c log_rates[c][j] + bias[j] over the bins j < n_bins, out[t, :, b] = (posterior
    mean x, y; MAP centre x, y — the lowest j among the maxima —; logsumexp l; softmax(l) at the MAP bin), six NaNs where
    no bin has a finite bias.  inputs_l: uint8 counts (T, n_l, B), or float32 rates (T, n_l, B) which are multiplied by
    `scale` (the window's duration); log_rates_l float32 (n_l, Jp), Jp a multiple of 32 >= n_bins; bias float32 (Jp,), -inf
    for a bin that is not admissible; centres float32 (2, Jp).  block_tiles: 0, or 1 / 2 / 4 to force the number of 32-bin
    tiles per block (the results do not depend on it).  Returns float32 (T, 6, B)."""
    if not inputs or len(inputs) != len(log_rates) or len(inputs) > 8:
        raise ValueError("1..8 inputs, one log-rate table each")
    T, _, B = (int(x) for x in inputs[0].shape)
    dev, dtype = inputs[0].device, inputs[0].dtype
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError("inputs must be uint8 counts or float32 rates")
    if bias.dtype != torch.float32 or bias.dim() != 1 or not bias.is_contiguous() or bias.device != dev:
        raise ValueError("bias must be a contiguous float32 tensor (Jp,) on the inputs' device")
    Jp = int(bias.shape[0])
    arr = (_L.RiabFFInput * len(inputs))()
    for l, (x, w) in enumerate(zip(inputs, log_rates)):
        if x.dtype != dtype or x.dim() != 3 or not x.is_contiguous() or x.shape[0] != T or x.shape[2] != B or x.device != dev:
            raise ValueError("inputs must be contiguous (T, n_l, B) tensors of one dtype with equal T, B and device")
        if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.shape[0] != x.shape[1] or \
                w.shape[1] != Jp or w.device != dev:
            raise ValueError(f"log_rates[l] must be contiguous float32 (n_l, {Jp}) on the inputs' device")
        arr[l].rates, arr[l].wt, arr[l].n_in = x.data_ptr(), w.data_ptr(), int(x.shape[1])
    if centres.dtype != torch.float32 or tuple(centres.shape) != (2, Jp) or not centres.is_contiguous() or centres.device != dev:
        raise ValueError(f"centres must be a contiguous float32 tensor (2, {Jp}) on the inputs' device")
    out = torch.empty((T, _L.BAYES_OUT_ROWS, B), dtype=torch.float32, device=dev)
    _L.check(_L.lib.riab_bayes_decode(arr, len(inputs), 1 if dtype == torch.uint8 else 0, float(scale), _L.ptr(bias),
                                      _L.ptr(centres), int(n_bins), Jp, T, B, _L.ptr(out), int(block_tiles),
                                      _L.current_stream()), "riab_bayes_decode")
    return out


def bayes_filter_splits(Jp: int) -> int:
    """RIAB_BAYES_FILTER_SPLITS(Jp): how many ranges the bins are split into (a function of Jp alone)"""
    return Jp // 32 if Jp <= 512 else (Jp + 127) // 128


def bayes_filter_workspace_floats(Jp: int, B: int) -> int:
    """RIAB_BAYES_FILTER_WORKSPACE_FLOATS(Jp, B): the partial softmax states [S][5][B] and one 32-bit flag per column"""
    return (5 * bayes_filter_splits(Jp) + 1) * B


def bayes_smooth_workspace_floats(Jp: int, B: int) -> int:
    """RIAB_BAYES_SMOOTH_WORKSPACE_FLOATS(Jp, B): the partial states of gamma [S][5][B], the ceil(S / 4) partials of c and
    one 32-bit cut flag per column"""
    S = bayes_filter_splits(Jp)
    return (5 * S + (S + 3) // 4 + 1) * B


def _bayes_scan_args(loglik, taps, tensors, workspace, n_ws, restart):
    """The checks the scans over windows share -> (W, Jp, B, radius, the taps as a C array, restart as uint8 or None).
    `tensors`: (name, tensor, shape with "W" / "Jp" / "B" for loglik's sizes)."""
    if loglik.dtype != torch.float32 or loglik.dim() != 3 or not loglik.is_contiguous():
        raise ValueError("loglik must be a contiguous float32 tensor (W, Jp, B)")
    W, Jp, B = (int(x) for x in loglik.shape)
    dev, size = loglik.device, {"W": W, "Jp": Jp, "B": B}
    for name, t, shape in tensors:
        shape = tuple(size.get(d, d) for d in shape)
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{name} must be a contiguous float32 tensor {shape} on loglik's device")
    if workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != dev or \
            workspace.numel() < n_ws(Jp, B):
        raise ValueError(f"workspace must be a contiguous float32 tensor of {n_ws(Jp, B)} elements")
    if restart is not None:
        if restart.dtype == torch.bool:
            restart = restart.view(torch.uint8)
        if restart.dtype != torch.uint8 or tuple(restart.shape) != (W, B) or not restart.is_contiguous() or restart.device != dev:
            raise ValueError(f"restart must be a contiguous uint8 or bool tensor ({W}, {B}) on loglik's device")
    radius = len(taps) - 1
    if not 1 <= radius <= _L.BAYES_FILTER_MAX_RADIUS:
        raise ValueError(f"taps must hold g[0..R] for a radius R in 1..{_L.BAYES_FILTER_MAX_RADIUS}, got {len(taps)} values")
    return W, Jp, B, radius, (C.c_float * (radius + 1))(*[float(x) for x in taps]), restart


_TABLES = (("prior", ("Jp",)), ("inv_norm", ("Jp",)), ("centres", (2, "Jp")))


@_register("bayes_filter(Tensor loglik, int n_bins, int ny, int nx, float[] taps, float mixing, Tensor prior, Tensor inv_norm, "
           "Tensor centres, Tensor? restart, bool first, Tensor(a!) post, Tensor(b!) tmp, Tensor(c!) workspace, "
           "Tensor(d!) out) -> ()",
           lambda loglik, n_bins, ny, nx, taps, mixing, prior, inv_norm, centres, restart, first, post, tmp, workspace, out: None)
def bayes_filter(loglik: Tensor, n_bins: int, ny: int, nx: int, taps: List[float], mixing: float, prior: Tensor,
                 inv_norm: Tensor, centres: Tensor, restart: Optional[Tensor], first: bool, post: Tensor, tmp: Tensor,
                 workspace: Tensor, out: Tensor) -> None:
    """The Bayesian decoder's forward filter over W consecutive windows (riab_bayes_filter, two launches per window, all
    issued by one native call): l_t = loglik[t] + log pred_t with pred_t the last posterior carried through a Gaussian step of
    taps g[0..R] (restricted to admissible bins, normalised per source bin by `inv_norm`) mixed with the prior, pred = prior
    on a fresh column.  loglik float32 (W, Jp, B); taps R + 1 floats; prior, inv_norm float32 (Jp,); centres float32 (2, Jp);
    restart uint8 / bool (W, B) or None; first: a new run, else the state in post / tmp / workspace is continued; post, tmp
    float32 (Jp, B); workspace float32 of `bayes_filter_workspace_floats(Jp, B)` elements; out float32 (W, 6, B), written."""
    named = [(n, t, s) for (n, s), t in zip(_TABLES, (prior, inv_norm, centres))]
    named += [("post", post, ("Jp", "B")), ("tmp", tmp, ("Jp", "B")), ("out", out, ("W", _L.BAYES_OUT_ROWS, "B"))]
    W, Jp, B, radius, g, restart = _bayes_scan_args(loglik, taps, named, workspace, bayes_filter_workspace_floats, restart)
    _L.check(_L.lib.riab_bayes_filter(_L.ptr(loglik), W, int(n_bins), Jp, int(ny), int(nx), B, radius, g, float(mixing),
                                      _L.ptr(prior), _L.ptr(inv_norm), _L.ptr(centres),
                                      None if restart is None else _L.ptr(restart), 1 if first else 0, _L.ptr(post),
                                      _L.ptr(tmp), _L.ptr(workspace), _L.ptr(out), _L.current_stream()), "riab_bayes_filter")


@_register("bayes_filter_keep(Tensor loglik, int n_bins, int ny, int nx, float[] taps, float mixing, Tensor prior, "
           "Tensor inv_norm, Tensor centres, Tensor? restart, bool first, Tensor(a!) ells, Tensor(b!) tmp, "
           "Tensor(c!) workspace, Tensor(d!) out) -> ()",
           lambda loglik, n_bins, ny, nx, taps, mixing, prior, inv_norm, centres, restart, first, ells, tmp, workspace, out: None)
def bayes_filter_keep(loglik: Tensor, n_bins: int, ny: int, nx: int, taps: List[float], mixing: float, prior: Tensor,
                      inv_norm: Tensor, centres: Tensor, restart: Optional[Tensor], first: bool, ells: Tensor, tmp: Tensor,
                      workspace: Tensor, out: Tensor) -> None:
    """`bayes_filter` with every window's l kept (riab_bayes_filter_keep): ells float32 (W, Jp, B) stands in post's place,
    window w going through ells[w]; the same kernels and the same bits in out, tmp and the workspace.  What `bayes_smooth`
    reads."""
    named = [(n, t, s) for (n, s), t in zip(_TABLES, (prior, inv_norm, centres))]
    named += [("ells", ells, ("W", "Jp", "B")), ("tmp", tmp, ("Jp", "B")), ("out", out, ("W", _L.BAYES_OUT_ROWS, "B"))]
    W, Jp, B, radius, g, restart = _bayes_scan_args(loglik, taps, named, workspace, bayes_filter_workspace_floats, restart)
    _L.check(_L.lib.riab_bayes_filter_keep(_L.ptr(loglik), W, int(n_bins), Jp, int(ny), int(nx), B, radius, g, float(mixing),
                                           _L.ptr(prior), _L.ptr(inv_norm), _L.ptr(centres),
                                           None if restart is None else _L.ptr(restart), 1 if first else 0, _L.ptr(ells),
                                           _L.ptr(tmp), _L.ptr(workspace), _L.ptr(out), _L.current_stream()),
             "riab_bayes_filter_keep")


@_register("bayes_smooth(Tensor loglik, Tensor ells, Tensor filtered, int n_bins, int ny, int nx, float[] taps, float mixing, "
           "Tensor prior, Tensor inv_norm, Tensor centres, Tensor? restart, bool last, Tensor(a!) beta, Tensor(b!) tmp, "
           "Tensor(c!) workspace, Tensor(d!) out) -> ()",
           lambda loglik, ells, filtered, n_bins, ny, nx, taps, mixing, prior, inv_norm, centres, restart, last, beta, tmp,
           workspace, out: None)
def bayes_smooth(loglik: Tensor, ells: Tensor, filtered: Tensor, n_bins: int, ny: int, nx: int, taps: List[float],
                 mixing: float, prior: Tensor, inv_norm: Tensor, centres: Tensor, restart: Optional[Tensor], last: bool,
                 beta: Tensor, tmp: Tensor, workspace: Tensor, out: Tensor) -> None:
    """The backward pass behind `bayes_filter_keep` over W consecutive windows, last to first (riab_bayes_smooth, two launches
    per window, all issued by one native call): out[t] = the six rows of the smoothed posterior p(x_t | every window of the
    run), row 4 the filter's; on a window where the chain is cut (the run's last, before a restart or a NaN window, a NaN
    window) the filter's six rows, copied.  loglik, ells float32 (W, Jp, B) and filtered float32 (W, 6, B): what the filter
    was given and what it wrote; taps, prior, inv_norm, centres, restart: the filter's; last: these are the run's last
    windows, else the state in beta / tmp / workspace continues the run to the left (a run is given rightmost first); beta,
    tmp float32 (Jp, B); workspace float32 of `bayes_smooth_workspace_floats(Jp, B)` elements; out float32 (W, 6, B), written
    (not `filtered`)."""
    named = [(n, t, s) for (n, s), t in zip(_TABLES, (prior, inv_norm, centres))]
    named += [("ells", ells, ("W", "Jp", "B")), ("filtered", filtered, ("W", _L.BAYES_OUT_ROWS, "B")), ("beta", beta, ("Jp", "B")),
              ("tmp", tmp, ("Jp", "B")), ("out", out, ("W", _L.BAYES_OUT_ROWS, "B"))]
    W, Jp, B, radius, g, restart = _bayes_scan_args(loglik, taps, named, workspace, bayes_smooth_workspace_floats, restart)
    if W and out.data_ptr() == filtered.data_ptr():
        raise ValueError("out must not be the filter's outputs")
    _L.check(_L.lib.riab_bayes_smooth(_L.ptr(loglik), _L.ptr(ells), _L.ptr(filtered), W, int(n_bins), Jp, int(ny), int(nx), B,
                                      radius, g, float(mixing), _L.ptr(prior), _L.ptr(inv_norm), _L.ptr(centres),
                                      None if restart is None else _L.ptr(restart), 1 if last else 0, _L.ptr(beta),
                                      _L.ptr(tmp), _L.ptr(workspace), _L.ptr(out), _L.current_stream()), "riab_bayes_smooth")
