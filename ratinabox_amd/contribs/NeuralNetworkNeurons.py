"""`NeuralNetworkNeurons` — the rates of other populations through a user's `torch.nn.Module`, on the device
(reference ratinabox/contribs/NeuralNetworkNeurons.py).

    Env = Environment(); Ag = Agent(Env, {"n_agents": 1024})
    PCs = PlaceCells(Ag); GCs = GridCells(Ag)
    NNs = NeuralNetworkNeurons(Ag, {"input_layers": [PCs, GCs], "NeuralNetworkModule": my_module})

The input populations' rates are concatenated along the cell axis, passed through the module, and come back as a `Neurons`
population: `update()`, history, OU noise, spikes, `get_state()`, `Agent.simulate()` and use as an input layer of
FeedForwardLayer / ValueNeuron / SuccessorFeatures all work through the base class.

Two engines, chosen per call (`N.engine` says which):

  "fused"  the module is a plain multi-layer perceptron — this package's `MultiLayerPerceptron` or an `nn.Sequential`
           (nested allowed) of `nn.Linear` leaves, each followed by at most one of ReLU / Tanh / Sigmoid / Softplus (default
           beta, threshold) / Identity, first leaf a Linear, float32 contiguous parameters on the agent's device, every
           hidden width <= 128, at most 8 Linears and 8 input populations.  ONE launch (`riab_mlp_forward`,
           csrc/riab_mlp.hip) runs all layers on the fp32 matrix cores with the hidden activations kept in registers.  The
           kernel reads `nn.Linear`'s own weight and bias storage in place, and the pointers are re-read from the
           parameters at every call: an optimiser step, `load_state_dict` or an in-place edit is seen by the next
           `update()` with no refresh call and nothing to go stale.
  "torch"  anything else (a custom `forward`, LayerNorm, Dropout, a hidden width of 129, a `.double()` module, or
           `params["engine"] = "torch"`): the module itself runs under `torch.no_grad()` on the agent's device and the
           current stream, on the rates permuted to `(positions, n_in)`.

The constructor moves the module to the agent's device with `module.to(device)`.  `nn.Module.to` moves parameters in
place: the Parameter objects keep their identity, so an optimiser built BEFORE the population was constructed keeps
working.

Training: `firingrate_torch` is a property.  On access it runs the module through torch autograd on the device, on the
`(n_agents, n_in)` tensor of the input layers' CURRENT rates (`requires_grad=True`), and returns `(n_agents, n)` attached
to the graph — the reference's convention, the opposite of `firingrate`'s `(n, n_agents)`.  It is lazy, so the per-step loop
does not pay for a second forward pass; read it BEFORE the input populations are updated again, or it describes the new
inputs.  `get_state(..., save_torch=True)` stores the attached `(P, n)` result of that evaluation in the same attribute
until the next `update()`.

Step plans: `_population()` raises NotImplementedError — the step plan's population record is frozen by the ABI and has
no slot for a layer list — so `Agent.make_step_plan()` raises for this population, the unchanged per-step loop stays
eager and `Agent.simulate()` serves it through the chunk engine (`Agent.engine_runs["chunks"]`): one launch per chunk of
rows.  A plan kind for it is the follow-up."""
import warnings

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..Neurons import Neurons

_L = _lib

MAX_LAYERS, MAX_HIDDEN, MAX_INPUTS = 8, 128, 8   # include/riab_hip.h RIAB_MLP_MAX_LAYERS / RIAB_MLP_MAX_HIDDEN


class MultiLayerPerceptron(nn.Module):
    """A generic ReLU network, the default core of NeuralNetworkNeurons (reference NeuralNetworkNeurons.py:126-146):
    Linear layers n_in -> n_hidden[0] -> ... -> n_out with biases, a ReLU behind every layer but the last."""

    def __init__(self, n_in=20, n_out=1, n_hidden=[20, 20]):
        nn.Module.__init__(self)
        n = [n_in] + list(n_hidden) + [n_out]
        layers = nn.ModuleList()
        for i in range(len(n) - 1):
            layers.append(nn.Linear(n[i], n[i + 1]))
            if i < len(n) - 2:
                layers.append(nn.ReLU())
        self.net = nn.Sequential(*layers)

    def forward(self, X):
        """X (n_batch, n_in) -> (n_batch, n_out), attached to the graph."""
        return self.net(X)


def _leaves(module, out):
    """The leaf modules of a MultiLayerPerceptron / (nested) nn.Sequential in evaluation order; False when the module's
    forward is not known to be that chain (exact types: a subclass may override forward)."""
    if type(module) is MultiLayerPerceptron:
        return _leaves(module.net, out)
    if type(module) is not nn.Sequential:
        return False
    for child in module:
        if type(child) in (nn.Sequential, MultiLayerPerceptron):
            if not _leaves(child, out):
                return False
        else:
            out.append(child)
    return True


def _activation_of(leaf):
    """(RIAB_ACT_* code, the kernel's 4 parameters) of an activation leaf, or None."""
    t = type(leaf)
    if t is nn.ReLU:
        return _L.ACTIVATIONS["relu"], (1.0, 0.0, 0.0, 0.0)
    if t is nn.Tanh:
        return _L.ACTIVATIONS["tanh"], (1.0, 0.0, 0.0, 0.0)
    if t is nn.Sigmoid:       # (max_fr 1, min_fr 0, mid_x 0, beta 1)
        return _L.ACTIVATIONS["sigmoid"], (1.0, 0.0, 0.0, 1.0)
    if t is nn.Softplus:      # the kernel's softplus switches to the identity at 20, torch's default threshold
        if float(leaf.beta) == 1.0 and float(leaf.threshold) == 20.0:
            return _L.ACTIVATIONS["softmax"], (1.0, 0.0, 0.0, 0.0)
        return None
    if t is nn.Identity:
        return _L.ACTIVATIONS["linear"], (0.0, 0.0, 0.0, 0.0)
    return None


def lower_module(module, n_in=None):
    """The module as the layer list of `riab_mlp_forward`: [(nn.Linear, activation code, (p0, p1, p2, p3)), ...], or None
    when the module is not a plain multi-layer perceptron within the kernel's limits (see the module docstring).  Looks
    at the structure only; `NeuralNetworkNeurons._lowered()` adds the checks on the parameters' dtype, layout and device."""
    leaves = []
    if not _leaves(module, leaves) or not leaves or type(leaves[0]) is not nn.Linear:
        return None
    layers = []
    for leaf in leaves:
        if type(leaf) is nn.Linear:
            layers.append([leaf, _L.ACTIVATIONS["linear"], (0.0, 0.0, 0.0, 0.0), False])
            continue
        act = _activation_of(leaf)
        if act is None or layers[-1][3]:      # an unknown leaf, or a second activation behind the same Linear
            return None
        layers[-1][1], layers[-1][2], layers[-1][3] = act[0], act[1], True
    if len(layers) > MAX_LAYERS:
        return None
    for i, (lin, _a, _p, _h) in enumerate(layers):
        if i + 1 < len(layers) and (lin.out_features > MAX_HIDDEN or layers[i + 1][0].in_features != lin.out_features):
            return None
    if n_in is not None and layers[0][0].in_features != int(n_in):
        return None
    return [(lin, a, p) for lin, a, p, _h in layers]


class NeuralNetworkNeurons(Neurons):
    """See the module docstring.  Parameters: `input_layers` (a non-empty list of Neurons of the same Agent, all given at
    initialisation), `NeuralNetworkModule` (any nn.Module whose forward maps (n_batch, n_in) to (n_batch, n_out)) OR `n`
    (then a default `MultiLayerPerceptron(n_in, n, [20, 20])` is built, with a warning) — giving both or neither is a
    ValueError, as in the reference —, `name`, and the batched extension `engine` ("auto" | "torch")."""

    default_params = {
        "n": None,
        "input_layers": [],
        "NeuralNetworkModule": None,
        "name": "NeuralNetworkNeurons",
        # --- batched extension (not in the reference) ---
        "engine": "auto",   # "torch": always run the module itself, never the fused kernel
    }

    def __init__(self, Agent, params={}):
        self.Agent = Agent
        p = dict(__class__.default_params)
        p.update(params)   # (not deep-copied: the module and the input layers are the caller's objects)
        input_layers = p["input_layers"]
        assert isinstance(input_layers, list), "param['input_layers'] must be a list of Neurons."
        assert len(input_layers) > 0, ("No input layers have been provided. Hand them in in the params dictionary "
                                       "params['input_layers']=[list,of,inputs]")
        n_in = sum(int(layer.n) for layer in input_layers)
        n, module = p["n"], p["NeuralNetworkModule"]
        device = Agent._device
        # n is resolved here, before Neurons.__init__ allocates the state rows
        if n is None and module is not None:
            module.to(device)
            n = int(self._probe(module, n_in, device).shape[1])
        elif n is not None and module is None:
            module = MultiLayerPerceptron(n_in=n_in, n_out=int(n), n_hidden=[20, 20]).to(device)
            warnings.warn(f"No NeuralNetworkModule was provided so a default MLP with {n_in} inputs, {n} outputs and 2 "
                          "hidden ReLU layers of size 20 will be used. Alternatively provide one in the "
                          "params['NeuralNetworkModule']=<any-torch-nn.Module-with-a-.forward()-method> and don't set 'n'.")
        elif n is not None and module is not None:
            raise ValueError("You provided both 'n' and `NeuralNetworkModule` as parameters. These are mutually exclusive. "
                             "Either provide 'NeuralNetworkModule' and no 'n' (the output size of the NeuralNetworkModule "
                             "will be used as the number of neurons in this layer) or 'n' and no 'NeuralNetworkModule (a "
                             "default MLP will be initialised)")
        else:
            raise ValueError("You provided neither a 'NeuralNetworkModule' nor 'n' as parameters. Either provide "
                             "'NeuralNetworkModule' and no 'n' (the output size of the NeuralNetworkModule will be used as "
                             "the number of neurons in this layer) or 'n' and no 'NeuralNetworkModule (a default MLP will "
                             "be initialised)")
        self._probe(module, n_in, device)
        p["n"], p["NeuralNetworkModule"] = int(n), module
        self.params = p
        self._engine_request = "auto"
        self._lower_cache = None
        self._torch_saved = None
        super().__init__(Agent, p)
        if self._engine_request not in ("auto", "torch"):
            raise ValueError(f"params['engine'] must be 'auto' or 'torch', got {self._engine_request!r}")
        self.n_in = n_in
        for layer in self.input_layers:
            if layer.Agent is not Agent:
                raise ValueError(f"input layer {layer.name} belongs to another Agent")

    @staticmethod
    def _module_dtype(module):
        for q in module.parameters():
            if q.is_floating_point():
                return q.dtype
        return torch.float32

    @classmethod
    def _probe(cls, module, n_in, device):
        """The reference's check that the module takes (1, n_in) (NeuralNetworkNeurons.py:66-70)."""
        try:
            with torch.no_grad():
                y = module(torch.zeros(1, n_in, dtype=cls._module_dtype(module), device=device))
            assert y.dim() == 2 and y.shape[0] == 1
            return y
        except Exception:
            raise ValueError(f"You provided inputs layers with a total of {n_in} neurons but the NeuralNetworkModule you "
                             f"provided does not accept inputs of size (1,{n_in}) so they are incompatible") from None

    # ---- which engine ------------------------------------------------------------------------------
    @property
    def engine(self):
        """"fused" (riab_mlp_forward) or "torch": what the next call will run, decided from the module as it is now."""
        return "fused" if self._lowered() is not None else "torch"

    @engine.setter
    def engine(self, value):   # (the params dictionary's "engine" entry arrives here; reading gives the engine in use)
        self._engine_request = value

    def _lowered(self):
        """The module's layer list for the kernel, or None (torch engine).  The structural part is cached on the
        identity and type of every submodule; the parameters are looked at on every call (`.double()`, `.to()` or an
        assignment replace them without touching the structure)."""
        if self._engine_request == "torch" or len(self.input_layers) > MAX_INPUTS:
            return None
        module = self.NeuralNetworkModule
        key = tuple((id(m), type(m), getattr(m, "beta", None), getattr(m, "threshold", None)) for m in module.modules())
        hit = self._lower_cache
        if hit is None or hit[0] != key:
            hit = self._lower_cache = (key, lower_module(module, self.n_in))
        layers = hit[1]
        if layers is None:
            return None
        dev = self._device
        for lin, _act, _p in layers:
            for q, shape in ((lin.weight, (lin.out_features, lin.in_features)), (lin.bias, (lin.out_features,))):
                if q is None:
                    continue
                if q.dtype != torch.float32 or tuple(q.shape) != shape or not q.is_contiguous() or \
                        q.device.type != dev.type or (dev.type == "cuda" and dev.index is not None and
                                                      q.device.index != dev.index):
                    return None
        if layers[-1][0].out_features != int(self.n):
            return None
        return layers

    def lowered_layers(self):
        """[((n_out, n_in), activation code, (p0, p1, p2, p3), bias Parameter or None), ...] as the fused engine would be
        given them, or None on the torch engine."""
        layers = self._lowered()
        if layers is None:
            return None
        return [((lin.out_features, lin.in_features), act, tuple(p), lin.bias) for lin, act, p in layers]

    # ---- the forward pass on rows ---------------------------------------------------------------------
    def _forward(self, xs, T, B, out, stream):
        """out[T][n][B] = module(concatenated xs), xs[l] float32 [T][n_l][B] on the device."""
        layers = self._lowered()
        if layers is not None:
            from .. import ops
            ops.mlp_launch(xs, [lin.weight for lin, _a, _p in layers], [lin.bias for lin, _a, _p in layers],
                           [a for _l, a, _p in layers], [p for _l, _a, p in layers], out, stream)
            self._keep = (xs, out)
            return
        module = self.NeuralNetworkModule
        with torch.no_grad():   # (current stream: Agent.simulate()'s chunk engine has entered its rate stream)
            x = torch.cat([t.reshape(T, -1, B) for t in xs], dim=1) if len(xs) > 1 else xs[0].reshape(T, -1, B)
            x = x.permute(0, 2, 1).reshape(T * B, self.n_in).to(self._module_dtype(module))
            y = module(x)
            out.reshape(T, int(self.n), B).copy_(y.reshape(T, B, int(self.n)).permute(0, 2, 1))

    def _population(self, plan_index=None):
        raise NotImplementedError(f"{self.name}: a step plan cannot hold a NeuralNetworkNeurons population (the plan's "
                                  "population record has no layer list); update() and simulate() serve it")

    # ---- Neurons plumbing ------------------------------------------------------------------------------
    def _launch(self, px, py, hx, hy, pos_ld, T, B, rates, spikes, u_in, dt, step0, from_f64=False, stream=None):
        """update() path: the inputs are the input layers' LAST firing rates (evaluate_at='last')."""
        stream = _L.current_stream() if stream is None else stream
        xs = [layer._rates.reshape(1, *layer._rates.shape) for layer in self.input_layers]
        self._torch_saved = None
        self._forward(xs, 1, self._Bp, rates, stream)
        if spikes is not None:
            io = self._io(None, None, None, None, self._Bp, 1, self._Bp, rates, spikes, u_in, dt, step0)
            _L.check(_L.lib.riab_spikes(io, int(self.n), stream), "riab_spikes")

    def update(self, **kwargs):
        """Neurons.update(): rates from the input layers' last rates (+ OU noise), spikes, history.  The attached
        tensor is not computed here: read `firingrate_torch` when it is needed."""
        kwargs.pop("save_torch", None)
        super().update(**kwargs)

    def _input_rows(self, evaluate_at, kwargs):
        """([input rates [1, n_l, Pp]], P, Pp) for get_state's `evaluate_at`."""
        if evaluate_at == "last":
            return [layer._rates.reshape(1, *layer._rates.shape) for layer in self.input_layers], self._B, self._Bp
        xs, P = [], None
        for layer in self.input_layers:
            x = layer.get_state_tensor(evaluate_at, **kwargs)
            P = layer._last_P
            xs.append(x.reshape(1, *x.shape).contiguous())
        return xs, P, int(xs[0].shape[-1])

    def get_state_tensor(self, evaluate_at="last", save_torch=False, **kwargs):
        """Device rates float32 `[n, P_padded]`.  "last" (default): from the input layers' last rates; anything else is
        handed to each input's get_state_tensor(evaluate_at, **kwargs) and the results are fed through."""
        xs, P, Pp = self._input_rows(evaluate_at, kwargs)
        self._last_P = P
        if P == 0:
            return torch.empty((int(self.n), 0), dtype=torch.float32, device=self._device)
        out = torch.empty((1, int(self.n), Pp), dtype=torch.float32, device=self._device)
        self._forward(xs, 1, Pp, out, _L.current_stream())
        if save_torch:
            self._torch_saved = self._attached(xs, P)
        return out[0]

    def get_state(self, evaluate_at="last", save_torch=False, **kwargs):
        """Firing rates `(n, P)` float64 on the host, detached (reference NeuralNetworkNeurons.py:74-104).
        `save_torch=True` also stores the attached `(P, n)` tensor in `firingrate_torch`."""
        t = self.get_state_tensor(evaluate_at, save_torch=save_torch, **kwargs)
        return t[:, :self._last_P].cpu().numpy().astype(np.float64)

    def _attached(self, xs, P):
        """The module through torch autograd on the device: (P, n_in) inputs with requires_grad -> (P, n) attached."""
        x = torch.cat([t.reshape(t.shape[-2], t.shape[-1])[:, :P] for t in xs], dim=0).t().contiguous()
        x = x.to(self._module_dtype(self.NeuralNetworkModule)).detach().requires_grad_(True)
        self.inputs_torch = x
        return self.NeuralNetworkModule(x)

    @property
    def firingrate_torch(self):
        """`(n_agents, n)` attached to the autograd graph (see the module docstring): computed on access from the input
        layers' current rates, or the result `get_state(save_torch=True)` stored since the last update()."""
        if self._torch_saved is not None:
            return self._torch_saved
        self.Agent._sync_plan()
        return self._attached([layer._rates for layer in self.input_layers], self._B)

    def _rates_from_trajectory(self, traj, out, t0, tc, step0, dt, stream):
        """Agent.simulate()'s chunk engine: one launch per chunk on the input layers' rows of the same chunk, read in
        place; then, like every population, the OU noise pass and the spikes on the final rates."""
        outs = self.Agent._sim_outs
        order = list(outs)
        xs = []
        for layer in self.input_layers:
            if layer not in outs or order.index(layer) >= order.index(self):
                raise ValueError(f"simulate(): input layer {layer.name} must be in `neurons` BEFORE {self.name} "
                                 "(its rows of the chunk are read in place)")
            xs.append(layer._chunk_view(outs[layer], t0, tc)[0])
        fr, sp = self._chunk_view(out, t0, tc)
        self._torch_saved = None
        self._forward(xs, tc, self._Bp, fr, stream)
        if self.noise_std != 0:
            theta_dt, sigma_dt = self._noise_constants(dt)
            Ag = self.Agent
            rc = _L.lib.riab_neuron_noise(_L.ptr(self._noise), _L.ptr(fr), None, int(self.n), self._Bp, int(tc),
                                          theta_dt, sigma_dt, int(Ag.rng_seed), int(step0 + 1),
                                          int(self.pop_id), int(Ag.agent_id0), stream)
            _L.check(rc, "riab_neuron_noise")
        if sp is not None:
            io = self._io(None, None, None, None, self._Bp, tc, self._Bp, fr, sp, None, dt, step0 + 1)
            _L.check(_L.lib.riab_spikes(io, int(self.n), stream), "riab_spikes")
