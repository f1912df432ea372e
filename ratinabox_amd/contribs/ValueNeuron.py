"""`ValueNeuron` — continuous-time TD(lambda) value learning on the device (reference
ratinabox/contribs/ValueNeuron.py), for a batched Agent.

ONE learner is fed by the whole batch: the weights `inputs[name]["w"]` are one `(n, n_in)` matrix per input layer,
exactly like `FeedForwardLayer`, so `get_state(evaluate_at=None, pos=...)`, rate maps and `simulate()` of a frozen
learner keep working; every agent (lane) has its own value, `firingrate_deriv`, `td_error` and eligibility traces.
Per step and lane the reference's rule applies (ValueNeuron.py:59-101):

    update():            V    = act(sum_l W_l phi_l + biases)            (riab_feedforward)
                         dVdt = (V - V_last) / dt
                         e_l  = dt * phi_l + (1 - dt / tau_e) * e_l      (tau_e == 0: e_l = phi_l)
    update_weights(r):   td   = r + dVdt - V / tau
                         W_l += dt * eta * MEAN_b (td * V')[:, b] (x) e_l[:, b]  -  eta * dt * L2 * W_l

The weight change is the MEAN over the agents of the reference's per-agent outer product: with one agent it is the
reference's rule to the letter.  Everything runs on the device (csrc/riab_td.hip): `update_weights()`
takes `env.get_reward()` of a `TaskEnvironment` as it is, `reset(lanes=env.terminal)` takes its device mask, and no
call synchronises or copies to the host.  `learn(reward)` is `update()` + `update_weights(reward)` with the trace update
riding in the gradient kernel (the traces are read once per step instead of twice).

The device copy of the weights is the master: `inputs[name]["w"]` READS them back (float64 `(n, n_in)`, a copy: edit
it and assign it back, `inputs[name]["w"] = w`) and assigning replaces the device weights.

A `StepPlan` (`Ag.make_step_plan()`, `env.make_step_plan()`) holds a learning learner: every plan step then ends with
`learn(reward)` and, in a task plan with `auto_reset`, `reset(lanes=terminal)` — in that order, BEFORE the task resets the
terminal lanes (plan.py: "learn, then reset") — as two launches behind the forward pass (riab_td_learn_step).  The reward
is the task's, or a device tensor bound with `plan.bind_reward(VN, tensor)`.  The plan keeps the mode it recorded:
flipping `learning` afterwards has no effect on it — rebuild the plan.  One deviation from the eager loop: a learner that
keeps a history has its `firingrate` row IN the history, so the plan's reset leaves that row as recorded, where eager
`reset()` zeroes a clone of it; only the host-visible `VN.firingrate` of a lane that has just been reset differs.

Not supported (NotImplementedError): a learner inside `Agent.simulate()` or behind the unchanged `Ag.update(); N.update()`
loop's native stepper while `learning` is True (one weight update per step needs the step's reward; set
`VN.learning = False` to freeze it — a frozen learner is a `FeedForwardLayer`), recurrent inputs, callable activations.  The learner is not sharded: `parallel.py` shards the agents
of a run over GPUs, and one learner fed by all of them would need a gradient all-reduce, the step path's first
collective — an Agent that is a shard (`agent_id0 != 0`) is refused."""
import copy

import numpy as np
import torch

from .. import _lib as _L
from ..Neurons import FeedForwardLayer, Neurons

C = _L.C


class _LearnedInput(dict):
    """`inputs[name]` of a learner: the reference's dictionary, with `"w"` and `"eligibility_trace"` kept on the device."""
    _DEVICE_KEYS = ("w", "eligibility_trace")

    def __init__(self, owner, entry):
        super().__init__(entry)
        self._owner = owner
        self.wt = None      # float32 [n_in][Mp]: W^T as riab_feedforward reads it
        self.trace = None   # float32 [n_in][Bp]

    def __getitem__(self, key):
        if key == "w" and self.wt is not None:
            n = int(self._owner.n)
            return np.ascontiguousarray(self.wt[:, :n].t().cpu().numpy().astype(np.float64))
        if key == "eligibility_trace" and self.trace is not None:
            B = self._owner._B
            a = self.trace[:, :B].cpu().numpy().astype(np.float64)
            return a[:, 0] if B == 1 else a
        return super().__getitem__(key)

    def __contains__(self, key):
        return key in self._DEVICE_KEYS or super().__contains__(key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def __setitem__(self, key, value):
        if key == "w":
            self._owner._upload_weights(self, value)
        elif key == "eligibility_trace":
            self._owner._upload_trace(self, value)
        else:
            super().__setitem__(key, value)


class ValueNeuron(FeedForwardLayer):
    """TD(lambda) value learner over the rates of its input layers (module docstring).  Parameters as in the reference:
    `tau` discount horizon, `tau_e` eligibility-trace time scale (None: tau / 4), `eta` learning rate, `L2`
    regularisation, `activation_function` (relu), `n` value neurons (one per reward signal)."""

    default_params = {
        "tau": 2,
        "tau_e": None,
        "eta": 0.001,
        "L2": 0.001,
        "activation_function": {"activation": "relu"},
        "n": 1,
        "name": "ValueNeuron",
        # --- batched extension (not in the reference) ---
        "learning": True,   # False: frozen — the layer may then run inside Agent.simulate() and step plans
    }

    def __init__(self, Agent, params={}):
        self.params = copy.deepcopy(__class__.default_params)
        self.params.update(params)
        if int(getattr(Agent, "agent_id0", 0)) != 0:
            raise NotImplementedError("a learner on a shard of the agents (parallel.py) would need a gradient all-reduce "
                                      "between the GPUs; build it on an unsharded Agent")
        super().__init__(Agent, self.params)
        if self.tau_e is None:
            self.tau_e = self.tau / 4
        n, Bp, dev = int(self.n), self._Bp, self._device
        self._v_last = torch.zeros((n, Bp), dtype=torch.float32, device=dev)
        self._dvdt = torch.zeros((n, Bp), dtype=torch.float32, device=dev)
        self._td = torch.zeros((n, Bp), dtype=torch.float32, device=dev)
        self._workspace = None

    # ---- inputs --------------------------------------------------------------------------------------------------
    def add_input(self, input_layer, w=None, w_init_scale=1, recurrent=False, **kwargs):
        if recurrent or input_layer is self:
            raise NotImplementedError("recurrent inputs: the TD rule here reads every input layer's rates of the same step")
        super().add_input(input_layer, w=w, w_init_scale=w_init_scale, recurrent=False, **kwargs)
        plain = self.inputs[input_layer.name]
        entry = _LearnedInput(self, plain)
        dict.pop(entry, "w")
        entry["w"] = plain["w"]
        entry["eligibility_trace"] = np.zeros(int(plain["n"]))
        self.inputs[input_layer.name] = entry
        self._workspace = None

    add_input_layer = add_input

    def _upload_weights(self, entry, w):
        n, n_in = int(self.n), int(dict.__getitem__(entry, "n"))
        w = np.asarray(w, dtype=np.float64)
        assert w.shape == (n, n_in), f"w must have shape ({n}, {n_in})"
        wt = np.zeros((n_in, (n + 31) // 32 * 32), dtype=np.float32)
        wt[:, :n] = w.T
        t = torch.from_numpy(wt).to(self._device)
        if entry.wt is None:
            entry.wt = t
        else:
            entry.wt.copy_(t)   # (in place: a captured graph keeps reading the same memory)

    def _upload_trace(self, entry, e):
        n_in = int(dict.__getitem__(entry, "n"))
        e = np.asarray(e, dtype=np.float32)
        e = np.broadcast_to(e.reshape(n_in, -1), (n_in, self._B))
        full = np.zeros((n_in, self._Bp), dtype=np.float32)
        full[:, :self._B] = e
        t = torch.from_numpy(full).to(self._device)
        if entry.trace is None:
            entry.trace = t
        else:
            entry.trace.copy_(t)

    def _device_weights(self, entry):
        """The master copy (the parent hashes and uploads the host matrix on every call)."""
        return entry.wt

    # ---- read-outs -----------------------------------------------------------------------------------------------
    def _rows_to_host(self, t):
        a = t[:, :self._B].cpu().numpy().astype(np.float64)
        return a[:, 0] if self._B == 1 else a

    @property
    def firingrate_deriv(self):
        return self._rows_to_host(self._dvdt)

    @property
    def td_error(self):
        return self._rows_to_host(self._td)

    @property
    def td_error_tensor(self):
        """Device TD error of the last update_weights(): float32 `[n, B_padded]`."""
        return self._td

    # ---- the ABI's argument blocks (persistent; the library reads them before the call returns) ------------------
    def _args(self):
        entries = list(self.inputs.values())
        if not entries:
            raise ValueError(f"{self.name} has no input layers")
        hit = self.__dict__.get("_td_args")
        key = (float(self.Agent.dt), float(self.tau), float(self.tau_e), float(self.eta), float(self.L2), len(entries))
        if hit is None or hit[0] != key:
            p = _L.RiabTDParams()
            p.dt, p.tau, p.tau_e, p.eta, p.L2 = key[:5]
            p.B, p.Bp, p.n, p.Mp = self._B, self._Bp, int(self.n), (int(self.n) + 31) // 32 * 32
            hit = (key, p, (_L.RiabTDLayer * len(entries))())
            self._td_args = hit
        arr = hit[2]
        for l, e in enumerate(entries):
            x = dict.__getitem__(e, "layer")._rates
            arr[l].rates, arr[l].trace, arr[l].wt, arr[l].n_in = x.data_ptr(), e.trace.data_ptr(), e.wt.data_ptr(), int(x.shape[0])
        if self._workspace is None:
            need = int(_L.lib.riab_td_workspace(hit[1], arr, len(entries)))
            if need < 0:
                _L.check(need, "riab_td_workspace")
            self._workspace = torch.empty(need, dtype=torch.float32, device=self._device)
        return hit[1], arr, len(entries)

    def _tail(self, with_trace):
        p, arr, nl = self._args()
        _L.check(_L.lib.riab_td_forward_tail(p, arr, nl, _L.ptr(self._rates), _L.ptr(self._v_last), _L.ptr(self._dvdt),
                                             1 if with_trace else 0, _L.current_stream()), "riab_td_forward_tail")

    def _reward_tensor(self, reward):
        if torch.is_tensor(reward):
            r = reward
            if r.dtype not in (torch.float32, torch.float64):
                r = r.to(torch.float64)
        else:
            r = torch.from_numpy(np.ascontiguousarray(np.asarray(reward, dtype=np.float64)))
        return r if r.device == self._device else r.to(self._device)

    def _td_update(self, reward, fuse):
        from ..ops import _reward_strides
        r = self._reward_tensor(reward)
        ld_n, ld_b = _reward_strides(r, int(self.n), self._B, self._Bp)
        p, arr, nl = self._args()
        _L.check(_L.lib.riab_td_update(p, arr, nl, _L.ptr(r), 1 if r.dtype == torch.float64 else 0, ld_n, ld_b,
                                       _L.ptr(self._rates), _L.ptr(self._dvdt), _L.ptr(self._rates_prime), _L.ptr(self._td),
                                       1 if fuse else 0, _L.ptr(self._workspace), int(self._workspace.numel()),
                                       _L.current_stream()), "riab_td_update")
        self._keep_reward = r

    # ---- the reference's entry points ----------------------------------------------------------------------------
    def update(self, **kwargs):
        """firingrate = act(W phi) through the parent, then its temporal derivative and the eligibility traces
        (ValueNeuron.py:59-77)."""
        super().update(**kwargs)
        self._tail(True)

    def update_weights(self, reward):
        """The TD rule (ValueNeuron.py:79-101).  `reward`: a scalar, an `(n,)` vector (one per value neuron, the same for
        every agent), or one per agent — `(B,)` or `(n, B)`, NumPy or a device tensor (float32 / float64, read in place:
        `env.get_reward()` goes in as it is)."""
        self._td_update(reward, False)

    def learn(self, reward, **kwargs):
        """`update(); update_weights(reward)` in three launches: the trace update rides in the gradient kernel."""
        Neurons.update(self, **kwargs)
        self._tail(False)
        self._td_update(reward, True)

    def reset(self, lanes=None):
        """Wipe trace, firing rate, its derivative and the TD error (ValueNeuron.py:103-113) of every agent, or of the
        agents selected by a boolean mask `(B,)` (device or host, e.g. `env.terminal`).  Runs on the device."""
        mask = None
        if lanes is not None:
            mask = lanes if torch.is_tensor(lanes) else torch.from_numpy(np.ascontiguousarray(np.asarray(lanes).astype(np.uint8)))
            if mask.dtype == torch.bool:
                mask = mask.contiguous().view(torch.uint8)
            elif mask.dtype != torch.uint8:
                mask = (mask != 0).view(torch.uint8)
            if mask.device != self._device:
                mask = mask.to(self._device)
            mask = mask.contiguous()
            if mask.numel() < self._B:
                raise ValueError(f"lanes must be a mask of {self._B} agents")
        if self.save_history:
            self._rates = self._rates.clone()   # (the last row of the history keeps what was recorded)
        p, arr, nl = self._args()
        rows = (C.c_void_p * 4)(self._rates.data_ptr(), self._v_last.data_ptr(), self._dvdt.data_ptr(), self._td.data_ptr())
        _L.check(_L.lib.riab_td_reset(p, arr, nl, rows, 4, _L.ptr(mask), _L.current_stream()), "riab_td_reset")
        self._keep_mask = mask

    # ---- where a learner cannot run ------------------------------------------------------------------------------
    def _refuse_while_learning(self, where):
        if self.learning:
            raise NotImplementedError(f"{self.name} is learning: {where} advances many steps per call, and one weight "
                                      "update per step needs that step's reward.  Step it with update() / "
                                      "update_weights(reward), or freeze it (`learning = False`)")

    def _population(self, plan_index=None):
        self._refuse_while_learning("a step plan")
        return super()._population(plan_index)

    def _learner_record(self, plan_index):
        """A LEARNING learner as a `StepPlan` records it: the feed-forward descriptor and the learner block of
        riab_plan_set_learner — the persistent `_args()` structures (constants, traces) and `_workspace`."""
        pop = FeedForwardLayer._population(self, plan_index)
        p, arr, nl = self._args()
        traces = (C.c_void_p * nl)(*[arr[l].trace for l in range(nl)])
        return pop, {"params": p, "traces": traces, "reward": self._plan_reward(plan_index)}

    def _plan_reward(self, plan_index):
        """Where a plan finds this learner's reward when nobody binds one: `(kind, population index)`."""
        return _L.REWARD_NONE, -1

    def _rates_from_trajectory(self, traj, out, t0, tc, step0, dt, stream):
        self._refuse_while_learning("Agent.simulate()")
        return super()._rates_from_trajectory(traj, out, t0, tc, step0, dt, stream)
