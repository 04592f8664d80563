"""Optimizer specs: which torch.optim class to build, with which kwargs.

API and behaviour of exogym/strategy/optim.py:9-60: OptimSpec(cls, **kwargs),
OptimSpec.from_string(name, **kwargs) for adam/adamw/sgd/rmsprop/adagrad
(ValueError otherwise), .build(model), and ensure_optim_spec(optim, default,
**kwargs) which accepts None / str / OptimSpec (TypeError otherwise).

Beyond the reference: MuonAdamW ("muon"), torch.optim.Muon on the hidden matrices of
a model and torch.optim.AdamW on everything else, as one optimizer with two
parameter groups (torch's Muon refuses any parameter that is not 2-D, so the
reference's OptimSpec(torch.optim.Muon).build(model) fails on every model with a
bias, a norm or an embedding).  muon_matrix_mask is the selection rule; the fused
form over the arena is gym_amd.fused_optim.ArenaMuon.
"""
from dataclasses import dataclass
from typing import Any, Dict, Optional, Type, Union

import torch

MUON_KW = ("lr", "weight_decay", "momentum", "nesterov", "ns_coefficients", "eps", "ns_steps", "adjust_lr_fn")
ADAMW_KW = {"adamw_lr": "lr", "adamw_betas": "betas", "adamw_eps": "eps", "adamw_weight_decay": "weight_decay"}


def muon_matrix_mask(model, muon_exclude=("lm_head",), muon_params=None):
    """Per parameter of model.parameters(), in that order: True for a Muon matrix.
    The rule: requires_grad, 2-D, the `weight` of at least one nn.Linear and of no
    nn.Embedding (a tied lm_head / wte stays on AdamW), and none of the
    parameter's qualified names contains a string of `muon_exclude`.
    muon_params(name, param) -> bool replaces the rule (name: the first
    qualified name)."""
    names = {}
    for name, p in model.named_parameters(remove_duplicate=False):
        names.setdefault(id(p), []).append(name)
    if muon_params is not None:
        return [bool(muon_params(names[id(p)][0], p)) for p in model.parameters()]
    linear, embedding = set(), set()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Linear):
            linear.add(id(mod.weight))
        elif isinstance(mod, torch.nn.Embedding):
            embedding.add(id(mod.weight))
    return [bool(p.requires_grad and p.ndim == 2 and id(p) in linear and id(p) not in embedding
                 and not any(x in n for n in names[id(p)] for x in muon_exclude))
            for p in model.parameters()]


class MuonAdamW(torch.optim.Optimizer):
    """torch.optim.Muon on a model's Muon matrices (muon_matrix_mask) and
    torch.optim.AdamW (adamw_lr, adamw_betas, adamw_eps, adamw_weight_decay) on
    its other parameters.  param_groups[0] is Muon's group and param_groups[1]
    AdamW's -- the very dicts the two torch optimizers read -- so a scheduler
    such as LambdaLR scales both learning rates; the state is one dict of
    torch's per-parameter entries (momentum_buffer | step, exp_avg, exp_avg_sq).
    `model`: an nn.Module, or a parameter list with muon_mask (a bool per
    parameter).  muon_names: the qualified names of the selected matrices."""

    def __init__(self, model, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True,
                 ns_coefficients=(3.4445, -4.775, 2.0315), eps=1e-7, ns_steps=5, adjust_lr_fn=None, adamw_lr=1e-3,
                 adamw_betas=(0.9, 0.999), adamw_eps=1e-8, adamw_weight_decay=1e-2, muon_exclude=("lm_head",),
                 muon_params=None, muon_mask=None, fused=None):
        # fused: read by gym_amd.fused_optim.build_fused (True: ArenaMuon on an fp32 arena); unused here
        if isinstance(model, torch.nn.Module):
            params = list(model.parameters())
            if muon_mask is None:
                muon_mask = muon_matrix_mask(model, muon_exclude, muon_params)
            first = {}
            for name, p in model.named_parameters():
                first.setdefault(id(p), name)
            self.muon_names = [first[id(p)] for p, m in zip(params, muon_mask) if m]
        else:
            params = list(model)
            if muon_mask is None:
                raise ValueError("MuonAdamW: a parameter list needs muon_mask (a bool per parameter); "
                                 "pass the model to select by rule")
            self.muon_names = [str(i) for i, m in enumerate(muon_mask) if m]
        if len(muon_mask) != len(params):
            raise ValueError("MuonAdamW: muon_mask must hold a bool per parameter")
        self.muon_mask = [bool(m) for m in muon_mask]
        mats = [p for p, m in zip(params, self.muon_mask) if m]
        rest = [p for p, m in zip(params, self.muon_mask) if not m and p.requires_grad]
        for p in mats:
            if p.ndim != 2:
                raise ValueError(f"MuonAdamW: a Muon parameter must be 2-D, got {tuple(p.shape)}")
        self._muon = torch.optim.Muon(mats, lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov,
                                      ns_coefficients=tuple(ns_coefficients), eps=eps, ns_steps=ns_steps,
                                      adjust_lr_fn=adjust_lr_fn) if mats else None
        self._adamw = torch.optim.AdamW(rest, lr=adamw_lr, betas=tuple(adamw_betas), eps=adamw_eps,
                                        weight_decay=adamw_weight_decay) if rest else None
        groups = [o.param_groups[0] if o is not None else {"params": [], "lr": l}
                  for o, l in ((self._muon, lr), (self._adamw, adamw_lr))]
        super().__init__(groups, {})
        self._share()

    def _share(self):
        """The two torch optimizers read this optimizer's group dicts and state."""
        for o, g in zip((self._muon, self._adamw), self.param_groups):
            if o is not None:
                o.param_groups = [g]
                o.state = self.state

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._share()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for o in (self._muon, self._adamw):
            if o is not None:
                o.step()
        return loss


_BY_NAME = {
    "adam": torch.optim.Adam,
    "adamw": torch.optim.AdamW,
    "sgd": torch.optim.SGD,
    "rmsprop": torch.optim.RMSprop,
    "adagrad": torch.optim.Adagrad,
    "adafactor": torch.optim.Adafactor,  # beyond the reference; fused: gym_amd.fused_optim.ArenaAdafactor
    "muon": MuonAdamW,
}


@dataclass(init=False)
class OptimSpec:
    cls: Type[torch.optim.Optimizer] = torch.optim.AdamW
    kwargs: Dict[str, Any] = None

    def __init__(self, cls: Type[torch.optim.Optimizer], **kwargs: Any):
        self.cls = cls
        self.kwargs = kwargs

    @classmethod
    def from_string(cls, name: str, **kwargs) -> "OptimSpec":
        key = name.lower()
        if key not in _BY_NAME:
            raise ValueError(f"Unknown optimizer '{name}'. Available options: {', '.join(_BY_NAME)}")
        return cls(_BY_NAME[key], **kwargs)

    def build(self, model):
        if self.cls is MuonAdamW:  # selects the Muon matrices from the model's modules
            return MuonAdamW(model, **(self.kwargs or {}))
        params = model.parameters() if hasattr(model, "parameters") else model
        return self.cls(params, **(self.kwargs or {}))


def ensure_optim_spec(optim: Union[str, OptimSpec, None], default: Optional[OptimSpec] = None,
                      **kwargs) -> OptimSpec:
    if optim is None:
        return default if default is not None else OptimSpec(torch.optim.AdamW, **kwargs)
    if isinstance(optim, str):
        return OptimSpec.from_string(optim, **kwargs)
    if isinstance(optim, OptimSpec):
        if kwargs:
            return OptimSpec(optim.cls, **{**(optim.kwargs or {}), **kwargs})
        return optim
    raise TypeError(f"Expected str, OptimSpec, or None, got {type(optim)}")
