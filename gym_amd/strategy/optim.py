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
form over the arena is gym_amd.fused_optim.ArenaMuon.  AdamW8bit ("adamw8bit") is AdamW
with block-wise 8-bit moments; its fused form is gym_amd.fused_optim.ArenaAdam8bit.
"""
import math
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


ADAM8_BLOCK = 64  # elements under one scale of an 8-bit moment


def adam_scalars(group, t):
    """The scalars of an Adam / AdamW step at count t (torch's _single_tensor_adam), in
    double: what ga_adam_step and ga_adam8_step take and what AdamW8bit rounds to fp32."""
    lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
    decoupled = group["decoupled_weight_decay"]
    bc1 = 1 - b1 ** t
    bc2 = 1 - b2 ** t
    return dict(lerp_w=1 - b1, beta2=b2, one_m_beta2=1 - b2, eps=eps,
                wd_factor=(1 - lr * wd) if (decoupled and wd != 0) else 1.0,
                l2_wd=wd if (not decoupled and wd != 0) else 0.0, step_size=-(lr / bc1), bc2_sqrt=math.sqrt(bc2))


def _r32(x):
    """x (float64, or a Python scalar) rounded to fp32, as float64."""
    if not torch.is_tensor(x):
        return torch.tensor(x, dtype=torch.float32).item()
    return x.float().double()


def adam8_quantise(x, row):
    """(uint8 codes, fp32 scales) of the fp32 vector x of whole 64-element blocks with table
    row `row` of gym_amd.ops.adam8_tables (0 signed, 1 unsigned): absmax per block, x /
    absmax (0 in an all-zero block), code = the number of thresholds below it (ties to the
    lower code); in the unsigned row a value > 0 is never stored as code 0."""
    from ..ops import adam8_tables
    thr = adam8_tables(x.device)[1][row, :255].contiguous()
    xb = x.view(-1, ADAM8_BLOCK)
    am = xb.abs().amax(1) if xb.numel() else xb.new_zeros(0)
    xh = (xb.double() / am.double()[:, None]).float()  # the fp32 quotient: one rounding
    xh = torch.where(am[:, None] == 0, torch.zeros_like(xh), xh)
    q = torch.searchsorted(thr, xh.contiguous())
    if row == 1:
        q = torch.where((q == 0) & (xb > 0), torch.ones_like(q), q)
    return q.to(torch.uint8).view(-1), am


def adam8_dequantise(code, absmax, row):
    """codes[row][code] * absmax, one rounded fp32 product per element."""
    from ..ops import adam8_tables
    book = adam8_tables(code.device)[0][row]
    return (book[code.long()].view(-1, ADAM8_BLOCK) * absmax[:, None]).view(-1)


class AdamW8bit(torch.optim.Optimizer):
    """AdamW with block-wise 8-bit moments (Dettmers et al., "8-bit Optimizers via
    Block-wise Quantization"): exp_avg and exp_avg_sq are kept as uint8 codes of the
    code books of gym_amd.ops.adam8_tables under one fp32 scale per 64 elements (2.125
    bytes of state per element instead of 8), de-quantised, updated in fp32 in
    torch.optim.AdamW's op order and re-quantised in every step.  Plain torch on any
    device, per tensor, each tensor padded with zeros to whole blocks: the unfused form
    of gym_amd.fused_optim.ArenaAdam8bit (ga_adam8_step), with the same format and
    the same rounding -- every operation is computed in float64 from fp32 operands and
    rounded to fp32 once, which is the fp32 operation for + - x / sqrt and the fused
    multiply-add where ga_adam_step has one -- so the two agree wherever the kernel's true
    fma and the twice-rounded one do.  State per parameter: step, exp_avg_code,
    exp_avg_absmax, exp_avg_sq_code, exp_avg_sq_absmax."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        if isinstance(lr, torch.Tensor) or not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i, b in enumerate(betas):
            if not 0.0 <= b < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=True))

    @staticmethod
    def fresh_state(numel, device):
        """A parameter's state before its first step: zero moments (signed code 127,
        unsigned code 0, scales 0) over its whole blocks."""
        nb = -(-numel // ADAM8_BLOCK)
        return {"step": torch.tensor(0.0),
                "exp_avg_code": torch.full((nb * ADAM8_BLOCK,), 127, dtype=torch.uint8, device=device),
                "exp_avg_absmax": torch.zeros(nb, device=device),
                "exp_avg_sq_code": torch.zeros(nb * ADAM8_BLOCK, dtype=torch.uint8, device=device),
                "exp_avg_sq_absmax": torch.zeros(nb, device=device)}

    def load_state_dict(self, state_dict):
        # torch casts every state tensor to the parameter's dtype and keeps one that has it already:
        # step() writes the state in place, so it must not share memory with the dict it came from
        super().load_state_dict(state_dict)
        for st in self.state.values():
            for key in ("exp_avg_code", "exp_avg_sq_code"):
                if key in st:
                    st[key] = st[key].to(torch.uint8)
            for key in ("exp_avg_absmax", "exp_avg_sq_absmax"):
                if key in st:
                    st[key] = st[key].clone()
            if "step" in st:
                st["step"] = torch.as_tensor(float(st["step"]))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "step" not in st:
                    st.update(self.fresh_state(p.numel(), p.device))
                st["step"] += 1
                hp = {k: _r32(v) for k, v in adam_scalars(group, float(st["step"])).items()}
                n = p.numel()
                x, g = p.reshape(-1).double(), p.grad.reshape(-1).double()
                m = adam8_dequantise(st["exp_avg_code"], st["exp_avg_absmax"], 0)[:n].double()
                v = adam8_dequantise(st["exp_avg_sq_code"], st["exp_avg_sq_absmax"], 1)[:n].double()
                if hp["wd_factor"] != 1.0:
                    x = _r32(x * hp["wd_factor"])
                if hp["l2_wd"] != 0.0:
                    g = _r32(hp["l2_wd"] * x + g)
                d, w = _r32(g - m), hp["lerp_w"]
                m = _r32(w * d + m) if w < 0.5 else _r32(-d * _r32(1.0 - w) + g)  # ATen's lerp
                v = _r32(_r32(hp["one_m_beta2"] * g) * g + _r32(v * hp["beta2"]))
                denom = _r32(_r32(_r32(v.sqrt()) / hp["bc2_sqrt"]) + hp["eps"])
                x = _r32(hp["step_size"] * _r32(m / denom) + x)
                p.copy_(x.float().view_as(p))
                pad = st["exp_avg_code"].numel() - n
                for key, val, row in (("exp_avg", m, 0), ("exp_avg_sq", v, 1)):
                    code, am = adam8_quantise(torch.nn.functional.pad(val.float(), (0, pad)), row)
                    st[key + "_code"].copy_(code)
                    st[key + "_absmax"].copy_(am)
        return loss


_BY_NAME = {
    "adam": torch.optim.Adam,
    "adamw": torch.optim.AdamW,
    "sgd": torch.optim.SGD,
    "rmsprop": torch.optim.RMSprop,
    "adagrad": torch.optim.Adagrad,
    "adafactor": torch.optim.Adafactor,  # beyond the reference; fused: gym_amd.fused_optim.ArenaAdafactor
    "muon": MuonAdamW,
    "adamw8bit": AdamW8bit,  # beyond the reference; fused: gym_amd.fused_optim.ArenaAdam8bit
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
