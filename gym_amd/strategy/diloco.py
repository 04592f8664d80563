"""DiLoCo: local inner optimizer steps, an outer step every H steps.

API of exogym/strategy/diloco.py:14-89 (optim_spec = inner optimizer,
outer_optim_spec default SGD(lr=0.7, nesterov=True, momentum=0.9), H=100;
gradient clipping when "max_norm" is passed; outer step when
local_step % H == 0 and local_step > 0).

The reference's outer step is 148 per-tensor all-reduces, a GPU->CPU copy of
every tensor on rank 0, a CPU SGD step, a CPU->GPU copy and 148 broadcasts.
Here, for an SGD-family outer optimizer, it is ONE fused kernel per node
(ga_diloco_outer: average, pseudo-gradient master - avg, momentum/Nesterov,
master update, parameter write-back) around one reduce-scatter + one
all-gather over RCCL; the master copy and momentum are fp32 and sharded over
the ranks.  torch's Adam / AdamW as the outer optimizer take the same one pass
with an Adam update (ga_diloco_outer_adam, master and both moments sharded;
fused_outer=False keeps torch's optimizer).  Any other outer optimizer class
runs torch's optimizer on a GPU master copy (replicated on every rank) fed by
the same averaging kernel (engine.TorchOuter).  build_outer_engine picks among
them for both modes -- one node per process here, K nodes per process in
gym_amd.replica -- so neither holds outer-step arithmetic of its own.

outer_compression="int8" | "int4" (default None) exchanges the pseudo-gradients
block-quantised instead of in fp32 (engine.DiLoCoOuterQuant: ga_quant_encode, one
all-gather of the payload rows, ga_diloco_outer_dequant), outer_error_feedback=True
carries each node's quantisation error into its next outer step.  SGD-family outer
optimizers only; the master and momentum are then replicated on every rank.

Streaming DiLoCo (DESIGN §3 "Streaming outer step"): num_fragments=F cuts the arena
into F fragments that take their outer steps on staggered schedules (an outer event
moves about n / F elements), outer_delay=tau applies an exchange's result tau inner
steps after it was sent, and outer_mix=alpha blends it into the live parameters,
x <- alpha x + (1 - alpha) master, instead of overwriting them.  With any of them set
build_streaming_outer returns an engine.FragmentedOuter that both modes call on every
step; a delay or a mix needs a plain SGD outer optimizer and no compression.
"""
from typing import Optional, Union

import torch

from .. import ops
from ..engine import (QUANT_BITS, DiLoCoOuter, DiLoCoOuterAdam, DiLoCoOuterQuant, DiLoCoOuterStream, FragmentedOuter,
                      TorchOuter, fragment_bounds)
from .communicate_optimize_strategy import CommunicationModule
from .optim import OptimSpec, ensure_optim_spec
from .strategy import Strategy, build_inner_optimizer, clip_and_step


def fused_sgd_hparams(spec: OptimSpec):
    """Hyper-parameters for the fused kernel if `spec` is plain torch SGD."""
    if spec.cls is not torch.optim.SGD:
        return None
    kw = dict(spec.kwargs or {})
    if kw.pop("maximize", False):
        return None
    for k in ("foreach", "fused", "differentiable"):
        kw.pop(k, None)
    defaults = torch.optim.SGD([torch.zeros(1, requires_grad=True)]).defaults
    hp = dict(lr=float(kw.pop("lr", defaults["lr"])), momentum=float(kw.pop("momentum", 0.0)),
              dampening=float(kw.pop("dampening", 0.0)), weight_decay=float(kw.pop("weight_decay", 0.0)),
              nesterov=bool(kw.pop("nesterov", False)))
    if kw:
        return None
    if hp["nesterov"] and (hp["momentum"] <= 0 or hp["dampening"] != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")
    return hp


def fused_adam_hparams(spec: OptimSpec):
    """Hyper-parameters for the fused Adam outer step (DiLoCoOuterAdam) if `spec`
    is torch's Adam (L2 decay) or AdamW (decoupled decay) with options the kernel
    covers; None keeps torch's optimizer."""
    if spec.cls not in (torch.optim.Adam, torch.optim.AdamW):
        return None
    # a stand-in kernel layer (tests) written before ga_diloco_outer_adam keeps torch's optimizer
    if not hasattr(ops, "diloco_outer_adam"):
        return None
    kw = dict(spec.kwargs or {})
    for k in ("foreach", "fused"):
        kw.pop(k, None)
    decoupled = spec.cls is torch.optim.AdamW
    lr = kw.pop("lr", 1e-3)
    betas = kw.pop("betas", (0.9, 0.999))
    eps = kw.pop("eps", 1e-8)
    weight_decay = kw.pop("weight_decay", 1e-2 if decoupled else 0.0)  # torch's AdamW / Adam defaults
    if kw or isinstance(lr, torch.Tensor):  # amsgrad, maximize, capturable, differentiable, anything unknown
        return None
    return dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                weight_decay=float(weight_decay), decoupled=decoupled)


def check_outer_compression(compression, spec):
    """The bit width of outer_compression (None: off) for outer OptimSpec `spec`;
    ValueError for an unknown string or an outer optimizer without a quantised step."""
    if compression is None:
        return None
    if compression not in QUANT_BITS:
        raise ValueError(f"outer_compression={compression!r}: expected None, " + " or ".join(map(repr, QUANT_BITS)))
    if fused_sgd_hparams(spec) is None:
        raise ValueError(f"outer_compression={compression!r} needs a plain torch.optim.SGD outer optimizer (the "
                         f"quantised outer step has no other update); got {spec.cls.__name__} with "
                         f"{dict(spec.kwargs or {})}")
    return QUANT_BITS[compression]


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


def check_streaming(num_fragments, outer_delay, outer_mix, H, spec, compression):
    """(F, tau, alpha) of the streaming options for outer OptimSpec `spec`, outer period
    H and the outer_compression string; ValueError for a value out of range or a
    combination without a kernel."""
    if not _is_int(num_fragments) or not 1 <= num_fragments <= H:
        raise ValueError(f"num_fragments={num_fragments!r}: expected an integer with 1 <= num_fragments <= H = {H}")
    if not _is_int(outer_delay) or not 0 <= outer_delay < H:
        raise ValueError(f"outer_delay={outer_delay!r}: expected an integer with 0 <= outer_delay < H = {H}")
    if isinstance(outer_mix, bool) or not isinstance(outer_mix, (int, float)) or not 0.0 <= outer_mix < 1.0:
        raise ValueError(f"outer_mix={outer_mix!r}: expected a number with 0 <= outer_mix < 1")
    if outer_delay > 0 or outer_mix > 0:
        if fused_sgd_hparams(spec) is None:
            raise ValueError(f"outer_delay={outer_delay!r} / outer_mix={outer_mix!r} need a plain torch.optim.SGD "
                             f"outer optimizer (the delayed, mixed merge has no other update); got "
                             f"{spec.cls.__name__} with {dict(spec.kwargs or {})}")
        if compression is not None:
            raise ValueError(f"outer_delay={outer_delay!r} / outer_mix={outer_mix!r} cannot be combined with "
                             f"outer_compression={compression!r} (no delayed quantised step)")
    return int(num_fragments), int(outer_delay), float(outer_mix)


def streaming_options(strategy, spec):
    """(F, tau, alpha) of a DiLoCoStrategy, validated again (an option may have been set
    after construction), or None with all three at their defaults or for any other
    strategy: the outer step is then build_outer_engine's, called every H steps."""
    if not isinstance(strategy, DiLoCoStrategy):
        return None
    kw = strategy.kwargs
    opts = check_streaming(kw.get("num_fragments", 1), kw.get("outer_delay", 0), kw.get("outer_mix", 0.0),
                           strategy.H, spec, kw.get("outer_compression"))
    return None if opts == (1, 0, 0.0) else opts


def build_outer_engine(strategy, spec, coll, K_local, n, device, dtype, placement=None):
    """The outer step of outer OptimSpec `spec` over a [K_local, n] set:
    DiLoCoOuter for plain SGD, DiLoCoOuterAdam for Adam / AdamW unless the
    strategy was built with fused_outer=False (the A/B switch against torch's
    optimizer; SGD specs are always fused), TorchOuter (torch's optimizer on an
    fp32 master) for every other spec.  With outer_compression set:
    DiLoCoOuterQuant for plain SGD, ValueError for anything else.  placement: the
    engine's placement option, None for the strategy's."""
    placement = strategy.placement_opt if placement is None else placement
    bits = check_outer_compression(strategy.kwargs.get("outer_compression"), spec)
    hp = fused_sgd_hparams(spec)
    if bits is not None:
        return DiLoCoOuterQuant(coll, K_local, n, device, dtype, bits=bits, placement=placement,
                                error_feedback=bool(strategy.kwargs.get("outer_error_feedback", False)), **hp)
    if hp is not None:
        return DiLoCoOuter(coll, K_local, n, device, dtype, placement=placement, **hp)
    hp = fused_adam_hparams(spec) if strategy.kwargs.get("fused_outer", True) else None
    if hp is not None:
        return DiLoCoOuterAdam(coll, K_local, n, device, dtype, placement=placement, **hp)
    return TorchOuter(coll, K_local, n, device, dtype, spec)


def build_streaming_outer(strategy, spec, coll, K_local, n, device, dtype, offsets, opts):
    """The FragmentedOuter of streaming options opts = (F, tau, alpha) over a
    [K_local, n] set whose tensors start at `offsets`: the arena cut by
    engine.fragment_bounds in units of 512 * world elements, one engine per fragment
    -- DiLoCoOuterStream with a delay or a mix, otherwise whatever build_outer_engine
    chooses for the spec (DiLoCoOuter, DiLoCoOuterAdam, DiLoCoOuterQuant), without a
    placement search and with n the fragment's length.  A spec that takes torch's
    optimizer (TorchOuter) has no fragments."""
    F, delay, mix = opts
    bounds = fragment_bounds(offsets, n, F, 512 * coll.world)
    engines = []
    for a, b in zip(bounds, bounds[1:]):
        if delay > 0 or mix > 0:
            eng = DiLoCoOuterStream(coll, K_local, b - a, device, dtype, delay=delay, mix=mix, placement=False,
                                    **fused_sgd_hparams(spec))
        else:
            eng = build_outer_engine(strategy, spec, coll, K_local, b - a, device, dtype, placement=False)
            if isinstance(eng, TorchOuter):
                raise ValueError(f"num_fragments={F} needs a fused outer step (SGD, Adam or AdamW outer optimizer, "
                                 f"fused_outer=True); {spec.cls.__name__} with {dict(spec.kwargs or {})} runs "
                                 f"torch's optimizer")
        engines.append(eng)
    return FragmentedOuter(engines, bounds, strategy.H, delay)


def start_outer(holder, strategy, spec, arena):
    """One node's outer step (process mode), its master a copy of `arena`, and
    the names tests and Strategy.placement_records read: the fused engine as
    strategy.engine; torch's optimizer and the Parameter its state is keyed by
    as holder.outer_optimizer / holder.master (None / unset when fused)."""
    opts = streaming_options(strategy, spec)
    if opts is not None:
        outer = build_streaming_outer(strategy, spec, strategy.coll, 1, arena.n, arena.device, arena.dtype,
                                      arena.layout.offsets, opts)
    else:
        outer = build_outer_engine(strategy, spec, strategy.coll, 1, arena.n, arena.device, arena.dtype)
    outer.init_master(arena.flat)
    holder.outer_optimizer = None
    if isinstance(outer, TorchOuter):
        holder.outer_optimizer, holder.master = outer.optimizer, outer.master
    else:
        strategy.engine = outer
    return outer


def default_outer_spec():
    return OptimSpec(torch.optim.SGD, lr=0.7, nesterov=True, momentum=0.9)


class DiLoCoCommunicator(CommunicationModule):
    """DiLoCo's outer step as a communication module of a
    CommunicateOptimizeStrategy (the name sparta_diloco.py:6 imports): every H
    steps (local_step % H == 0 and local_step > 0, diloco.py:62) the outer
    optimizer steps a master copy on master - average and every node takes the
    master.  The same outer step as DiLoCoStrategy (build_outer_engine)."""

    def __init__(self, H: int = 100, outer_optim: Optional[Union[str, OptimSpec]] = None, **kwargs):
        super().__init__(**kwargs)
        self.H = H
        self.outer_optim_spec = ensure_optim_spec(outer_optim, default_outer_spec())
        self.outer_optimizer = None

    def _init_node(self, model, rank, num_nodes):
        s = self.strategy
        # the reference's master copy is rank 0's initial model (diloco.py:81-82)
        s.coll.broadcast_(s.arena.flat, 0)
        self._outer = start_outer(self, s, self.outer_optim_spec, s.arena)

    def communicate(self, model, rank: int, num_nodes: int, local_step: int) -> None:
        if local_step % self.H == 0 and local_step > 0:
            self.strategy.arena.check_bound()
            self._outer(self.strategy.arena.flat.view(1, -1))


class DiLoCoStrategy(Strategy):
    def __init__(self, optim_spec: Optional[Union[str, OptimSpec]] = None,
                 outer_optim_spec: Optional[Union[str, OptimSpec]] = None, H: int = 100,
                 outer_compression: Optional[str] = None, outer_error_feedback: bool = False,
                 num_fragments: int = 1, outer_delay: int = 0, outer_mix: float = 0.0, **kwargs):
        self.inner_optim_spec = ensure_optim_spec(optim_spec, OptimSpec(torch.optim.AdamW))
        self.outer_optim_spec = ensure_optim_spec(outer_optim_spec, default_outer_spec())
        self.H = H
        check_outer_compression(outer_compression, self.outer_optim_spec)
        num_fragments, outer_delay, outer_mix = check_streaming(num_fragments, outer_delay, outer_mix, H,
                                                                self.outer_optim_spec, outer_compression)
        # all reach build_outer_engine / build_streaming_outer through self.kwargs, as fused_outer does
        super().__init__(outer_compression=outer_compression, outer_error_feedback=bool(outer_error_feedback),
                         num_fragments=num_fragments, outer_delay=outer_delay, outer_mix=outer_mix, **kwargs)

    def _init_node(self, model, rank, num_nodes):
        super()._init_node(model, rank, num_nodes)
        arena = self._bind_arena(model)
        # the reference's master copy is rank 0's initial model (diloco.py:81-82)
        self.coll.broadcast_(arena.flat, 0)
        self.outer = start_outer(self, self, self.outer_optim_spec, arena)
        self.optim = build_inner_optimizer(self.inner_optim_spec, model, arena, self.placement_opt)
        self._setup_scheduler()

    @property
    def engine(self):
        """The fused engine (Strategy.placement_records reads its record), None
        while the outer step is torch's optimizer.  Assigning an engine replaces
        the outer step, as it did when this was the only place it lived."""
        outer = getattr(self, "outer", None)
        return None if isinstance(outer, TorchOuter) else outer

    @engine.setter
    def engine(self, engine):
        self.outer = engine

    def _outer_step(self):
        self.arena.check_bound()
        self.outer(self.arena.flat.view(1, -1))

    def step(self):
        clip_and_step(self.optim, self.arena, self.kwargs.get("max_norm"))  # diloco.py:52-59
        if isinstance(self.outer, FragmentedOuter):  # the streaming schedule: asked on every step
            self.arena.check_bound()
            self.outer.step(self.arena.flat.view(1, -1), self.local_step)
        elif self.local_step % self.H == 0 and self.local_step > 0:
            self._outer_step()
        super().step()

    def finish(self):
        outer = getattr(self, "outer", None)
        if isinstance(outer, FragmentedOuter):
            outer.finish()  # merges still pending are discarded, the parameters stay as they are
        super().finish()
