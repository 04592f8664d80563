"""One simulated node's training loop (caller of the strategy step).

Constructor and loop semantics of exogym/train_node.py:19-626: seeding (42),
dataset-or-factory handling, rank 0's initial parameters broadcast to every
node, gradient accumulation over batch_size // minibatch_size minibatches
with `grad /= batch_size / minibatch_size`, `strategy.zero_grad()` /
`strategy.step()`, evaluation every val_interval steps (rank 0 evaluates its
local model, rank 1 the node-averaged model), a barrier every step.

MI355X changes: the initial broadcast and the evaluation average run over the
strategy's flat parameter arena (one collective + one ga_replica_mean launch
instead of one per tensor); the model-correlation metric the reference disables
(train_node.py:498-573) runs on the arena every `correlation_interval` steps
(gym_amd.metrics.NodeDrift; off by default).  Logging is a small in-memory recorder (the
reference's wandb/CSV loggers and its disabled checkpointing are out of scope).
"""
import copy
from typing import Callable, Union

import numpy as np
import torch
import torch.distributed as dist
from torch.utils.data import DataLoader

from . import ops
from .strategy.communicate import all_reduce, broadcast
from .strategy.strategy import Strategy
from .utils import LogModule


class RunLog:
    """Rank 0's record of the run: train losses, evaluation losses, learning rates."""

    def __init__(self, strategy, max_steps):
        self.step = 0
        self.max_steps = max_steps
        self.train = []
        self.evals = []
        self.lrs = []
        self.metrics = []
        strategy.lr_callbacks.append(self.log_lr)

    def log_train(self, loss):
        self.train.append((self.step, float(loss)))

    def log_loss(self, loss, name):
        self.evals.append((self.step, name, float(loss)))

    def log_lr(self, lr):
        self.lrs.append((self.step, float(lr)))

    def log_metric(self, name, value):
        self.metrics.append((self.step, name, float(value)))

    def increment_step(self):
        self.step += 1

    def summary(self):
        """Plain lists (picklable through the trainer's result queue)."""
        return {"train": list(self.train), "evals": list(self.evals), "lrs": list(self.lrs),
                "metrics": list(self.metrics)}


def watch_reached(params):
    """A set that autograd fills with the trainable parameters it accumulates a
    gradient into (a post-accumulate-grad hook on each: it fires with a .grad
    bound beforehand too).  The strategies' zero_grad() zeroes the gradient
    arena and keeps every .grad bound to it, so after backward a parameter the
    loss did not depend on holds zeros where the reference holds None
    (optim.zero_grad() sets None and autograd never fills it); the train step
    clears the set after zero_grad() and, after backward, drop_unreached()
    restores None for the rest."""
    reached = set()
    for p in params:
        if p.requires_grad:
            p.register_post_accumulate_grad_hook(reached.add)
    return reached


def drop_unreached(params, reached):
    """.grad = None for the trainable parameters backward did not reach: the
    state the reference is in at strategy.step(), which skips them in the
    all-reduce (strategy.py:131), the optimizer (torch skips a None grad) and
    SPARTA's average (sparta.py:29).  The next zero_grad() binds them again."""
    for p in params:
        if p.requires_grad and p not in reached:
            p.grad = None


class TrainNode(LogModule):
    def __init__(self, model: torch.nn.Module,
                 train_dataset: Union[torch.utils.data.Dataset, Callable[[int, int, bool], torch.utils.data.Dataset]],
                 train_sampler: torch.utils.data.Sampler,
                 val_dataset: Union[torch.utils.data.Dataset, Callable[[int, int, bool], torch.utils.data.Dataset]],
                 strategy: Strategy, device: torch.device, rank: int, num_nodes: int, num_epochs: int,
                 max_steps: int = None, batch_size: int = 16, minibatch_size: int = 16, val_size: int = 64,
                 val_interval: int = 100, checkpoint_interval: int = 100, autocast: bool = False,
                 correlation_interval: int = None, drift_detail: bool = False, **kwargs):
        seed = kwargs.get("seed", 42)
        torch.manual_seed(seed)
        torch.cuda.manual_seed(seed)
        np.random.seed(seed)
        self.model = model
        if callable(train_dataset):
            self.train_dataset = train_dataset(rank, num_nodes, False)
            self.train_sampler = None
        else:
            self.train_dataset = train_dataset
            self.train_sampler = train_sampler
        self.val_dataset = val_dataset(rank, num_nodes, True) if callable(val_dataset) else val_dataset
        self.strategy = strategy
        self.device = device
        self.rank = rank
        self.num_nodes = num_nodes
        self.num_epochs = num_epochs
        self.max_steps = max_steps
        self.batch_size = batch_size
        self.minibatch_size = minibatch_size
        self.val_size = val_size
        self.val_interval = val_interval
        self.autocast = autocast
        self.checkpoint_interval = checkpoint_interval
        self.correlation_interval = correlation_interval
        self.drift_detail = drift_detail
        self.kwargs = kwargs
        self.build_dataloaders()
        torch.manual_seed(42)
        torch.cuda.manual_seed(42)
        if self.num_nodes > 1:  # every node starts from rank 0's parameters
            arena = getattr(strategy, "arena", None)
            if arena is not None:
                broadcast(arena.flat, src=0)
            else:
                for p in self.model.parameters():
                    broadcast(p.data, src=0)
        self.local_step = 0
        self.epoch = 0
        self.logger = None
        self.drift = None  # NodeDrift, built at the first measurement (correlation_interval set)
        self._reached = watch_reached(self.model.parameters())

    def build_dataloaders(self):
        self.train_dataloader = DataLoader(self.train_dataset, batch_size=self.minibatch_size,
                                           sampler=self.train_sampler, shuffle=(self.train_sampler is None))
        self.val_dataloader = DataLoader(self.val_dataset, batch_size=self.minibatch_size, shuffle=True)
        self.train_data_iter = iter(self.train_dataloader)
        self.val_data_iter = iter(self.val_dataloader)

    def _get_batch(self, eval=False):
        if not eval or self.val_data_iter is None:
            try:
                batch = next(self.train_data_iter)
            except StopIteration:
                self.epoch += 1
                self.train_data_iter = iter(self.train_dataloader)
                batch = next(self.train_data_iter)
        else:
            try:
                batch = next(self.val_data_iter)
            except StopIteration:
                self.val_data_iter = iter(self.val_dataloader)
                batch = next(self.val_data_iter)
        if isinstance(batch, (tuple, list)):
            return tuple(x.to(self.device) for x in batch)
        return batch.to(self.device)

    def _forward(self, model, minibatch):
        if self.autocast:
            with torch.autocast(device_type=torch.device(self.device).type, dtype=torch.bfloat16):
                return model(minibatch)
        return model(minibatch)

    def _train_step(self):
        self.strategy.zero_grad()
        self._reached.clear()
        accum = self.batch_size // self.minibatch_size
        loss = None
        for _ in range(accum):
            loss = self._forward(self.model, self._get_batch())
            loss.backward()
        drop_unreached(self.model.parameters(), self._reached)
        for p in self.model.parameters():
            if p.requires_grad and p.grad is not None:
                p.grad /= self.batch_size / self.minibatch_size
        self.strategy.step()
        if self.rank == 0 and self.logger is not None:
            self.logger.log_train(loss=loss.item())

    def _averaged_model(self):
        """A copy of the model holding the node-averaged parameters
        (train_node.py:183-189): one all-reduce of the arena + one division launch."""
        clone = copy.deepcopy(self.model)
        arena = getattr(self.strategy, "arena", None)
        if arena is None:
            for p in clone.parameters():
                all_reduce(p.data, op=dist.ReduceOp.SUM)
                p.data = p.data / dist.get_world_size()
            return clone
        avg = arena.flat.detach().clone()
        dist.all_reduce(avg, op=dist.ReduceOp.SUM)
        ops.replica_mean(avg, avg, divisor=dist.get_world_size())
        with torch.no_grad():
            for p, v in zip(clone.parameters(), arena.layout.views(avg)):
                p.copy_(v)
        return clone

    def _evaluate(self):
        if self.val_size == 0:
            return
        clone = self._averaged_model() if self.num_nodes > 1 else self.model
        this_model = None
        if self.rank == 0:
            this_model = self.model
        if self.rank == 1:
            this_model = clone
        loss_total = 0.0
        if this_model is not None:
            this_model.eval()
            accum = self.batch_size // self.minibatch_size
            with torch.no_grad():
                for _ in range(int(self.val_size / self.batch_size)):
                    for _ in range(accum):
                        loss_total += self._forward(this_model, self._get_batch(eval=True)).item() / accum
            this_model.train()
        n_eval = int(self.val_size / self.batch_size)
        if self.rank == 0 and self.logger is not None:
            self.logger.log_loss(loss=loss_total / n_eval, name="local")
        if self.num_nodes > 1:
            g = torch.empty(1, device=next(self.model.parameters()).device)
            if self.rank == 1:
                g[0] = loss_total / n_eval
            broadcast(g, src=1)
            if self.rank == 0 and self.logger is not None:
                self.logger.log_loss(loss=g.item(), name="global")

    def _node_drift(self):
        """Model correlation and consensus distance over the nodes
        (train_node.py:498-573 through ga_replica_gram): every rank calls it,
        rank 0 records the two numbers, and with drift_detail (through
        ga_replica_gram_centered) avg_model_decorrelation and
        max_pairwise_distance as well.  The vector is the strategy's parameter
        arena, or a flat copy of model.parameters() for a strategy without one."""
        from .comm import Collective
        from .metrics import NodeDrift, flat_parameters
        arena = getattr(self.strategy, "arena", None)
        if arena is not None:
            flat, n_true = arena.flat, arena.layout.n_params
        else:
            flat, n_true = flat_parameters(self.model)
        if self.drift is None:
            self.drift = NodeDrift(Collective(), 1, flat.numel(), flat.numel(), n_true, flat.device, flat.dtype,
                                   detail=self.drift_detail)
        out = self.drift(flat)
        if out is not None and self.rank == 0 and self.logger is not None:
            self.logger.log_metric("avg_model_correlation", out["avg_model_correlation"])
            self.logger.log_metric("consensus_distance", out["consensus_distance"])
            if self.drift_detail:
                self.logger.log_metric("avg_model_decorrelation", out["avg_model_decorrelation"])
                self.logger.log_metric("max_pairwise_distance", out["max_pairwise_distance"])
        return out

    def train(self):
        if self.max_steps is None:
            self.max_steps = self.num_epochs * len(self.train_dataloader) / (self.batch_size // self.minibatch_size)
        self.strategy.max_steps = self.max_steps
        if self.rank == 0:
            self.logger = RunLog(self.strategy, self.max_steps)
        while self.local_step < self.max_steps:
            if self.local_step % self.val_interval == 0:
                self._evaluate()
            self._train_step()
            self.local_step += 1
            if self.rank == 0:
                self.logger.increment_step()
            if self.correlation_interval and self.local_step % self.correlation_interval == 0:
                self._node_drift()  # the condition of train_node.py:615
            if self.num_nodes > 1:
                dist.barrier()
        self.strategy.finish()
        self._evaluate()
        return self.model.state_dict()

    def __config__(self):
        return super().__config__(remove_keys=["model", "train_dataloader", "val_dataloader", "strategy"])
