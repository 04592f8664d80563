"""SPARTA inside DiLoCo: an inner step, SPARTA's sparse average every step,
DiLoCo's outer step every H steps.

API of exogym/strategy/sparta_diloco.py:9-42: SPARTADiLoCoStrategy(inner_optim=None,
outer_optim=None, p_sparta=0.005, H=100, **kwargs), a CommunicateOptimizeStrategy
over [SparseCommunicator(RandomIndexSelector(p_sparta)), DiLoCoCommunicator(H=H,
outer_optim=outer_optim)].  The reference module does not import (its
DiLoCoCommunicator was never written), so the semantics are the ones its
docstring and constructor state, with DiLoCoStrategy's outer step
(diloco.py:62-74) and default outer optimizer; the step order is
CommunicateOptimizeStrategy.step: clip -> inner optimizer -> sparse average ->
(every H) outer step.  The SPARTA iteration counter and the torch generator
advance every step, outer steps included.

mask_source= and placement= pass through as on SPARTAStrategy / DiLoCoStrategy.
fuse_boundary (default True, batched-replica mode in one process): on a step
where both modules fire the sparse average only changes the arithmetic of the
average the outer step forms, so the two run as ONE pass
(ga_diloco_outer_masked) with bit-identical results.  mask_source="philox"
keeps no mask in memory: its boundary steps run the two launches and
fuse_boundary reads False.

outer_compression= / outer_error_feedback= as on DiLoCoStrategy (int8 / int4
block-quantised pseudo-gradients, SGD-family outer optimizers).  The quantised
outer step has no masked form: the two modules run in sequence and
fuse_boundary reads False.
"""
from typing import Optional, Union

from .communicate_optimize_strategy import CommunicateOptimizeStrategy
from .diloco import DiLoCoCommunicator, check_outer_compression
from .optim import OptimSpec
from .sparta import RandomIndexSelector, SparseCommunicator


class SPARTADiLoCoStrategy(CommunicateOptimizeStrategy):
    def __init__(self, inner_optim: Optional[Union[str, OptimSpec]] = None,
                 outer_optim: Optional[Union[str, OptimSpec]] = None, p_sparta: float = 0.005, H: int = 100,
                 mask_source="torch", fuse_boundary=True, outer_compression: Optional[str] = None,
                 outer_error_feedback: bool = False, **kwargs):
        index_selector = RandomIndexSelector(p_sparta, mask_source=mask_source)
        sparse_comm = SparseCommunicator(index_selector)
        diloco_comm = DiLoCoCommunicator(H=H, outer_optim=outer_optim)
        check_outer_compression(outer_compression, diloco_comm.outer_optim_spec)
        super().__init__(communication_modules=[sparse_comm, diloco_comm], inner_optim=inner_optim,
                         outer_compression=outer_compression, outer_error_feedback=bool(outer_error_feedback),
                         **kwargs)
        self.index_selector = index_selector
        self.p_sparta = p_sparta
        self.H = H
        self.outer_optim_spec = diloco_comm.outer_optim_spec
        self.fuse_boundary = bool(fuse_boundary) and mask_source != "philox" and outer_compression is None
        self.mask_draw = None  # which mask draw the last step ran ("philox" | "fused" | "torch")
