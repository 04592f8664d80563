"""Strategy API — same import surface as exogym.strategy (exogym/strategy/__init__.py:3-21).

SPARTADiLoCoStrategy is provided although the reference's module cannot be
imported (sparta_diloco.py:6 imports a DiLoCoCommunicator that was never
written; its import is commented out of the package, __init__.py:10): the
communicator lives in .diloco, where that import looks for it.
"""
from .communicate_optimize_strategy import CommunicateOptimizeStrategy, CommunicationModule
from .demo import DeMoStrategy
from .diloco import DiLoCoCommunicator, DiLoCoStrategy
from .federated_averaging import FedAvgStrategy
from .island_diloco import IslandDiLoCoCommunicator, IslandDiLoCoStrategy
from .optim import OptimSpec, ensure_optim_spec
from .sparta import SPARTAStrategy
from .sparta_diloco import SPARTADiLoCoStrategy
from .strategy import SimpleReduceStrategy, Strategy

__all__ = [
    "Strategy",
    "SimpleReduceStrategy",
    "DiLoCoStrategy",
    "OptimSpec",
    "SPARTAStrategy",
    "FedAvgStrategy",
    "CommunicateOptimizeStrategy",
    "DeMoStrategy",
    "SPARTADiLoCoStrategy",
    "DiLoCoCommunicator",
    "IslandDiLoCoStrategy",
    "IslandDiLoCoCommunicator",
]
