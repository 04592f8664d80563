"""exogym.strategy -> gym_amd.strategy (names of exogym/strategy/__init__.py:3-12).

The reference's __all__ also lists "SPARTADiLoCoStrategy", whose import is
commented out (exogym/strategy/__init__.py:10,20), so `from exogym.strategy
import *` raises AttributeError there; here the name resolves, and
DiLoCoCommunicator (the name its module fails to import) is exported beside it.
"""
from gym_amd.strategy import (CommunicateOptimizeStrategy, DeMoStrategy, DiLoCoCommunicator, DiLoCoStrategy,
                              FedAvgStrategy, IslandDiLoCoCommunicator, IslandDiLoCoStrategy, OptimSpec,
                              SimpleReduceStrategy, SPARTADiLoCoStrategy, SPARTAStrategy, Strategy)

__all__ = [
    "Strategy",
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
