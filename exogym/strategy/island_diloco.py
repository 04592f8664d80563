"""exogym.strategy.island_diloco -> gym_amd.strategy.island_diloco (the same module object: attribute
look-ups, monkeypatching and isinstance checks see gym_amd's implementation)."""
import sys

from gym_amd.strategy import island_diloco as _impl

sys.modules[__name__] = _impl
