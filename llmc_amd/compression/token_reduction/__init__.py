from .base_blockwise_token_reduction import TokenReduction  # noqa: F401
from .token_reduction_module import TokenReductionModule  # noqa: F401
from .divprune import DivPrune  # noqa: F401
