from .base_blockwise_sparsification import BaseBlockwiseSparsification  # noqa: F401
from .wanda import Wanda  # noqa: F401
from .magnitude import Magnitude  # noqa: F401
from .sparsegpt import SparseGPT  # noqa: F401
from .dense import Dense  # noqa: F401
from .shortgpt import ShortGPT  # noqa: F401
from .kvsparse import SinkKVCache  # noqa: F401
