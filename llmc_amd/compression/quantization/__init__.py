from .quant import (BaseQuantizer, FloatQuantizer, IntegerQuantizer,  # noqa: F401
                    dequant_fpx, pack_awq_gemm, pack_fp4, pack_lsb)
from .module_utils import (AutoawqRealQuantLinear, EffcientFakeQuantLinear,  # noqa: F401
                           FakeQuantLinear, LlmcFp8Linear, LlmcRMSNorm, OriginFloatLinear, RotateLinear, Rotater,
                           VllmRealQuantLinear)
from .base_blockwise_quantization import BaseBlockwiseQuantization  # noqa: F401
from .auto_clip import AutoClipper  # noqa: F401
from .rtn import RTN  # noqa: F401
from .gptq import GPTQ  # noqa: F401
from .awq import Awq  # noqa: F401
from .spqr import SpQR  # noqa: F401
from .hqq import HQQ  # noqa: F401
from .smoothquant import SmoothQuant  # noqa: F401
from .osplus import OsPlus  # noqa: F401
from .quarot import Quarot  # noqa: F401
from .quik import QUIK  # noqa: F401
from .llmint8 import LlmInt8  # noqa: F401
from .adadim import AdaDim  # noqa: F401
