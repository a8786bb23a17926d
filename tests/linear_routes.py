"""llmc_test_linear_route for the tests: what llmc_linear_eval / llmc_linear_eval_kt would launch for a call (a pure host call)."""
from types import SimpleNamespace

import numpy as np

from llmc_amd import _ffi

FIELDS = ('status', 'kernel', 'grid', 'threads', 'sbm', 'sbn', 'nrounds', 'ksplit', 'store', 'stage_y', 'ntm', 'ntn')
ROW_MAJOR, KTILED = 0, 1
STORE_NONE, STORE_SCALAR, STORE_ROWS, STORE_BLOCKED, STORE_SPLITK = -1, 0, 1, 2, 3
EINVAL, ENOTSUP = -22, -95
DT = {'f16': _ffi.F16, 'bf16': _ffi.BF16}


def route(tiled, dt, N, K, R, mode=0, blocked=False, y=None, y0=False, loss=None, ws=None, mis=(0, 0, 0, 0, 0), cus=0, flags=None):
    """tiled: llmc_linear_eval_kt, else llmc_linear_eval. mode 0 / 1; blocked: LLMC_LINEAR_YBLOCKED; y, y0, loss, ws: whether the
    call passes Yout, Y0 (a bias in mode 0), loss_sum and a workspace (y, loss and ws default to what the mode needs); mis: bytes
    added to the 16-B aligned addresses of X, W, Yout, Y0, ws; cus: the device's compute units (0: the current device's); flags
    overrides the mode word. Returns the hook's fields; after a refusal only `status` and `error` mean anything."""
    y = (mode == 0) if y is None else y
    loss = (mode == 1) if loss is None else loss
    ws = (mode == 1) if ws is None else ws
    word = (mode | (_ffi.LINEAR_YBLOCKED if blocked else 0)) if flags is None else flags
    inp = np.array([int(tiled), DT.get(dt, dt), N, K, R, word, int(y), int(bool(y0) or mode == 1), int(loss), int(ws), *mis, cus],
                   dtype=np.int64)
    out = np.zeros(len(FIELDS), dtype=np.int32)
    rc = _ffi.lib().llmc_test_linear_route(inp.ctypes.data, out.ctypes.data)
    assert rc == 0, rc
    r = SimpleNamespace(**{k: int(v) for k, v in zip(FIELDS, out)})
    r.error = _ffi.last_error() if r.status else ''
    r.tiles = r.ntm * r.ntn
    return r


def route_of_out(x, w, dt, bias=None, tiled=False, blocked=False, y_mis=0):
    """The route awq_ops.linear_out(x, w, bias, tiled, blocked) takes: it passes a workspace to the k-tiled entry exactly when
    llmc_linear_eval_ws_bytes asks for more than the loss partials (a product the launcher may cut into k-slices)."""
    N, K, R = x.shape[0], x.shape[1], w.shape[0]
    ws = tiled and not blocked and _ffi.lib().llmc_linear_eval_ws_bytes(N, K, R) > 4 * ((N + 255) // 256) * ((R + 255) // 256)
    return route(tiled, dt, N, K, R, 0, blocked, y0=bias is not None, ws=ws, mis=(0, 0, y_mis, 0, 0))


def route_of_loss(x, w, dt, y0, tiled=False, blocked=False):
    """The route awq_ops.linear_loss_sum(x, w, y0, tiled=..., y0_blocked=...) takes for this Y0 tensor (its address decides whether
    the k-tiled kernel stages it through LDS)."""
    return route(tiled, dt, x.shape[0], x.shape[1], w.shape[0], 1, blocked, mis=(0, 0, 0, y0.data_ptr() % 16, 0))
