"""Host-side layer helpers shared by the models composed in Python (the FPN detector, the N4 FPN pieces, LXMERT): the
dtype table, the stream argument of the C-ABI calls, the weight packer and the conv / linear call wrappers."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

# precision name -> (library dtype code, torch dtype)
DTYPES = {"fp32": (L.VK_F32, torch.float32), "fp16": (L.VK_F16, torch.float16), "bf16": (L.VK_BF16, torch.bfloat16)}
# library dtype code -> torch dtype (stage tensors include the integer ones)
TORCH_DTYPES = dict(DTYPES.values()) | {L.VK_I64: torch.int64, L.VK_I32: torch.int32}


def stream(device):
    """The current torch stream of `device` as the `void *stream` argument of the C ABI."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def f32(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)


def pack(w, dt, bn=None, bias=None, groups=1):
    """Conv weight [cout, cin/groups, kh, kw] or linear weight [cout, cin] (+ BN [gamma, beta, mean, var], folded by the
    library) (+ bias) -> (packed weight bytes, f32 bias [packed cout]) as host numpy arrays (vk_pack_conv_weight)."""
    w = f32(w)
    if w.ndim == 2:
        w = w.reshape(w.shape[0], w.shape[1], 1, 1)
    cout, cin, kh, kw = w.shape
    cin *= groups
    lib = L.load()
    wp = np.zeros(lib.vk_packed_weight_bytes(cout, cin, kh, kw, groups, dt), np.uint8)
    bp = np.zeros(lib.vk_packed_cout(cout), np.float32)
    bnp = np.ascontiguousarray(np.concatenate([f32(v).reshape(-1) for v in bn])) if bn is not None else None
    bi = f32(bias) if bias is not None else None
    L.call("vk_pack_conv_weight", w.ctypes.data_as(C.c_void_p), bnp.ctypes.data_as(C.c_void_p) if bnp is not None else None,
           bi.ctypes.data_as(C.c_void_p) if bi is not None else None, cout, cin, kh, kw, groups, dt,
           wp.ctypes.data_as(C.c_void_p), bp.ctypes.data_as(C.c_void_p))
    return wp, bp


class Conv:
    """conv (+ folded BN / bias) (+ residual) (+ ReLU) on NHWC device tensors: Conv2d.forward frcnn.py:794-822."""

    def __init__(self, w, precision, device, bn=None, bias=None, stride=1, pad=0, dil=1, groups=1):
        w = f32(w)
        self.cout, self.cin, self.k = w.shape[0], w.shape[1] * groups, w.shape[2]
        self.stride, self.pad, self.dil, self.groups = stride, pad, dil, groups
        self.dt, self.tdt = DTYPES[precision]
        self.device = torch.device(device)
        wp, bp = pack(w, self.dt, bn, bias, groups)
        self.w, self.b = torch.from_numpy(wp).to(self.device), torch.from_numpy(bp).to(self.device)

    def out_hw(self, H, W):
        e = self.dil * (self.k - 1) + 1
        return (H + 2 * self.pad - e) // self.stride + 1, (W + 2 * self.pad - e) // self.stride + 1

    def __call__(self, x, relu=False, residual=None, out_f32=False):
        N, H, W, cin = x.shape
        assert cin == self.cin, (cin, self.cin)
        Ho, Wo = self.out_hw(H, W)
        ldy = (self.cout + 7) // 8 * 8
        y = torch.empty((N, Ho, Wo, ldy), dtype=torch.float32 if out_f32 else self.tdt, device=self.device)
        L.call("vk_conv2d", x.data_ptr(), N, H, W, cin, self.w.data_ptr(), self.b.data_ptr(),
               residual.data_ptr() if residual is not None else None, y.data_ptr(), self.cout, ldy, self.k, self.k,
               self.stride, self.pad, self.dil, self.groups, int(relu), self.dt, L.VK_F32 if out_f32 else self.dt, stream(self.device))
        return y


class Linear:
    """nn.Linear (+ ReLU) through the MFMA GEMMs (vk_linear) on [M, K] device tensors."""

    def __init__(self, w, bias, precision, device):
        w = f32(w)
        self.nout, self.k = w.shape
        self.dt, self.tdt = DTYPES[precision]
        self.device = torch.device(device)
        wp, bp = pack(w, self.dt, bias=bias)
        self.w, self.b = torch.from_numpy(wp).to(self.device), torch.from_numpy(bp).to(self.device)

    def __call__(self, x, relu=False, out_f32=False):
        M = x.shape[0]
        assert x.shape[1] == self.k and x.is_contiguous() and x.dtype == self.tdt
        ldy = (self.nout + 7) // 8 * 8
        y = torch.empty((M, ldy), dtype=torch.float32 if out_f32 else self.tdt, device=self.device)
        if M:
            L.call("vk_linear", x.data_ptr(), M, self.k, self.w.data_ptr(), self.b.data_ptr(), None, y.data_ptr(), self.nout, ldy,
                   L.VK_ACT_RELU if relu else L.VK_ACT_NONE, self.dt, L.VK_F32 if out_f32 else self.dt, stream(self.device))
        return y
