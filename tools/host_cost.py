"""Host cost of the pieces of one launch through the ctypes boundary (no device synchronisation inside the timed loops)."""
import sys, os, time, ctypes, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from masic_amd import ops, _lib
x = torch.randn(64, device="cuda"); y = torch.empty_like(x)
def t(name, fn, n=20000):
    for _ in range(100): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    dt = (time.perf_counter() - t0) / n * 1e6
    torch.cuda.synchronize()
    print(f"{name:50s} {dt:7.2f} us")
t("ops._stream()", ops._stream)
t("torch.cuda.current_stream().cuda_stream", lambda: torch.cuda.current_stream().cuda_stream)
t("torch.empty_like(x)", lambda: torch.empty_like(x))
t("torch.empty(n, int16)", lambda: torch.empty(4096, dtype=torch.int16, device=x.device))
t("ops._p(x) x3", lambda: (ops._p(x), ops._p(y), ops._p(None)))
t("x.is_contiguous(); x.shape", lambda: (x.is_contiguous(), x.shape))
st = ops._stream()
t("raw lib.masic_elementwise (launch only)", lambda: _lib.lib.masic_elementwise(ops._p(x), None, ops._p(y), 64, int(ops.EW_SQUARE), 0.0, 0.0, st), 5000)
t("ops.elementwise(EW_SQUARE, x)", lambda: ops.elementwise(ops.EW_SQUARE, x), 5000)
d16 = ops.make_conv_desc(1, 16, 16, 16, 128, 5, 5, 2, 2, prec=_lib.PREC_BF16); x16 = torch.zeros(16 * 256, dtype=torch.int16, device="cuda")
wp = ops.pack_conv_f16k_weight(torch.zeros(128, 16, 5, 5, device="cuda"), d16); y16 = torch.empty(128 * 64, dtype=torch.int16, device="cuda")
t("raw lib.masic_conv_f16k_gdn_fwd (launch only)", lambda: _lib.lib.masic_conv_f16k_gdn_fwd(ops._p(x16), ops._p(wp), None, None, None, 0, None, ops._p(y16), ctypes.byref(d16), st), 5000)
wpg = ops.pack_gemm_f16k_weight(torch.zeros(32, 16, device="cuda"), 16, 32, False); yg = torch.empty(32 * 256, dtype=torch.int16, device="cuda")
t("raw lib.masic_gemm_f16k_fwd (launch only)", lambda: _lib.lib.masic_gemm_f16k_fwd(ops._p(x16), ops._p(wpg), None, ops._p(yg), None, 1, 16, 32, 256, 32, 0, 0, st), 5000)
x3 = torch.zeros(32 * 512, dtype=torch.int16, device="cuda"); wp3 = ops.pack_conv3x3_resident_weight(torch.zeros(32, 32, 3, 3, device="cuda")); y3 = torch.empty_like(x3)
t("raw lib.masic_conv3x3_resident_fwd (launch only)", lambda: _lib.lib.masic_conv3x3_resident_fwd(ops._p(x3), ops._p(wp3), None, None, None, 0, None, 0.0, None, ops._p(y3), 1, 32, 32, 16, 32, 32, 0, 32, 0, 0, st), 5000)
dwg = ops.make_conv_desc(1, 32, 16, 16, 32, 3, 3, 1, 1); xw = torch.zeros(1, 32, 16, 16, device="cuda"); dw = torch.empty(32, 32, 3, 3, device="cuda")
wsw = torch.zeros(32 * 32 * 9, device="cuda")      # a clean workspace: zeros on entry, zeros again after every call
t("raw lib.masic_conv2d_wgrad_ws (launch only)", lambda: _lib.lib.masic_conv2d_wgrad_ws(ops._p(xw), ops._p(xw), ops._p(dw), ops._p(wsw), ctypes.byref(dwg), 1, st), 5000)
xk = torch.zeros(32 * 256, dtype=torch.int16, device="cuda")
t("raw lib.masic_conv3x3_wgrad_f16k_ws (launch only)", lambda: _lib.lib.masic_conv3x3_wgrad_f16k_ws(ops._p(xk), ops._p(xk), ops._p(dw), ops._p(wsw), 1, 32, 32, 16, 16, 1, st), 5000)
dcv = ops.make_conv_desc(1, 32, 16, 16, 32, 3, 3, 1, 1); wcv = ops.pack_conv_weight(torch.zeros(32, 32, 3, 3, device="cuda"), dcv); ycv = torch.empty(1, 32, 16, 16, device="cuda")
t("raw lib.masic_conv2d_fwd (launch only)", lambda: _lib.lib.masic_conv2d_fwd(ops._p(xw), ops._p(wcv), None, None, ops._p(ycv), ctypes.byref(dcv), st), 5000)
d = ops.make_conv_desc(2, 32, 16, 16, 32, 3, 3, 1, 1)
t("make_conv_desc", lambda: ops.make_conv_desc(2, 32, 16, 16, 32, 3, 3, 1, 1))
t("torch add (aten) x + y", lambda: x + y, 5000)
class F(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a): return a
    @staticmethod
    def backward(ctx, g): return g
xr = x.clone().requires_grad_(True)
t("autograd.Function.apply (identity)", lambda: F.apply(xr), 5000)
from masic_amd import nn as mnn
from masic_amd.f16k import F16K
cv = mnn.Conv2d(16, 128, 5, stride=2, padding=2).cuda(); xv = F16K.wrap(x16, 1, 16, 16, 16)
t("Conv2d.run_f16k (whole F16K, 1 x 16 -> 128, 5x5 s2, 16^2)", lambda: cv.run_f16k(xv), 5000)
c3 = mnn.Conv2d(32, 32, 3, padding=1).cuda(); x3v = F16K.wrap(x3, 1, 32, 16, 32); view = F16K.empty(1, 96, 16, 32, "cuda").channels(64, 32)
t("Conv2d.run_f16k_res (into a channel view of 96)", lambda: c3.run_f16k_res(x3v, act=ops.ACT_LEAKY, out=view), 5000)
