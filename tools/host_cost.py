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
# the own-layer kernels on the layers of a synthetic-weight model, each at the smallest shape it takes: what the
# eval forward asks per layer (supported, preferred) and the launch through the module
sys.path.insert(0, os.path.join(ROOT, "coremasic", "mywork"))
import MASIC
from masic_amd import conv_s2, d2s_layer, deconv, latent, synth
net = MASIC.HSIC(128, 192, 5); net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=31)); net = net.cuda().eval()
enc, dec = net.encoder1, net.decoder1
xa = F16K.wrap(torch.zeros(128 * 8 * 8, dtype=torch.int16, device="cuda"), 1, 128, 8, 8)
xl = F16K.wrap(torch.zeros(128 * 5 * 7, dtype=torch.int16, device="cuda"), 1, 128, 5, 7)
with torch.no_grad():
    t("conv_s2.supported (g_a_conv2, 1 x 8 x 8)", lambda: conv_s2.supported(enc.g_a_conv2, enc.g_a_gdn2, 1, 8, 8))
    t("deconv.supported (g_s_conv2, 1 x 8 x 8)", lambda: deconv.supported(dec.g_s_conv2, dec.g_s_gdn2, 1, 8, 8))
    t("latent.supported and preferred (g_a_conv4, 8 x 64 x 64)", lambda: latent.supported(enc.g_a_conv4, 8, 64, 64) and latent.preferred(enc.g_a_conv4, 8, 64, 64))
    t("d2s_layer.supported and preferred (g_s_conv4, 8 x 256 x 256)", lambda: d2s_layer.supported(dec.g_s_conv4, 8, 256, 256) and d2s_layer.preferred(dec.g_s_conv4, 8, 256, 256))
    t("conv_s2.run (g_a_conv2, 1 x 8 x 8)", lambda: conv_s2.run(enc.g_a_conv2, enc.g_a_gdn2, xa), 5000)
    t("deconv.run (g_s_conv2, 1 x 8 x 8)", lambda: deconv.run(dec.g_s_conv2, dec.g_s_gdn2, xa), 5000)
    wl, bl = enc.g_a_conv4.packed_f16k_weight(enc.g_a_conv4._desc_of(xl, nchw=True)), enc.g_a_conv4._bias()
    t("latent.launch (g_a_conv4, 1 x 5 x 7, four outputs)", lambda: latent.launch(xl.buf, wl, bl, 1, 5, 7), 5000)
    assert d2s_layer.takes_row(512, 32, 32)           # the pack of a shape conv_f16k runs on d2s_layer.ROW is the kernel's stream at every shape
    _, wd, bd = dec.g_s_conv4.packed_d2s(512, 32, 32)
    t("d2s_layer.launch (g_s_conv4, 1 x 5 x 7)", lambda: d2s_layer.launch(xl.buf, wd, bd, 1, 5, 7, 3), 5000)
