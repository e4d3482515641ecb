"""Every kernel instantiation of CONV_ROWS (masic_amd/csrc/conv.hip) against the float64 reference of tests/conv_ref.py, one case each
at ragged tiles, a ragged channel block, a batch and a partial last K chunk (tests/conv_row_cases.py: the table and the search that
wrote it); per tile shape a four-phase transposed 5x5 and a gate + two residuals + activation + channel views case, the bf16 one also as
F16K output into a wider buffer; and the digest's eleven forms on the digest's own inputs.  tests/test_cpu_conv_rows.py holds every
case to its kernel and to its properties without a GPU.

Gates (tests/conv_ref.py: gate_of): float32 RTOL; bf16 operands 2e-5 against the reference on bf16-rounded operands; F16K output 2^-8
against that reference rounded to bf16.  The seven large F16K cases run on whole-number operands (tests/conv_ref.py, inputs()): float32
accumulation is exact there, so they must also equal the reference bit for bit.  Channels outside the output view keep the prefill
exactly.  Measured errors: DESIGN.md section 2.1."""
import ctypes

import pytest
import torch

from tests import conv_ref as R
from tests.conv_row_cases import all_cases
from tests.util import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_conv_row_vs_float64(case):
    from masic_amd import ops
    name, kernel, c = case.id, case.kernel, case.case
    x, w, bias, gate, res1, res2 = R.inputs(c, case.seed, case.integers)
    ref = R.conv_ref(c, x, w, bias, gate, res1, res2)
    d = R.desc_of(c)
    _, _, out_ctot, out_coff = R.views(c)
    dev = lambda t: None if t is None else t.to(DEV)
    packed = ops.pack_conv_weight(dev(w), d)
    if c.form & R.F16K_OUT:
        y16 = ops.conv2d_f16k_out(dev(x), packed, dev(bias), d)
        y = ops.f16k_to_nchw(y16, c.B, out_ctot, d.Ho, d.Wo)
        # ops.conv2d_f16k_out allocates its buffer; the entry point once more into a prefilled one (0x3f00: bf16 0.5): same bits, neighbours kept
        z16 = torch.full_like(y16, 0x3f00)
        ops.check(ops.lib.masic_conv2d_f16k_out_fwd(ops._p(dev(x)), ops._p(packed), ops._p(dev(bias)), ops._p(z16), ctypes.byref(d), ops._stream()),
                  "conv2d_f16k_out_fwd")
        z = ops.f16k_to_nchw(z16, c.B, out_ctot, d.Ho, d.Wo)
        assert torch.equal(z[:, out_coff:out_coff + c.Cout], y[:, out_coff:out_coff + c.Cout]), f"{name}: two calls differ"
        outside = torch.cat([z[:, :out_coff], z[:, out_coff + c.Cout:]], 1)
        assert bool((outside == R.PREFILL).all()), f"{name}: channels outside the output view were written"
    else:
        y = torch.full((c.B, out_ctot, d.Ho, d.Wo), R.PREFILL, device=DEV)
        ops.conv2d(dev(x), packed, dev(bias), d, out=y, gate=dev(gate), res1=dev(res1), res2=dev(res2))
        outside = torch.cat([y[:, :out_coff], y[:, out_coff + c.Cout:]], 1)
        assert bool((outside == R.PREFILL).all()), f"{name}: channels outside the output view were written"
    y = y.cpu()
    own = slice(out_coff, out_coff + c.Cout)
    scale = float(ref[:, own].abs().max())
    err = float((y[:, own].double() - ref[:, own]).abs().max()) / scale
    print(f"conv_rows | {name} | {kernel} | {tuple(c)} | gate {R.gate_of(c):.3e} | relative error {err:.3e}")
    assert_close(y[:, own], ref[:, own], name, R.gate_of(c))
    if case.integers:
        assert torch.equal(y[:, own].double(), ref[:, own]), f"{name}: exact operands, exact sums -- only the bf16 rounding can differ"
