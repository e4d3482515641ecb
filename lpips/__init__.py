"""lpips 0.1.4's public name on the HIP path (masic_amd/lpips.py).

The reference's evaluators `import lpips` at module scope and build `lpips.LPIPS(net='alex', spatial=False)`
(coremasic/mywork/test2_real.py:36-37, test3_real.py:33-34); with the repository root on sys.path this package answers that
import, as pytorch_msssim/ and compressai/ do for theirs.  It shadows a separately installed lpips.  Trained lin weights, when
present, are read from `weights/v0.1/alex.pth` next to this file (none ship with the repository; nothing is downloaded).
"""
from masic_amd.lpips import LPIPS

__all__ = ["LPIPS"]
