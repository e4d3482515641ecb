"""pytorch_msssim 0.2.1's public names on the HIP path (masic_amd/ssim.py).

The reference drivers import `from pytorch_msssim import ssim, ms_ssim, SSIM, MS_SSIM` at module scope
(coremasic/mywork/test3_real.py:17, newtrain_cqe_real.py:22); with the repository root on sys.path this package answers that
import, as compressai/ does for the codec.  It shadows a separately installed pytorch_msssim.
"""
from masic_amd.ssim import MS_SSIM, SSIM, ms_ssim, ssim

__all__ = ["ssim", "ms_ssim", "SSIM", "MS_SSIM"]
