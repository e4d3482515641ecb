"""deconv_igdn_f16k's host-only answers: which shapes run, and which kernel each takes.  (What include/masic_deconv.h declares and how it
is bound: tests/test_cpu_side_headers.py.)"""


def test_shape_answers_need_no_device():
    """host code only: which shapes run, and which kernel each takes"""
    from masic_amd import _lib, deconv
    assert _lib.lib.masic_deconv_igdn_f16k_supported(8, 128, 128) == 1
    assert _lib.lib.masic_deconv_igdn_f16k_supported(0, 128, 128) == 0
    assert _lib.lib.masic_deconv_igdn_f16k_supported(1, 4096, 4096) == 0
    assert deconv.kernel_name(8, 128, 128) == "deconv_igdn_f16k<8, 2, 5>"
    assert deconv.kernel_name(8, 64, 64) == "deconv_igdn_f16k<8, 2, 5>"
    assert deconv.kernel_name(8, 32, 32) == "deconv_igdn_f16k<8, 1, 5>"
    assert deconv.kernel_name(8, 32, 32, tile=1) == "deconv_igdn_f16k<8, 2, 5>"
