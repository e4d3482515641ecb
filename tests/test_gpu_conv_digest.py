"""The outputs of ops.conv2d / ops.conv2d_f16k_out, one case per entry of CONV_ROWS (masic_amd/csrc/conv.hip) plus gate / residual /
channel-view / partial-tile / F16K-output forms, have the bits recorded in tests/golden/conv_fwd_digest.json
(tests/golden/make_conv_fwd_digest.py: written before the host side became a plan and a table).  No atomics: the digests are exact.
tests/test_cpu_conv_plan.py::test_digest_cases_select_their_kernels holds every case to the kernel it was recorded on."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_conv_fwd_digests_are_the_recorded():
    spec = importlib.util.spec_from_file_location("make_conv_fwd_digest", os.path.join(HERE, "golden", "make_conv_fwd_digest.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(HERE, "golden", "conv_fwd_digest.json")) as f:
        want = {k: v["sha256"] for k, v in json.load(f)["cases"].items()}
    got = gen.digests()
    assert got.keys() == want.keys() and len(got) == 7 * 10 + 5 + len(gen.FORM_CASES)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{len(bad)} of {len(want)} digests differ: {bad[:8]}"
