"""The outputs of the four F16K kernel families -- conv_f16k / conv_f16k_multi (masic_amd/csrc/conv_f16k.hip), the first analysis layer
(conv_a.hip), the 1x1 GEMMs (gemm_f16k.hip) and the resident 3x3 kernel (conv3x3_resident.hip) --, one case per entry point and form at
the smallest shape with a partial tile or a second co-block, have the bits recorded in tests/golden/f16k_digest.json
(tests/golden/make_f16k_digest.py: written while all four were one source file).  No atomics: the digests are exact.  Every conv_f16k
case is held to the kernel it was recorded on."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_f16k_digests_are_the_recorded():
    spec = importlib.util.spec_from_file_location("make_f16k_digest", os.path.join(HERE, "golden", "make_f16k_digest.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(HERE, "golden", "f16k_digest.json")) as f:
        rec = json.load(f)["cases"]
    assert list(rec) == list(gen.CASES) and len(rec) == 8 + 6 + 5 + 4
    kernels = gen.kernels()
    assert kernels == {k: v["kernel"] for k, v in rec.items() if v["kernel"] is not None} and None not in kernels.values()
    got = gen.digests()
    bad = [k for k in rec if got[k] != rec[k]["sha256"]]
    assert not bad, f"{len(bad)} of {len(rec)} digests differ: {bad[:8]}"
