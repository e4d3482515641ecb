"""Pins the host-side decisions of the conv_f16k family (masic_amd/csrc/conv_f16k.hip) over a fixed sweep of descriptors:
masic_conv_f16k_supported, _packed_bytes, _multi_supported and _kernel_name with flags 0 and (Cout = 128 only) 1, as answered by
the library of the checkout it runs in -> tests/golden/f16k_plan.npz.  Pure host queries: runs without a GPU.  The committed file
was written by this script placed in a built checkout of the commit BEFORE the dispatch table (plan_f16k) existed, so that the table
is held to the if-ladders it replaced; regenerate it only from a commit whose decisions are meant to become the new reference.

    python tests/golden/make_f16k_plan_golden.py

tests/test_cpu_f16k_plan.py imports sweep() / answers() from here and compares the current library's answers with the file."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "f16k_plan.npz")

# (KH = KW, stride, transposed, masked)
LAYERS = [(5, 2, 0, 0), (5, 2, 1, 0), (3, 2, 0, 0), (3, 1, 0, 0), (3, 1, 1, 0), (5, 1, 0, 0), (5, 1, 0, 1)]
CHANNELS = [(16, 128), (48, 128), (16, 64), (48, 32), (128, 128), (128, 192), (192, 128), (32, 32), (64, 64), (96, 96), (96, 32),
            (128, 32), (32, 64), (64, 96), (128, 64), (256, 128)]
SIZES = [(8, 16), (34, 18), (64, 64), (48, 192), (128, 128), (256, 256)]
BATCHES = [1, 2, 8, 9]
PRECS = [1, 2]          # MASIC_PREC_BF16, MASIC_PREC_FP8
FIELDS = ("k", "stride", "transposed", "masked", "Cin", "Cout", "Hi", "Wi", "B", "prec")


def sweep():
    """[N][len(FIELDS)] int32, in a fixed order."""
    return np.array([(k, s, t, m, ci, co, h, w, b, p) for (k, s, t, m) in LAYERS for (ci, co) in CHANNELS for (h, w) in SIZES
                     for b in BATCHES for p in PRECS], dtype=np.int32)


def desc_of(row, act=0):
    from masic_amd import ops
    k, s, t, m, ci, co, h, w, b, p = (int(v) for v in row)
    return ops.make_conv_desc(b, ci, h, w, co, k, k, s, k // 2, transposed=bool(t), masked=bool(m), act=act, prec=p)


def kernel_name(lib, d, flags):
    """(return code, name)"""
    buf = ctypes.create_string_buffer(96)
    rc = lib.masic_conv_f16k_kernel_name(ctypes.byref(d), flags, buf, 96)
    return rc, buf.value.decode()


def answers(lib, S):
    """The recorded answers for sweep S: names as indices into a sorted list ('' = no name; name1 only asked where Cout = 128)."""
    sup, pb, multi, rc0, n0, rc1, n1 = [], [], [], [], [], [], []
    for row in S:
        d = desc_of(row)
        sup.append(lib.masic_conv_f16k_supported(ctypes.byref(d)))
        pb.append(lib.masic_conv_f16k_packed_bytes(ctypes.byref(d)))
        multi.append(lib.masic_conv_f16k_multi_supported(ctypes.byref(d)))
        rc, name = kernel_name(lib, d, 0)
        rc0.append(rc), n0.append(name)
        rc, name = kernel_name(lib, d, 1) if int(row[5]) == 128 else (0, "")
        rc1.append(rc), n1.append(name)
    names = sorted(set(n0) | set(n1))
    idx = {n: i for i, n in enumerate(names)}
    return {"sweep": S, "supported": np.array(sup, np.int8), "packed_bytes": np.array(pb, np.int64), "multi_supported": np.array(multi, np.int8),
            "rc0": np.array(rc0, np.int8), "name0": np.array([idx[n] for n in n0], np.int8),
            "rc1": np.array(rc1, np.int8), "name1": np.array([idx[n] for n in n1], np.int8), "names": np.array(names)}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from masic_amd import _lib
    A = answers(_lib.lib, sweep())
    np.savez_compressed(OUT, **A)
    print(f"{OUT}: {len(A['sweep'])} descriptors, {int(A['supported'].sum())} supported, {len(A['names']) - 1} names, "
          f"{os.path.getsize(OUT)} bytes (library {_lib.LIB_PATH})")
