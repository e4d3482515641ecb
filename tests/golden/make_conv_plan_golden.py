"""Pins the host-side decisions of the NCHW convolution launcher (masic_amd/csrc/conv.hip) over a fixed sweep: the launch a call
issues -- kernel with every template argument, grid, block, dynamic LDS bytes and the integers of its argument struct --, its return
code, and the answers of masic_conv_packed_bytes, masic_conv_kernel_name and masic_conv2d_f16k_out_supported
->  tests/golden/conv_plan.npz.  Runs without a GPU.

The committed file was recorded from commit b955ed7, the commit BEFORE plan_conv / CONV_ROWS existed.  That commit cannot name its
launch with the form's operands, so its launches are recorded from its unmodified source: tests/golden/conv_plan_record.h turns
hipLaunchKernelGGL into a recorder, a stand-alone program includes the commit's conv.hip after it, links misc.hip and calls
masic_conv2d_fwd_ex / masic_conv2d_f16k_out_fwd with dummy pointers.  The three queries come from that commit's built library.
Regenerate only from a commit whose decisions are meant to become the new reference:

    python tests/golden/make_conv_plan_golden.py REV [path of a libmasic_hip.so built from REV]

(without a library path, REV's library is built first, which takes minutes).

tests/test_cpu_conv_plan.py imports the sweep and pack() from here and compares the current library's masic_conv_plan_name output."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "conv_plan.npz")
GATE, RES1, RES2, F16K_OUT = 1, 2, 4, 8          # MASIC_CONV_*
F32, BF16, FP8 = 0, 1, 2                         # MASIC_PREC_*
SOFTMAX = 3                                      # MASIC_ACT_SOFTMAX_C

# (k, stride, transposed, masked): 1x1, 3x3 s1, 3x3 s2, 5x5 s1, 5x5 s2, 5x5 s2 transposed, 3x3 s1 transposed, 5x5 s1 masked
KINDS = [(1, 1, 0, 0), (3, 1, 0, 0), (3, 2, 0, 0), (5, 1, 0, 0), (5, 2, 0, 0), (5, 2, 1, 0), (3, 1, 1, 0), (5, 1, 0, 1)]
CHANNELS = [(3, 3), (6, 3), (3, 8), (128, 3), (16, 4), (2, 12), (3, 128), (24, 32), (32, 32), (64, 64), (48, 96), (96, 96), (128, 128),
            (192, 128), (128, 192), (192, 384), (128, 256)]
SIZES = [(5, 7), (8, 16), (16, 12), (34, 18), (64, 64), (48, 192), (128, 128), (256, 256)]
BATCHES = [1, 2, 8, 9]
FORMS = [0, GATE, RES1, RES1 | RES2, F16K_OUT]
FIELDS = ("k", "stride", "transposed", "masked", "Cin", "Cout", "Hi", "Wi", "B", "prec", "in_op", "act", "form")
NINTS = 12                                       # integers after a plan line, at most (the igemm kernels'); shorter lists padded with -1


def sweep():
    """The product is thinned where an axis cannot change the decision it is crossed with: every (kind, channels, size, batch, precision,
    in_op) plainly; every form and the channel softmax over every (kind, channels, size, precision) at two batches; a few fp8."""
    S = []
    for kind in KINDS:
        for (ci, co) in CHANNELS:
            for (h, w) in SIZES:
                for p in (F32, BF16):
                    for b in BATCHES:
                        S += [kind + (ci, co, h, w, b, p, op, 0, 0) for op in (0, 1, 2)]
                    for b in (1, 8):
                        S += [kind + (ci, co, h, w, b, p, 0, 0, f) for f in FORMS[1:]]
                        if co <= 8:
                            S += [kind + (ci, co, h, w, b, p, 0, SOFTMAX, f) for f in (0, GATE)]
    S += [kind + (ci, co, 16, 12, 2, FP8, 0, 0, f) for kind in KINDS for (ci, co) in ((6, 3), (128, 3), (32, 32), (128, 128)) for f in (0, F16K_OUT)]
    return np.array(S, dtype=np.int32)


def desc_of(row):
    """the descriptor of a sweep entry; the F16K-output form writes into a buffer of whole 16-channel records"""
    from masic_amd import ops
    k, s, t, m, ci, co, h, w, b, p, op, act, form = (int(v) for v in row)
    return ops.make_conv_desc(b, ci, h, w, co, k, k, s, k // 2, transposed=bool(t), masked=bool(m), in_op=op, act=act, prec=p,
                              gate_ctot=1 if form & GATE else 0, out_ctot=(co + 15) // 16 * 16 if form & F16K_OUT else None)


# descriptors make_conv_desc does not make: an empty output (pad 0, 5x5 on 2x2: MASIC_OK without a launch), 7x7, stride 3, a view past
# its buffer; as (22 descriptor integers, form)
def extra_cases():
    from masic_amd import ops
    out = []
    for form in (0, GATE | RES1):
        for (ci, co) in ((128, 3), (128, 128)):
            out.append((ops.make_conv_desc(2, ci, 2, 2, co, 5, 5, 1, 0, prec=BF16), form))
    out.append((ops.make_conv_desc(2, 32, 16, 16, 32, 7, 7, 1, 3), 0))
    out.append((ops.make_conv_desc(2, 32, 16, 16, 32, 3, 3, 3, 1), 0))
    out.append((ops.make_conv_desc(2, 32, 16, 16, 32, 3, 3, 1, 1, out_ctot=40, out_coff=16), 0))
    out.append((ops.make_conv_desc(2, 32, 16, 16, 32, 3, 3, 1, 1, out_ctot=40, out_coff=16, prec=BF16), F16K_OUT))
    return [(d, f) for d, f in out]


def cases():
    """every call of the recording: (descriptor, form), the sweep first"""
    return [(desc_of(r), int(r[12])) for r in sweep()] + extra_cases()


def desc_ints(d):
    return np.frombuffer(bytes(d), dtype=np.int32)


def queries(lib, C):
    """what the library answers natively, per call of the recording (the form does not enter)"""
    nbytes, names, rcs, sup = [], [], [], []
    buf = ctypes.create_string_buffer(96)
    for d, _ in C:
        nbytes.append(lib.masic_conv_packed_bytes(ctypes.byref(d)))
        buf.value = b""
        rcs.append(lib.masic_conv_kernel_name(ctypes.byref(d), buf, 96))
        names.append(buf.value.decode() if rcs[-1] == 0 else "")
        sup.append(lib.masic_conv2d_f16k_out_supported(ctypes.byref(d)))
    uniq = sorted(set(names))
    idx = {n: i for i, n in enumerate(uniq)}
    return {"packed_bytes": np.array(nbytes, np.int64), "kname_rc": np.array(rcs, np.int16), "kname_names": np.array(uniq),
            "kname": np.array([idx[n] for n in names], np.int16), "f16k_out_supported": np.array(sup, np.int8)}


def pack(plans):
    """plans: per call (return code, [(name, gx, gy, gz, block, lds, (integers...)), ...]) -> arrays, names as indices into a sorted list"""
    names = sorted({l[0] for _, ls in plans for l in ls})
    idx = {n: i for i, n in enumerate(names)}
    flat = [(i, idx[l[0]]) + tuple(l[1:6]) + tuple(l[6]) + (-1,) * (NINTS - len(l[6])) for i, (_, ls) in enumerate(plans) for l in ls]
    return {"rc": np.array([rc for rc, _ in plans], np.int16), "names": np.array(names),
            "launches": np.array(flat, np.int64).reshape(-1, 7 + NINTS).astype(np.int32)}


def parse_plan_text(text):
    """the lines of masic_conv_plan_name and of the recorder: 'name | gx,gy,gz | block | lds | integers'"""
    out = []
    for line in text.splitlines():
        name, grid, block, lds, ints = (s.strip() for s in line.split(" |"))
        out.append((normalise(name),) + tuple(int(v) for v in grid.split(",")) + (int(block), int(lds), tuple(int(v) for v in ints.split())))
    return out


# ------------------------------------------------------------------------------------------------ recording a commit without the query
TU = """#include <hip/hip_runtime.h>
#include "conv_plan_record.h"
#include "%s"
#define CONV_RECORD_DRIVER 1
#include "conv_plan_record.h"
"""


def normalise(kernel):
    """the launch site's spelling of a kernel -> the name with its template arguments as values"""
    kernel = kernel.strip("() ")
    for name, v in (("MASIC_INOP_NONE", "0"), ("MASIC_INOP_ABS", "1"), ("MASIC_INOP_ROUND", "2")):
        kernel = kernel.replace(name, v)
    return kernel


def record(src_root, C):
    """build the recording program for conv.hip of the checkout at src_root, feed it the calls, parse its output"""
    csrc = os.path.join(src_root, "masic_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        tu, exe = os.path.join(tmp, "record.hip"), os.path.join(tmp, "record")
        with open(tu, "w") as f:
            f.write(TU % os.path.join(csrc, "conv.hip"))
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-I" + HERE,
                               "-I" + csrc, "-I" + os.path.join(src_root, "include"), tu, os.path.join(csrc, "misc.hip"), "-o", exe])
        text = subprocess.run([exe], input="\n".join(" ".join(str(int(v)) for v in list(desc_ints(d)) + [f]) for d, f in C) + "\n", text=True,
                              check=True, stdout=subprocess.PIPE).stdout
    plans, lines = [], text.splitlines()
    i = 0
    while i < len(lines):
        _, rc, n = lines[i].split()
        plans.append((int(rc), parse_plan_text("\n".join(lines[i + 1:i + 1 + int(n)]))))
        i += 1 + int(n)
    assert len(plans) == len(C)
    return plans


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as src:
        subprocess.check_call(f"git -C {ROOT} archive {rev} masic_amd/csrc include | tar -x -C {src}", shell=True)
        if len(sys.argv) > 2:
            libpath = sys.argv[2]
        else:
            subprocess.check_call(["make", "-s", "-C", os.path.join(src, "masic_amd", "csrc"), "-j8", "OUT=librev.so"])
            libpath = os.path.join(src, "masic_amd", "csrc", "librev.so")
        lib = ctypes.CDLL(libpath)      # (not through masic_amd._lib: REV's library lacks the symbols _lib declares today)
        lib.masic_conv_packed_bytes.restype = ctypes.c_size_t
        C = cases()
        A = {"sweep": sweep(), "extra": np.array([list(desc_ints(d)) + [f] for d, f in extra_cases()], np.int32)}
        A.update(queries(lib, C))
        A.update(pack(record(src, C)))
    np.savez_compressed(OUT, **A)
    print(f"{OUT}: {len(C)} calls, {len(A['launches'])} launches, {len(A['names'])} names, {os.path.getsize(OUT)} bytes "
          f"(recorded from {rev}, library {libpath})")
    for n in A["names"]:
        print("   ", n)
    print("refused:", {int(c): int((A["rc"] == c).sum()) for c in np.unique(A["rc"])})
