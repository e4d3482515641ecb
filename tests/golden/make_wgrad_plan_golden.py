"""Pins the host-side decisions of the weight-gradient launchers (masic_amd/csrc/conv_wgrad.hip, wgrad_f16k.hip) over a fixed sweep:
every launch a call issues -- kernel with every template argument, grid, block, dynamic LDS bytes, the fill and the finishing pass
included, in order -- its return code, and the answers of masic_conv2d_wgrad_workspace_bytes, every *_det_workspace_bytes and
masic_conv2d_wgrad_bf16in_supported  ->  tests/golden/wgrad_plan.npz.  Runs without a GPU.

The committed file was recorded from commit 37681ab, the commit BEFORE plan_wgrad / WGRAD_ROWS / wg3_run / wg1_run existed.  That commit
cannot name its choice, so its launches are recorded from its unmodified sources: tests/golden/wgrad_plan_record.h turns
hipLaunchKernelGGL into a recorder, a stand-alone program includes the commit's conv_wgrad.hip (a second one wgrad_f16k.hip) after
it, links misc.hip and calls the entry points with dummy pointers; the override covers every launch site of both files.  The byte
queries come from that commit's built library.  Regenerate only from a commit whose decisions are meant to become the new reference:

    python tests/golden/make_wgrad_plan_golden.py REV [path of a libmasic_hip.so built from REV]

(without a library path, REV's library is built first, which takes minutes).  Kernel names are normalised to the full template argument
list, defaults spelled out: conv_wgrad_k5s2_bf16<true> is recorded as conv_wgrad_k5s2_bf16<true, false>; the two slab transposes of
that commit are recorded under the one name they have now, wgrad_slab_transpose_kernel.

tests/test_cpu_wgrad_plan.py imports the sweeps and pack() from here and compares the current library's masic_*_plan_name output."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "wgrad_plan.npz")
DET, IN16, CLEAN = 1, 2, 4          # MASIC_WGRAD_*

# NCHW family: (k, stride, transposed)
LAYERS = [(5, 2, 0), (5, 2, 1), (5, 1, 0), (5, 1, 1), (3, 1, 0), (3, 1, 1), (3, 2, 0), (1, 1, 0), (1, 1, 1)]
CHANNELS = [(3, 128), (128, 3), (3, 6), (6, 3), (6, 8), (8, 128), (48, 32), (128, 128), (192, 128), (128, 192), (320, 192)]
SIZES = [(8, 16), (34, 18), (30, 30), (64, 64), (256, 256)]
BATCHES = [1, 2, 8]
PRECS = [0, 1]                      # MASIC_PREC_F32, MASIC_PREC_BF16
NCHW_FLAGS = [0, CLEAN, DET, IN16, IN16 | CLEAN, IN16 | DET]     # every form that has an entry point
NCHW_FIELDS = ("k", "stride", "transposed", "Cin", "Cout", "Hi", "Wi", "B", "prec", "flags")
# 3x3 / 5x5 F16K and 1x1 F16K
K35_CHANNELS = [(32, 32), (64, 96), (96, 64), (128, 128), (160, 128), (192, 320), (288, 384)]
K35_SIZES = [(8, 8), (16, 24), (32, 32), (256, 256)]
K1_CHANNELS = [(32, 48), (96, 160), (768, 1152), (1152, 768), (768, 960)]
K1_HW = [15, 64, 1024]
# forms the launchers refuse (compared by return code): 7x7, stride 3; channels off the 32 / 16 grid, empty batch, 32-bit offsets, bias_of
NCHW_REFUSED = [(7, 1, 0, 48, 32, 34, 18, 2, 0, 0), (7, 1, 0, 48, 32, 34, 18, 2, 1, DET), (3, 3, 0, 48, 32, 30, 30, 2, 0, 0),
                (5, 3, 1, 128, 128, 8, 16, 1, 1, CLEAN)]
F16K_REFUSED = [(3, 1, 48, 32, 8, 8, 0), (3, 1, 32, 48, 8, 8, DET), (5, 2, 32, 40, 8, 8, CLEAN), (5, 0, 32, 32, 8, 8, 0),
                (3, 8, 288, 384, 1024, 1024, 0), (1, 3, 1, 32, 48, 64, 0), (1, 0, 1, 24, 48, 64, DET), (1, 1, 8, 1152, 768, 1 << 18, 0)]
F16K_FIELDS = ("kind", "a", "b", "c", "d", "e", "flags")      # kind 3 / 5: B Cin Cout H W; kind 1: bias_of B CA CQ HW


def nchw_sweep():
    return np.array([(k, s, t, ci, co, h, w, b, p, f) for (k, s, t) in LAYERS for (ci, co) in CHANNELS for (h, w) in SIZES
                     for b in BATCHES for p in PRECS for f in NCHW_FLAGS] + NCHW_REFUSED, dtype=np.int32)


def f16k_sweep():
    k35 = [(ks, b, ci, co, h, w, f) for ks in (3, 5) for (ci, co) in K35_CHANNELS for (h, w) in K35_SIZES for b in (1, 2, 8)
           for f in (0, CLEAN, DET)]
    k1 = [(1, bias, b, ca, cq, hw, f) for (ca, cq) in K1_CHANNELS for hw in K1_HW for b in (1, 3, 8) for bias in (0, 1, 2) for f in (0, DET)]
    return np.array(k35 + k1 + F16K_REFUSED, dtype=np.int32)


def desc_of(row):
    from masic_amd import ops
    k, s, t, ci, co, h, w, b, p = (int(v) for v in row[:9])
    return ops.make_conv_desc(b, ci, h, w, co, k, k, s, k // 2, transposed=bool(t), prec=p)


def desc_ints(d):
    return np.frombuffer(bytes(d), dtype=np.int32)


def byte_queries(lib, SN, SF):
    """what the library answers natively: per distinct descriptor of the NCHW sweep and per deterministic entry of the F16K sweep"""
    ws, det, sup = [], [], []
    for row in SN:
        d = desc_of(row)
        ws.append(lib.masic_conv2d_wgrad_workspace_bytes(ctypes.byref(d)))
        det.append(lib.masic_conv2d_wgrad_det_workspace_bytes(ctypes.byref(d)))
        sup.append(lib.masic_conv2d_wgrad_bf16in_supported(ctypes.byref(d)))
    fdet = []
    for kind, a, b, c, d_, e, f in SF.tolist():
        q = {3: lib.masic_conv3x3_wgrad_f16k_det_workspace_bytes, 5: lib.masic_conv5x5_wgrad_f16k_det_workspace_bytes,
             1: lib.masic_gemm_wgrad_bias_f16k_det_workspace_bytes}[kind]
        fdet.append(q(a, b, c, d_, e))
    return {"ws_bytes": np.array(ws, np.int64), "det_bytes": np.array(det, np.int64), "bf16in_supported": np.array(sup, np.int8),
            "f16k_det_bytes": np.array(fdet, np.int64)}


def pack(prefix, plans):
    """plans: per sweep entry (return code, [(name, gx, gy, gz, block, lds), ...]) -> arrays, names as indices into a sorted list"""
    names = sorted({l[0] for _, ls in plans for l in ls})
    idx = {n: i for i, n in enumerate(names)}
    flat = [(i, idx[l[0]]) + tuple(l[1:]) for i, (_, ls) in enumerate(plans) for l in ls]
    return {prefix + "rc": np.array([rc for rc, _ in plans], np.int16), prefix + "names": np.array(names),
            prefix + "launches": np.array(flat, np.int64).reshape(-1, 7).astype(np.int32)}


def parse_plan_text(text):
    """the lines of masic_*_plan_name: 'name | gx,gy,gz | block | lds'"""
    out = []
    for line in text.splitlines():
        name, grid, block, lds = (s.strip() for s in line.split(" | "))
        out.append((name,) + tuple(int(v) for v in grid.split(",")) + (int(block), int(lds)))
    return out


# ------------------------------------------------------------------------------------------------ recording a commit without the query
NARGS = {"conv_wgrad_f32": 4, "conv_wgrad_packed_f32": 3, "conv_wgrad_1x1_bf16": 1, "conv_wgrad_k5s2_bf16": 2, "wgrad1x1_f16k": 1}
RENAMED = {"wgrad3_slab_transpose_kernel": "wgrad_slab_transpose_kernel"}
TU = """#include <hip/hip_runtime.h>
#include "wgrad_plan_record.h"
#include "%s"
#define WGRAD_RECORD_DRIVER %d
#include "wgrad_plan_record.h"
"""


def normalise(kernel, where):
    kernel = kernel.strip("() ")
    if kernel == "kfn":              # launch<MA, NQ, KS, DET> of wgrad_f16k.hip: the arguments are in the enclosing function's name
        m = re.search(r"\[MA = (\d+), NQ = (\d+), KS = (\d+), DET = (true|false)\]", where)
        return "wgrad3x3_f16k<%s, %s, %s, %s>" % m.groups()
    base, _, args = kernel.partition("<")
    base = RENAMED.get(base, base)
    if base in NARGS:
        a = [s.strip() for s in args.rstrip(">").split(",")]
        return "%s<%s>" % (base, ", ".join(a + ["false"] * (NARGS[base] - len(a))))
    return kernel if args else base


def record(src_root, source, driver, cases):
    """build the recording program for one source file of the checkout at src_root, feed it the cases, parse its output"""
    csrc = os.path.join(src_root, "masic_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        tu, exe = os.path.join(tmp, "record.hip"), os.path.join(tmp, "record")
        with open(tu, "w") as f:
            f.write(TU % (os.path.join(csrc, source), driver))
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-I" + HERE,
                               "-I" + csrc, "-I" + os.path.join(src_root, "include"), tu, os.path.join(csrc, "misc.hip"), "-o", exe])
        text = subprocess.run([exe], input="\n".join(" ".join(str(int(v)) for v in c) for c in cases) + "\n", text=True, check=True,
                              stdout=subprocess.PIPE).stdout
    plans, lines = [], text.splitlines()
    i = 0
    while i < len(lines):
        _, rc, n = lines[i].split()
        ls = []
        for line in lines[i + 1:i + 1 + int(n)]:
            kernel, where, grid, block, lds = (s.strip() for s in line.split(" | "))
            ls.append((normalise(kernel, where),) + tuple(int(v) for v in grid.split(",")) + (int(block), int(lds)))
        plans.append((int(rc), ls))
        i += 1 + int(n)
    assert len(plans) == len(cases)
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
        for q in ("masic_conv2d_wgrad_workspace_bytes", "masic_conv2d_wgrad_det_workspace_bytes", "masic_conv3x3_wgrad_f16k_det_workspace_bytes",
                  "masic_conv5x5_wgrad_f16k_det_workspace_bytes", "masic_gemm_wgrad_bias_f16k_det_workspace_bytes"):
            getattr(lib, q).restype = ctypes.c_size_t
        SN, SF = nchw_sweep(), f16k_sweep()
        A = {"nchw_sweep": SN, "f16k_sweep": SF}
        A.update(byte_queries(lib, SN, SF))
        A.update(pack("nchw_", record(src, "conv_wgrad.hip", 1, [list(desc_ints(desc_of(r))) + [int(r[9])] for r in SN])))
        A.update(pack("f16k_", record(src, "wgrad_f16k.hip", 2, SF.tolist())))
    np.savez_compressed(OUT, **A)
    print(f"{OUT}: {len(SN)} + {len(SF)} calls, {len(A['nchw_launches'])} + {len(A['f16k_launches'])} launches, "
          f"{len(A['nchw_names'])} + {len(A['f16k_names'])} names, {os.path.getsize(OUT)} bytes (recorded from {rev}, library {libpath})")
    for n in list(A["nchw_names"]) + list(A["f16k_names"]):
        print("   ", n)
