"""Pins the C ABI as ctypes sees it  ->  tests/golden/abi.json.  Runs without a GPU; needs the system C compiler.

    python tests/golden/make_abi_golden.py

  signatures  what masic_amd._lib derives from include/masic_hip.h, as strings: "masic_sse": ["int", ["void*", ..., "size_t", ...]]
  structs     sizeof, and every field's offsetof and size, of each struct of the header
  constants   every enumerator and integer #define of the header, MASIC_ prefix removed

structs and constants are what the C COMPILER says, not the parser: this script writes a C99 program that includes the header and
prints them, compiles it with `cc -std=c99` and records its output.  Only the names come from the parser; a wrong one does not compile.
Regenerate after every change of the header.  tests/test_cpu_abi.py compares the binding with this file and imports signature_strings
from here."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "abi.json")
SCALAR_NAMES = {None: "void", ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_size_t: "size_t",
                ctypes.c_void_p: "void*", ctypes.c_char_p: "char*"}


def type_string(t):
    """the C spelling of a restype / argtype: KeyError for one the ABI does not use"""
    return t._type_.__name__ + "*" if hasattr(t, "contents") else SCALAR_NAMES[t]


def signature_strings(signatures):
    return {name: [type_string(res), [type_string(a) for a in args]] for name, (res, args) in signatures.items()}


def ask_compiler(structs, constants):
    """(structs {name: {"size": n, "fields": [[field, offset, size], ...]}}, constants {name: value}) printed by a C program"""
    src = ['#include <stdio.h>', '#include "masic_hip.h"', 'int main(void) {']
    for s, cls in structs.items():
        src.append(f'    printf("struct {s} %zu\\n", sizeof({s}));')
        src += [f'    printf("field {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f, _ in cls._fields_]
    src += [f'    printf("constant {c} %lld\\n", (long long)MASIC_{c});' for c in constants]
    src += ['    return 0;', '}', '']
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "abi.c"), os.path.join(tmp, "abi")
        with open(c, "w") as f:
            f.write("\n".join(src))
        subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), c, "-o", exe])
        text = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout
    S, C = {}, {}
    for kind, name, *v in (line.split() for line in text.splitlines()):
        if kind == "struct":
            cur = S[name] = {"size": int(v[0]), "fields": []}
        elif kind == "field":
            cur["fields"].append([name, int(v[0]), int(v[1])])
        else:
            C[name] = int(v[0])
    return S, C


def dumps(abi):
    """one line per entry: a header change shows as the lines of the entries it touches"""
    out = []
    for section, entries in abi.items():
        body = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in entries.items())
        out.append(f' {json.dumps(section)}: {{\n{body}\n }}')
    return "{\n" + ",\n".join(out) + "\n}\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from masic_amd import _lib
    structs, constants = ask_compiler(_lib.STRUCTS, _lib.CONSTANTS)
    abi = {"signatures": signature_strings(_lib.SIGNATURES), "structs": structs, "constants": constants}
    with open(OUT, "w") as f:
        f.write(dumps(abi))
    print(f"{OUT}: {len(abi['signatures'])} prototypes, {len(structs)} structs, {len(constants)} constants, {os.path.getsize(OUT)} bytes")
