"""ctypes binding of libmasic_hip.so, derived from include/masic_hip.h.

The header is the only statement of the C ABI: its prototypes become SIGNATURES, its enumerators and integer #defines become
this module's constants (MASIC_ prefix removed), its structs become ctypes.Structure classes.  The header is parsed once, at
import.  A declaration the parser does not understand raises; none is skipped.

The product path has no CPU fallback: if the header or the shared library is missing, or a symbol declared in the header is
not exported, importing this module raises.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MASIC_HIP_LIB") or os.path.join(_HERE, "lib", "libmasic_hip.so")   # override: kernel experiments (tools/)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "masic_hip.h")

# The one fact the header does not state: which structs callers fill in HOST memory.  A pointer to one of these becomes
# POINTER(<struct>) (ctypes.byref(desc), an array of groups).  Records of every other struct (masic_code_stream_t,
# masic_view_desc_t, masic_udh_view_desc_t) live in DEVICE memory and are passed as c_void_p(tensor.data_ptr()), which a typed
# POINTER would reject -- as every other pointer, they become c_void_p.
HOST_STRUCTS = ("masic_conv_desc_t", "masic_gemm_group_t", "masic_f16k_multi_out_t")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "char": ctypes.c_char, "unsigned char": ctypes.c_ubyte, "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16,
            "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}


def _ctype(decl, structs, what, named=True, void_ok=False, header="masic_hip.h"):
    """ctypes type of one C declarator: 'const float* const* liks', 'int32_t B', a return type (named=False)"""
    words = [t for t in decl.replace("*", " ").split() if t != "const"]
    stars = decl.count("*")
    name = words.pop() if named and words else "_"
    base = " ".join(words)
    if not name.isidentifier() or not (base in _SCALARS or base in structs or base == "void"):
        raise ValueError(f"{header}: unknown type in '{' '.join(decl.split())}' of {what}")
    if stars == 0:
        if base == "void" and void_ok:
            return None
        if base not in _SCALARS:
            raise ValueError(f"{header}: '{' '.join(decl.split())}' of {what} is passed by value")
        return _SCALARS[base]
    if stars == 1 and base == "char":
        return ctypes.c_char_p
    if stars == 1 and base in HOST_STRUCTS:
        return ctypes.POINTER(structs[base])
    return ctypes.c_void_p


def parse_header(text, header="masic_hip.h"):
    """(signatures {name: (restype, [argtypes])}, constants {name: int}, structs {C name: Structure class}) of a C header
    written as include/masic_hip.h is; ValueError naming the declaration for anything else.  `header`: the name its messages start
    with (the library's side headers are parsed by bind_header)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, structs, signatures = {}, {}, {}

    def define(m):
        name, value = m.group(1), m.group(2).strip()
        if value:
            if not name.startswith("MASIC_") or not re.fullmatch(r"-?\d+", value):
                raise ValueError(f"{header}: #define {name} {value} is not MASIC_<NAME> <integer>")
            constants[name[6:]] = int(value)
        return " "

    def enum(m):
        nxt = 0
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            e = re.fullmatch(r"MASIC_(\w+)(?:\s*=\s*(-?\d+))?", item)
            if not e:
                raise ValueError(f"{header}: enumerator '{item}' is not MASIC_<NAME> [= <integer>]")
            nxt = constants[e.group(1)] = int(e.group(2)) if e.group(2) else nxt
            nxt += 1
        return " "

    def struct(m):
        name, fields = m.group(2), []
        for line in filter(None, (s.strip() for s in m.group(1).split(";"))):
            first, *more = line.split(",")
            ctype = _ctype(first, structs, f"struct {name}", header=header)
            if "*" in line:
                ctype = ctypes.c_void_p
            for n in [first] + more:
                n = n.replace("*", " ").split()
                if not n or not re.fullmatch(r"[A-Za-z_]\w*", n[-1]) or ("*" in line and more):
                    raise ValueError(f"{header}: field '{line}' of struct {name}")
                fields.append((n[-1], ctype))
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": name})
        return " "

    text = re.sub(r"^[ \t]*#[ \t]*define[ \t]+(\w+)([^\n]*)$", define, text, flags=re.M)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)                   # include guard, #include, #ifdef __cplusplus
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    def unparsed(s):
        name = re.search(r"\bmasic_\w+(?=\s*\()", s)
        return ValueError(f"{header}: cannot parse " + (f"the declaration of {name.group(0)}" if name else f"'{' '.join(s.split())[:80]}'"))

    *statements, tail = text.split(";")                 # what is left: prototypes, each up to its semicolon
    if tail.strip():
        raise unparsed(tail)
    for s in statements:
        m = re.fullmatch(r"([^()]*?)\b(masic_\w+)\s*\(([^()]*)\)\s*", s)
        if not m:
            raise unparsed(s)
        name, params = m.group(2), m.group(3).strip()
        args = [] if params == "void" else [_ctype(p, structs, name, header=header) for p in params.split(",")]
        signatures[name] = (_ctype(m.group(1), structs, name, named=False, void_ok=True, header=header), args)
    return signatures, constants, structs


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f"masic_amd: {HEADER_PATH} is missing: the binding is derived from it (MASIC_HIP_LIB moves the library "
                          "only).  There is no CPU fallback for the HIP path.")
    with open(HEADER_PATH) as f:
        return f.read()


# name -> (restype, argtypes) of every prototype; MASIC_<NAME> -> value; C struct name -> ctypes.Structure
SIGNATURES, CONSTANTS, STRUCTS = parse_header(_read_header())
globals().update(CONSTANTS)             # ACT_*, INOP_*, PREC_*, F16K_*, WGRAD_*, CONV_*, SSIM_*, EB_PARAMS_PER_CHANNEL, ...
ConvDesc, GemmGroup, F16kMultiOut, CodeStream = (STRUCTS[f"masic_{n}_t"] for n in ("conv_desc", "gemm_group", "f16k_multi_out", "code_stream"))


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"masic_amd: {LIB_PATH} not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C masic_amd/csrc`). There is no CPU fallback for the HIP path.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def header_path(filename):
    """The path of a side header: a file beside include/masic_hip.h (or an absolute path)."""
    return os.path.join(os.path.dirname(HEADER_PATH), filename)


def bind_header(filename, prefix):
    """Bind a side header of libmasic_hip.so: a file of header_path that holds prototypes only, each a `prefix`* entry point outside
    the pinned ABI of masic_hip.h (SIGNATURES, tests/golden/abi.json), which stays as it is.  Parses it, sets restype and argtypes of
    every prototype on `lib` and returns {name: (restype, argtypes)}."""
    path, header = header_path(filename), os.path.basename(filename)
    if not os.path.exists(path):
        raise ImportError(f"masic_amd.{prefix[len('masic_'):].rstrip('_')}: {path} is missing: the binding is derived from it.  There is "
                          "no CPU fallback for the HIP path.")
    with open(path) as f:
        signatures, constants, structs = parse_header(f.read(), header=header)
    if constants or structs:
        raise ValueError(f"{header}: declares constants or structs; it holds prototypes only")
    for name, (res, args) in signatures.items():
        if not name.startswith(prefix) or name in SIGNATURES:
            raise ValueError(f"{header}: {name} is not a {prefix}* entry point of its own")
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    return signatures


def check(rc, what=""):
    if rc != 0:
        msg = lib.masic_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"masic_hip {what}: error {rc}: {msg}")
