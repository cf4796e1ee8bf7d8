"""ctypes loader for csrc/libmfr_hip.so.  include/mfr_hip.h is the only statement of the C-ABI:
the signatures are parsed from it at the first load(), and call() is the one checked way into
an entry point that returns a status.

torch is imported first so that its bundled HIP runtime (libamdhip64.so.7) is the one the
library binds to -- device pointers and streams handed over from torch tensors then belong to
the same runtime.  Loading fails loudly; nothing in this package falls back to a CPU path.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "csrc", "libmfr_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mfr_hip.h")

_lib = None
_calls = {}      # name -> (n_args, indices of the pointer parameters, has trailing stream, parameter names)
SIGNATURES = {}  # name -> (restype, argtypes); filled from the header by load()

# the header's whole type vocabulary; a new C type is added here on purpose
_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "long long": C.c_longlong, "uint64_t": C.c_uint64}
_POINTEES = {"void", "float", "double", "int", "int32_t", "int64_t", "long long", "uint8_t", "uint16_t", "uint64_t"}
_DECL = re.compile(r"(?:^|[;{}])\s*([A-Za-z_][\w\s*]*?)\b(mfr_[a-z0-9_]+)\s*\(([^()]*)\)\s*(?=;)")
_VALUE_INT = {"mfr_abi_version", "mfr_conv_igemm_k"}   # `int` is a value here, not a status: called as lib.mfr_x(...), like the size queries
_CURRENT = object()


class MfrLibraryError(RuntimeError):
    pass


def _ctype(decl, what, ret=False):
    m = re.fullmatch(r"(const )?([\w ]+?) ?(\*?)", decl)
    const, base, star = m.groups() if m else (None, None, None)
    if ret and (const, base, star) == ("const ", "char", "*"):
        return C.c_char_p
    if star and base in _POINTEES:
        return C.c_void_p
    if not star and not const and base in _SCALARS:
        return _SCALARS[base]
    raise MfrLibraryError(f"{what}: C type '{decl}' is not in _lib's type map")


def parse_header(text):
    """[(name, restype, argtypes, parameter names)] for every `ret mfr_x(args);` of the header text"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    decls = []
    for ret, name, params in _DECL.findall(text):
        params = [" ".join(p.split()) for p in params.split(",")]
        argtypes, argnames = [], []
        for p in [] if params == ["void"] else params:
            m = re.fullmatch(r"(.*?)(\w+)", p)
            if m is None:
                raise MfrLibraryError(f"{name}: cannot read parameter '{p}'")
            argtypes.append(_ctype(m.group(1).strip(), f"{name}({m.group(2)})"))
            argnames.append(m.group(2))
        decls.append((name, _ctype(" ".join(ret.split()), f"{name} return", ret=True), argtypes, argnames))
    named = set(re.findall(r"\b(mfr_[a-z0-9_]+)\s*\(", text))
    if len(decls) != len(named) or {d[0] for d in decls} != named:
        raise MfrLibraryError(f"mfr_hip.h names {len(named)} entry points but {len(decls)} declarations could be read: "
                              f"{sorted(named.symmetric_difference(d[0] for d in decls))}")
    return decls


def load(require_gpu=False):
    """Load libmfr_hip.so and bind every symbol the header declares.  Raises MfrLibraryError if the
    library, the header (or, with require_gpu, a GPU) is missing -- never falls back."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (binds the HIP runtime first)
        if not os.path.exists(SO_PATH):
            raise MfrLibraryError(
                f"{SO_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        if not os.path.exists(HEADER_PATH):
            raise MfrLibraryError(f"{HEADER_PATH} not found: the C-ABI is bound from it")
        with open(HEADER_PATH) as f:
            decls = parse_header(f.read())
        lib = C.CDLL(SO_PATH)
        for name, res, args, names in decls:
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise MfrLibraryError(f"libmfr_hip.so does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
            SIGNATURES[name] = (res, args)
            if res is C.c_int and name not in _VALUE_INT:
                has_stream = bool(names) and names[-1] == "stream" and args[-1] is C.c_void_p
                n = len(args) - has_stream
                _calls[name] = (n, tuple(i for i in range(n) if args[i] is C.c_void_p), has_stream, names)
        _lib = lib
    if require_gpu:
        import torch
        if not torch.cuda.is_available():
            raise MfrLibraryError("no HIP device visible: the HIP path cannot run (there is no CPU fallback)")
    return _lib


def check(rc, what):
    if rc != 0:
        raise MfrLibraryError(f"{what} failed with code {rc} (see include/mfr_hip.h MFR_E_*)")


def ptr(t):
    """device (or host) pointer of a contiguous torch tensor, or None"""
    if t is None:
        return None
    assert t.is_contiguous(), "C-ABI needs contiguous buffers"
    return t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def call(name, *args, stream=_CURRENT):
    """Enter the status-returning entry point `name`.  The argument count is checked against the header;
    a pointer parameter takes a contiguous tensor, None or an address (int); a trailing `void *stream` is
    filled with the current stream unless stream= is given (None = the null stream); a non-zero status raises."""
    if _lib is None:
        load()
    try:
        n, pointers, has_stream, names = _calls[name]
    except KeyError:
        raise MfrLibraryError(f"{name} is not a status-returning entry point of include/mfr_hip.h") from None
    if len(args) != n:
        raise TypeError(f"{name} takes {n} arguments ({', '.join(names[:n])}), got {len(args)}")
    args = list(args)
    for i in pointers:
        a = args[i]
        if a is not None and not isinstance(a, int):
            if not hasattr(a, "data_ptr"):
                raise TypeError(f"{name}: parameter {names[i]} takes a tensor, None or an address, got {type(a).__name__}")
            args[i] = ptr(a)
    if has_stream:
        args.append(stream_ptr() if stream is _CURRENT else stream)
    elif stream is not _CURRENT:
        raise TypeError(f"{name} has no stream parameter")
    try:
        rc = getattr(_lib, name)(*args)              # looked up on the library object, as lib.mfr_x(...) is: a test may wrap an entry there
    except C.ArgumentError as e:                     # a scalar parameter given something else (ctypes' own argtypes check)
        raise TypeError(f"{name}: {e}") from None
    check(rc, name)
