"""The ctypes binding without a GPU: the signatures _lib derives from include/mfr_hip.h against declarations pinned here by hand (one for
every C type the map knows), the parser's loud failures on header text it must not guess about, what _lib.call checks before it enters the
library, and that no second hand-typed table of the C-ABI is left in the package."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import mapfree_reloc_amd as mfr

_lib = mfr._lib
PKG = os.path.dirname(os.path.abspath(_lib.__file__))
vp, i, f, d, ll, u64, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_uint64, C.c_size_t

PINNED = {
    "mfr_target_arch": (C.c_char_p, []),
    "mfr_pnp_workspace_bytes": (sz, [i, i, i]),
    "mfr_pnp_solve_batch": (i, [vp, vp, vp, i, i, vp, i, i, vp, vp, i, i, d, d, u64, vp, vp, sz, vp, vp, vp, vp, vp, vp]),
    "mfr_gemm_f16x2_batched": (i, [vp, i, ll, vp, vp, vp, i, ll, i, i, i, i, i, vp]),
    "mfr_gemm_f16x2_pack_batched": (i, [vp, i, i, ll, i, i, f, vp, vp]),
    "mfr_da_patch_rows": (i, [vp, i, i, i, i, i, i, f, f, f, f, f, f, vp, i, vp]),
    "mfr_sp_nms_candidates": (i, [vp, i, i, i, i, f, i, vp, vp, i, vp, vp]),
    "mfr_sift_level_offset": (ll, [i, i, i, i, i, vp, vp]),
    "mfr_magsac_lut": (i, [vp, i]),
    "mfr_bias_relu_nchw": (i, [vp, vp, i, i, i, vp]),
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()                                                   # loads without a GPU


@pytest.fixture
def null_ok():
    """a non-null, 16-byte aligned host address: no launch happens behind a refused argument"""
    buf = C.create_string_buffer(4096)
    yield C.addressof(buf) // 16 * 16 + 16


# ------------------------------------------------------------------------------------------------ the derived table
def test_pinned_signatures(lib):
    for name, (res, args) in PINNED.items():
        assert _lib.SIGNATURES[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_parser_reads_names_comments_and_void():
    text = """/* int mfr_in_a_comment(int a); */
    #define MFR_X 1   /* int mfr_in_a_define(void); */
    extern "C" {
    int mfr_abi_version(void);
    const char *mfr_target_arch(void);
    long long mfr_off(int B, int *Ho_host /* [1] */, const long long *tab);   // trailing
    int mfr_k(const uint16_t *x, uint64_t seed, size_t n, double t, float e,
              void *stream);
    }"""
    got = {name: (res, args, names) for name, res, args, names in _lib.parse_header(text)}
    assert got == {"mfr_abi_version": (i, [], []), "mfr_target_arch": (C.c_char_p, [], []),
                   "mfr_off": (ll, [i, vp, vp], ["B", "Ho_host", "tab"]),
                   "mfr_k": (i, [vp, u64, sz, d, f, vp], ["x", "seed", "n", "t", "e", "stream"])}


@pytest.mark.parametrize("decl", ["int mfr_x(short a, void *stream);",            # a scalar the map does not know
                                  "int mfr_x(const char *name);",                 # char pointers are a return type only
                                  "int mfr_x(float **rows);",                     # pointer to pointer
                                  "unsigned mfr_x(int a);",                       # unknown return type
                                  "int mfr_x(const int a);"])
def test_unknown_type_is_an_error(decl):
    with pytest.raises(_lib.MfrLibraryError, match="type map"):
        _lib.parse_header("int mfr_ok(int a);\n" + decl)


@pytest.mark.parametrize("decl", ["int mfr_x(int (*cb)(int), void *stream);",     # function-pointer parameter
                                  "int mfr_x(int a, void *stream)"])              # no semicolon
def test_unreadable_declaration_is_an_error_not_a_missing_binding(decl):
    with pytest.raises(_lib.MfrLibraryError, match="mfr_x"):
        _lib.parse_header("int mfr_ok(int a);\n" + decl + "\nint mfr_ok2(void);")


def test_missing_header_is_an_error(lib, monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "mfr_hip.h"))
    with pytest.raises(_lib.MfrLibraryError, match="mfr_hip.h"):
        _lib.load()


# ------------------------------------------------------------------------------------------------ call
def test_call_checks_the_argument_count_before_the_library(lib, monkeypatch):
    entered = []
    monkeypatch.setattr(lib, "mfr_bias_relu_nchw", lambda *a: entered.append(a) or 0)
    for args in [(None, None, 1, 4), (None, None, 1, 4, 16, 0)]:                  # one short, one too many
        with pytest.raises(TypeError, match="mfr_bias_relu_nchw takes 5 arguments"):
            _lib.call("mfr_bias_relu_nchw", *args, stream=None)
    assert entered == []
    _lib.call("mfr_bias_relu_nchw", None, None, 1, 4, 16, stream=None)            # the declared five do arrive
    assert entered == [(None, None, 1, 4, 16, None)]


def test_call_pointer_parameters(lib, null_ok):
    p = null_ok
    with pytest.raises(AssertionError, match="contiguous"):
        _lib.call("mfr_lg_rotary_table", torch.zeros(4, 4).t(), p, 4, p, stream=None)
    with pytest.raises(TypeError, match=r"mfr_lg_rotary_table: parameter wr"):
        _lib.call("mfr_lg_rotary_table", p, [0.0], 4, p, stream=None)
    with pytest.raises(TypeError, match=r"mfr_lg_rotary_table: parameter wr"):
        _lib.call("mfr_lg_rotary_table", p, 1.5, 4, p, stream=None)


def test_call_scalar_parameters_go_through_ctypes(lib, null_ok):
    p = null_ok
    # (ctypes converts through __index__, so the one tensor it takes for an int is an integer tensor of exactly one element)
    for bad in (torch.zeros(4, 2), torch.zeros(1), torch.zeros(3, dtype=torch.int32), 4.0, None):
        with pytest.raises(TypeError, match="mfr_lg_rotary_table"):
            _lib.call("mfr_lg_rotary_table", p, p, bad, p, stream=None)
    with pytest.raises(TypeError, match="mfr_lg_ln_gelu"):
        _lib.call("mfr_lg_ln_gelu", p, 512, 4, p, p, torch.zeros(2), stream=None)   # a tensor for a float


def test_refused_call_names_the_function(lib, null_ok):
    p = null_ok
    with pytest.raises(_lib.MfrLibraryError, match="mfr_lg_rotary_table failed with code -1"):
        _lib.call("mfr_lg_rotary_table", None, p, 4, p, stream=None)               # null where a pointer is required
    with pytest.raises(_lib.MfrLibraryError, match="mfr_bias_relu_nchw failed with code -1"):
        _lib.call("mfr_bias_relu_nchw", torch.zeros(4), None, 1, 4, 16, stream=None)   # a (host) tensor goes through ptr(); the null bias is refused


def test_value_returning_entry_points_are_not_calls(lib):
    for name in ("mfr_pnp_workspace_bytes", "mfr_target_arch", "mfr_sift_level_offset", "mfr_no_such_entry",
                 "mfr_abi_version", "mfr_conv_igemm_k"):                            # the last two return an int that is a value
        with pytest.raises(_lib.MfrLibraryError, match=name + " is not a status-returning entry point"):
            _lib.call(name, 1, 2, 3)
    assert lib.mfr_abi_version() == 6 and lib.mfr_conv_igemm_k(64, 3, 3) == 576


def test_entry_without_a_stream_parameter(lib):
    M = 16
    want = np.zeros((M + 1, 2)); got = np.zeros((M + 1, 2))
    assert lib.mfr_magsac_lut(want.ctypes.data, M) == 0
    _lib.call("mfr_magsac_lut", got.ctypes.data, M)                                # nothing is appended: two parameters, two arguments
    assert want.any() and np.array_equal(got, want)
    with pytest.raises(TypeError, match="mfr_magsac_lut has no stream parameter"):
        _lib.call("mfr_magsac_lut", got.ctypes.data, M, stream=None)
    with pytest.raises(TypeError, match="mfr_magsac_lut takes 2 arguments"):
        _lib.call("mfr_magsac_lut", got.ctypes.data, M, None)


def test_stream_fill(lib, monkeypatch):
    seen = []
    monkeypatch.setattr(lib, "mfr_bias_relu_nchw", lambda *a: seen.append(a) or 0)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0x5E471E1)
    x = torch.zeros(64)
    _lib.call("mfr_bias_relu_nchw", x, x.data_ptr() + 16, 1, 4, 16)
    assert seen.pop() == (x.data_ptr(), x.data_ptr() + 16, 1, 4, 16, 0x5E471E1)     # the sentinel arrives last, tensors as addresses

    def never():
        raise AssertionError("stream_ptr() consulted although stream= was given")
    monkeypatch.setattr(_lib, "stream_ptr", never)
    _lib.call("mfr_bias_relu_nchw", x, None, 1, 4, 16, stream=None)
    _lib.call("mfr_bias_relu_nchw", x, None, 1, 4, 16, stream=77)
    assert seen == [(x.data_ptr(), None, 1, 4, 16, None), (x.data_ptr(), None, 1, 4, 16, 77)]


# ------------------------------------------------------------------------------------------------ one statement of the ABI
def test_no_hand_typed_signature_lists_left():
    assign = re.compile(r"\.(argtypes|restype)\b[^=\n]*=[^=]")
    hits = {}
    for path in glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True):
        lines = [ln for ln in open(path).read().splitlines() if assign.search(ln)]
        if lines:
            hits[os.path.relpath(path, PKG)] = lines
    assert sorted(hits) == ["_lib.py", "datasets.py"], sorted(hits)
    assert len(hits["_lib.py"]) == 2                                               # the one binding loop: fn.restype, fn.argtypes
    assert all("mfr_host_" in ln for ln in hits["datasets.py"])                    # libmfr_host.so, declared in no header
