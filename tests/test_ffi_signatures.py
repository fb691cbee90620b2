"""CPU tests of the typed binding (_ffi.py): the signatures read from include/rrx_hip.h are those of the symbols the library exports,
and a Lib bound through the header refuses a call that disagrees with its entry's declaration before the library is entered."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import abi
from rte_rrtmgp_cpp_amd import _ffi
from rte_rrtmgp_cpp_amd._ffi import BoolArg, PtrArg

# the parameter types of include/rrx_hip.h, F standing for the entry's precision
KNOWN_TYPES = {"int", "F", "RrxBool", "long long", "unsigned long long",
               "const F*", "F*", "const int*", "int*", "const RrxBool*", "RrxBool*", "unsigned long long*", "const unsigned long long*",
               "long long*", "const long long*", "unsigned char*", "void*", "const void*",
               "void**", "const F* const*", "F* const*"}
# an entry whose zero-extent call returns 0 without touching HIP, and whose negative-extent call answers before it reads a pointer
FUSED = "rrx_lw_solver_noscat_fractions_rescaled"
GAS_HEAD = ["ncol", "nlay", "nband", "ngpt", "ngas", "nflav", "neta", "npres", "ntemp"]
GAS_MINOR = ["nminorlower", "nminorklower", "nminorupper", "nminorkupper", "idx_h2o", "gpoint_flavor", "band_lims_gpt"]
GAS_TABLES = ["kmajor", "kminor_lower", "kminor_upper", "minor_limits_gpt_lower", "minor_limits_gpt_upper",
              "minor_scales_with_density_lower", "minor_scales_with_density_upper", "scale_by_complement_lower", "scale_by_complement_upper",
              "idx_minor_lower", "idx_minor_upper", "idx_minor_scaling_lower", "idx_minor_scaling_upper", "kminor_start_lower",
              "kminor_start_upper", "flavor", "press_ref_log", "temp_ref", "press_ref_log_delta", "temp_ref_min", "temp_ref_delta",
              "press_ref_trop_log", "vmr_ref"]
SPOT = {
    "rrx_apply_BC_0": ["ncol", "nlay", "ngpt", "top_at_1", "gpt_flux_dn", "stream"],
    "rrx_gas_optics_sw_direct_allsky": GAS_HEAD + GAS_MINOR + GAS_TABLES + [
        "play", "tlay", "col_gas", "col_dry", "krayl", "tau", "ssa", "g", "cld_tau", "cld_ssa", "cld_g", "stream"],
    "rrx_gas_optics_lw_fractions_allsky": GAS_HEAD + ["nPlanckTemp"] + GAS_MINOR + ["gpoint_bands"] + GAS_TABLES + [
        "play", "tlay", "tlev", "tsfc", "sfc_lay", "col_gas", "pfracin", "totplnk_delta", "totplnk",
        "tau", "pfrac", "blay", "blev", "sfc_src", "sfc_src_jac", "cld_tau", "stream"],
}


def test_signatures_are_those_of_the_exported_symbols():
    abi.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", abi.LIB], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines() if l.split()[-1].startswith("rrx_")}
    assert exported == set(abi.signatures())


def test_every_parameter_type_is_a_known_one():
    for name, sig in abi.signatures().items():
        F = {"_f64": "double", "_f32": "float"}.get(name[-4:])
        for ctype, pname in sig.params:
            assert (ctype.replace(F, "F") if F else ctype) in KNOWN_TYPES, (name, ctype, pname)
            assert _ffi._kind(ctype) is not None
    assert abi.signatures()["rrx_last_error"] == ("rrx_last_error", "const char*", ())
    assert abi.signatures()["rrx_workspace_bytes"] == ("rrx_workspace_bytes", "unsigned long long", (("void*", "stream"),))


@pytest.mark.parametrize("entry", sorted(SPOT))
def test_parameter_names_of_three_entries(entry):
    for sfx in abi.SFXS:
        assert abi.names(entry, sfx) == SPOT[entry]
    longest = max(abi.signatures().values(), key=lambda s: len(s.params))
    assert len(longest.params) == 58 == len(SPOT["rrx_gas_optics_lw_fractions_allsky"])
    assert longest.name.startswith("rrx_gas_optics_lw_fractions_allsky")


def test_an_unknown_type_or_a_missing_header_is_an_error(tmp_path):
    bad = tmp_path / "bad.h"
    bad.write_text(abi.header_text().replace("int rrx_set_device(int dev);", "int rrx_set_device(short dev);"))
    with pytest.raises(RuntimeError, match="rrx_set_device.*short dev"):
        _ffi.read_signatures(str(bad))
    with pytest.raises(RuntimeError, match="no_such.h"):
        _ffi.Lib(abi.LIB, np.float64, header=str(tmp_path / "no_such.h"))


def _refused(lib, error, match, entry, args):
    """the call raises before the library is entered: the last error is still the one left there"""
    assert lib.call("rrx_set_lw_variant", 99) != 0
    before = abi.last_error(lib)
    assert "rrx_set_lw_variant" in before
    with pytest.raises(error, match=match):
        lib.call(entry, *args)
    assert abi.last_error(lib) == before


@pytest.mark.parametrize("sfx", abi.SFXS)
def test_a_call_that_disagrees_with_the_declaration_is_refused_before_the_library(sfx):
    lib = abi.lib()
    entry = FUSED + sfx
    own, other = (np.float64, np.float32) if sfx == "_f64" else (np.float32, np.float64)
    assert lib.call(entry, *abi.arguments(FUSED, sfx, ncol=0, top_at_1=1)) == 0
    # a refusal that failed would enter the library with ncol = -1, which it answers with an error of its own
    good = lambda **kw: abi.arguments(FUSED, sfx, **{**dict(ncol=-1, top_at_1=1), **kw})
    assert lib.call(entry, *good()) != 0 and abi.last_error(lib).startswith(FUSED)
    n = len(good())
    _refused(lib, TypeError, rf"{entry} takes {n} arguments, {n-1} given: stream is the first one missing", entry, good()[:-1])
    _refused(lib, TypeError, rf"{entry} takes {n} arguments, {n+1} given", entry, good() + [None])
    _refused(lib, TypeError, rf"{entry}: tau .*float", entry, good(tau=np.zeros(4, dtype=other)))
    _refused(lib, TypeError, rf"{entry}: gpoint_bands .*int32.*int64", entry, good(gpoint_bands=np.zeros(4, dtype=np.int64)))
    _refused(lib, ValueError, rf"{entry}: pfrac.*contiguous", entry, good(pfrac=np.zeros((4, 2), dtype=own)[:, 0]))
    _refused(lib, OverflowError, rf"{entry}: nlay .*2147483648", entry, good(nlay=2**31))
    _refused(lib, TypeError, rf"{entry}: top_at_1", entry, good(top_at_1=ctypes.c_int(1)))                # a ctypes scalar of another class
    _refused(lib, TypeError, rf"{entry}: ngpt", entry, good(ngpt=8.0))
    _refused(lib, TypeError, rf"{entry}: ngpt", entry, good(ngpt=True))
    _refused(lib, OverflowError, rf"rrx_fill{sfx}: n .*-1", "rrx_fill" + sfx, [-1, 1.0, None, None])


@pytest.mark.parametrize("sfx", abi.SFXS)
def test_what_the_declaration_allows_is_accepted(sfx):
    lib = abi.lib()
    F, cF = (np.float64, ctypes.c_double) if sfx == "_f64" else (np.float32, ctypes.c_float)
    # an int at an F parameter goes as the float value
    n, value, arr, stream = lib.converters("rrx_fill" + sfx)
    assert type(value(3)) is float and value(3) == 3.0 and value(np.int32(3)) == 3.0 and value(F(0.5)) == 0.5 and value(cF(0.25)) == 0.25
    assert lib.call("rrx_fill" + sfx, 0, 3, np.zeros(0, dtype=F), None) == 0
    assert n(2**64 - 1) == 2**64 - 1 and n(ctypes.c_ulonglong(5)) == 5 and n(np.int64(7)) == 7
    # booleans
    top = lib.converters("rrx_apply_BC_0" + sfx)[3]
    assert [top(v) for v in (True, 1, BoolArg(True), np.bool_(True), ctypes.c_byte(1))] == [1] * 5
    assert [top(v) for v in (False, 0, BoolArg(False))] == [0] * 3
    for v in (True, 1, BoolArg(True)):
        assert lib.call(FUSED + sfx, *abi.arguments(FUSED, sfx, ncol=0, top_at_1=v)) == 0
    # pointers: None, arrays of the pointee's type, ctypes arrays of it; void* takes any array, a PtrArg or an int
    assert arr(None) is None and arr((cF * 4)()) != 0
    a = np.zeros(4, dtype=F)
    assert arr(a) == a.ctypes.data
    with pytest.raises(TypeError):
        arr((ctypes.c_int * 4)())
    with pytest.raises(TypeError):
        arr(PtrArg(16))
    assert stream(PtrArg(16)) == 16 and stream(16) == 16 and stream(None) is None and stream(np.zeros(2, dtype=np.int16)) != 0
    mask = lib.converters("rrx_mcica_cloud_mask" + sfx)[-2]
    assert all(mask(np.zeros(4, dtype=t)) for t in (np.uint8, np.int8, np.bool_))
    counts = lib.converters("rrx_rt_counts_to_flux" + sfx)[1]
    assert all(counts(np.zeros(4, dtype=t)) for t in (np.uint64, np.int64))
    with pytest.raises(TypeError):
        counts(np.zeros(4, dtype=np.int32))
    # arrays of pointers
    full = lib.converters("rrx_get_from_subset" + sfx)[6]
    assert full((ctypes.c_void_p * 4)()) != 0
    with pytest.raises(TypeError):
        full(np.zeros(4, dtype=np.int64))


def test_torch_tensors_are_checked_like_arrays():
    import torch
    lib = abi.lib()
    tau = lib.converters(FUSED + "_f64")[7]
    t = torch.zeros(4, 2, dtype=torch.float64)
    assert tau(t) == t.data_ptr()
    with pytest.raises(TypeError, match="tau"):
        tau(t.float())
    with pytest.raises(ValueError, match="tau"):
        tau(t[:, 0])


def test_a_lib_without_a_header_marshals_as_before():
    """by reference, types from the Python values: the oracle's convention (include/rrtmgp_kernels.h)"""
    import oracle_py
    path = oracle_py.lib_path("oracle", np.float64)
    if not os.path.exists(path):
        pytest.fail(f"{path} not built: run __graft_entry__.build()")
    lib = _ffi.Lib(path, np.float64, by_ref=True)
    assert lib.signatures is None
    ncol, nlev, ngpt = 3, 2, 4
    gpt_flux = np.arange(ngpt*nlev*ncol, dtype=np.float64).reshape(ngpt, nlev, ncol)
    out = np.zeros((nlev, ncol))
    lib.call("rte_sum_broadband", ncol, nlev, ngpt, gpt_flux, out)
    assert np.array_equal(out, gpt_flux.sum(axis=0))
    with pytest.raises(TypeError, match="BoolArg"):
        lib.call("rte_sum_broadband", True, nlev, ngpt, gpt_flux, out)
    keep = []
    assert isinstance(lib._marshal(5, keep), type(ctypes.byref(ctypes.c_int(5)))) and keep[0].value == 5
    by_value = _ffi.Lib(path, np.float32)
    assert isinstance(by_value._marshal(5, []), ctypes.c_int) and isinstance(by_value._marshal(0.5, []), ctypes.c_float)
    assert by_value._marshal(BoolArg(3), []).value == 1 and by_value._marshal(None, []).value is None
