"""What the CPU tests of the C ABI share: the built library behind the signatures of include/rrx_hip.h (the package's own reader,
_ffi.read_signatures), and calls whose positional argument lists are made from those signatures, so that no test writes an entry's
argument order down a second time."""
import ctypes
import os
import re

import numpy as np
import pytest

from rte_rrtmgp_cpp_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = _ffi.HEADER_PATH
LIB = os.path.join(ROOT, "rte-rrtmgp-cpp_amd", "lib", "librrx_hip.so")
SFXS = ("_f64", "_f32")
# the extents a call takes when the test does not say; any other scalar left out is 1 (a flag: 0)
DEFAULTS = dict(ncol=4, nlay=3, ngpt=8, nbnd=2, nlev=4)
_DTYPES = {"double": np.float64, "float": np.float32, "int": np.int32, "long long": np.int64, "unsigned long long": np.uint64,
           "RrxBool": np.int8, "unsigned char": np.uint8, "void": np.uint8}


def lib():
    """librrx_hip.so bound through the header (status codes are returned, not raised); fails the test if it is not built"""
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} not built: run __graft_entry__.build()")
    return _ffi.Lib(LIB, np.float64, header=HEADER)


def last_error(lib):
    return lib.call("rrx_last_error").decode()


def signatures():
    return _ffi.read_signatures(HEADER)


def declared_symbols():
    return sorted(signatures())


def header_text():
    return open(HEADER).read()


def header_macro():
    """the text of RRX_DECLARE, comments included: the entries' declarations and the semantics written above them"""
    text = header_text()
    return text[text.index("#define RRX_DECLARE"):text.index("RRX_DECLARE(double")]


def declares(entry):
    """whether RRX_DECLARE declares the entry, and so both precisions of it"""
    return re.search(r"\b" + entry + r"##SFX\s*\(", header_macro()) is not None and all(entry + s in signatures() for s in SFXS)


def params(entry, sfx=""):
    """((C type, name), ...) of entry + sfx; of a per-precision entry named without its suffix, the _f64 one"""
    sigs = signatures()
    return sigs[entry + sfx if entry + sfx in sigs else entry + "_f64"].params


def names(entry, sfx=""):
    return [n for _, n in params(entry, sfx)]


def pointers(entry, sfx=""):
    """the names of the entry's pointer parameters but the stream, in order"""
    return [n for t, n in params(entry, sfx) if "*" in t and n != "stream"]


def arguments(entry, sfx, null=(), **scalars):
    """The positional list that the declaration of entry + sfx asks for: every pointer a live host buffer of the declared type (they
    stand in for device pointers: the argument checks answer before anything dereferences them) unless named in null, the stream
    NULL unless given, every scalar the value given by name or the default above."""
    args = []
    unknown = set(scalars) - set(names(entry, sfx))     # (a name in null that the entry does not have is no argument of its call)
    assert not unknown, f"{entry + sfx} has no parameter {sorted(unknown)}: {names(entry, sfx)}"
    for ctype, name in params(entry, sfx):
        base, depth = _ffi._kind(ctype)
        if depth and name in null:
            args.append(None)
        elif name in scalars:                           # (a test may give a pointer's buffer as well)
            args.append(scalars[name])
        elif depth == 0:
            args.append(DEFAULTS.get(name, 0 if base == "RrxBool" else 1))
        elif name == "stream":
            args.append(None)
        else:
            args.append(np.zeros(4, dtype=_DTYPES[base]) if depth == 1 else (ctypes.c_void_p * 4)())
    return args


def call(lib, entry, sfx, null=(), **scalars):
    """Calls entry + sfx with arguments(...). Returns (status, the last-error text)."""
    status = lib.call(entry + sfx, *arguments(entry, sfx, null, **scalars))
    return status, last_error(lib)
