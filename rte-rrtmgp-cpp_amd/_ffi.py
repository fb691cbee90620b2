"""ctypes marshalling shared by the HIP binding (this package) and the test-only oracle bindings.

A ``Lib`` wraps one shared object and one calling convention:
  header=path  : librrx_hip.so. Every call is checked against the signature that include/rrx_hip.h declares for the entry
                 (read_signatures) before the library is entered: the argument count, the range of every integer, the dtype and
                 contiguity of every array. Scalars by value.
  by_ref=False : no header: scalars by value, types guessed from the Python values (oracle/_ref)
  by_ref=True  : no header: every scalar passed by address (the Fortran bind(C) convention of include/rrtmgp_kernels.h)
Without a header: int -> c_int, float -> Float, BoolArg -> signed char, numpy array / torch tensor -> data pointer,
None -> NULL, ctypes objects are passed through.
"""
import collections
import ctypes
import functools
import numbers
import os
import re
import numpy as np

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rrx_hip.h")


class BoolArg:
    """Marks a scalar that must be marshalled as the reference's Bool (signed char)."""
    def __init__(self, value):
        self.value = 1 if value else 0


class PtrArg:
    """A raw pointer value (e.g. a hipStream_t)."""
    def __init__(self, value):
        self.value = int(value) if value else 0


# ---- the signatures of include/rrx_hip.h ------------------------------------------------------------------------------------------
Signature = collections.namedtuple("Signature", "name restype params")      # params: ((C type, name), ...)

# C scalar -> (ctypes class, smallest, largest) for the integers, (ctypes class,) for the floats
_SCALARS = {"int": (ctypes.c_int, -2**31, 2**31 - 1), "long long": (ctypes.c_longlong, -2**63, 2**63 - 1),
            "unsigned long long": (ctypes.c_ulonglong, 0, 2**64 - 1), "RrxBool": (ctypes.c_byte, 0, 1),
            "double": (ctypes.c_double,), "float": (ctypes.c_float,)}
# pointee -> the dtype names an array may have, the element types a ctypes array may have
_BYTES = (("int8", "uint8", "bool"), (ctypes.c_byte, ctypes.c_ubyte, ctypes.c_bool))
_WORDS = (("int64", "uint64"), (ctypes.c_longlong, ctypes.c_ulonglong))
_POINTEES = {"double": (("float64",), (ctypes.c_double,)), "float": (("float32",), (ctypes.c_float,)),
             "int": (("int32",), (ctypes.c_int,)), "long long": _WORDS, "unsigned long long": _WORDS,
             "RrxBool": _BYTES, "unsigned char": _BYTES, "void": (None, None)}
_RESTYPES = {"int": ctypes.c_int, "const char*": ctypes.c_char_p, "unsigned long long": ctypes.c_ulonglong}


def _kind(ctype):
    """(base type, pointer depth) of a parameter's C type, or None for a type this module does not know"""
    base = re.sub(r"\bconst\b|\*", " ", ctype).split()
    base, depth = " ".join(base), ctype.count("*")
    known = (_SCALARS, _POINTEES, ("void", "double", "float"))
    return (base, depth) if depth < 3 and base in known[depth] else None


@functools.lru_cache(maxsize=None)
def read_signatures(path=HEADER_PATH):
    """{symbol: Signature} for every function that the header declares, the RRX_DECLARE entries once per precision with ##SFX and
    F expanded. A declaration that cannot be read in full (a return or parameter type not known here) is an error."""
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: the binding reads the signatures of librrx_hip.so from it")
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S).replace("\\\n", " ")
    macro = re.search(r"^#define RRX_DECLARE\(F, SFX\)(.*)$", text, re.M)
    uses = re.findall(r"^RRX_DECLARE\((\w+), (\w+)\)", text, re.M)
    if not macro or not uses:
        raise RuntimeError(f"{path}: no RRX_DECLARE(F, SFX) with its uses")
    text = text.replace(macro.group(0), "") + "".join(re.sub(r"\bF\b", f, macro.group(1)).replace("##SFX", sfx) for f, sfx in uses)
    sigs = {}
    for m in re.finditer(r"(?:^|[;{}])\s*([\w \*]+?)\s*\b(rrx_\w+)\s*\(([^()]*)\)\s*(?=;)", text, re.M):
        restype, name, params = (re.sub(r"\s+", " ", s).strip() for s in m.groups())
        params = [] if params == "void" else [re.match(r"(.*?)\s*(\w+)$", p.strip()).groups() for p in params.split(",")]
        params = tuple((re.sub(r"\s*\*", "*", t), n) for t, n in params)
        bad = [f"{t} {n}" for t, n in params if _kind(t) is None] + ([] if restype in _RESTYPES else [f"return type {restype}"])
        if bad or name in sigs:
            raise RuntimeError(f"{path}: cannot bind {name}: " + (", ".join(bad) if bad else "declared twice"))
        sigs[name] = Signature(name, restype, params)
    missed = set(re.findall(r"\b(rrx_\w+)\s*\(", text)) - set(sigs)
    if missed:
        raise RuntimeError(f"{path}: declarations not understood: {sorted(missed)}")
    return sigs


# ---- one converter per parameter: the Python value -> what ctypes passes under the entry's argtypes, or an exception ----------------
def _is_int(a):
    return isinstance(a, (int, np.integer)) and not isinstance(a, (bool, np.bool_))


def _scalar(where, base):
    ctype, *limits = _SCALARS[base]
    if not limits:
        def conv(a):
            if type(a) is float:
                return a
            if isinstance(a, ctype):
                return a.value
            if isinstance(a, numbers.Real) and not isinstance(a, (bool, np.bool_)):
                return float(a)
            raise TypeError(f"{where} ({base}) takes a real number, not {type(a).__name__}")
        return conv
    lo, hi = limits
    is_bool = base == "RrxBool"

    def conv(a):
        if type(a) is not int:
            if isinstance(a, (ctype, BoolArg) if is_bool else ctype):
                a = a.value
            elif _is_int(a) or (is_bool and isinstance(a, (bool, np.bool_))):
                a = int(a)
            else:
                raise TypeError(f"{where} ({base}) takes {'a bool, 0 or 1' if is_bool else 'an integer'}, not {type(a).__name__}")
        if not lo <= a <= hi:
            raise OverflowError(f"{where} ({base}): {a} is outside {lo} .. {hi}")
        return a
    return conv


def _pointer(where, ctype, base):
    names, elements = _POINTEES[base]
    known = {}                  # dtype object (numpy's or torch's) -> whether it is one of names

    def conv(a):
        if a is None:
            return None
        try:
            dtype = a.dtype
        except AttributeError:
            if isinstance(a, ctypes.Array) and (elements is None or a._type_ in elements):
                return ctypes.addressof(a)
            if elements is None and isinstance(a, (PtrArg, ctypes.c_void_p)):
                return a.value
            if elements is None and _is_int(a):
                return int(a)
            raise TypeError(f"{where} ({ctype}) does not take {type(a).__name__}"
                            + (f" of {a._type_.__name__}" if isinstance(a, ctypes.Array) else "")) from None
        ok = known.get(dtype)
        if ok is None:
            ok = known[dtype] = names is None or str(dtype).rsplit(".", 1)[-1] in names
        if not ok:
            raise TypeError(f"{where} ({ctype}) takes {' or '.join(names)}, not {dtype}")
        if isinstance(a, np.ndarray):
            if not a.flags.c_contiguous:
                raise ValueError(f"{where}: the array must be contiguous")
            return a.ctypes.data
        if not a.is_contiguous():                       # torch tensor
            raise ValueError(f"{where}: the tensor must be contiguous")
        return a.data_ptr()
    return conv


def _pointer_array(where, ctype):
    def conv(a):
        if a is None:
            return None
        if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
            return ctypes.addressof(a)
        raise TypeError(f"{where} ({ctype}) takes a ctypes array of c_void_p, not {type(a).__name__}")
    return conv


def _converter(entry, ctype, pname):
    base, depth = _kind(ctype)
    where = f"{entry}: {pname}"
    if depth == 0:
        return _scalar(where, base)
    return _pointer(where, ctype, base) if depth == 1 else _pointer_array(where, ctype)


class Lib:
    def __init__(self, path, float_dtype, by_ref=False, returns_status=False, error_fn=None, header=None):
        self.path = path
        self.cdll = ctypes.CDLL(path)
        self.float_dtype = np.dtype(float_dtype)
        self.cfloat = ctypes.c_double if self.float_dtype == np.float64 else ctypes.c_float
        self.by_ref = by_ref
        self.returns_status = returns_status
        self.error_fn = error_fn
        if header is not None and by_ref:
            raise ValueError("a header states a by-value interface")
        self.signatures = read_signatures(header) if header is not None else None
        self._bound = {}            # entry -> (function with argtypes, converters, Signature), made on first use

    def has(self, name):
        return hasattr(self.cdll, name)

    def _marshal(self, a, keep):
        if a is None:
            return ctypes.c_void_p(0)
        if isinstance(a, BoolArg):
            v = ctypes.c_byte(a.value)
        elif isinstance(a, PtrArg):
            return ctypes.c_void_p(a.value)
        elif isinstance(a, (bool, np.bool_)):
            raise TypeError("wrap booleans in BoolArg")
        elif isinstance(a, (int, np.integer)):
            v = ctypes.c_int(int(a))
        elif isinstance(a, (float, np.floating)):
            v = self.cfloat(float(a))
        elif isinstance(a, np.ndarray):
            if not a.flags["C_CONTIGUOUS"]:
                raise ValueError("array arguments must be contiguous")
            keep.append(a)
            return ctypes.c_void_p(a.ctypes.data)
        elif hasattr(a, "data_ptr"):                     # torch tensor
            if not a.is_contiguous():
                raise ValueError("tensor arguments must be contiguous")
            keep.append(a)
            return ctypes.c_void_p(a.data_ptr())
        elif isinstance(a, ctypes._SimpleCData) or isinstance(a, ctypes.Array):
            return a
        else:
            raise TypeError(f"cannot marshal {type(a)}")
        if self.by_ref:
            keep.append(v)
            return ctypes.byref(v)
        return v

    def _bind(self, name):
        sig = self.signatures.get(name)
        if sig is None:
            raise AttributeError(f"{name} is not declared in the header of {self.path}")
        fn = getattr(self.cdll, name)
        fn.restype = _RESTYPES[sig.restype]
        fn.argtypes = [ctypes.c_void_p if "*" in t else _SCALARS[_kind(t)[0]][0] for t, _ in sig.params]
        bound = self._bound[name] = (fn, tuple(_converter(name, t, n) for t, n in sig.params), sig)
        return bound

    def converters(self, name):
        """The converters of a declared entry, one per parameter (tests look at what they return)."""
        return (self._bound.get(name) or self._bind(name))[1]

    def call(self, name, *args):
        if self.signatures is None:
            fn = getattr(self.cdll, name)
            fn.restype = ctypes.c_int if self.returns_status else None
            keep = []
            rc = fn(*[self._marshal(a, keep) for a in args])
        else:
            fn, convs, sig = self._bound.get(name) or self._bind(name)
            if len(args) != len(convs):
                raise TypeError(f"{name} takes {len(convs)} arguments, {len(args)} given: " + (
                    f"{sig.params[len(args)][1]} is the first one missing" if len(args) < len(convs) else "too many"))
            rc = fn(*[c(a) for c, a in zip(convs, args)])
            if sig.restype != "int":
                return rc
        if self.returns_status and rc != 0:
            msg = self.error_fn() if self.error_fn else ""
            raise RuntimeError(f"{name} failed (status {rc}): {msg}")
        return rc
