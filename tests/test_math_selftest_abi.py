"""CPU tests of the test entry rrx_math_selftest (the solvers' device math primitives applied element-wise): declared for both
precisions, bound in hip_kernels.py under the names of csrc/rrx_common.h, and its argument checks answer before any HIP call. What the
primitives compute is tested on the device (tests/test_gpu_math_primitives.py)."""
import os
import re

import pytest

import abi

ENTRY = "rrx_math_selftest"


def test_declared_and_exported_in_both_precisions():
    assert abi.declares(ENTRY)
    lib = abi.lib()
    for sfx in abi.SFXS:
        assert abi.names(ENTRY, sfx) == ["which", "n", "x", "y", "stream"]
        assert lib.has(ENTRY + sfx)
    F = {"_f64": "double", "_f32": "float"}
    for sfx in abi.SFXS:
        assert [t for t, _ in abi.params(ENTRY, sfx)] == ["int", "int", f"const {F[sfx]}*", f"{F[sfx]}*", "void*"]


def test_python_binding_names_the_primitives_of_the_header():
    src = open(os.path.join(abi.ROOT, "rte-rrtmgp-cpp_amd", "hip_kernels.py")).read()
    m = re.search(r"MATH_PRIMITIVES = \(([^)]*)\)", src)
    assert m and re.findall(r'"(\w+)"', m.group(1)) == ["exp_neg", "exp_neg_table", "fast_rcp", "sqrt_pos", "sqrt_nonneg"]
    text = abi.header_macro()
    doc = text[:text.index(ENTRY + "##SFX")].rsplit("/*", 1)[1]
    for i, name in enumerate(("exp_neg", "exp_neg", "fast_rcp", "sqrt_pos", "sqrt_nonneg")):
        assert re.search(rf"\b{i}: {name}\b", doc), (i, name)
    common = open(os.path.join(abi.ROOT, "rte-rrtmgp-cpp_amd", "csrc", "rrx_common.h")).read()
    for name in ("exp_neg", "fast_rcp", "sqrt_pos", "sqrt_nonneg", "exp_table_fill"):
        assert re.search(rf"\b{name}\(", common), name


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("case", ["which5", "which_negative", "n_negative", "null_x", "null_y"])
def test_bad_arguments_are_refused_before_any_launch(sfx, case):
    lib = abi.lib()
    scalars = dict(which=0, n=4)
    null = ()
    if case == "which5": scalars["which"] = 5
    elif case == "which_negative": scalars["which"] = -1
    elif case == "n_negative": scalars["n"] = -1
    else: null = (case[-1],)
    rc, msg = abi.call(lib, ENTRY, sfx, null=null, **scalars)
    assert rc != 0 and ENTRY in msg, (rc, msg)


@pytest.mark.parametrize("sfx", abi.SFXS)
def test_nothing_to_do_returns_zero(sfx):
    rc, _ = abi.call(abi.lib(), ENTRY, sfx, null=("x", "y"), which=4, n=0)
    assert rc == 0
