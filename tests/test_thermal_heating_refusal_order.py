"""The ORDER in which the thermal tracer's heating entries refuse their arguments (CPU): the test of
test_raytracer_refusal_order.py for rrx_heating3d_counts, rrx_heating3d_counts_spectral and rrx_heating3d_render,
made with that file's calls. For every pair i < j of faults that do not concern the same argument both are applied and fault i's
message must come back, prefixed with the entry's name; a zero extent returns 0 before any later fault is looked at."""
import itertools

import pytest

import abi
import test_raytracer_refusal_order as RO

COUNTS, SPECTRAL, RENDER = "rrx_heating3d_counts", "rrx_heating3d_counts_spectral", "rrx_heating3d_render"
ENTRIES = (COUNTS, SPECTRAL, RENDER)
NAN = float("nan")


def _call(lib, entry, sfx, faults):
    """test_raytracer_refusal_order._call on a valid scene of the entry: the loop's host arrays are its top_radiance and its rays"""
    base = {"top_radiance": "top", "rays_per_cell_gpt": "m"} if entry == RENDER else {}
    return RO._call(lib, entry, sfx, [base] + list(faults))


def ORDER(entry):
    """[(fault, the word of its message)] in the order in which entry reports them, read from check_entry and ray_list of
    csrc/rrx_rt_host.h and the entries' own checks in csrc/rrx_raytracer_heating.hip"""
    null = lambda name: {"null": (name,)}
    order = []
    add = lambda fault, word, when=True: order.append((fault, word)) if when and all(a in abi.names(entry) for a in RO._arguments(fault)) else None
    spectral = entry != COUNTS
    add({"nx": -1}, "nx is negative"); add({"ngpt": -1}, "ngpt is negative"); add({"nrays": -1}, "nrays is negative")
    add({"nbnd": -1}, "nbnd is negative")
    add({"ngpt": 1025}, "ngpt must be <= 1024", spectral); add({"ray0": -1}, "ray0 is negative")
    for name in ("tau", "sfc_emis", "lay_src", "sfc_src") + (("band_lims_gpt", "ray_end", "weight0", "rays_per_cell_gpt") if spectral else ()) \
              + ("k_null", "counts", "flux_conv", "n_capped", "n_clamped"):
        add(null(name), name + " is NULL")
    add(null("cld_ssa"), "cld_tau, cld_ssa, cld_g must be all NULL or all given")
    add(null("band_lims_gpt"), "band_lims_gpt is NULL", not spectral); add({"nbnd": 0}, "nbnd must be >= 1 with a cloud triple")
    add({"igpt": 9}, "igpt is outside")
    add({"dx": 0.}, "dx, dy, dz must be > 0")
    if entry == RENDER:
        for value in ("top_negative", "top_nan"):
            add({"top_radiance": value}, "top_radiance must be finite and >= 0")
        add({"rays_per_cell_gpt": "m_negative"}, "rays_per_cell_gpt is negative at g-point 1")
        add({"rays_per_cell_gpt": "m_huge"}, "the ray list exceeds 2^63 - 1")
    for value in (-1., NAN):
        add({"top_radiance": value}, "top_radiance must be finite and >= 0", entry == COUNTS)
    add({"max_events": 0}, "max_events must be >= 1")
    add({"knx": 3}, "knx does not divide nx"); add({"knz": 3}, "knz does not divide nz")
    return order


def test_the_entries_are_the_declared_heating_entries():
    declared = {n[:-4] for n in abi.declared_symbols() if n.endswith("_f64") and n.startswith("rrx_heating3d_")}
    assert declared == set(ENTRIES) and not set(ENTRIES) & set(RO.ENTRIES)
    assert all(len(ORDER(e)) >= 10 for e in ENTRIES), {e: len(ORDER(e)) for e in ENTRIES}


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_of_two_faults_the_one_that_is_checked_first_is_reported(entry, sfx):
    lib = abi.lib()
    order = ORDER(entry)
    for fault, word in order:          # (each fault alone gives its message)
        status, msg = _call(lib, entry, sfx, [fault])
        assert status != 0 and msg.startswith(entry + sfx + ": ") and word in msg, (fault, msg)
    pairs = list(itertools.combinations(order, 2))
    tried = 0
    for (first, word), (second, _) in pairs:
        if RO._arguments(first) & RO._arguments(second):
            continue
        tried += 1
        status, msg = _call(lib, entry, sfx, [second, first])
        assert status != 0 and msg.startswith(entry + sfx + ": ") and word in msg, (first, second, msg)
    assert 4*tried >= 3*len(pairs), (tried, len(pairs))


@pytest.mark.parametrize("sfx", abi.SFXS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_zero_extent_returns_zero_before_any_later_fault(entry, sfx):
    lib = abi.lib()
    later = [f for f, w in ORDER(entry) if "negative" not in w and "nz" not in f]
    assert len(later) >= 6
    for fault in later:
        assert _call(lib, entry, sfx, [fault, {"nz": 0}])[0] == 0, fault
