"""CPU test of pipeline.ResidentSolver.resolve_options, the one place that holds the solver's option rules: over the whole matrix of
options it accepts exactly the combinations that the rules below accept, names the LW form each of them takes, and names both options
of a refused pair. The rules are stated here on their own, form by form, not read from the solver's table; no backend is involved."""
import itertools
import types

import numpy as np
import pytest

from rte_rrtmgp_cpp_amd import pipeline

NLAY, NCOL = 5, 8
ATM = types.SimpleNamespace(nlay=NLAY, ncol=NCOL)
KD_FIT = types.SimpleNamespace(optimal_angle_fit=np.ones((2, 4)))
KD_BARE = types.SimpleNamespace()
LUTS = ("lw cloud table", "sw cloud table")

resolve = pipeline.ResidentSolver.resolve_options


def expected_form(do_broadband, byband, jacobian, optimal_angles, lw_scattering, lw_rescaling, n_gauss_angles, mcica, sunlit):
    """The LW form of an option set, None where the set is refused."""
    several = n_gauss_angles > 1
    if mcica and (lw_scattering or lw_rescaling or sunlit):
        return None
    if not do_broadband:            # per g-point: any number of angles, nothing else
        return None if (byband or jacobian or optimal_angles or lw_scattering or lw_rescaling) else "per_gpoint"
    if lw_rescaling:                # alone
        return None if (lw_scattering or byband or jacobian or several or optimal_angles) else "rescaled"
    if lw_scattering:               # alone
        return None if (byband or jacobian or several or optimal_angles) else "two_stream"
    if byband:                      # no Jacobian, one fixed angle
        return None if (jacobian or several or optimal_angles) else "byband"
    if optimal_angles:              # one angle; Jacobian admitted
        return None if several else "optimal"
    return "angles" if several else "fractions"         # Jacobian admitted by both


def options(do_broadband, byband, jacobian, optimal_angles, lw_scattering, lw_rescaling, n_gauss_angles, mcica, sunlit):
    kw = dict(do_broadband=do_broadband, byband=byband, jacobian=jacobian, optimal_angles=optimal_angles, lw_scattering=lw_scattering,
              lw_rescaling=lw_rescaling, n_gauss_angles=n_gauss_angles, sunlit=sunlit)
    if mcica:
        kw.update(cloud_fraction=np.full((NLAY, NCOL), 0.5), cloud_luts=LUTS)
    return kw


MATRIX = list(itertools.product((False, True), (False, True), (False, True), (False, True), (False, True), (False, True), (1, 3),
                                (False, True), (False, True)))


def test_the_whole_matrix_is_accepted_or_refused_as_the_rules_say():
    assert len(MATRIX) == 512
    forms = set()
    for cell in MATRIX:
        want = expected_form(*cell)
        if want is None:
            with pytest.raises(ValueError, match="ResidentSolver: .* is not supported"):
                resolve(ATM, KD_FIT, **options(*cell))
        else:
            assert resolve(ATM, KD_FIT, **options(*cell)) == want, cell
            forms.add(want)
    assert forms == {"per_gpoint", "fractions", "angles", "optimal", "byband", "two_stream", "rescaled"}
    assert forms == set(pipeline._LW_FORMS)


# every refused pair on its own: the option whose form refuses the other comes first in the message
PAIRS = [(dict(lw_rescaling=True), "lw_rescaling", other, word) for other, word in (
             (dict(lw_scattering=True), "lw_scattering"), (dict(byband=True), "byband"), (dict(jacobian=True), "jacobian"),
             (dict(n_gauss_angles=3), "n_gauss_angles"), (dict(optimal_angles=True), "optimal_angles"))]
PAIRS += [(dict(lw_scattering=True), "lw_scattering", other, word) for other, word in (
              (dict(byband=True), "byband"), (dict(jacobian=True), "jacobian"), (dict(n_gauss_angles=3), "n_gauss_angles"),
              (dict(optimal_angles=True), "optimal_angles"))]
PAIRS += [(dict(optimal_angles=True), "optimal_angles", dict(n_gauss_angles=3), "n_gauss_angles"),
          (dict(optimal_angles=True), "optimal_angles", dict(byband=True), "byband"),
          (dict(byband=True), "byband", dict(n_gauss_angles=3), "n_gauss_angles"),
          (dict(byband=True), "byband", dict(jacobian=True), "jacobian")]
MCICA = dict(cloud_fraction=np.full((NLAY, NCOL), 0.5), cloud_luts=LUTS)
PAIRS += [(MCICA, "cloud_fraction", other, word) for other, word in (
              (dict(lw_scattering=True), "lw_scattering"), (dict(lw_rescaling=True), "lw_rescaling"), (dict(sunlit=True), "sunlit"))]


@pytest.mark.parametrize("first,first_word,other,other_word", PAIRS, ids=[f"{p[1]}-{p[3]}" for p in PAIRS])
def test_a_refused_pair_is_named_in_the_message(first, first_word, other, other_word):
    with pytest.raises(ValueError, match=f"ResidentSolver: {first_word}.* with {other_word}.* is not supported"):
        resolve(ATM, KD_FIT, do_broadband=True, **first, **other)
    resolve(ATM, KD_FIT, do_broadband=True, **first)        # (each half alone is served)
    resolve(ATM, KD_FIT, do_broadband=True, **other)


@pytest.mark.parametrize("kw,word", [(dict(byband=True), "byband"), (dict(jacobian=True), "jacobian"), (dict(optimal_angles=True), "optimal_angles"),
                                     (dict(lw_scattering=True), "lw_scattering"), (dict(lw_rescaling=True), "lw_rescaling")])
def test_every_form_but_the_per_gpoint_one_needs_broadband(kw, word):
    with pytest.raises(ValueError, match=f"ResidentSolver: do_broadband=False with {word}=True is not supported"):
        resolve(ATM, KD_FIT, do_broadband=False, **kw)
    for n in (1, 2, 3, 4):
        assert resolve(ATM, KD_FIT, do_broadband=False, n_gauss_angles=n) == "per_gpoint"


def test_angle_counts_and_the_optimal_angle_fit():
    for n in (0, 5):
        for bb in (False, True):
            with pytest.raises(ValueError, match="n_gauss_angles"):
                resolve(ATM, KD_FIT, do_broadband=bb, n_gauss_angles=n)
    for kd in (KD_BARE, None, types.SimpleNamespace(optimal_angle_fit=None)):
        with pytest.raises(ValueError, match="optimal_angle_fit"):
            resolve(ATM, kd, do_broadband=True, optimal_angles=True)
        assert resolve(ATM, kd, do_broadband=True) == "fractions"
    assert resolve(ATM, KD_FIT, do_broadband=True, optimal_angles=True, jacobian=True) == "optimal"


def test_cloud_fraction_needs_cloud_luts_and_a_consistent_overlap():
    frac = np.full((NLAY, NCOL), 0.5)
    alpha = np.full((NLAY-1, NCOL), 0.7)
    assert resolve(ATM, KD_FIT, do_broadband=True, cloud_fraction=frac, cloud_luts=LUTS, cloud_overlap="exp_ran", overlap_param=alpha) == "fractions"
    with pytest.raises(ValueError, match="cloud_luts"):
        resolve(ATM, KD_FIT, do_broadband=True, cloud_fraction=frac)
    with pytest.raises(ValueError, match="overlap_param"):
        resolve(ATM, KD_FIT, do_broadband=True, cloud_fraction=frac, cloud_luts=LUTS, cloud_overlap="exp_ran")
    with pytest.raises(ValueError, match="overlap_param"):
        resolve(ATM, KD_FIT, do_broadband=True, cloud_fraction=frac, cloud_luts=LUTS, overlap_param=alpha)
    with pytest.raises(ValueError, match="overlap_param"):
        resolve(ATM, KD_FIT, do_broadband=True, overlap_param=alpha)
    with pytest.raises(ValueError, match="cloud_overlap"):
        resolve(ATM, KD_FIT, do_broadband=True, cloud_fraction=frac, cloud_luts=LUTS, cloud_overlap="random")
    with pytest.raises(ValueError, match="cloud_fraction .* is not"):
        resolve(ATM, KD_FIT, do_broadband=True, cloud_fraction=frac[:-1], cloud_luts=LUTS)
    with pytest.raises(ValueError, match="overlap_param .* is not"):
        resolve(ATM, KD_FIT, do_broadband=True, cloud_fraction=frac, cloud_luts=LUTS, cloud_overlap="exp_ran", overlap_param=alpha[:, :-1])


def test_the_solver_stores_the_form_it_resolved_before_it_touches_a_backend():
    """ResidentSolver(None, ...) gets past the rules and fails at the first use of the backend; a refused set never gets there."""
    with pytest.raises(AttributeError):
        pipeline.ResidentSolver(None, KD_FIT, None, ATM, do_broadband=True, sort_columns="0", byband=True)
    with pytest.raises(ValueError, match="byband.*jacobian"):
        pipeline.ResidentSolver(None, KD_FIT, None, ATM, do_broadband=True, sort_columns="0", byband=True, jacobian=True)
