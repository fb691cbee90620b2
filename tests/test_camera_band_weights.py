"""CPU tests of camera.band_weights, the matrix from the bands of a k-distribution to the channels of a sensor, and of the keywords
of pipeline.render_sw that take it. The expected values are closed forms: a response of one over whole bands passes
all of their energy, whatever Planck's law says inside them."""
import numpy as np
import pytest

from rte_rrtmgp_cpp_amd import camera, pipeline

# four shortwave bands in cm-1, the last one out of spectral order, as a k-distribution may hold them
LIMS = np.array([[12850., 16000.], [16000., 22650.], [22650., 29000.], [2600., 3250.]])
NM = lambda wavenumber: 1.0e7 / wavenumber


def test_a_boxcar_that_covers_bands_exactly_gives_one_and_zero():
    M = camera.band_weights(LIMS, [NM(22650.), NM(12850.)], [1., 1.])
    assert M.shape == (1, 4)
    assert np.allclose(M, [[1., 1., 0., 0.]], rtol=0, atol=1e-12)
    two = camera.band_weights(LIMS, [NM(22650.), NM(12850.)], [[1., 1.], [0.5, 0.5]])
    assert np.allclose(two[1], 0.5*two[0], rtol=0, atol=1e-12)


def test_two_disjoint_boxcars_that_tile_a_band_sum_to_one_there():
    split = NM(14000.)
    lam = [NM(16000.), split, split, NM(12850.)]
    M = camera.band_weights(LIMS, lam, [[1., 1., 0., 0.], [0., 0., 1., 1.]])
    assert np.all(M[:, 0] > 0.2) and abs(M[:, 0].sum() - 1.0) <= 1e-12
    assert not M[:, 1:].any()
    # the share follows Planck's law at the sun's temperature: a cooler source puts more of the band's energy at the long wavelengths
    cool = camera.band_weights(LIMS, lam, [[1., 1., 0., 0.], [0., 0., 1., 1.]], t_sun=3000.0)
    assert cool[1, 0] > M[1, 0]


def test_a_response_outside_all_bands_gives_zeros_and_a_ramp_lies_between():
    assert not camera.band_weights(LIMS, [100., 200.], [1., 1.]).any()
    ramp = camera.band_weights(LIMS, [NM(16000.), NM(12850.)], [0., 1.])
    assert 0.3 < ramp[0, 0] < 0.7 and not ramp[0, 1:].any()
    with pytest.raises(ValueError, match="do not descend"):
        camera.band_weights(LIMS, [700., 400.], [1., 1.])
    with pytest.raises(ValueError, match="response is"):
        camera.band_weights(LIMS, [400., 700.], [1., 1., 1.])


def test_render_sw_refuses_channels_without_allocation_flux():
    with pytest.raises(ValueError, match="channels needs allocation='flux'"):
        pipeline.render_sw(None, None, None, 4, 4, 100., 100., 50., 0.3, None, 4, 1, channels="bands")
    with pytest.raises(ValueError, match="allocation is None or 'flux'"):
        pipeline.render_sw(None, None, None, 4, 4, 100., 100., 50., 0.3, None, 4, 1, allocation="equal")
