"""NumPy reference of the RRTMGP gas optics, written from the formulas (Pincus, Mlawer & Delamere 2019, and the interpolation
conventions of the RRTMGP kernels: truncating indices, clamped to the tables, weights that extrapolate beyond them) -- not from the
oracle's loop nests and not from the HIP kernels. Vectorised over the cells, plain loops over g-points and contributors.

Arrays are in the package's tensor convention: cells (nlay, ncol), g-point arrays (ngpt, nlay, ncol), band arrays (nbnd, nlay, ncol),
col_gas (ngas+1, nlay, ncol) with the dry-air column in row 0, the interpolation state as rrx_interpolation lays it out. `kd` is a
synthetic.KDist. Every function takes `dtype`, the precision the arithmetic runs in: np.float64, or np.longdouble for the rounding
floor of the fp64 arithmetic. `work` is the precision whose constants the thresholds use (tiny, epsilon: those of the kernels
under test), np.float64 unless a float32 build is checked."""
import numpy as np


def _tiny(work):
    return float(np.finfo(work).tiny)


def _trunc_clip(x, lo, hi):
    """int(x) of C, then clamped to lo..hi."""
    return np.clip(np.trunc(x), lo, hi).astype(np.int64)


def interpolation(kd, play, tlay, col_gas, dtype=np.float64, work=np.float64):
    """Table positions and weights of every cell: jtemp, jpress (1-based lower nodes), tropo (lower regime), and per flavor and
    temperature node jeta, col_mix, fminor[eta], fmajor[pressure][eta]."""
    F = np.dtype(dtype).type
    p, t, cg = np.asarray(play, dtype), np.asarray(tlay, dtype), np.asarray(col_gas, dtype)
    temp_ref, vmr_ref, prl = np.asarray(kd.temp_ref, dtype), np.asarray(kd.vmr_ref, dtype), np.asarray(kd.press_ref_log, dtype)
    dT, dP, Tmin = F(kd.temp_ref_delta), F(kd.press_ref_log_delta), F(kd.temp_ref_min)
    nlay, ncol = p.shape
    jtemp = _trunc_clip((t - (Tmin - dT)) / dT, 1, kd.ntemp - 1)
    ftemp = (t - temp_ref[jtemp - 1]) / dT
    lnp = np.log(p)
    locpress = F(1) + (lnp - prl[0]) / dP
    jpress = _trunc_clip(locpress, 1, kd.npres - 1)
    fpress = locpress - jpress.astype(dtype)
    tropo = lnp > F(kd.press_ref_trop_log)
    itropo = np.where(tropo, 0, 1)
    jeta = np.zeros((kd.nflav, nlay, ncol, 2), np.int64)
    col_mix = np.zeros((kd.nflav, nlay, ncol, 2), dtype)
    fminor = np.zeros((kd.nflav, nlay, ncol, 2, 2), dtype)
    fmajor = np.zeros((kd.nflav, nlay, ncol, 2, 2, 2), dtype)
    for iflav in range(kd.nflav):
        gas1, gas2 = (int(x) for x in kd.flavor[iflav])
        for itemp in range(2):
            ratio_eta_half = vmr_ref[jtemp + itemp - 1, gas1, itropo] / vmr_ref[jtemp + itemp - 1, gas2, itropo]
            cmix = cg[gas1] + ratio_eta_half * cg[gas2]
            with np.errstate(divide="ignore", invalid="ignore"):
                eta = np.where(cmix > F(2 * _tiny(work)), cg[gas1] / cmix, F(0.5))
            loceta = eta * F(kd.neta - 1)
            jeta[iflav, :, :, itemp] = np.minimum(np.trunc(loceta).astype(np.int64) + 1, kd.neta - 1)
            feta = np.fmod(loceta, F(1))
            ftemp_term = ftemp if itemp == 1 else F(1) - ftemp
            col_mix[iflav, :, :, itemp] = cmix
            fminor[iflav, :, :, itemp, 0] = (F(1) - feta) * ftemp_term
            fminor[iflav, :, :, itemp, 1] = feta * ftemp_term
            fmajor[iflav, :, :, itemp, 0, :] = (F(1) - fpress)[..., None] * fminor[iflav, :, :, itemp, :]
            fmajor[iflav, :, :, itemp, 1, :] = fpress[..., None] * fminor[iflav, :, :, itemp, :]
    return dict(jtemp=jtemp, jpress=jpress, tropo=tropo, jeta=jeta, col_mix=col_mix, fminor=fminor, fmajor=fmajor)


def positions(kd, play, tlay, col_gas, dtype=np.longdouble, work=np.float64):
    """Continuous table coordinates of every cell, in units of a table spacing: temperature, pressure, eta per (flavor, temperature
    node), and ln p - press_ref_trop_log. What a builder of test atmospheres checks its distance to the nodes with."""
    F = np.dtype(dtype).type
    p, t, cg = np.asarray(play, dtype), np.asarray(tlay, dtype), np.asarray(col_gas, dtype)
    it = interpolation(kd, play, tlay, col_gas, dtype, work)
    xt = (t - (F(kd.temp_ref_min) - F(kd.temp_ref_delta))) / F(kd.temp_ref_delta)
    xp = F(1) + (np.log(p) - np.asarray(kd.press_ref_log, dtype)[0]) / F(kd.press_ref_log_delta)
    xe = np.zeros(it["col_mix"].shape, dtype)
    for iflav in range(kd.nflav):
        gas1 = int(kd.flavor[iflav, 0])
        for itemp in range(2):
            cmix = it["col_mix"][iflav, :, :, itemp]
            with np.errstate(divide="ignore", invalid="ignore"):
                xe[iflav, :, :, itemp] = np.where(cmix > F(2 * _tiny(work)), cg[gas1] / cmix, F(0.5)) * F(kd.neta - 1)
    return dict(temp=xt, press=xp, eta=xe, trop=np.log(p) - F(kd.press_ref_trop_log))


def _cell_flavor(kd, it, igpt):
    """0-based flavor of g-point igpt in every cell (lower or upper regime)."""
    return np.where(it["tropo"], int(kd.gpoint_flavor[igpt, 0]) - 1, int(kd.gpoint_flavor[igpt, 1]) - 1)


def _grid(shape):
    return np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")


def _major_interp(table_g, it, iflav, weights, dtype):
    """Sum over the 2 x 2 x 2 corners (temperature, pressure, eta) of one g-point's table (npres+1, neta, ntemp); `weights`
    multiplies each temperature node's sum (col_mix for optical depths, None for Planck fractions)."""
    L, C = _grid(iflav.shape)
    jt, itropo = it["jtemp"], np.where(it["tropo"], 0, 1)
    jp = it["jpress"] + itropo                         # the upper regime's tables start one node later
    out = np.zeros(iflav.shape, dtype)
    for itemp in range(2):
        je = it["jeta"][iflav, L, C, itemp]
        s = np.zeros(iflav.shape, dtype)
        for ip in range(2):
            for ie in range(2):
                s = s + np.asarray(it["fmajor"], dtype)[iflav, L, C, itemp, ip, ie] * table_g[jp - 1 + ip, je - 1 + ie, jt - 1 + itemp]
        out = out + (s if weights is None else np.asarray(weights, dtype)[iflav, L, C, itemp] * s)
    return out


def _minor_interp(table_row, it, iflav, dtype):
    """Sum over the 2 x 2 corners (temperature, eta) of one row (neta, ntemp) of a minor-contributor or Rayleigh table."""
    L, C = _grid(iflav.shape)
    jt = it["jtemp"]
    out = np.zeros(iflav.shape, dtype)
    for itemp in range(2):
        je = it["jeta"][iflav, L, C, itemp]
        for ie in range(2):
            out = out + np.asarray(it["fminor"], dtype)[iflav, L, C, itemp, ie] * table_row[je - 1 + ie, jt - 1 + itemp]
    return out


def tau_major(kd, it, dtype=np.float64):
    kmajor = np.asarray(kd.kmajor, dtype)
    nlay, ncol = it["jtemp"].shape
    tau = np.zeros((kd.ngpt, nlay, ncol), dtype)
    for igpt in range(kd.ngpt):
        tau[igpt] = _major_interp(kmajor[igpt], it, _cell_flavor(kd, it, igpt), it["col_mix"], dtype)
    return tau


def tau_minor(kd, it, play, tlay, col_gas, dtype=np.float64):
    """Minor contributors of both regimes. A contributor's amount is its gas column; where it scales with density, times
    0.01 p / T and, with a scaling gas, times that gas's dry mixing ratio (or its complement). The interpolation state of the whole
    interval is that of the flavor of the interval's FIRST g-point."""
    F = np.dtype(dtype).type
    p, t, cg = np.asarray(play, dtype), np.asarray(tlay, dtype), np.asarray(col_gas, dtype)
    nlay, ncol = p.shape
    tau = np.zeros((kd.ngpt, nlay, ncol), dtype)
    for r, sfx in enumerate(("lower", "upper")):
        kminor = np.asarray(getattr(kd, "kminor_" + sfx), dtype)
        lims = np.asarray(getattr(kd, "minor_limits_gpt_" + sfx)).reshape(-1, 2)
        in_regime = it["tropo"] if r == 0 else ~it["tropo"]
        for i in range(lims.shape[0]):
            amount = cg[int(getattr(kd, "idx_minor_" + sfx)[i])]
            if getattr(kd, "minor_scales_with_density_" + sfx)[i]:
                amount = amount * (F(0.01) * p / t)
                iscal = int(getattr(kd, "idx_minor_scaling_" + sfx)[i])
                if iscal > 0:
                    vmr_fact = F(1) / cg[0]
                    dry_fact = F(1) / (F(1) + cg[kd.idx_h2o] * vmr_fact)
                    x = cg[iscal] * vmr_fact * dry_fact
                    amount = amount * ((F(1) - x) if getattr(kd, "scale_by_complement_" + sfx)[i] else x)
            g0, g1 = int(lims[i, 0]) - 1, int(lims[i, 1])
            iflav = np.full((nlay, ncol), int(kd.gpoint_flavor[g0, r]) - 1)
            row0 = int(getattr(kd, "kminor_start_" + sfx)[i]) - 1
            for ig in range(g1 - g0):
                k = _minor_interp(kminor[row0 + ig], it, iflav, dtype)
                tau[g0 + ig] = tau[g0 + ig] + np.where(in_regime, k * amount, F(0))
    return tau


def tau_absorption(kd, it, play, tlay, col_gas, dtype=np.float64):
    return tau_major(kd, it, dtype) + tau_minor(kd, it, play, tlay, col_gas, dtype)


def tau_rayleigh(kd, it, col_dry, col_gas, dtype=np.float64):
    krayl, cg = np.asarray(kd.krayl, dtype), np.asarray(col_gas, dtype)
    wet = cg[kd.idx_h2o] + np.asarray(col_dry, dtype)
    nlay, ncol = it["jtemp"].shape
    tau = np.zeros((kd.ngpt, nlay, ncol), dtype)
    for igpt in range(kd.ngpt):
        iflav = _cell_flavor(kd, it, igpt)
        k = np.where(it["tropo"], _minor_interp(krayl[0, igpt], it, iflav, dtype), _minor_interp(krayl[1, igpt], it, iflav, dtype))
        tau[igpt] = k * wet
    return tau


def combine(tau_abs, tau_ray, dtype=np.float64, work=np.float64):
    """tau, ssa, g of absorption + Rayleigh scattering; ssa = 0 below the CPU threshold 2 epsilon, g = 0."""
    F = np.dtype(dtype).type
    ta, tr = np.asarray(tau_abs, dtype), np.asarray(tau_ray, dtype)
    tau = ta + tr
    with np.errstate(divide="ignore", invalid="ignore"):
        ssa = np.where(tau > F(2 * float(np.finfo(work).eps)), tr / tau, F(0))
    return tau, ssa, np.zeros_like(tau)


def band_planck(kd, temp, dtype=np.float64):
    """Band-integrated Planck function (nbnd, ...) at the temperatures `temp`: linear in the table totplnk, whose first node is
    temp_ref_min; index = int(x) + 1 clamped to 1..n-1, fraction = x - int(x) whatever the clamp did."""
    F = np.dtype(dtype).type
    totplnk = np.asarray(kd.totplnk, dtype)
    x = (np.asarray(temp, dtype) - F(kd.temp_ref_min)) / F(kd.totplnk_delta)
    whole = np.trunc(x)
    frac = x - whole
    idx = np.clip(whole.astype(np.int64) + 1, 1, kd.nPlanckTemp - 1)
    return totplnk[:, idx - 1] + frac[None] * (totplnk[:, idx] - totplnk[:, idx - 1])


def planck_source(kd, it, tlay, tlev, tsfc, sfc_lay, dtype=np.float64):
    """Planck fractions per g-point, band Planck functions at layers and levels, and the sources made of them: lay_src, lev_src
    (the fraction at an interior level is the geometric mean of its two layers'), sfc_src at the surface layer `sfc_lay` (1-based),
    sfc_src_jac its change for +1 K."""
    F = np.dtype(dtype).type
    pf_tab = np.asarray(kd.planck_frac, dtype)
    nlay, ncol = it["jtemp"].shape
    pfrac = np.zeros((kd.ngpt, nlay, ncol), dtype)
    for igpt in range(kd.ngpt):
        pfrac[igpt] = _major_interp(pf_tab[igpt], it, _cell_flavor(kd, it, igpt), None, dtype)
    blay, blev = band_planck(kd, tlay, dtype), band_planck(kd, tlev, dtype)
    ts = np.asarray(tsfc, dtype)
    bsfc, bsfc1 = band_planck(kd, ts, dtype), band_planck(kd, ts + F(1), dtype)
    bnd = np.asarray(kd.gpoint_bands, np.int64) - 1
    lay_src = pfrac * blay[bnd]
    lev_frac = np.zeros((kd.ngpt, nlay + 1, ncol), dtype)
    lev_frac[:, 0], lev_frac[:, nlay] = pfrac[:, 0], pfrac[:, nlay - 1]
    lev_frac[:, 1:nlay] = np.sqrt(pfrac[:, 1:] * pfrac[:, :-1])
    lev_src = lev_frac * blev[bnd]
    sfc_src = pfrac[:, sfc_lay - 1] * bsfc[bnd]
    sfc_src_jac = pfrac[:, sfc_lay - 1] * (bsfc1[bnd] - bsfc[bnd])
    return dict(lay_src=lay_src, lev_src=lev_src, sfc_src=sfc_src, sfc_src_jac=sfc_src_jac, pfrac=pfrac, blay=blay, blev=blev)


def add_by_band_1scalar(kd, tau, cld_tau, dtype=np.float64):
    """tau of every g-point plus the optical depth of its band (absorption only: the LW all-sky forms)."""
    bnd = np.asarray(kd.gpoint_bands, np.int64) - 1
    return np.asarray(tau, dtype) + np.asarray(cld_tau, dtype)[bnd]


def add_by_band_2stream(kd, tau, ssa, g, cld_tau, cld_ssa, cld_g, dtype=np.float64, work=np.float64):
    """Two-stream properties of every g-point combined with those of its band: optical depths add, ssa is weighted by optical
    depth, g by scattering optical depth; denominators are kept above 3 tiny."""
    F = np.dtype(dtype).type
    bnd = np.asarray(kd.gpoint_bands, np.int64) - 1
    t1, w1, g1 = (np.asarray(x, dtype) for x in (tau, ssa, g))
    t2, w2, g2 = (np.asarray(x, dtype)[bnd] for x in (cld_tau, cld_ssa, cld_g))
    eps = F(3 * _tiny(work))
    tau12 = t1 + t2
    scat12 = t1 * w1 + t2 * w2
    return tau12, scat12 / np.maximum(eps, tau12), (t1 * w1 * g1 + t2 * w2 * g2) / np.maximum(scat12, eps)
