"""The arguments of the ray tracers' C entries, gathered once per call of HipKernels: RtScene holds the grid, the
cloud and aerosol triples, the background and the phase table by name, decides the form of the call and hands out the argument
groups in the order include/rrx_hip.h declares them. The checks raise in the order the steps are taken: RtScene() (the camera's
band_lims), set_grid (ncol, the cloud's band_lims), the method's own host arrays, set_medium (the background's shapes, the
background cloud's and the aerosols' band_lims, the profile of a single-launch entry, the phase table)."""
import ctypes

import numpy as np

NO_TRIPLE = (None, None, None)
NO_TABLE = (0, 0, 0.0, 0.0, None, None, None, None)
POINTERS3 = ctypes.c_void_p * 3
# The band_lims rule: an entry is passed band_lims as given when one of the triples it reads is there, NULL otherwise; the camera
# entries keep their counts by band and always take it.
LIMS_READERS = {"k_null": ("cloud", "aer"), "trace": ("cloud", "aer"), "profile": ("bg_cloud", "bg_aer"),
                "loop": ("cloud", "aer", "bg_cloud", "bg_aer")}


def rt_form(grid, spectral, aerosol, background):
    """The form of a call: "grid" (the methods without background= and aerosol=), "spectral", "aer" when aerosol= or
    background.aerosol is given (a triple of None is given too), otherwise "bg"."""
    if grid:
        return "grid"
    if spectral:
        return "spectral"
    given = aerosol is not None or (background is not None and getattr(background, "aerosol", None) is not None)
    return "aer" if given else "bg"


def rt_entry(base, table_given, form):
    """(the entry, its phase-table slot: None for no slot, True filled, False zero-filled). The grid form is base or base_phase;
    base_bg, base_aer and base_spectral always have the slot."""
    if form == "grid":
        return (base + "_phase", True) if table_given else (base, None)
    return base + "_" + form, table_given


class RtScene:
    # what a call without them has: no triples, no background (nbg = 0), the grid form
    cloud = aer = bg_cloud = bg_aer = NO_TRIPLE
    nbg, dz_bg, bg_tau, bg_ssa, bg_profile = 0, None, None, None, None
    form, entry, table = "grid", None, ()

    def __init__(self, be, band_lims, camera=False):
        if camera and band_lims is None:
            raise ValueError("raytracer: the camera's spectral form needs band_lims")
        self.be, self.band_lims = be, band_lims
        self.nbnd = int(band_lims.shape[0]) if band_lims is not None else 0
        self.has = set()          # the triples that are there: cloud, aer, bg_cloud, bg_aer

    def need_lims(self, what, *triples):
        if self.band_lims is None and not self.has.isdisjoint(triples):
            raise ValueError(f"raytracer: {what} needs band_lims")

    def lims(self, kind):
        """band_lims as an entry of this kind is passed it: k_null, profile, trace (single launch), loop, camera"""
        return self.band_lims if kind == "camera" or not self.has.isdisjoint(LIMS_READERS[kind]) else None

    def set_grid(self, tau, nx, ny, dz, kn_grid, top_at_1, cloud, ssa=None, dx=None, dy=None, sfc_albedo=None, mu0=None, azimuth=None,
                 independent_column=False):
        ngpt, nz, ncol = tau.shape
        if ncol != nx*ny:
            raise ValueError(f"raytracer: ncol = {ncol} is not nx ny = {nx}*{ny}")
        if cloud is not None:
            self.cloud = tuple(cloud)
            self.has.add("cloud")
            self.need_lims("a cloud triple", "cloud")
        self.ngpt, self.nz, self.ncol, self.dims = ngpt, nz, ncol, (int(nx), int(ny), nz, ngpt, self.nbnd)
        self.kn = tuple(map(int, kn_grid))
        self.tau, self.ssa, self.flags = tau, ssa, (top_at_1, independent_column)
        self.geometry = (dx, dy, dz, sfc_albedo, mu0, azimuth)
        return self

    def set_aerosol(self, aerosol):
        if aerosol is not None and aerosol[0] is not None:
            self.aer = tuple(aerosol)
            self.has.add("aer")
        self.need_lims("an aerosol triple", "aer", "bg_aer")
        return self

    def set_background(self, background, aerosol="own"):
        """background: None, or an object with dz, tau, ssa, cloud and aerosol. aerosol=: a triple (None: none) in place of its own."""
        if background is None:
            return self
        dz = np.ascontiguousarray(background.dz, dtype=self.be.np_dtype).reshape(-1)
        if tuple(background.tau.shape[1:]) != (dz.size,) or tuple(background.ssa.shape) != tuple(background.tau.shape):
            raise ValueError(f"raytracer: the background's tau, ssa are (ngpt, nbg = {dz.size}), got {tuple(background.tau.shape)}, "
                             f"{tuple(background.ssa.shape)}")
        self.nbg, self.dz_bg, self.bg_tau, self.bg_ssa = dz.size, dz, background.tau, background.ssa
        if background.cloud is not None:
            self.bg_cloud = tuple(background.cloud)
            self.has.add("bg_cloud")
        aerosol = getattr(background, "aerosol", None) if isinstance(aerosol, str) else aerosol
        if aerosol is not None and aerosol[0] is not None:
            self.bg_aer = tuple(aerosol)
            self.has.add("bg_aer")
        return self

    def set_medium(self, kind, base, phase, background=None, aerosol=None, grid=False, spectral=False, igpt=None, bg_profile=None):
        """The background, the aerosols, the form and the phase table of a trace (single launch: bg_profile is made when None, for
        igpt, or for all g-points in the spectral form) or a loop."""
        self.set_background(background)
        if kind == "loop":
            self.need_lims("a background cloud triple", "bg_cloud")
        self.set_aerosol(aerosol)
        self.form = rt_form(grid, spectral, aerosol, background)
        if kind == "trace" and background is not None and bg_profile is None:
            bg_profile = (self.be.rt_bg_profile_all(background, self.band_lims) if spectral else
                          self.be.rt_bg_profile(background, igpt, self.band_lims, aerosol=self.bg_aer if self.form == "aer" else None))
        self.bg_profile = bg_profile
        self.entry, slot = rt_entry(base, phase is not None, self.form)
        self.table = () if slot is None else self._table(base if grid else base + "_bg", phase) if slot else NO_TABLE
        return self

    def _table(self, who, phase):
        """the eight arguments of a tabulated phase function (rrx_rt_phase.h), checked against the grid"""
        if phase.cld_re is None:
            raise ValueError(f"{who}: the phase table has no cell radius (PhaseTable.with_radius)")
        nbnd, nre, nmu = phase.phase.shape
        if nbnd != self.nbnd or tuple(phase.cdf.shape) != (nbnd, nre, nmu) or tuple(phase.mu.shape) != (nmu,):
            raise ValueError(f"{who}: phase, cdf are (nbnd = {self.nbnd}, nre, nmu) and mu (nmu,), got {tuple(phase.phase.shape)}, "
                             f"{tuple(phase.cdf.shape)}, {tuple(phase.mu.shape)}")
        if tuple(phase.cld_re.shape) != (self.nz, self.ncol):
            raise ValueError(f"{who}: cld_re is (nz, ncol) = {(self.nz, self.ncol)}, got {tuple(phase.cld_re.shape)}")
        return (nmu, nre, phase.re0, phase.dre, phase.mu, phase.phase, phase.cdf, phase.cld_re)

    # ---- the argument groups, each in the header's order: dims (nx ny nz ngpt nbnd; igpt follows it where there is one), flags (top_at_1,
    # independent_column; the backward entries take the first), kn, table, and
    def grid(self, kind):
        """tau ... azimuth"""
        return (self.tau, self.ssa, self.lims(kind), *self.cloud, *self.geometry)

    def run(self, seed, max_events, *span):
        """seed (the unsigned 64-bit key), the range of a single launch, max_events"""
        return (int(seed) & 0xFFFFFFFFFFFFFFFF, *span, self.be.RT_MAX_EVENTS if max_events is None else max_events)

    @property
    def bg_tail(self):
        """the background of a single-launch entry"""
        return () if self.form == "grid" else (self.nbg, self.dz_bg, self.bg_profile)

    @property
    def bg_medium(self):
        """the background of a loop, and of the profile entries"""
        return () if self.form == "grid" else (self.nbg, self.dz_bg, self.bg_tau, self.bg_ssa, *self.bg_cloud)

    def aer_tail(self, shape):
        """the aerosol arguments of the aer and spectral forms: "trace" the grid's three pointers, "arrays" two host arrays of three
        pointers (NULL for no triple), "pointers" the grid's and the background's six"""
        if self.form not in ("aer", "spectral"):
            return ()
        if shape == "trace":
            return self.aer
        if shape == "pointers":
            return (*self.aer, *self.bg_aer)
        return tuple(None if t is None else POINTERS3(t.data_ptr(), w.data_ptr(), g.data_ptr()) for t, w, g in (self.aer, self.bg_aer))
