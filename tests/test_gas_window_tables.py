"""The index tables of the windowed gas optics (gas_window_tables_kernel): the packed per-(regime, chunk) records the windowed kernel
reads by scalar loads, the per-g-point bands and key species, and the counts of unusable chunks -- read back from the device
(rrx_gas_window_tables_read) and compared with a NumPy restatement written here; one windowed launch per spectral shape against
the oracle; and the rebuild of the tables when a k-distribution changes in place."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cases
from rte_rrtmgp_cpp_amd import synthetic, pipeline

pytestmark = pytest.mark.gpu

GCH, NCW, NXW = 16, 6, 12                   # g-points per chunk at most; contributor boxes of a chunk; contributors a chunk may list
TOL = 1e-12                                 # the windowed kernel against the oracle: FMA contraction and one Newton reciprocal apart

# (ngpt, nbnd, columns, layers): 16-g-point bands, the 14-band shortwave shape, 8-g-point bands (band-aligned chunks of 8);
# 300 columns = one full and one partial 256-column block, 130 columns < 192 = workgroups of 64 columns x 4 layers (geometry 0:
# 140 layers there, so that four neighbouring layers fit the pressure extent of a box)
SHAPES = [(256, 16, 300, 24), (224, 14, 130, 140), (128, 16, 520, 20)]
IDS = ["256-16", "224-14", "128-16"]


def read_tables(be):
    lay = (ctypes.c_int * 16)()
    assert be.lib.cdll.rrx_gas_window_tables_read(None, 0, lay) == 0
    buf = np.zeros(lay[0], dtype=np.int32)
    assert be.lib.cdll.rrx_gas_window_tables_read(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), buf.size, lay) == 0
    names = ("ints", "ngpt", "nmax", "ncmax", "cinfo", "lists", "mmeta", "cuni", "order", "gx", "bad", "rec", "LIT", "MM", "REC", "RH")
    return buf, dict(zip(names, list(lay)))


def restate(kd, ncmax, nlist, with_bands, with_lims):
    """What the tables must hold, from the k-distribution alone (0-based g-points, half-open intervals)."""
    ngpt = kd.ngpt
    gflav = kd.gpoint_flavor.T.astype(np.int64) - 1                                   # [regime][g-point]
    lims = [np.asarray(kd.minor_limits_gpt_lower, dtype=np.int64).reshape(-1, 2), np.asarray(kd.minor_limits_gpt_upper, dtype=np.int64).reshape(-1, 2)]
    meta = []
    for r, sfx in enumerate(("lower", "upper")):
        meta.append(dict(lo=lims[r][:, 0] - 1, hi=lims[r][:, 1], gas=getattr(kd, "idx_minor_" + sfx), swd=getattr(kd, "minor_scales_with_density_" + sfx),
                         scal=getattr(kd, "idx_minor_scaling_" + sfx), sbc=getattr(kd, "scale_by_complement_" + sfx), start=getattr(kd, "kminor_start_" + sfx)))
    # a chunk starts where a flavor changes, where a contributor's interval starts or has just ended, and every GCH g-points between
    cuts = {g for g in range(1, ngpt) if (gflav[:, g] != gflav[:, g-1]).any()}
    for m in meta:
        cuts |= {int(x) for x in np.concatenate([m["lo"], m["hi"]]) if 0 < x < ngpt}
    starts, s = [], 0
    for p in sorted(cuts) + [ngpt]:
        while s < p:
            starts.append(s); s = min(s + GCH, p)
    if len(starts) > ncmax:
        starts = list(range(0, ngpt, GCH))
    starts.append(ngpt)
    nchunk = len(starts) - 1
    band = kd.gpoint_bands.astype(np.int64) - 1 if with_bands else np.full(ngpt, -1)
    bl = kd.band_lims_gpt.astype(np.int64)
    cband = np.array([int(np.nonzero(g + 1 <= bl[:, 1])[0][0]) for g in range(ngpt)]) if with_lims else np.full(ngpt, -1)
    out = dict(nchunk=nchunk, regular=int(all(starts[c] == c*GCH for c in range(nchunk))), starts=starts, band=band, cband=cband, recs={}, order={}, bad={},
               species=[kd.flavor[gflav[r]] for r in range(2)])
    for r in range(2):
        m = meta[r]
        fl_of = [int(gflav[r, starts[c]]) for c in range(nchunk)]
        order = [c for f in dict.fromkeys(fl_of) for c in range(nchunk) if fl_of[c] == f]          # flavor by flavor, stable
        bad = [0]
        for c in range(nchunk):
            c0, c1 = starts[c], starts[c+1]
            items = [i for i in range(len(m["lo"])) if m["lo"][i] < c1 and m["hi"][i] > c0]          # ascending = the summation order
            ok = bool((gflav[r, c0:c1] == fl_of[c]).all()) and len(items) <= nlist and all(gflav[r, m["lo"][i]] == fl_of[c] for i in items[:nlist])
            head = [c0, c1, fl_of[c], len(items), int(kd.flavor[fl_of[c], 0]), int(kd.flavor[fl_of[c], 1]), int(band[c0]), int(band[c1-1]),
                    int(cband[c0]), int(with_lims and c1 <= bl[cband[c0], 1]), int(ok), order[c]]
            cont = [[int(m["lo"][i]), int(m["hi"][i]), int(m["start"][i]) - 1 - int(m["lo"][i]), int(m["gas"][i]), int(bool(m["swd"][i])),
                     int(m["scal"][i]), int(bool(m["sbc"][i])), 0] for i in items[:nlist]]
            out["recs"][(r, c)] = (head, cont, items)
            bad.append(bad[-1] + (0 if ok else 1))
        out["order"][r], out["bad"][r] = order, bad
    return out


def check_tables(buf, L, want, nlist):
    ngpt, ncmax, REC, RH = L["ngpt"], L["ncmax"], L["REC"], L["RH"]
    assert L["rec"] % 4 == 0 and REC % 4 == 0 and RH % 4 == 0, "records are read as 16- and 32-byte words"
    assert L["rec"] + 2*ncmax*REC == L["ints"] - 8
    nchunk = want["nchunk"]
    assert buf[L["cinfo"]] == nchunk and buf[L["cinfo"] + 1] == want["regular"]
    assert list(buf[L["cinfo"] + 2: L["cinfo"] + 3 + nchunk]) == want["starts"]                    # chunk limits
    gx = buf[L["gx"]: L["gx"] + 6*ngpt].reshape(ngpt, 6)
    assert np.array_equal(gx[:, 0], want["band"]) and np.array_equal(gx[:, 1], want["cband"])     # bands
    for r in range(2):
        assert np.array_equal(gx[:, 2+2*r: 4+2*r], want["species"][r]), f"key species, regime {r}"
        bad = buf[L["bad"] + r*(ncmax + 1): L["bad"] + (r + 1)*(ncmax + 1)]
        assert list(bad[:nchunk + 1]) == want["bad"][r] and (bad[nchunk:] == bad[nchunk]).all()
        assert list(buf[L["order"] + r*ncmax: L["order"] + r*ncmax + nchunk]) == want["order"][r]
        for c in range(ncmax):
            rec = buf[L["rec"] + (r*ncmax + c)*REC: L["rec"] + (r*ncmax + c + 1)*REC]
            if c >= nchunk:
                assert not rec.any(), f"record ({r}, {c}) behind the last chunk is not empty"
                continue
            head, cont, items = want["recs"][(r, c)]
            assert list(rec[:RH]) == head, f"record ({r}, {c}) header {list(rec[:RH])} != {head}"
            assert rec[RH: RH + 8*len(cont)].reshape(-1, 8).tolist() == cont, f"record ({r}, {c}) contributors"
            assert not rec[RH + 8*len(cont):].any()
            lst = buf[L["lists"] + (r*ncmax + c)*L["LIT"]: L["lists"] + (r*ncmax + c + 1)*L["LIT"]]
            assert lst[0] == len(items) and list(lst[1: 1 + min(len(items), nlist)]) == items[:nlist]   # contributor lists


def run_windowed(be, kind, kd, atm):
    """One solve with the census of its windowed launches: (outputs, handed back, workgroups)."""
    os.environ["RRX_GW_STATS"] = "1"
    be.lib.cdll.rrx_gas_window_stats(None, None, 1)
    try:
        r = (pipeline.solve_lw if kind == "lw" else pipeline.solve_sw)(be, kd, atm, keep=True, do_broadband=True)
    finally:
        os.environ.pop("RRX_GW_STATS", None)
    handed, total = ctypes.c_longlong(0), ctypes.c_longlong(0)
    be.lib.cdll.rrx_gas_window_stats(ctypes.byref(handed), ctypes.byref(total), 1)
    return r, handed.value, total.value


@pytest.mark.parametrize("kind", ["lw", "sw"])
@pytest.mark.parametrize("ngpt,nbnd,ncol,nlay", SHAPES, ids=IDS)
def test_records_match_numpy_and_launch_matches_oracle(kind, ngpt, nbnd, ncol, nlay, hip_f64, oracle_f64):
    kd0 = synthetic.make_kdist(kind, ngpt=ngpt, nbnd=nbnd)
    atm0 = synthetic.make_atmosphere(ncol, nlay, nbnd_lw=nbnd, nbnd_sw=nbnd, seed=29)
    h, handed, total = run_windowed(hip_f64, kind, hip_f64.upload_kdist(kd0), pipeline.upload_atmosphere(hip_f64, atm0))
    buf, L = read_tables(hip_f64)
    # the broadband LW chain launches the fractions form (bands ride along, up to NXW contributors listed), the SW form lists NCW
    nlist = NXW if kind == "lw" else NCW
    assert (L["ngpt"], L["ncmax"]) == (ngpt, (ngpt + GCH - 1)//GCH + nbnd)
    want = restate(kd0, L["ncmax"], nlist, with_bands=(kind == "lw"), with_lims=False)
    assert want["nchunk"] == nbnd and want["regular"] == int(ngpt // nbnd == GCH)
    check_tables(buf, L, want, nlist)
    # the windowed kernel ran (geometry 0 hands back at most the workgroups around the tropopause) ...
    assert total > 0 and handed <= (0 if ncol >= 192 else total // 3), (handed, total)
    # ... and agrees with the oracle
    o = pipeline.solve_lw(oracle_f64, oracle_f64.upload_kdist(kd0), pipeline.upload_atmosphere(oracle_f64, atm0), keep=True, do_broadband=True) \
        if kind == "lw" else pipeline.solve_sw(oracle_f64, oracle_f64.upload_kdist(kd0), pipeline.upload_atmosphere(oracle_f64, atm0), keep=True, do_broadband=True)
    errs = {k: cases.rel_err(hip_f64.to_numpy(h[k]), oracle_f64.to_numpy(o[k])) for k in (("tau", "lay_src", "lev_src", "sfc_src") if kind == "lw" else ("tau", "ssa"))}
    print(f"windowed {kind} {ngpt}/{nbnd}, {ncol} columns: handed back {handed} of {total};", {k: f"{e:.2e}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= TOL, f"{kind} {k}: {e:.3e}"


def test_allsky_records_carry_the_by_band_bands(hip_f64, oracle_f64):
    """All-sky launches add the by-band cloud properties where the gas optics is stored: their records name the band of each chunk."""
    nbnd = 16
    kd0 = synthetic.make_kdist("sw", ngpt=128, nbnd=nbnd)
    atm0 = synthetic.make_atmosphere(260, 20, nbnd_lw=nbnd, nbnd_sw=nbnd, seed=31, clouds=True)
    lut = synthetic.make_cloud_lut(nbnd, "sw")
    res = []
    for be in (hip_f64, oracle_f64):
        r = pipeline.solve_sw(be, be.upload_kdist(kd0), pipeline.upload_atmosphere(be, atm0), cloud_lut=be.upload_lut(lut), keep=True, do_broadband=True)
        res.append({k: be.to_numpy(r[k]) for k in ("tau", "ssa", "g")})
        if be is hip_f64:
            buf, L = read_tables(hip_f64)
            check_tables(buf, L, restate(kd0, L["ncmax"], NCW, with_bands=False, with_lims=True), NCW)
    for k in ("tau", "ssa", "g"):
        assert cases.rel_err(res[0][k], res[1][k]) <= 1e-9, k      # (the by-band combination: the bound of the all-sky parity tests)


def test_changed_in_place_is_rebuilt(hip_f64):
    """Same device addresses, other contents: flavors, contributor intervals, and -- which only the records hold -- band numbers
    and key species. The tables of the next launch are those of the new contents."""
    be = hip_f64
    nbnd = 4
    kds = [synthetic.make_kdist("lw", ngpt=64, nbnd=nbnd, npres=14, nflav=4, nminor_lower=6, nminor_upper=4, seed=s) for s in (3, 4)]
    atm = pipeline.upload_atmosphere(be, synthetic.make_atmosphere(256, 12, nbnd_lw=nbnd, nbnd_sw=nbnd))
    dev = be.upload_kdist(kds[0])

    def overwrite(kd0):
        other = be.upload_kdist(kd0)
        for name, t in vars(dev).items():
            src = getattr(other, name)
            if torch.is_tensor(t):
                assert t.shape == src.shape, name
                t.copy_(src)
            elif not isinstance(t, (list, tuple, dict)):
                setattr(dev, name, src)
        torch.cuda.synchronize()

    def tables_of(kd0):
        pipeline.solve_lw(be, dev, atm, do_broadband=True)
        buf, L = read_tables(be)
        check_tables(buf, L, restate(kd0, L["ncmax"], NXW, with_bands=True, with_lims=False), NXW)
        return buf

    first = tables_of(kds[0])
    overwrite(kds[1])
    assert not np.array_equal(first, tables_of(kds[1]))
    # only the key species of the flavors change (index arrays as before): the records follow
    import copy
    kd2 = copy.deepcopy(kds[1])
    kd2.flavor = np.ascontiguousarray(kd2.flavor[:, ::-1])
    assert not np.array_equal(kd2.flavor, kds[1].flavor)
    overwrite(kd2)
    tables_of(kd2)
    # ... and only the band of each g-point
    kd3 = copy.deepcopy(kd2)
    kd3.gpoint_bands = kd3.gpoint_bands.copy()
    kd3.gpoint_bands[kd3.gpoint_bands == 2] = 1                # (still ascending: the second band's g-points join the first)
    assert not np.array_equal(kd3.gpoint_bands, kd2.gpoint_bands)
    overwrite(kd3)
    tables_of(kd3)
