"""Quantity 2 of the correlator (mass-weighted velocity autocorrelation, gpumd_amd/csrc/nep_corr.h) through nepmi_corr_sample on
synthetic frames, in both tiers, and nepmi_dos_from_mvac against a numpy restatement.  Drivers, VAC frames, group layout and
engines are those of test_corr_kernels.py.

Expected sums: sample s goes to slot s % num_corr, from s >= num_corr - 1 on every sample is a time origin and adds, per lag l,
group and component, sum_i (w_i v_i(s)) v_i(s - l) -- formed in numpy with that association.  Weights: seeded uniform(1, 250);
one case with the two PbTe masses only.

Bound (derived, not measured): a term (w v) v' carries two roundings, 2 x 2^-52 of itself, and any summation order of m doubles
deviates from the exact sum by at most m 2^-52 sum|terms| to first order: (m + 2) 2^-52 sum|terms| per group, component and lag,
m = (atoms of the group) x (time origins).  Counters are exact; two identical runs are equal bit for bit.

With every weight 1.0 the premultiplication is exact and the sums must be those of quantity 1, bit for bit (same tiles, same
order).  With weight 0 on every atom of one group that group's sums are exactly zero and the other groups' bits do not move.

nepmi_dos_from_mvac: plain double arithmetic on the host, Nc terms per output value.  Tolerance Nc 2^-50 sum|terms| per output
value: the summation bound Nc 2^-52 sum|terms|, four times for the cosine and the products (the numpy side forms the cosine's
argument with the same association, so only the two cosine implementations' last digit differs).  One physical check: 2,000
atoms with v_i(s) = a_i cos(w0 s dt + phi_i); the maximum of the DOS lies within 2 pi / (Nc dt), the half width of the window's
main lobe, of w0."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
import test_corr_kernels as CK

SIZES = CK.SIZES
NUM_CORR = CK.NUM_CORR
EPS = CK.EPS


def _weights(n, seed, pbte=False):
    rng = np.random.default_rng(1000 + seed)
    if pbte:
        return np.where(rng.integers(0, 2, n) == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    return rng.uniform(1.0, 250.0, n)


def _expected(frames, w, upto, num_corr, groups, num_groups):
    """-> sums, sum|terms| [num_groups, 3, num_corr], origins after the first `upto` frames"""
    sums, mags, origins = np.zeros((num_groups, 3, num_corr)), np.zeros((num_groups, 3, num_corr)), 0
    for s in range(num_corr - 1, upto):
        origins += 1
        wv = w[None, :] * frames[s]
        for lag in range(num_corr):
            t = wv * frames[s - lag]
            for g in range(num_groups):
                sel = groups == g
                sums[g, :, lag] += t[:, sel].sum(axis=1)
                mags[g, :, lag] += np.abs(t[:, sel]).sum(axis=1)
    return sums, mags, origins


def _run(drv, quantity, n, num_corr, groups, num_groups, frames, checkpoints, weights):
    from gpumd_amd.nep import Correlator
    c = Correlator(CK._engine(drv, n), quantity, 1, num_corr, group_of_atom=groups, num_groups=num_groups, weights=weights)
    out = {}
    if 0 in checkpoints:
        out[0] = c.read()
    for s in range(len(frames)):
        c.sample(drv.dev(frames[s].reshape(-1)))
        if s + 1 in checkpoints:
            out[s + 1] = c.read()
    c.close()
    return out


def _check(drv, n, num_corr, groups=None, num_groups=1, seed=0, pbte=False):
    count = 3 * num_corr + 1
    frames = CK._frames("vac", n, count, seed)
    w = _weights(n, seed, pbte)
    checkpoints = (num_corr - 1, num_corr, count)
    got = _run(drv, "mvac", n, num_corr, groups, num_groups, frames, checkpoints, w)
    again = _run(drv, "mvac", n, num_corr, groups, num_groups, frames, checkpoints, w)
    gsel = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups)
    worst = 0.0
    for upto in checkpoints:
        sums, origins, samples = got[upto]
        exp, mag, exp_origins = _expected(frames, w, upto, num_corr, gsel, num_groups)
        assert samples == upto and origins == exp_origins == max(0, upto - (num_corr - 1)), (samples, origins, exp_origins)
        if origins == 0:
            assert not sums.any()
        for g in range(num_groups):
            m = int((gsel == g).sum()) * origins
            bound = (m + 2) * EPS * mag[g]
            dev = np.abs(sums[g] - exp[g])
            assert (dev <= bound).all(), (n, num_corr, g, upto, dev.max(), bound.max())
            if m > 0 and mag[g].max() > 0:
                worst = max(worst, float((dev / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(sums, again[upto][0]) and again[upto][1:] == (origins, samples)
    print("\n[%s mvac n=%d num_corr=%d groups=%d] largest deviation / bound %.3g" % (drv.name, n, num_corr, num_groups, worst))
    assert np.abs(exp).max() > 0.0
    return got


def _unit_weights(drv, n, num_corr, groups, num_groups):
    count = 3 * num_corr + 1
    frames = CK._frames("vac", n, count, 17)
    vac = _run(drv, "vac", n, num_corr, groups, num_groups, frames, (count,), None)[count]
    mvac = _run(drv, "mvac", n, num_corr, groups, num_groups, frames, (count,), np.ones(n))[count]
    assert vac[0].any() and np.array_equal(vac[0], mvac[0]) and vac[1:] == mvac[1:]


def _zero_weights(drv):
    n, num_corr, groups = 2000, 7, CK._groups(2000)
    count = 3 * num_corr + 1
    frames = CK._frames("vac", n, count, 23)
    w = _weights(n, 23)
    full = _run(drv, "mvac", n, num_corr, groups, 4, frames, (count,), w)[count][0]
    for dead in (2, 3):  # (group 2 ends inside a tile that group 3 does not share: the tile table is cut at the boundary)
        w0 = np.where(groups == dead, 0.0, w)
        part = _run(drv, "mvac", n, num_corr, groups, 4, frames, (count,), w0)[count][0]
        assert full[dead].any() and not part[dead].any()
        for g in range(4):
            if g != dead:
                assert np.array_equal(part[g], full[g]), (dead, g)


def _refusals(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import Correlator
    eng = CK._engine(drv, 65)
    w = np.full(65, 2.0)
    for q in ("msd", "vac", 0, 1):
        with pytest.raises(_capi.NepmiError, match="weights belong to quantity 2"):
            Correlator(eng, q, 1, 3, weights=w)
    with pytest.raises(_capi.NepmiError, match="quantity"):  # nepmi_corr_create: as before
        Correlator(eng, "mvac", 1, 3)
    out = C.c_void_p()
    st = drv.lib.nepmi_corr_create_weighted(eng.handle, 2, 65, 1, 3, None, 1, None, C.byref(out))  # no weight array
    assert st == -4 and not out.value and "weight" in drv.lib.nepmi_last_error().decode()
    for bad in (np.nan, np.inf, -1.0):
        wb = w.copy()
        wb[64] = bad
        with pytest.raises(_capi.NepmiError, match="weight"):
            Correlator(eng, "mvac", 1, 3, weights=wb)
    with pytest.raises(ValueError, match="weights"):
        Correlator(eng, "mvac", 1, 3, weights=w[:64])
    with pytest.raises(_capi.NepmiError, match="positive"):
        Correlator(eng, "mvac", 0, 3, weights=w)
    a, b = Correlator(eng, "mvac", 1, 3, weights=w), Correlator(eng, "mvac", 2, 5, weights=w)
    eng.attach(a)  # like VAC: no unwrapped positions needed
    eng.attach(b)
    with pytest.raises(_capi.NepmiError, match="already"):
        eng.attach(a)
    eng.detach(a)
    with pytest.raises(_capi.NepmiError, match="not attached"):
        eng.detach(a)
    b.close()  # destroying an attached correlator detaches it first
    sums, origins, samples = a.read()
    assert not sums.any() and (origins, samples) == (0, 0)
    with pytest.raises(ValueError, match="mvac"):
        Correlator(eng, "vac", 1, 3).dos(0.002, 100.0)


# ---- nepmi_dos_from_mvac -----------------------------------------------------------------------------------------------------
def _dos_numpy(sums, size, dt_ps, omega_max, npts):
    """-> omega, mvac, dos, sum|terms| of dos"""
    ng, _, nc = sums.shape
    s0 = sums[:, :, 0:1]
    ok = s0 != 0.0
    mvac = np.where(ok, sums / np.where(ok, s0, 1.0), 0.0)
    lag = np.arange(nc)
    hann = (np.cos((np.pi * lag) / nc) + 1.0) * 0.5
    win = mvac * np.where(lag == 0, hann, 2.0 * hann)
    d_omega = omega_max / npts
    omega = d_omega + np.arange(npts) * d_omega
    cosf = np.cos(omega[:, None] * lag[None, :] * dt_ps)  # ((omega l) dt), [npts, nc]
    terms = win[:, :, None, :] * cosf[None, None, :, :]
    scale = (dt_ps * 2.0 * size.astype(np.float64))[:, None, None]
    return omega, mvac, terms.sum(axis=3) * scale, np.abs(terms).sum(axis=3) * scale


def _dos_case(lib, ng, nc, npts, seed):
    from gpumd_amd.nep import dos_from_mvac
    rng = np.random.default_rng(seed)
    sums = rng.normal(0.0, 40.0, (ng, 3, nc))
    sums[:, :, 0] = np.abs(sums[:, :, 0]) + 25.0
    size = rng.integers(1, 5000, ng).astype(np.int64)
    if ng > 1:
        sums[1], size[1] = 0.0, 0  # an empty group
    dt_ps, omega_max = 0.004, 300.0
    omega, mvac, dos = dos_from_mvac(lib, sums, size, dt_ps, omega_max, npts)
    e_omega, e_mvac, e_dos, mag = _dos_numpy(sums, size, dt_ps, omega_max, npts)
    assert mvac.shape == (ng, 3, nc) and dos.shape == (ng, 3, npts)
    assert np.array_equal(omega, e_omega)
    tol = nc * 2.0 ** -50
    assert (np.abs(mvac - e_mvac) <= tol * np.abs(e_mvac)).all()
    assert (np.abs(dos - e_dos) <= tol * mag).all(), float((np.abs(dos - e_dos) / np.maximum(tol * mag, 1e-300)).max())
    assert (mvac[:, :, 0] == np.where(sums[:, :, 0] != 0, 1.0, 0.0)).all()
    if ng > 1:
        assert not mvac[1].any() and not dos[1].any() and np.isfinite(dos).all()
        assert dos[0].any() and dos[2].any()


def _dos_refusals(lib):
    from gpumd_amd import _capi
    from gpumd_amd.nep import dos_from_mvac
    sums, size = np.ones((1, 3, 4)), np.array([10])
    for args in ((0.0, 100.0, 4), (0.002, 0.0, 4), (0.002, 100.0, 0)):
        with pytest.raises(_capi.NepmiError, match="positive"):
            dos_from_mvac(lib, sums, size, *args)
    assert dos_from_mvac(lib, sums, size, 0.002, 100.0)[2].shape == (1, 3, 4)  # num_dos_points defaults to Nc


def _oscillators(drv):
    """every atom one cosine of the same angular frequency w0, seeded amplitudes and phases: MVAC ~ cos(w0 l dt)"""
    from gpumd_amd.nep import Correlator
    n, nc, dt_ps, w0, omega_max, npts = 2000, 64, 0.005, 60.0, 200.0, 200
    rng = np.random.default_rng(41)
    a, phi = rng.uniform(0.5, 1.5, (3, n)), rng.uniform(0.0, 2.0 * np.pi, (3, n))
    mass = _weights(n, 41, pbte=True)
    c = Correlator(CK._engine(drv, n), "mvac", 1, nc, weights=mass)
    for s in range(2 * nc):
        c.sample(drv.dev((a * np.cos(w0 * s * dt_ps + phi)).reshape(-1)))
    omega, mvac, dos = c.dos(dt_ps, omega_max, npts)
    c.close()
    half_width = 2.0 * np.pi / (nc * dt_ps)
    assert (mvac[0, :, 0] == 1.0).all()
    for d in range(3):
        peak = omega[np.argmax(dos[0, d])]
        print("\n[%s oscillators] component %d: DOS maximum at %.2f THz, w0 %.2f, window half width %.2f" % (drv.name, d, peak, w0, half_width))
        assert abs(peak - w0) <= half_width, (d, peak, w0, half_width)
        # (random phases: the second-harmonic part of an origin's sum is 1.2 / sqrt(n) = 0.027 rms of lag 0, in numerator and
        # denominator, before the average over the 65 origins: 0.1 is more than three times that)
        assert np.abs(mvac[0, d] - np.cos(w0 * np.arange(nc) * dt_ps)).max() < 0.1


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


@pytest.mark.gpu
@pytest.mark.parametrize("num_corr", NUM_CORR)
@pytest.mark.parametrize("n", SIZES)
def test_sums_on_gpu(gpu, n, num_corr):
    _check(gpu, n, num_corr, seed=n + num_corr)


@pytest.mark.gpu
def test_groups_on_gpu(gpu):
    _check(gpu, 2000, 7, groups=CK._groups(2000), num_groups=4, seed=3)


@pytest.mark.gpu
def test_the_two_pbte_masses_on_gpu(gpu):
    _check(gpu, 5000, 7, seed=5, pbte=True)


@pytest.mark.gpu
def test_many_lags_are_cut_into_chunks_on_gpu(gpu):
    _check(gpu, 65, 150, seed=11)


@pytest.mark.gpu
@pytest.mark.parametrize("n, num_corr, grouped", [(5000, 7, False), (513, 2, False), (1, 1, False), (2000, 7, True)])
def test_unit_weights_give_the_bits_of_vac_on_gpu(gpu, n, num_corr, grouped):
    _unit_weights(gpu, n, num_corr, CK._groups(n) if grouped else None, 4 if grouped else 1)


@pytest.mark.gpu
def test_zero_weights_silence_one_group_on_gpu(gpu):
    _zero_weights(gpu)


@pytest.mark.gpu
def test_refusals_on_gpu(gpu):
    _refusals(gpu)


@pytest.mark.gpu
def test_oscillators_peak_at_their_frequency_on_gpu(gpu):
    _oscillators(gpu)


@pytest.mark.parametrize("num_corr", NUM_CORR)
@pytest.mark.parametrize("n", SIZES)
def test_sums_on_emulator(emu, n, num_corr):
    _check(emu, n, num_corr, seed=n + num_corr)


def test_groups_on_emulator(emu):
    _check(emu, 2000, 7, groups=CK._groups(2000), num_groups=4, seed=3)


def test_the_two_pbte_masses_on_emulator(emu):
    _check(emu, 5000, 7, seed=5, pbte=True)


@pytest.mark.parametrize("n, num_corr, grouped", [(5000, 7, False), (513, 2, False), (1, 1, False), (2000, 7, True)])
def test_unit_weights_give_the_bits_of_vac_on_emulator(emu, n, num_corr, grouped):
    _unit_weights(emu, n, num_corr, CK._groups(n) if grouped else None, 4 if grouped else 1)


def test_zero_weights_silence_one_group_on_emulator(emu):
    _zero_weights(emu)


def test_refusals_on_emulator(emu):
    _refusals(emu)


def test_oscillators_peak_at_their_frequency_on_emulator(emu):
    _oscillators(emu)


@pytest.mark.parametrize("npts", [1, 50, 77])
@pytest.mark.parametrize("nc", [1, 2, 50])
@pytest.mark.parametrize("ng", [1, 3])
def test_dos_from_mvac_against_numpy(emu, ng, nc, npts):
    _dos_case(emu.lib, ng, nc, npts, seed=100 * ng + 10 * nc + npts)


def test_dos_from_mvac_refusals(emu):
    _dos_refusals(emu.lib)


@pytest.mark.gpu
def test_dos_from_mvac_in_the_product_library(gpu):
    _dos_case(gpu.lib, 3, 50, 77, seed=7)
    _dos_refusals(gpu.lib)
