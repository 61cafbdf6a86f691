"""The correlation kernels alone (gpumd_amd/csrc/nep_corr.h) through nepmi_corr_sample on synthetic frames, in both tiers: the
GPU tier runs the tiled kernel + the fixed-order reduction, the CPU tier (kernel emulator) the plain body on the same ring, lag
mapping and tile table.

Frames: a seeded random walk (MSD) and seeded normal vectors on a common drift (VAC), so that the lags correlate.  Expected sums:
the definition restated in numpy, in double -- sample s goes to slot s % num_corr, from s >= num_corr - 1 on every sample is a time
origin and adds, per lag l, group and component, sum_i (u_i(s) - u_i(s - l))^2 or sum_i v_i(s) v_i(s - l).

Shapes: n in {1, 63, 64, 65, tile - 1, tile + 1, 5000} (a wavefront is 64 lanes, a tile 512 atoms = 256 lanes x 2; 5000 atoms are ten
tiles, the last one partial), num_corr in {1, 2, 7}; every correlator is read after num_corr - 1 samples (no origin yet: all sums
zero), after exactly num_corr samples and after 3 num_corr + 1 samples (the ring has wrapped three times).  Groups: one atom, an
empty group, atoms marked -1, a group boundary strictly inside what would be one tile, group membership interleaved in the
caller's order.

Bound (derived, not measured): any summation order of m doubles deviates from any other by at most m 2^-52 sum|terms|; per lag
with m = (atoms of the group) x (time origins) and sum|terms| from the numpy side.  Counters are exact; two identical runs are
equal bit for bit."""
import numpy as np
import pytest

import helpers as H

NEP = H.golden("PbTe", "nep.txt")
TILE = 512
SIZES = [1, 63, 64, 65, TILE - 1, TILE + 1, 5000]
NUM_CORR = [1, 2, 7]
EPS = 2.0 ** -52


def _frames(quantity, n, count, seed):
    rng = np.random.default_rng(seed)
    if quantity == "msd":
        return np.cumsum(rng.normal(0.0, 0.05, (count, 3, n)), axis=0) + rng.uniform(0.0, 30.0, (1, 3, n))
    return rng.normal(0.0, 1.0, (count, 3, n)) + rng.normal(0.0, 2.0, (1, 3, n))  # (the drift: every lag correlates)


def _expected(quantity, frames, upto, num_corr, groups, num_groups):
    """-> sums, sum|terms| [num_groups, 3, num_corr], origins after the first `upto` frames"""
    sums, mags, origins = np.zeros((num_groups, 3, num_corr)), np.zeros((num_groups, 3, num_corr)), 0
    for s in range(num_corr - 1, upto):
        origins += 1
        for lag in range(num_corr):
            t = (frames[s] - frames[s - lag]) ** 2 if quantity == "msd" else frames[s] * frames[s - lag]
            for g in range(num_groups):
                sel = groups == g
                sums[g, :, lag] += t[:, sel].sum(axis=1)
                mags[g, :, lag] += np.abs(t[:, sel]).sum(axis=1)
    return sums, mags, origins


_engines = {}


def _engine(drv, n):
    if (drv.name, n) not in _engines:
        _engines[(drv.name, n)] = drv.engine(drv.model(NEP), n)
    return _engines[(drv.name, n)]


def _run(drv, quantity, n, num_corr, groups, num_groups, frames, checkpoints):
    """samples the frames one by one -> {checkpoint: (sums, origins, samples)}"""
    from gpumd_amd.nep import Correlator
    c = Correlator(_engine(drv, n), quantity, 1, num_corr, group_of_atom=groups, num_groups=num_groups)
    out = {}
    if 0 in checkpoints:
        out[0] = c.read()
    for s in range(len(frames)):
        d_q = drv.dev(frames[s].reshape(-1))
        c.sample(d_q)
        if s + 1 in checkpoints:
            out[s + 1] = c.read()
    c.close()
    return out


def _check(drv, quantity, n, num_corr, groups=None, num_groups=1, seed=0):
    count = 3 * num_corr + 1
    frames = _frames(quantity, n, count, seed)
    checkpoints = (num_corr - 1, num_corr, count)
    got = _run(drv, quantity, n, num_corr, groups, num_groups, frames, checkpoints)
    again = _run(drv, quantity, n, num_corr, groups, num_groups, frames, checkpoints)
    gsel = np.zeros(n, dtype=np.int64) if groups is None else np.asarray(groups)
    worst = 0.0
    for upto in checkpoints:
        sums, origins, samples = got[upto]
        exp, mag, exp_origins = _expected(quantity, frames, upto, num_corr, gsel, num_groups)
        assert samples == upto and origins == exp_origins == max(0, upto - (num_corr - 1)), (samples, origins, exp_origins)
        if origins == 0:
            assert not sums.any()
        for g in range(num_groups):
            m = int((gsel == g).sum()) * origins
            bound = m * EPS * mag[g]
            dev = np.abs(sums[g] - exp[g])
            assert (dev <= bound).all(), (quantity, n, num_corr, g, upto, dev.max(), bound.max())
            if m > 0 and mag[g].max() > 0:
                worst = max(worst, float((dev / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(sums, again[upto][0]) and again[upto][1:] == (origins, samples)
    print("\n[%s %s n=%d num_corr=%d groups=%d] largest deviation / bound %.3g" % (drv.name, quantity, n, num_corr, num_groups, worst))
    if quantity == "msd" and num_corr > 1 and num_groups == 1:
        assert exp[:, :, 1:].min() > 0.0  # the walk moves: the sums are not trivially zero
    return got


def _groups(n):
    """group 0: one atom; group 1: empty; group 2 and 3 interleaved in the caller's order, group 2 with 700 atoms (odd count + 2 in
    front of it: its end lies inside what would be the second tile of a ring without boundaries); every 11th atom unsampled"""
    g = np.full(n, 3, dtype=np.int32)
    g[::11] = -1
    free = np.flatnonzero(g == 3)
    g[free[5]] = 0
    take = free[free != free[5]][::2][:701]
    g[take] = 2
    assert (g == 0).sum() == 1 and (g == 2).sum() == 701 and (g == 3).sum() > TILE and (g == -1).sum() > 0
    return g


def _refusals(drv):
    from gpumd_amd import _capi
    from gpumd_amd.nep import Correlator
    eng = _engine(drv, 65)
    with pytest.raises(_capi.NepmiError, match="quantity"):
        Correlator(eng, 2, 1, 3)
    with pytest.raises(_capi.NepmiError, match="positive"):
        Correlator(eng, "vac", 0, 3)
    with pytest.raises(_capi.NepmiError, match="positive"):
        Correlator(eng, "vac", 1, 0)
    with pytest.raises(_capi.NepmiError, match="group"):
        Correlator(eng, "vac", 1, 3, group_of_atom=np.full(65, 2, dtype=np.int32), num_groups=2)
    msd = Correlator(eng, "msd", 1, 3)
    with pytest.raises(_capi.NepmiError, match="unwrapped"):  # no nepmi_engine_set_unwrapped yet
        eng.attach(msd)
    vac, vac2 = Correlator(eng, "vac", 1, 3), Correlator(eng, "vac", 2, 5)
    eng.attach(vac)
    eng.attach(vac2)  # two at once
    with pytest.raises(_capi.NepmiError, match="already"):
        eng.attach(vac)
    eng.detach(vac)
    with pytest.raises(_capi.NepmiError, match="not attached"):
        eng.detach(vac)
    vac2.close()  # destroying an attached correlator detaches it first
    eng.attach(vac)
    eng.detach(vac)
    sums, origins, samples = vac.read()
    assert not sums.any() and (origins, samples) == (0, 0)


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
@pytest.mark.parametrize("quantity", ["msd", "vac"])
def test_sums_on_gpu(gpu, quantity, n, num_corr):
    _check(gpu, quantity, n, num_corr, seed=n + num_corr)


@pytest.mark.gpu
@pytest.mark.parametrize("quantity", ["msd", "vac"])
def test_groups_on_gpu(gpu, quantity):
    _check(gpu, quantity, 2000, 7, groups=_groups(2000), num_groups=4, seed=3)


@pytest.mark.gpu
def test_many_lags_are_cut_into_chunks_on_gpu(gpu):
    """150 lags on 65 atoms: one tile, so the lags are spread over workgroups (at most 64 per workgroup), the last chunk partial"""
    _check(gpu, "vac", 65, 150, seed=11)


@pytest.mark.gpu
def test_refusals_on_gpu(gpu):
    _refusals(gpu)


@pytest.mark.parametrize("num_corr", NUM_CORR)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("quantity", ["msd", "vac"])
def test_sums_on_emulator(emu, quantity, n, num_corr):
    _check(emu, quantity, n, num_corr, seed=n + num_corr)


@pytest.mark.parametrize("quantity", ["msd", "vac"])
def test_groups_on_emulator(emu, quantity):
    _check(emu, quantity, 2000, 7, groups=_groups(2000), num_groups=4, seed=3)


def test_refusals_on_emulator(emu):
    _refusals(emu)
