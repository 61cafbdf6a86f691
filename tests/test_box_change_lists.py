"""Per-call force evaluations under a changing box with the option "keep_lists_on_box_change": the engine re-metrics itself
(Engine::remetric -- cells, Verlet lists and window tables are integers that a homogeneous strain leaves alone) instead of
rebuilding, and the skin rule, with the rebuild-time positions kept in the old metric, decides about rebuilds like the reference's
Neighbor::find_neighbor_global (neighbor.cu:646-684, :741-800).

  strained evaluation  evaluate at h, then at h' = F h with x' = F x: num_rebuild unchanged; energies, forces, virials against the
                       oracle AT h' with the tolerances of the header of parity_cases.py; the per-step radial and angular lists equal
                       the oracle's at h' entry for entry.  The Verlet list is KEPT, so it must equal the oracle's Verlet list of the
                       rebuild-time state (h, x) entry for entry -- the oracle's list at h' differs from it by the pairs the strain
                       carried across rc + skin, which is what the skin exists for.
  F                    isotropic 1 + 3e-4 and an anisotropic diagonal strain on H.rocksalt_orthogonal((7, 8, 7)); a shear on the
                       triclinic PbTe cell ((3, 3, 3) on the GPU: the window kernels run; (2, 2, 2) on the emulator)
  forms                gather, and on the GPU the pinned scatter form (set_win_lanes(1) + set_force_form(1), describe() asserted)
  repeated strain      1 + 1e-3 per call until helpers.oracle_skin_moved fires: the engine's rebuild count equals that rule's, call
                       for call
  option off           every box change rebuilds (the default; passes without the feature)
  refusals             a pbc change rebuilds; a box strained into the small-box branch takes that branch (and the next large box
                       rebuilds)
The rebuild-count assertions of the option-on cases fail without the feature."""
import functools

import numpy as np
import pytest

import helpers as H

SCATTER = "lds_scatter_of_own_halves"
NEP = H.golden("PbTe", "nep.txt")
STRAINS = {
    "iso": np.eye(3) * (1.0 + 3e-4),
    "aniso": np.diag([1.0 + 4e-4, 1.0 - 2e-4, 1.0 + 1e-4]),
    "shear": np.array([[1.0 + 1e-4, 2e-4, -1e-4], [2e-4, 1.0 - 1e-4, 1.5e-4], [-1e-4, 1.5e-4, 1.0 + 2e-4]]),
}


@functools.lru_cache(maxsize=None)
def _system(name):
    if name == "ortho":
        h, typ, x = H.rocksalt_orthogonal((7, 8, 7), rattle=0.02, seed=9)
    else:
        h, typ, x = H.pbte_supercell({"tri3": (3, 3, 3), "tri2": (2, 2, 2)}[name], rattle=0.02, seed=31)
    return np.array(h, dtype=np.float64).reshape(9), typ, x


def _strained(F, h, x):
    """h' = F h (lattice vectors are the columns of h), x' = F x, wrapped into h'"""
    n = x.size // 3
    h2 = (F @ h.reshape(3, 3)).reshape(9)
    if np.count_nonzero(F - np.diag(np.diag(F))) == 0:  # keep an orthogonal box exactly orthogonal
        h2 = h2 * (h != 0)
    return h2, H.oracle_apply_pbc(h2, (F @ x.reshape(3, n)).reshape(-1))


def _engine(drv, n, form, keep=True):
    eng = drv.engine(drv.model(NEP), n)
    if form == "scatter":
        eng.set_win_lanes(1)
        eng.set_force_form(1)
    if keep:
        eng.set_option("keep_lists_on_box_change", 1)
    return eng


def _assert_parity(tag, orc, typ, h, x, pe, f, v):
    n = len(typ)
    pe64, f64, v64 = orc.compute(typ, h, x, precision=64, path=0)
    pe32, f32, v32 = orc.compute(typ, h, x, precision=32, path=0)
    print("\n[%s] max |f - f64| %.2e, |f - f32| %.2e eV/A, |w - w64| %.2e eV, E rel %.2e"
          % (tag, np.abs(f - f64).max(), np.abs(f - f32).max(), np.abs(v - v64).max(), abs(pe.sum() / pe64.sum() - 1.0)))
    np.testing.assert_allclose(pe.sum(), pe64.sum(), rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(pe, pe64, rtol=1e-5, atol=2e-5)
    assert np.all(np.abs(f - f64) <= 1e-4 * np.abs(f64) + 3e-5), np.abs(f - f64).max()
    assert np.all(np.abs(f - f32) <= 1e-4 * np.abs(f32) + 2e-5), np.abs(f - f32).max()
    assert np.all(np.abs(v - v64) <= 1e-4 * np.abs(v64) + 1e-4), np.abs(v - v64).max()
    assert np.abs(f.reshape(3, n).sum(axis=1)).max() < 1e-4 * np.sqrt(n)


def _strained_evaluation(drv, sysname, strain, form):
    h, typ, x = _system(sysname)
    n = len(typ)
    orc = H.Oracle(NEP)
    eng = _engine(drv, n, form)
    H.engine_force(drv, eng, h, typ, x)
    assert eng.stats().num_rebuild == 1
    h2, x2 = _strained(STRAINS[strain], h, x)
    assert not H.oracle_skin_moved(h2, x2, x), "the strain alone trips the skin rule: choose a smaller one"
    xw, pe, f, v = H.engine_force(drv, eng, h2, typ, x2)
    desc = eng.describe()
    assert (SCATTER in desc) == (form == "scatter"), desc
    assert eng.stats().num_rebuild == 1, "the box change rebuilt the lists"
    assert np.abs(xw - x2).max() < 1e-9  # (not array_equal: another wrap rounds H (H^-1 x) anew, ~1e-14 A)
    x2 = xw
    _assert_parity("%s %s %s %s" % (drv.name, sysname, strain, form), orc, typ, h2, x2, pe, f, v)
    L2, L1 = orc.lists(typ, h2, x2, path=0), orc.lists(typ, h, x, path=0)
    for which, key, L in ((0, "radial", L2), (1, "angular", L2), (2, "skin", L1)):
        onn, onl = L[key]
        mx, nn, nl = H.engine_lists(drv, eng, n, which, ld=int(onn.max()) + 2)
        H.assert_lists_equal(nn, nl, onn, onl)
    # the kept Verlet list still holds every pair inside the cutoffs at h' (what the skin guarantees)
    assert (L2["radial"][0] <= L1["skin"][0]).all()
    # ... and the same engine, rebuilt at h', agrees with itself on kept lists to summation order
    eng.invalidate()
    _, pe_r, f_r, v_r = H.engine_force(drv, eng, h2, typ, x2)
    assert eng.stats().num_rebuild == 2
    assert np.abs(f - f_r).max() < 2e-5 and np.abs(pe - pe_r).max() < 2e-5, (np.abs(f - f_r).max(), np.abs(pe - pe_r).max())


def _repeated_strain(drv, sysname, form, ncalls=12):
    h, typ, x = _system(sysname)
    n = len(typ)
    orc = H.Oracle(NEP)
    eng = _engine(drv, n, form)
    F = np.eye(3) * (1.0 + 1e-3)
    H.engine_force(drv, eng, h, typ, x)
    x_rebuild, expect, counts, rule = x.copy(), 1, [], []
    pe = f = v = None
    for _ in range(ncalls):
        h, x = _strained(F, h, x)
        if H.oracle_skin_moved(h, x, x_rebuild):
            x_rebuild, expect = x.copy(), expect + 1
        x, pe, f, v = H.engine_force(drv, eng, h, typ, x)
        counts.append(eng.stats().num_rebuild)
        rule.append(expect)
    print("\n[%s %s %s repeated strain] rebuilds after each call: engine %s, skin rule %s" % (drv.name, sysname, form, counts, rule))
    assert counts == rule
    assert 1 < rule[-1] < ncalls + 1, "the run must hold a rebuild and calls on kept lists"
    _assert_parity("%s %s repeated strain, last call" % (drv.name, form), orc, typ, h, x, pe, f, v)


def _option_off(drv):
    h, typ, x = _system("tri2")
    eng = _engine(drv, len(typ), "gather", keep=False)
    H.engine_force(drv, eng, h, typ, x)
    for k in range(3):
        h, x = _strained(STRAINS["iso"], h, x)
        H.engine_force(drv, eng, h, typ, x)
        assert eng.stats().num_rebuild == 2 + k
    H.engine_force(drv, eng, h, typ, x)  # the same box again: the lists stand
    assert eng.stats().num_rebuild == 4


def _refusals(drv):
    orc = H.Oracle(NEP)
    # a pbc change rebuilds
    h, typ, x = _system("tri2")
    n = len(typ)
    eng = _engine(drv, n, "gather")
    H.engine_force(drv, eng, h, typ, x)
    h2, x2 = _strained(STRAINS["iso"], h, x)
    H.engine_force(drv, eng, h2, typ, x2)
    assert eng.stats().num_rebuild == 1
    eng.pbc = (1, 1, 0)
    h3, x3 = _strained(STRAINS["iso"], h2, x2)
    H.engine_force(drv, eng, h3, typ, x3)
    assert eng.stats().num_rebuild == 2
    # a box strained into the small-box branch (a periodic thickness <= 2.5 (rc + skin) = 22.5 A) takes that branch
    h, typ, x = H.rocksalt_orthogonal((4, 4, 4), rattle=0.02, seed=9)
    h, n = np.array(h, dtype=np.float64).reshape(9), len(typ)
    eng = _engine(drv, n, "gather")
    H.engine_force(drv, eng, h, typ, x)
    hs, xs = _strained(np.diag([1.08, 1.08, 22.4 / h[8]]), h, x)
    assert orc.lists(typ, h, x)["path"] == 0 and orc.lists(typ, hs, xs)["path"] == 1
    _, pe, f, v = H.engine_force(drv, eng, hs, typ, xs)
    assert eng.stats().num_rebuild == 1  # (the small-box branch keeps no lists)
    pe64, f64, v64 = orc.compute(typ, hs, xs, precision=64)
    np.testing.assert_allclose(pe.sum(), pe64.sum(), rtol=1e-5)
    assert np.all(np.abs(f - f64) <= 1e-4 * np.abs(f64) + 3e-5), np.abs(f - f64).max()
    _, pe, f, v = H.engine_force(drv, eng, h, typ, x)  # back in the large box: no list to keep
    assert eng.stats().num_rebuild == 2
    _assert_parity("%s back from the small box" % drv.name, orc, typ, h, x, pe, f, v)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    return H.GpuDriver()


@pytest.fixture(scope="module")
def emu():
    return H.EmuDriver()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gather", "scatter"])
@pytest.mark.parametrize("sysname,strain", [("ortho", "iso"), ("ortho", "aniso"), ("tri3", "shear")])
def test_strained_evaluation_keeps_lists_on_gpu(gpu, sysname, strain, form):
    _strained_evaluation(gpu, sysname, strain, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gather", "scatter"])
def test_repeated_strain_rebuilds_by_the_skin_rule_on_gpu(gpu, form):
    _repeated_strain(gpu, "ortho", form)


@pytest.mark.gpu
def test_option_off_and_refusals_on_gpu(gpu):
    _option_off(gpu)
    _refusals(gpu)


@pytest.mark.parametrize("sysname,strain", [("ortho", "iso"), ("ortho", "aniso"), ("tri2", "shear")])
def test_strained_evaluation_keeps_lists_on_emulator(emu, sysname, strain):
    _strained_evaluation(emu, sysname, strain, "gather")


def test_repeated_strain_rebuilds_by_the_skin_rule_on_emulator(emu):
    _repeated_strain(emu, "ortho", "gather")


def test_option_off_on_emulator(emu):
    _option_off(emu)


def test_refusals_on_emulator(emu):
    _refusals(emu)
