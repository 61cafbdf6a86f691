"""GPU tier: the two walks of the per-step radial list without the work their sums never use (engine option "lean_list_walks"
= 1, the default) against the former bodies (option = 0).

Radial pass (nep_window.h: RadialWin2Body<S, SYNC, 1>): list A of a two-type shape evaluates the two candidates of a half-word
side by side, once each, and adds each to the half of its type -- the same two fma per half of the packed sums on the same
operands in the same order as the former body, which evaluated every candidate in both halves and multiplied the half of the
other type by 0.  Scatter form (nep_scatter.h: LEAN): a padding place of a wave-synchronous word is read like any other place
and its pair coefficient is replaced by 0; the former body gave it a weight of 0.  Both clamp the distance with one integer
minimum.  Only products with 1 and sums with 0 are left out, so every returned array must be equal under numpy.array_equal.

Cases: PbTe (two types: both changes), the same with the type-wise ZBL, carbon (one type: list A is already paired, the
scatter walk changes), BaZrO3 (three types: neither change reaches it, describe() says so), a dilute gas (most places of most
words are padding, a lane can have an empty stream beside a full one), and two-rank runs with forward-mode and reverse-mode
ghosts over the in-process device transport (ghost lanes return before the walk; the ranks' engines take the option's default
from the environment).  Cutoffs: the envelope at a padding place's clamped distance rc is exactly zero only where the device's
unrounded rc * (1 / rc) - 0.5 is exactly 0.5, which holds for the 8 and 4.2 A of the models above and does not for 7 A (sine
term -1.8e-7), 6.5 A or cutoffs per type (the device's 1-ulp reciprocal); the lean walk must not depend on it, so PbTe with
radial cutoffs of 7 and 6.5 A, PbTe with per-type cutoffs and the shipped C_2024 model (7 A, on its prebuilt JIT core) run too.

The scatter kernel exists on the device only; the emulator accepts the option (its radial pass is the same template)."""
import os

import numpy as np
import pytest

import helpers as H
import parity_cases as P

SYNC = "radial_list=wave_synchronous_words"
SCATTER = "lds_scatter_of_own_halves"
LEAN, CLASSIC = "list_walks=lean ", "list_walks=classic "


@pytest.fixture(scope="module")
def drv():
    return H.GpuDriver()


def _engine(drv, model, n, lean, pin=True):
    eng = drv.engine(model, n)
    eng.set_lean_list_walks(lean)
    if pin:  # (systems below the size the run loops' rule asks for: the one-lane scatter form)
        eng.set_win_lanes(1)
        eng.set_force_form(1)
    return eng


def _per_call(drv, model, h, typ, x, lean, token):
    n = len(typ)
    eng = _engine(drv, model, n, lean)
    _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
    d = eng.describe()
    assert SCATTER in d and token in d, d
    q = drv.zeros(model.info.dim * n, dtype=np.float32)
    fp = drv.zeros(model.info.dim * n, dtype=np.float32)
    eng.descriptors(q, fp)
    return {"pe": pe, "f": f, "v": v, "q": drv.host(q), "fp": drv.host(fp)}


def _run(drv, model, h, typ, x, mass, temp, lean, token, nsteps=20, dt_fs=2.0, jit=False):
    """20 steps with thermo_every=5: steps that record (the OUT instantiation of the scatter kernel) among forces-only ones"""
    n = len(typ)
    vel = H.maxwell_velocities(mass, temp, seed=4)
    eng = _engine(drv, model, n, lean)
    d_t, d_m, d_x, d_v = drv.dev(typ), drv.dev(mass), drv.dev(x), drv.dev(vel)
    d_pe, d_f, d_w = drv.zeros(n), drv.zeros(3 * n), drv.zeros(9 * n)
    eng.force_compute(h, d_t, d_x, d_pe, d_f, d_w)
    r0 = eng.stats().num_rebuild
    th = eng.run_nve(h, d_t, d_m, dt_fs / H.TIME_UNIT, nsteps, d_x, d_v, d_pe, d_f, d_w, thermo_every=5)
    d = eng.describe()
    print(d)
    assert SYNC in d and SCATTER in d and token in d, d
    assert ("shape=jit(" in d) == jit, d
    return {"x": drv.host(d_x), "vel": drv.host(d_v), "f": drv.host(d_f), "pe": drv.host(d_pe), "w": drv.host(d_w),
            "th": np.asarray(th)}, eng.stats().num_rebuild - r0


def _same(a, b):
    for key in a:
        print("%-4s equal=%s  max|diff|=%.3e" % (key, np.array_equal(a[key], b[key]), np.abs(a[key] - b[key]).max()))
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), (key, np.abs(a[key] - b[key]).max())


def _tokens(two_walks=True):
    return ((0, CLASSIC), (1, LEAN if two_walks else CLASSIC))


def _pbte(reps=(3, 3, 3)):
    h, typ, x = H.pbte_supercell(reps, rattle=0.03, seed=17)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    return h, typ, x, mass


@pytest.mark.gpu
def test_pbte_nve_with_a_list_rebuild(drv):
    """6,750 atoms of PbTe at 2500 K, one evaluation with the exports and 20 steps of 2 fs with a list rebuild inside"""
    h, typ, x, mass = _pbte()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    a, b = (_per_call(drv, model, h, typ, x, lean, tok) for lean, tok in _tokens())
    assert np.abs(a["f"]).max() > 0.0 and np.abs(a["fp"]).max() > 0.0
    _same(a, b)
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 2500.0, lean, tok) for lean, tok in _tokens())
    print("list rebuilds inside the run: %d / %d" % (nb0, nb1))
    assert nb0 >= 1 and nb1 == nb0, (nb0, nb1)
    _same(r0, r1)


@pytest.mark.gpu
def test_pbte_with_typewise_zbl(drv, tmp_path):
    import test_model_variants as V
    h, typ, x, mass = _pbte()
    model = drv.model(V.make_typewise_zbl(tmp_path))
    _same(*(_per_call(drv, model, h, typ, x, lean, tok) for lean, tok in _tokens()))
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 2500.0, lean, tok) for lean, tok in _tokens())
    assert nb0 >= 1 and nb1 == nb0, (nb0, nb1)
    _same(r0, r1)


@pytest.mark.gpu
@pytest.mark.parametrize("cutoff", ["7 4 73 8", "6.5 4 73 8", "8 4 7.2 3.6 73 8"], ids=["rc7", "rc6.5", "per_type"])
def test_pbte_with_cutoffs_whose_envelope_is_not_zero_at_the_clamp(drv, tmp_path, cutoff):
    """the PbTe model with another `cutoff` line: a padding place's envelope and derivative come out as 1e-8 .. 4e-7 instead of 0,
    which a weight of 0 hid in the former body; an own force without its reaction or a virial term would show here"""
    import test_model_variants as V
    L = V._pbte_lines()
    assert L[1].startswith("cutoff")
    model = drv.model(V._write(tmp_path, "cut.txt", [L[0], "cutoff " + cutoff] + L[2:]))
    h, typ, x, mass = _pbte()
    a, b = (_per_call(drv, model, h, typ, x, lean, tok) for lean, tok in _tokens())
    assert np.abs(a["f"]).max() > 0.0
    _same(a, b)
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 1500.0, lean, tok) for lean, tok in _tokens())
    assert nb1 == nb0, (nb0, nb1)
    _same(r0, r1)


@pytest.mark.gpu
def test_carbon_2024_radial_cutoff_of_7(monkeypatch):
    """the shipped C_2024 model (radial cutoff 7 A, one type) on the JIT core that build() makes for its shape (NEPMI_JIT=2: a
    prebuilt core or none, never the compiler), 5,832 atoms of diamond in windows of about 5,900 slots (the 768-thread form of
    the scatter kernel)"""
    monkeypatch.setenv("NEPMI_JIT", "2")
    drv = H.GpuDriver()
    nep_rel, build, _ = P.MODELS["C-2024-window"]
    h, typ, x = build()
    model = drv.model(H.golden(*nep_rel.split("/")))
    a, b = (_per_call(drv, model, h, typ, x, lean, tok) for lean, tok in _tokens())
    assert np.abs(a["f"]).max() > 0.0
    _same(a, b)
    mass = np.full(len(typ), H.MASS["C"], dtype=np.float64)
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 2000.0, lean, tok, nsteps=10, dt_fs=1.0, jit=True) for lean, tok in _tokens())
    assert nb1 == nb0, (nb0, nb1)
    _same(r0, r1)


@pytest.mark.gpu
def test_carbon_one_type(drv):
    """one type: list A was paired before, the scatter walk and the clamp change"""
    nep_rel, build, _ = P.MODELS["C-2022"]
    h, typ, x = build()
    model = drv.model(H.golden(*nep_rel.split("/")))
    a, b = (_per_call(drv, model, h, typ, x, lean, tok) for lean, tok in _tokens())
    assert np.abs(a["f"]).max() > 0.0
    _same(a, b)
    mass = np.full(len(typ), H.MASS["C"], dtype=np.float64)
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 2000.0, lean, tok, dt_fs=1.0) for lean, tok in _tokens())
    assert nb1 == nb0, (nb0, nb1)
    _same(r0, r1)


@pytest.mark.gpu
def test_three_types_keep_their_bodies(drv):
    """BaZrO3: the many-type radial pass and scatter kernel are not touched -- describe() names the former walks under both
    values of the option"""
    nep_rel, build, _ = P.MODELS["BaZrO3"]
    h, typ, x = build()
    model = drv.model(H.golden(*nep_rel.split("/")))
    out = []
    for lean in (0, 1):
        eng = _engine(drv, model, len(typ), lean)
        _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
        d = eng.describe()
        print(d)
        assert CLASSIC in d, d
        out.append({"pe": pe, "f": f, "v": v})
    assert np.abs(out[0]["f"]).max() > 0.0
    _same(*out)


@pytest.mark.gpu
def test_dilute_gas_of_mostly_padding(drv):
    """the dilute gas of tests/test_fused_pair_trip.py (4,000 atoms, a handful of radial neighbours each): the words of a
    wavefront are as long as its busiest lane's, so most places are padding and one stream of a lane can be empty"""
    import test_fused_pair_trip as T
    h, typ, x, pos, L = T._sparse_gas()
    model = drv.model(H.golden("PbTe", "nep.txt"))
    a, b = (_per_call(drv, model, h, typ, x, lean, tok) for lean, tok in _tokens())
    assert np.abs(a["f"]).max() > 0.0
    _same(a, b)
    mass = np.where(typ == 0, H.MASS["Te"], H.MASS["Pb"]).astype(np.float64)
    (r0, nb0), (r1, nb1) = (_run(drv, model, h, typ, x, mass, 300.0, lean, tok, dt_fs=1.0) for lean, tok in _tokens())
    assert nb0 == nb1
    _same(r0, r1)


@pytest.mark.gpu
@pytest.mark.parametrize("ghosts", [0, 1], ids=["forward_ghosts", "reverse_ghosts"])
def test_decomposed_run_on_two_ranks(monkeypatch, ghosts):
    """Two ranks as threads over the in-process device transport, the scatter form pinned: ghost lanes return before the walk,
    reverse-mode ghosts only collect.  The local engines are not reachable from here: the option's default comes from the
    environment."""
    import test_dist as T
    import test_dist_inproc as TI
    if not os.path.exists(TI.LIB["gpu"]):
        pytest.skip("tests/inproc transports not built")
    from gpumd_amd.dist import DistMD
    spec = dict(T._spec("gpu", "PbTe-reps", (8, 4, 4), (2, 1, 1), "nve", 20, 3000.0, ghosts=ghosts), force_form=1, thermo_every=5)
    said = []  # what each rank's engine ran last, taken when the rank (a thread of this process) closes its driver
    close = DistMD.close

    def close_and_tell(self):
        if getattr(self, "handle", None):
            said.append(self.engine_describe())
        close(self)

    monkeypatch.setattr(DistMD, "close", close_and_tell)
    out = []
    for lean, token in (("0", CLASSIC), ("1", LEAN)):
        monkeypatch.setenv("NEPMI_LEAN_LIST_WALKS", lean)
        del said[:]
        out.append(TI._run_threads(2, spec))
        print(said)
        assert len(said) == 2 and all(SYNC in d and SCATTER in d and token in d for d in said), said
    for ra, rb in zip(*out):
        assert int(ra["ndec"]) == int(rb["ndec"]) and int(ra["reverse"]) == ghosts and int(rb["reverse"]) == ghosts
        assert int(ra["nhand"]) == 0 and int(rb["nhand"]) == 0  # (no hand-over to the gather form: the scatter kernel ran throughout)
        for key in ("i0", "f0", "i1", "x1", "v1", "f1", "th1", "th", "w1"):
            assert np.array_equal(ra[key], rb[key]), (key, np.abs(ra[key] - rb[key]).max())


def test_option_is_accepted_where_the_kernels_do_not_exist():
    """emulator tier: no scatter kernel -- the option is known and the forces do not move"""
    drv = H.EmuDriver()
    h, typ, x = H.pbte_supercell((2, 2, 2))
    model = drv.model(H.golden("PbTe", "nep.txt"))
    out = []
    for lean in (0, 1):
        eng = drv.engine(model, len(typ))
        eng.set_lean_list_walks(lean)
        _, pe, f, v = H.engine_force(drv, eng, h, typ, x)
        assert SCATTER not in eng.describe(), eng.describe()
        out.append({"pe": pe, "f": f, "v": v})
    _same(*out)
