"""`ensemble npt_ber` at the MD level against the REFERENCE ITSELF on the same GPU (see test_ref_md_parity.py for the pairing:
oracle/_ref/gpumd_ref is the reference's own gpumd compiled for gfx950, oracle/_ref/gpumd_ref_mi the reference's host over
libnepmi.so): 20 steps, thermo.out every step, velocities from model.xyz.

  pbte_iso     `npt_ber 300 300 100 0 40 1000` on an ORTHOGONAL rock-salt PbTe cell of 13,824 atoms written here -- the golden
               PbTe cell behind ref_compare's pbte_16k is triclinic, and both programs refuse one pressure component on it
               (integrate.cu:665-669)
  carbon_nvt   ref_compare's diamond case (64,000 atoms, orthogonal) with three components
  pbte_16k     ref_compare's triclinic PbTe case with six components and shear targets

gpumd-mi against gpumd_ref: T, K, U and the stresses with the tolerances of test_ref_md_parity.CASES; the box columns within
2 x 20 x max p_coupling [1/GPa] x ap [GPa] (the stress tolerance propagated through mu over 20 steps, margin 2 for the two
programs' independent roundings), as a strain: |dh| <= that x max|h|.  The same inputs through gpumd_ref_mi with
NEPMI_KEEP_LISTS=1 in its environment (its NPT steps keep the Verlet lists): its rows against the reference's, same tolerances."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

pytestmark = pytest.mark.gpu

STEPS = 20
# case: (ensemble line, base case of ref_compare or None, (rtol T/K, rtol U, atol P [GPa]) of test_ref_md_parity.CASES, max p_coupling [1/GPa])
NPT_CASES = {
    "pbte_iso": ("npt_ber 300 300 100 0 40 1000", None, (1e-6, 1e-6, 1e-3), 1.0 / (3 * 1000 * 40.0)),
    "carbon_nvt": ("npt_ber 300 300 100 0 1 2 400 500 600 500", "carbon_nvt", (2e-6, 2e-6, 1e-3), 1.0 / (3 * 500 * 400.0)),
    "pbte_16k": ("npt_ber 300 300 100 0 0 0 0.5 -0.5 1 40 40 40 40 40 40 500", "pbte_16k", (1e-6, 1e-6, 1e-3), 1.0 / (3 * 500 * 40.0)),
}


def _inputs(case, d):
    import ref_compare as R
    line, base, _, _ = NPT_CASES[case]
    if base is not None:
        R.FINE = STEPS
        try:
            R.case_inputs(base, d)
        finally:
            R.FINE = 0
        text = open(os.path.join(d, "run.in")).read()
        text, k = re.subn(r"ensemble [^\n]*\n", "ensemble %s\n" % line, text)
        assert k == 1
    else:
        import shutil
        from gpumd_amd import structures as S
        os.makedirs(d, exist_ok=True)
        a, cells = 6.5704, (12, 12, 12)
        basis = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5], [.5, 0, 0], [0, .5, 0], [0, 0, .5], [.5, .5, .5]]) * a
        spec0 = ["Pb"] * 4 + ["Te"] * 4
        spec, pos = [], []
        for i in range(cells[0]):
            for j in range(cells[1]):
                for k in range(cells[2]):
                    spec += spec0
                    pos.append(basis + np.array([i, j, k]) * a)
        pos = np.concatenate(pos) + np.random.default_rng(11).normal(0.0, 0.02, (len(spec), 3))
        mass = np.array([S.MASS[e] for e in spec])
        vel = S.maxwell_velocities(mass, 300.0, seed=3).reshape(3, -1).T / S.TIME_UNIT
        with open(os.path.join(d, "model.xyz"), "w") as f:
            f.write('%d\npbc="T T T" Lattice="%.12g 0 0 0 %.12g 0 0 0 %.12g" Properties=species:S:1:pos:R:3:vel:R:3\n'
                    % (len(spec), a * cells[0], a * cells[1], a * cells[2]))
            for e, p, v in zip(spec, pos, vel):
                f.write("%s %.12f %.12f %.12f %.15e %.15e %.15e\n" % (e, p[0], p[1], p[2], v[0], v[1], v[2]))
        shutil.copy(os.path.join(R.GOLD, "PbTe", "nep.txt"), os.path.join(d, "nep.txt"))
        text = "potential nep.txt\nensemble %s\ntime_step 1\ndump_thermo 1\nrun %d\n" % (line, STEPS)
    open(os.path.join(d, "run.in"), "w").write(text)


def _compare(tag, b, a, tol, pc_per_gpa):
    rt, ru, ap = tol
    assert a is not None and b is not None and a.shape == b.shape == (STEPS, 18)
    strain = 2 * STEPS * pc_per_gpa * ap
    hscale = np.abs(a[:, 9:]).max()
    moved = np.abs(a[-1, 9:] - a[0, 9:]).max() / hscale
    print("\n[%s] max rel dT %.2e dK %.2e dU %.2e, max |dP| %.2e GPa, box deviation %.2e (strain; tolerance %.2e; the box moved by %.2e)"
          % (tag, np.abs(b[:, 0] / a[:, 0] - 1).max(), np.abs(b[:, 1] / a[:, 1] - 1).max(), np.abs(b[:, 2] / a[:, 2] - 1).max(),
             np.abs(b[:, 3:9] - a[:, 3:9]).max(), np.abs(b[:, 9:] - a[:, 9:]).max() / hscale, strain, moved))
    assert moved > 10 * strain, "the reference's box must move far beyond what the tolerance hides"
    np.testing.assert_allclose(b[:, 0], a[:, 0], rtol=rt)
    np.testing.assert_allclose(b[:, 1], a[:, 1], rtol=rt)
    np.testing.assert_allclose(b[:, 2], a[:, 2], rtol=ru)
    np.testing.assert_allclose(b[:, 3:9], a[:, 3:9], rtol=0, atol=ap)
    assert np.abs(b[:, 9:] - a[:, 9:]).max() <= strain * hscale


@pytest.mark.parametrize("case", sorted(NPT_CASES))
def test_npt_ber_rows_match_reference_gpumd(case, tmp_path, monkeypatch):
    import ref_compare as R
    if not os.path.exists(R.REF):
        pytest.skip("oracle/_ref/gpumd_ref not built (needs the reference sources at build time)")
    assert os.path.exists(R.MI), "gpumd-mi is not built"
    _, _, tol, pc = NPT_CASES[case]
    th = {}
    runs = [("ref", R.REF, False), ("mi", R.MI, False)]
    if os.path.exists(R.REF_MI):
        runs.append(("ref_mi", R.REF_MI, True))
    for tag, exe, keep in runs:
        d = str(tmp_path / tag)
        _inputs(case, d)
        if keep:
            monkeypatch.setenv("NEPMI_KEEP_LISTS", "1")
        res, th[tag] = R.run_binary(exe, d, 300.0)
        monkeypatch.delenv("NEPMI_KEEP_LISTS", raising=False)
        out = open(os.path.join(d, "stdout.txt")).read()
        assert res["rc"] == 0, out[-2000:]
        if tag == "ref_mi":
            assert "through libnepmi (NEP_MI)" in out
    _compare("%s gpumd-mi / gpumd_ref" % case, th["mi"], th["ref"], tol, pc)
    if "ref_mi" in th:
        _compare("%s gpumd_ref_mi with NEPMI_KEEP_LISTS=1 / gpumd_ref" % case, th["ref_mi"], th["ref"], tol, pc)
