"""`compute_dos` of gpumd-mi against the reference's own program on the same GPU: oracle/_ref/gpumd_ref (see
test_ref_md_parity.py) and gpumd-mi run ref_compare's `pbte_16k` (16,000 atoms of two masses, velocities from model.xyz) for 60
steps of 1 fs with `compute_dos 2 10 400.0 num_dos_points 20`: 30 samples, 21 time origins, dt_ps = 0.002.  Skipped where the
reference binary is not built.

Row counts and the first column (time, omega): equal as printed.  Values, per printed number (`%g`: six digits, so each of the two
printed numbers carries up to 5e-6 of itself in print quantisation, q below), with r = CASES["pbte_16k"][0] = 1e-6, the case's
relative tolerance on a product of two velocities (the project's existing tolerance, NOT a measurement of this feature):
  mvac.out: a ratio of two such sums, |mvac| <= about 1:  |d| <= 2 r + q;
  dos.out:  dt_ps 2 N times the windowed sum of mvac values, F = the sum of the window factors:  |d| <= dt_ps 2 N F 2 r + q.
Where oracle/_ref/gpumd_ref_mi is built (the reference's own DOS code on this library's forces) it runs too and its deviations
from the reference are printed beside gpumd-mi's: that pair shows what the force path alone contributes.

Measured on an MI355X: every printed value of mvac.out equal to gpumd_ref's (0 of the bound); the largest deviation in
dos.out is 1e-5 (the largest |dos| is 610), 0.76 % of the bound.  gpumd_ref_mi against gpumd_ref: the same figures."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

pytestmark = pytest.mark.gpu

STEPS, INTERVAL, NC, OMEGA, NP = 60, 2, 10, 400.0, 20
Q = 5e-6  # print quantisation of one `%g` number, relative


def _rows(path):
    lines = open(path).read().split("\n")
    lines = [l for l in lines if l.strip()]
    return [l.split()[0] for l in lines], np.array([[float(x) for x in l.split()] for l in lines])


def test_mvac_and_dos_match_reference_gpumd(tmp_path):
    import ref_compare as R
    from test_ref_md_parity import CASES
    if not os.path.exists(R.REF):
        pytest.skip("oracle/_ref/gpumd_ref not built (the reference's sources were not there at build time)")
    assert os.path.exists(R.MI), "gpumd-mi is not built"
    r = CASES["pbte_16k"][0]
    assert r == 1e-6
    exes = [("ref", R.REF), ("mi", R.MI)] + ([("ref_mi", R.REF_MI)] if os.path.exists(R.REF_MI) else [])
    R.FINE = STEPS
    try:
        out = {}
        for tag, exe in exes:
            d = str(tmp_path / tag)
            n = R.case_inputs("pbte_16k", d)
            run_in = os.path.join(d, "run.in")
            text = open(run_in).read()
            assert "\nrun %d" % STEPS in text and "time_step 1\n" in text
            open(run_in, "w").write(text.replace("\nrun ", "\ncompute_dos %d %d %.1f num_dos_points %d\nrun " % (INTERVAL, NC, OMEGA, NP)))
            res, _ = R.run_binary(exe, d, 300.0)
            assert res["rc"] == 0, open(os.path.join(d, "stdout.txt")).read()[-2000:]
            out[tag] = (_rows(os.path.join(d, "mvac.out")), _rows(os.path.join(d, "dos.out")))
    finally:
        R.FINE = 0
    assert n == 16000
    (mt, mr), (dt_, dr) = out["ref"]
    assert mr.shape == (NC, 4) and dr.shape == (NP, 4)
    dt_ps = 1.0 * INTERVAL / 1000.0
    lag = np.arange(NC)
    hann = (np.cos(np.pi * lag / NC) + 1.0) * 0.5
    F = float(np.where(lag == 0, hann, 2.0 * hann).sum())
    b_mvac, b_dos = 2.0 * r, dt_ps * 2.0 * n * F * 2.0 * r
    worst = {}
    for tag in [t for t, _ in exes if t != "ref"]:
        (t1, m1), (t2, d1) = out[tag]
        assert t1 == mt and t2 == dt_, (tag, t1, mt, t2, dt_)  # row counts and the first column, as printed
        dm, dd = np.abs(m1 - mr)[:, 1:], np.abs(d1 - dr)[:, 1:]
        qm, qd = Q * (np.abs(m1) + np.abs(mr))[:, 1:], Q * (np.abs(d1) + np.abs(dr))[:, 1:]
        worst[tag] = (float((dm / (b_mvac + qm)).max()), float((dd / (b_dos + qd)).max()))
        print("\n[%s vs gpumd_ref] mvac.out: max |d| %.3e; dos.out: max |d| %.3e (largest |dos| %.3e); largest |d| / bound: mvac.out %.3g,"
              " dos.out %.3g" % (tag, dm.max(), dd.max(), np.abs(dr[:, 1:]).max(), worst[tag][0], worst[tag][1]))
    (_, m1), (_, d1) = out["mi"]
    assert (np.abs(m1 - mr)[:, 1:] <= b_mvac + Q * (np.abs(m1) + np.abs(mr))[:, 1:]).all(), worst
    assert (np.abs(d1 - dr)[:, 1:] <= b_dos + Q * (np.abs(d1) + np.abs(dr))[:, 1:]).all(), worst
