"""`ensemble npt_ber` in gpumd-mi's run.in (Integrate::parse_ensemble, integrate.cu:631-715, :1107-1154), CPU tier: the host
built against the kernel emulator (tests/emu/gpumd-mi-emu).

  the three forms   `npt_ber T1 T2 Tc p C tau_p` (8 tokens), `... pxx pyy pzz Cxx Cyy Czz tau_p` (12), six pressures + six moduli +
                    tau_p (18) parse and run; the box columns of thermo.out change from row to row, the dump_xyz lattice and
                    restart.xyz carry the box of their step
  invalid forms     the reference's messages"""
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as H

EMU_EXE = os.path.join(H.ROOT, "tests", "emu", "gpumd-mi-emu")
NEP = H.golden("PbTe", "nep.txt")


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(H.ROOT, "tests", "emu"), "all"], check=True)


def _workdir(tmp_path, ensemble_line, orthogonal, pbc="T T T", steps=4, extra=""):
    if orthogonal:  # rock-salt PbTe, 4 x 4 x 4 conventional cells: 26.3 A, above the small-box limit of 22.5 A
        h, typ, x = H.rocksalt_orthogonal((4, 4, 4), rattle=0.02, seed=9)
        n = len(typ)
        lines = ["%d" % n, 'pbc="%s" Lattice="%.10f 0 0 0 %.10f 0 0 0 %.10f" Properties=species:S:1:pos:R:3' % (pbc, h[0], h[4], h[8])]
        lines += ["%s %.12f %.12f %.12f" % ("Te" if typ[i] == 0 else "Pb", x[i], x[n + i], x[2 * n + i]) for i in range(n)]
        (tmp_path / "model.xyz").write_text("\n".join(lines) + "\n")
        head = ""
    else:  # the 250-atom triclinic cell, 2 x 2 x 2
        text = open(H.golden("PbTe", "model.xyz")).read()
        (tmp_path / "model.xyz").write_text(text.replace('pbc="T T T"', 'pbc="%s"' % pbc))
        head = "replicate 2 2 2\n"
    (tmp_path / "run.in").write_text("%spotential %s\nvelocity 300 seed 7\n%s\ntime_step 1\ndump_thermo 1\n%srun %d\n"
                                     % (head, NEP, ensemble_line, extra, steps))
    return str(tmp_path)


FORMS = [("ensemble npt_ber 300 300 100 1 40 100", True, 1),
         ("ensemble npt_ber 300 300 100 0 1 2 40 50 60 100", True, 3),
         ("ensemble npt_ber 300 300 100 0 0 0 0.5 -0.5 1 40 40 40 40 40 40 100", False, 6)]


@pytest.mark.parametrize("line,orthogonal,num_p", FORMS)
def test_npt_ber_forms_parse_and_move_the_box(tmp_path, line, orthogonal, num_p):
    wd = _workdir(tmp_path, line, orthogonal, extra="dump_xyz 2 d.xyz\ndump_restart 4\n")
    out = subprocess.run([EMU_EXE], cwd=wd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "Use NPT ensemble for this run." in out.stdout and "choose the Berendsen method." in out.stdout
    assert "tau_p is 100 time_step." in out.stdout
    th = np.loadtxt(tmp_path / "thermo.out")
    assert th.shape == (4, 18) and np.isfinite(th).all()
    box = th[:, 9:]
    start = H.read_xyz_frames(str(tmp_path / "model.xyz"))[0]["h"]
    h0 = np.asarray(start, dtype=np.float64).reshape(9) * (1 if orthogonal else 2)
    rows = box[:, [0, 3, 6, 1, 4, 7, 2, 5, 8]]  # columns ax ay az bx by bz cx cy cz -> h
    steps = np.abs(np.diff(np.vstack([h0, rows]), axis=0)).max(axis=1)
    print("\n[%d components] largest box component change per step: %s" % (num_p, steps))
    assert (steps > 1e-7).all(), "the box must change on every step"
    if num_p == 1:  # one factor for the three lengths
        r = rows[:, [0, 4, 8]] / h0[[0, 4, 8]]
        assert np.abs(r - r[:, :1]).max() < 1e-12
    if num_p != 6:
        assert (rows[:, [1, 2, 3, 5, 6, 7]] == 0).all()
    else:
        assert np.abs(rows[-1, 1] / h0[1] - rows[-1, 5] / h0[5]) > 1e-9  # the shear targets act
    # the lattice of the dumped frames and of restart.xyz is the box of their step
    frames = open(tmp_path / "d.xyz").read()
    lat = [np.array(m.split(), dtype=float) for m in re.findall(r'Lattice="([^"]*)"', frames)]
    assert len(lat) == 2
    np.testing.assert_allclose(lat[0], box[1], atol=1e-7)
    np.testing.assert_allclose(lat[1], box[3], atol=1e-7)
    rl = np.array(re.findall(r'Lattice="([^"]*)"', open(tmp_path / "restart.xyz").read())[0].split(), dtype=float)
    np.testing.assert_allclose(rl, box[3], rtol=1e-9)


@pytest.mark.parametrize("line,orthogonal,pbc,msg", [
    ("ensemble npt_ber 300 300 100 0 40", True, "T T T", "ensemble npt_ber should have 6, 10, or 16 parameters."),
    ("ensemble npt_ber 300 300 0.5 0 40 100", True, "T T T", "Temperature coupling should >= 1."),
    ("ensemble npt_ber 300 300 100 0 40 0.5", True, "T T T", "Pressure coupling should >= 1."),
    ("ensemble npt_ber 300 300 100 0 -40 100", True, "T T T", "elastic modulus should > 0."),
    ("ensemble npt_ber 300 300 100 0 0 0 40 0 40 100", True, "T T T", "elastic modulus should > 0."),
    ("ensemble npt_ber 300 300 100 x 40 100", True, "T T T", "Pressure should be a number."),
    ("ensemble npt_ber 300 300 100 0 40 100", False, "T T T", "Cannot use triclinic box with only 1 target pressure component."),
    ("ensemble npt_ber 300 300 100 0 0 0 40 40 40 100", False, "T T T", "Cannot use triclinic box with only 3 target pressure components."),
    ("ensemble npt_ber 300 300 100 0 40 100", True, "T T F", "Cannot use isotropic pressure with non-periodic boundary in any direction."),
    ("ensemble npt_ber 300 300 100 0 0 0 0 0 0 40 40 40 40 40 40 100", False, "T F T",
     "Cannot use 6 pressure components with non-periodic boundary in any direction."),
    ("ensemble npt_scr 300 300 100 0 40 100", True, "T T T", "npt_scr is not available"),
    ("ensemble npt_mttk temp 300 300 iso 0 0", True, "T T T", "npt_mttk is not available")])
def test_npt_ber_input_errors(tmp_path, line, orthogonal, pbc, msg):
    wd = _workdir(tmp_path, line, orthogonal, pbc=pbc)
    out = subprocess.run([EMU_EXE, "--check-input"], cwd=wd, capture_output=True, text=True)
    assert out.returncode == 1, out.stdout[-2000:]
    assert "Input Error" in out.stdout and msg in out.stdout, out.stdout[-2000:]


def test_three_components_leave_an_open_direction_alone(tmp_path):
    """cpu_pressure_orthogonal: a direction with pbc = 0 keeps its length"""
    wd = _workdir(tmp_path, "ensemble npt_ber 300 300 100 0 1 2 40 50 60 100", True, pbc="T T F", steps=2)
    out = subprocess.run([EMU_EXE], cwd=wd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    th = np.loadtxt(tmp_path / "thermo.out")
    h0 = H.read_xyz_frames(str(tmp_path / "model.xyz"))[0]["h"]
    assert (th[:, 17] == np.asarray(h0).reshape(9)[8]).all() and (np.abs(np.diff(th[:, 9])) > 1e-7).all()
