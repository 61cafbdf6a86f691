"""`compute_dos` in gpumd-mi (gpumd_amd/host/run.cpp), in the manner of test_host_corr.py: the run dumps the velocities of every
step in double precision, and mvac.out / dos.out are recomputed in numpy from the dumped frames and the masses of model.xyz's
species -- DOS::process (ring of Nc frames, every sample from the (Nc - 1)-th on a time origin, sum_i m_i v_i(t) v_i(t - l)),
normalize_vac (division by lag 0), find_dos (window (cos(pi l / Nc) + 1) / 2, doubled for l > 0; cosine transform at
omega_k = (k + 1) omega_max / Np; times dt_ps 2 N_g).  Both files have no header: one block of Nc (Np) rows `%g %g %g %g` per group.

Tolerance per printed number: rtol 1e-5 (`%g` prints six digits) plus an absolute term -- mvac 1e-11; dos dt_ps 2 N_g F 1e-11 with
F the sum of the window factors.  Derivation: a dumped velocity carries 1e-15 of itself, a sum of m <= 2e4 terms m 2^-52 = 4e-12
of sum|terms|; the normalised value is a ratio of two such sums, <= 1e-11; a DOS value is dt_ps 2 N_g times a sum of such values
with the window factors as weights (|cos| <= 1).

CPU tier: the host linked against the kernel emulator; one GPU case with the product binary.  The 250-atom PbTe cell is a small
box (the loop that steps on the caller's arrays and samples through nepmi_corr_sample); replicated 2 x 2 x 2 it runs the
device-resident loop."""
import os
import socket
import subprocess

import numpy as np
import pytest

import helpers as H
from test_host_cli import _grouped_workdir
from test_host_corr import DT_FS, DUMP as _DUMP, EMU, EXE, HEAD, _run, _workdir

DUMP = _DUMP.replace("unwrapped_position ", "")
OMEGA = 400.0


@pytest.fixture(scope="module", autouse=True)
def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(H.ROOT, "tests", "emu"), "all"], check=True)


def _expected(frames, interval, nc, omega_max, npts, groups):
    """groups: list of boolean masks -> rows of mvac.out [len(groups) nc, 4], of dos.out [len(groups) npts, 4], the absolute
    tolerances of the dos rows"""
    v = np.array([f["vel"] for f in frames[interval - 1::interval]])  # [samples, n, 3]
    mass = np.array([H.MASS[s] for s in frames[0]["species"]])
    assert len(v) - (nc - 1) >= 1
    dt_ps = DT_FS * interval / 1000.0
    lag = np.arange(nc)
    hann = (np.cos(np.pi * lag / nc) + 1.0) * 0.5
    window = np.where(lag == 0, hann, 2.0 * hann)
    omega = (np.arange(npts) + 1.0) * (omega_max / npts)
    mrows, drows, dtol = [], [], []
    for sel in groups:
        s = np.zeros((nc, 3))
        for t in range(nc - 1, len(v)):
            for l in range(nc):
                s[l] += (mass[:, None] * v[t] * v[t - l])[sel].sum(axis=0)
        mvac = s / s[0]
        scale = dt_ps * 2.0 * sel.sum()
        dos = scale * (np.cos(omega[:, None] * lag[None, :] * dt_ps) @ (window[:, None] * mvac))
        mrows += [[l * dt_ps] + list(mvac[l]) for l in range(nc)]
        drows += [[omega[k]] + list(dos[k]) for k in range(npts)]
        dtol += [scale * window.sum() * 1e-11] * npts
    return np.array(mrows), np.array(drows), np.array(dtol)


def _compare(wd, frames, interval, nc, omega_max, npts, groups, rows=slice(None), drows=slice(None), tag=""):
    em, ed, dtol = _expected(frames, interval, nc, omega_max, npts, groups)
    mv = np.loadtxt(os.path.join(wd, "mvac.out"), ndmin=2)[rows]
    dv = np.loadtxt(os.path.join(wd, "dos.out"), ndmin=2)[drows]
    assert mv.shape == em.shape and dv.shape == ed.shape, (mv.shape, em.shape, dv.shape, ed.shape)
    dm, dd = np.abs(mv - em), np.abs(dv - ed)
    bm, bd = 1e-5 * np.abs(em) + 1e-11, 1e-5 * np.abs(ed) + dtol[:, None]
    print("\n[%s n=%d groups=%d] mvac.out largest deviation / tolerance %.3g, dos.out %.3g"
          % (tag, frames[0]["n"], len(groups), (dm / bm).max(), (dd / bd).max()))
    assert (dm <= bm).all(), (dm / bm).max()
    assert (dd <= bd).all(), (dd / bd).max()
    assert (em[0, 1:] == 1.0).all() and np.abs(ed[:, 1:]).max() > 0.0
    return mv, dv


def _plain(exe, tmp_path, replicate, option="", npts=None, nc=4):
    wd = _workdir(tmp_path, replicate + HEAD + "compute_dos 1 %d %g%s\n" % (nc, OMEGA, option) + DUMP + "run 8\n")
    out = _run(exe, wd)
    assert "Compute phonon DOS." in out and "    sample interval is 1." in out
    assert "    number of correlation steps is %d." % nc in out and "    maximal angular frequency is 400 THz." in out
    if npts is not None:
        assert "    num_dos_points is %d." % npts in out
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 8
    everyone = np.ones(frames[0]["n"], dtype=bool)
    _compare(wd, frames, 1, nc, OMEGA, nc if npts is None else npts, [everyone], tag=os.path.basename(exe))
    return wd


def test_mvac_and_dos_against_the_dumped_frames_on_emulator(tmp_path):
    """2,000 atoms: the device-resident loop"""
    _plain(EMU, tmp_path, "replicate 2 2 2\n")


def test_small_box_run_samples_on_the_callers_arrays_on_emulator(tmp_path):
    """the 250-atom cell: the loop that steps on the caller's arrays (nepmi_corr_sample)"""
    _plain(EMU, tmp_path, "")


def test_num_dos_points_on_emulator(tmp_path):
    wd = _plain(EMU, tmp_path, "", option=" num_dos_points 30", npts=30)
    omega = np.loadtxt(os.path.join(wd, "dos.out"))[:, 0]
    np.testing.assert_allclose(omega, (np.arange(30) + 1.0) * OMEGA / 30, rtol=1e-5)


@pytest.mark.gpu
def test_mvac_and_dos_against_the_dumped_frames_on_gpu(tmp_path):
    _plain(EXE, tmp_path, "replicate 3 3 3\n")


@pytest.mark.parametrize("option", ["group 0 1", "group 0 -1"])
def test_groups_on_emulator(tmp_path, option):
    """grouping method 0 of the fixture is by species (Te 0, Pb 1); a negative group id is every group of the method"""
    body = HEAD + "compute_dos 1 4 %g %s num_dos_points 6\n" % (OMEGA, option) + DUMP + "run 8\n"
    wd, src = _grouped_workdir(tmp_path, "replicate 2 2 2\n" + body)
    out = _run(EMU, wd)
    assert "    grouping method is 0 and group ID is %s." % option.split()[2] in out
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    species = np.array(frames[0]["species"])
    te, pb = species == "Te", species == "Pb"
    if option == "group 0 1":
        _compare(wd, frames, 1, 4, OMEGA, 6, [pb], tag=option)
    else:
        mv, dv = _compare(wd, frames, 1, 4, OMEGA, 6, [te, pb], tag=option)
        assert mv.shape == (8, 4) and dv.shape == (12, 4)
        assert np.abs(mv[3, 1:] - mv[7, 1:]).min() > 1e-4  # the two species do move differently


def test_two_runs_append_on_emulator(tmp_path):
    """a second `run` appends its own blocks to both files and does not inherit the keyword of the first; a third has none"""
    wd = _workdir(tmp_path, HEAD + "compute_dos 1 4 %g\n" % OMEGA + DUMP + "run 8\ncompute_dos 2 2 200 num_dos_points 5\n"
                  + DUMP + "run 8\nrun 4\n")
    _run(EMU, wd)
    frames = H.read_xyz_frames(os.path.join(wd, "d.xyz"))
    assert len(frames) == 16
    everyone = np.ones(frames[0]["n"], dtype=bool)
    assert len(np.loadtxt(os.path.join(wd, "mvac.out"))) == 4 + 2 and len(np.loadtxt(os.path.join(wd, "dos.out"))) == 4 + 5
    _compare(wd, frames[:8], 1, 4, OMEGA, 4, [everyone], rows=slice(0, 4), drows=slice(0, 4), tag="first run")
    _compare(wd, frames[8:], 2, 2, 200.0, 5, [everyone], rows=slice(4, 6), drows=slice(4, 9), tag="second run")


@pytest.mark.parametrize("line, message", [
    ("compute_dos 1 3", "compute_dos should have at least 3 parameters."),
    ("compute_dos 1 3 400 group 0 1 num_dos_points 30 x", "compute_dos has too many parameters."),
    ("compute_dos 1.5 3 400", "sample interval should be an integer."),
    ("compute_dos 0 3 400", "sample interval should be positive."),
    ("compute_dos 1 x 400", "number of correlation steps should be an integer."),
    ("compute_dos 1 0 400", "number of correlation steps should be positive."),
    ("compute_dos 1 3 x", "maximal angular frequency should be a number."),
    ("compute_dos 1 3 -400", "maximal angular frequency should be positive."),
    ("compute_dos 1 3 400 every 4", "Unrecognized argument in compute_dos."),
    ("compute_dos 1 3 400 all_groups 0", "Unrecognized argument in compute_dos."),
    ("compute_dos 1 3 400 group 0", "Not enough arguments for option 'group'."),
    ("compute_dos 1 3 400 group x 0", "Grouping method should be an integer."),
    ("compute_dos 1 3 400 group -1 0", "Grouping method should >= 0."),
    ("compute_dos 1 3 400 group 2 0", "Grouping method should < number of grouping methods."),
    ("compute_dos 1 3 400 group 0 x", "Group ID should be an integer."),
    ("compute_dos 1 3 400 group 0 2", "Group ID should < number of groups."),
    ("compute_dos 1 3 400 num_dos_points", "Not enough arguments for option 'num_dos_points'."),
    ("compute_dos 1 3 400 num_dos_points x", "number of DOS points should be an integer."),
    ("compute_dos 1 3 400 num_dos_points 0", "number of DOS points must be > 0."),
])
def test_input_errors_have_the_reference_messages(tmp_path, line, message):
    wd, _ = _grouped_workdir(tmp_path, HEAD + line + "\nrun 8\n")
    _run(EMU, wd, expect_error=message, args=("--check-input",))


def test_all_groups_is_accepted_at_the_input_check(tmp_path):
    wd, _ = _grouped_workdir(tmp_path, HEAD + "compute_dos 1 3 400 group 1 -1 num_dos_points 7\nrun 8\n")
    out = _run(EMU, wd, args=("--check-input",))
    assert "    grouping method is 1 and group ID is -1." in out and "    num_dos_points is 7." in out


def test_sampling_below_the_nyquist_rate_is_refused(tmp_path):
    """DOS::initialize_parameters (dos.cu:284-288): 1 / dt_ps = 250 < 1000 / pi; 785 = 250 pi - 0.4 passes"""
    wd = _workdir(tmp_path, HEAD + "compute_dos 2 3 1000\nrun 8\n")
    _run(EMU, wd, expect_error="Velocity sampling rate < Nyquist frequency.")
    ok = _workdir(tmp_path / "ok", HEAD + "compute_dos 2 3 785\nrun 8\n")
    _run(EMU, ok)


def test_more_correlation_time_than_steps_is_refused(tmp_path):
    """the reference would divide by zero time origins; refused like compute_msd and compute_sdc"""
    wd = _workdir(tmp_path, HEAD + "compute_dos 2 5 400\nrun 8\n")
    _run(EMU, wd, expect_error="DOS correlation times sampling interval should be <= number of MD steps.")
    ok = _workdir(tmp_path / "ok", HEAD + "compute_dos 2 4 400\nrun 8\n")
    _run(EMU, ok)


def test_multi_rank_launch_refuses(tmp_path):
    wd = _workdir(tmp_path, "replicate 4 2 2\npotential NEP x\nvelocity 300 seed 7\nensemble nve\ntime_step 1\ncompute_dos 1 2 400\nrun 4\n")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   NEPMI_TRANSPORT="tcp", OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([EMU], cwd=wd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode != 0 for p in procs), outs[0][-2000:]
    assert "compute_dos is not available in multi-GPU runs" in outs[0], outs[0][-2000:]
