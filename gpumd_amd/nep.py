"""Host-side mirror of the reference's NEP potential object (src/force/nep.cuh `class NEP :
public Potential`) on top of the C ABI.  Arrays are torch CUDA tensors in GPUMD's SoA layout:

    position/velocity/force : float64 [3*N]  (x.. | y.. | z..)
    virial                  : float64 [9*N]  planes xx,yy,zz,xy,xz,yz,yx,zx,zy
    potential               : float64 [N];  type: int32 [N];  mass: float64 [N]
    box                     : 9 host floats ax,bx,cx,ay,by,cy,az,bz,cz (Box::cpu_h[0..8])
"""
import ctypes as C
import weakref

import numpy as np

from . import _capi


def _h9(box):
    h = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(9))
    return h, h.ctypes.data_as(_capi.c_dp)


def _pbc3(pbc):
    p = np.ascontiguousarray(np.asarray(pbc, dtype=np.int32).reshape(3))
    return p, p.ctypes.data_as(_capi.c_ip)


class Model:
    """Parsed nep.txt (host only; mirrors the parsing half of NEP::NEP, nep.cu:100-377)."""

    def __init__(self, path, lib=None):
        from . import load_library
        self.lib = lib if lib is not None else load_library()
        self.path = path
        self.handle = self.lib.nepmi_model_load(path.encode())
        if not self.handle:
            raise _capi.NepmiError(-2, self.lib.nepmi_last_error().decode())
        self.info = _capi.NepmiInfo()
        _capi.check(self.lib, self.lib.nepmi_model_info(self.handle, C.byref(self.info)))
        self.symbols = [self.lib.nepmi_model_symbol(self.handle, t).decode() for t in range(self.info.num_types)]

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nepmi_model_free(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


class NEP:
    """One NEP potential instance bound to `n_atoms` atoms on the current HIP device.

    `compute(box, type, position, potential, force, virial)` has the argument meaning of
    Potential::compute (src/force/potential.cuh:37-43): it ADDS to the three output arrays.
    `force_compute` is Force::compute (force.cu:771-855): wrap, zero, compute.
    """

    def __init__(self, model, n_atoms, stream=None, pbc=(1, 1, 1), lib=None):
        import torch
        if isinstance(model, str):
            model = Model(model, lib=lib)
        self.model = model
        self.lib = model.lib
        if lib is None:
            if not torch.cuda.is_available():
                raise RuntimeError("gpumd_amd.NEP needs an MI355X (gfx950) device; there is no CPU fallback")
        self.n = int(n_atoms)
        self.pbc = tuple(int(p) for p in pbc)
        self._stream = stream
        sp = None
        if stream is not None:
            sp = C.c_void_p(stream.cuda_stream)
        elif lib is None:
            sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.handle = self.lib.nepmi_engine_create(model.handle, self.n, sp)
        if not self.handle:
            raise _capi.NepmiError(-5, self.lib.nepmi_last_error().decode())

    # -- helpers -------------------------------------------------------------------------------
    @staticmethod
    def _ptr(t):
        if t is None:
            return None
        if hasattr(t, "data_ptr"):
            return C.c_void_p(t.data_ptr())
        return C.c_void_p(t.ctypes.data)  # numpy (emulator tests only)

    def _ck(self, st):
        return _capi.check(self.lib, st)

    def close(self):
        for c in list(getattr(self, "_correlators", ())):  # (nepmi.h: a correlator goes before its engine)
            c.close()
        if getattr(self, "handle", None):
            self.lib.nepmi_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    # -- the plugin surface --------------------------------------------------------------------
    def compute(self, box, type, position, potential, force, virial):
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        self._ck(self.lib.nepmi_potential_compute(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(position), self._ptr(potential),
            self._ptr(force), self._ptr(virial)))

    def compute_levels(self, box, pbc, n, type, position, level, potential, force, virial):
        """Potential::compute on a local (owned + ghost) system; see nepmi_potential_compute_levels."""
        _, hp = _h9(box)
        _, pp = _pbc3(pbc)
        self._ck(self.lib.nepmi_potential_compute_levels(
            self.handle, hp, pp, int(n), self._ptr(type), self._ptr(position), self._ptr(level),
            self._ptr(potential), self._ptr(force), self._ptr(virial)))

    def compute_levels_begin(self, box, pbc, n, type, position, level, potential, force, virial):
        """First half (owned atoms final, ghosts in flight) -> True if interior work was enqueued."""
        _, hp = _h9(box)
        _, pp = _pbc3(pbc)
        return self._ck(self.lib.nepmi_potential_compute_levels_begin(
            self.handle, hp, pp, int(n), self._ptr(type), self._ptr(position), self._ptr(level),
            self._ptr(potential), self._ptr(force), self._ptr(virial))) == 1

    def compute_levels_end(self, box, pbc, n, type, position, level, potential, force, virial):
        _, hp = _h9(box)
        _, pp = _pbc3(pbc)
        self._ck(self.lib.nepmi_potential_compute_levels_end(
            self.handle, hp, pp, int(n), self._ptr(type), self._ptr(position), self._ptr(level),
            self._ptr(potential), self._ptr(force), self._ptr(virial)))

    def set_external_skin(self, on=True):
        self._ck(self.lib.nepmi_engine_set_external_skin(self.handle, 1 if on else 0))

    def set_unwrapped(self, unwrapped=None):
        """Atom::unwrapped_position: a [3N] f64 array that every first half-step adds its drift to (None: off)."""
        self._unwrapped = unwrapped  # keep the storage alive while the engine points at it
        self._ck(self.lib.nepmi_engine_set_unwrapped(self.handle, self._ptr(unwrapped) if unwrapped is not None else None))

    def attach(self, corr):
        """The run_* methods sample `corr` (a Correlator, an RDF or an ADF of this engine) every corr.interval completed steps."""
        if isinstance(corr, ARDF):
            self._ck(self.lib.nepmi_ardf_attach(self.handle, corr.handle))
        elif isinstance(corr, OrientOrder):
            self._ck(self.lib.nepmi_orient_attach(self.handle, corr.handle))
        elif isinstance(corr, ADF):
            self._ck(self.lib.nepmi_adf_attach(self.handle, corr.handle))
        elif isinstance(corr, RDF):
            self._ck(self.lib.nepmi_rdf_attach(self.handle, corr.handle))
        else:
            self._ck(self.lib.nepmi_corr_attach(self.handle, corr.handle))

    def detach(self, corr):
        if isinstance(corr, ARDF):
            self._ck(self.lib.nepmi_ardf_detach(self.handle, corr.handle))
        elif isinstance(corr, OrientOrder):
            self._ck(self.lib.nepmi_orient_detach(self.handle, corr.handle))
        elif isinstance(corr, ADF):
            self._ck(self.lib.nepmi_adf_detach(self.handle, corr.handle))
        elif isinstance(corr, RDF):
            self._ck(self.lib.nepmi_rdf_detach(self.handle, corr.handle))
        else:
            self._ck(self.lib.nepmi_corr_detach(self.handle, corr.handle))

    def invalidate(self):
        self._ck(self.lib.nepmi_engine_invalidate(self.handle))

    def force_compute(self, box, type, position, potential, force, virial, n=None):
        """n: number of atoms in the arrays (default: the capacity the engine was created with)."""
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        self._ck(self.lib.nepmi_force_compute(
            self.handle, hp, pp, self.n if n is None else int(n), self._ptr(type), self._ptr(position), self._ptr(potential),
            self._ptr(force), self._ptr(virial)))

    def apply_pbc(self, box, position):
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        self._ck(self.lib.nepmi_apply_pbc(self.handle, hp, pp, self.n, self._ptr(position)))

    def zero_properties(self, potential, force, virial):
        """initialize_properties (force.cu:314-333)."""
        self._ck(self.lib.nepmi_zero_properties(self.handle, self.n, self._ptr(potential), self._ptr(force),
                                                self._ptr(virial)))

    def average_properties(self, denominator, potential, force, virial):
        """gpu_average_properties (force.cu:461-480): the closing division of the "average" multi-potential mode."""
        self._ck(self.lib.nepmi_average_properties(self.handle, self.n, float(denominator), self._ptr(potential),
                                                   self._ptr(force), self._ptr(virial)))

    def vv_step1(self, dt, mass, force, position, velocity):
        self._ck(self.lib.nepmi_vv_step1(self.handle, self.n, float(dt), self._ptr(mass), self._ptr(force),
                                         self._ptr(position), self._ptr(velocity)))

    def vv_step2(self, dt, mass, force, velocity):
        self._ck(self.lib.nepmi_vv_step2(self.handle, self.n, float(dt), self._ptr(mass), self._ptr(force),
                                         self._ptr(velocity)))

    def find_thermo(self, volume, mass, potential, velocity, virial, thermo8):
        self._ck(self.lib.nepmi_find_thermo(self.handle, self.n, float(volume), self._ptr(mass),
                                            self._ptr(potential), self._ptr(velocity), self._ptr(virial),
                                            self._ptr(thermo8)))

    def run_nve(self, box, type, mass, dt, nsteps, position, velocity, potential, force, virial,
                thermo_every=0):
        """Run::perform_a_run for `ensemble nve` -> thermo array [(nsteps // thermo_every), 8] (host)."""
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        nrec = (nsteps // thermo_every) if thermo_every > 0 else 0
        th = np.zeros((max(nrec, 1), 8))
        self._ck(self.lib.nepmi_run_nve(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(mass), float(dt), int(nsteps),
            self._ptr(position), self._ptr(velocity), self._ptr(potential), self._ptr(force),
            self._ptr(virial), int(thermo_every), th.ctypes.data_as(_capi.c_dp)))
        return th[:nrec]

    def run_nvt_ber(self, box, type, mass, dt, nsteps, t1, t2, t_coup, position, velocity, potential, force,
                    virial, thermo_every=0):
        """`ensemble nvt_ber T1 T2 T_coup` (Ensemble_BER) -> thermo array like run_nve."""
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        nrec = (nsteps // thermo_every) if thermo_every > 0 else 0
        th = np.zeros((max(nrec, 1), 8))
        self._ck(self.lib.nepmi_run_nvt_ber(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(mass), float(dt), int(nsteps), float(t1),
            float(t2), float(t_coup), self._ptr(position), self._ptr(velocity), self._ptr(potential),
            self._ptr(force), self._ptr(virial), int(thermo_every), th.ctypes.data_as(_capi.c_dp)))
        return th[:nrec]

    @staticmethod
    def _pressure6(p_target, p_coupling):
        """1, 3 or 6 target pressures and couplings (natural units; Voigt xx yy zz yz xz xy for 6) -> num_p and two 6-arrays"""
        pt = np.atleast_1d(np.asarray(p_target, dtype=np.float64)).reshape(-1)
        pc = np.atleast_1d(np.asarray(p_coupling, dtype=np.float64)).reshape(-1)
        if len(pt) != len(pc) or len(pt) not in (1, 3, 6):
            raise ValueError("p_target and p_coupling need 1, 3 or 6 components each")
        p6, c6 = np.zeros(6), np.zeros(6)
        p6[:len(pt)], c6[:len(pc)] = pt, pc
        return len(pt), p6, c6

    def berendsen_pressure(self, box, p_target, p_coupling, thermo8, position):
        """The barostat step of `ensemble npt_ber` (Ensemble_BER::compute2, type 11) for a host that steps by hand: from
        find_thermo's row `thermo8` (device) the box is scaled IN PLACE (`box`: a writable float64 numpy array of 9) and the
        positions with it; no wrap."""
        num_p, p6, c6 = self._pressure6(p_target, p_coupling)
        h, hp = _h9(box)
        self._ck(self.lib.nepmi_berendsen_pressure(
            self.handle, self.n, num_p, p6.ctypes.data_as(_capi.c_dp), c6.ctypes.data_as(_capi.c_dp), self._ptr(thermo8),
            hp, self._ptr(position)))
        np.asarray(box).reshape(-1)[:9] = h

    def run_npt_ber(self, box, type, mass, dt, nsteps, t1, t2, t_coup, p_target, p_coupling, position, velocity, potential,
                    force, virial, thermo_every=0):
        """`ensemble npt_ber T1 T2 T_coup ...` (Ensemble_BER with the Berendsen barostat; p_target / p_coupling: 1, 3 or 6
        components in natural units, p_coupling = 1 / (3 tau_p C)) -> (thermo rows like run_nve, box rows [records, 9]: the box
        after each record step's scaling).  `box` (a writable float64 numpy array of 9) is updated in place to the final box."""
        num_p, p6, c6 = self._pressure6(p_target, p_coupling)
        h, hp = _h9(box)
        if h is box or np.shares_memory(h, np.asarray(box)):
            h = h.copy()
            hp = h.ctypes.data_as(_capi.c_dp)
        _, pp = _pbc3(self.pbc)
        nrec = (nsteps // thermo_every) if thermo_every > 0 else 0
        th = np.zeros((max(nrec, 1), 8))
        bx = np.zeros((max(nrec, 1), 9))
        self._ck(self.lib.nepmi_run_npt_ber(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(mass), float(dt), int(nsteps), float(t1),
            float(t2), float(t_coup), num_p, p6.ctypes.data_as(_capi.c_dp), c6.ctypes.data_as(_capi.c_dp),
            self._ptr(position), self._ptr(velocity), self._ptr(potential), self._ptr(force), self._ptr(virial),
            int(thermo_every), th.ctypes.data_as(_capi.c_dp), bx.ctypes.data_as(_capi.c_dp)))
        np.asarray(box).reshape(-1)[:9] = h
        return th[:nrec], bx[:nrec]

    def set_keep_lists_on_box_change(self, on=True):
        """per-call force evaluations keep the Verlet lists across a box change (re-metric; the skin rule decides about rebuilds)"""
        self.set_option("keep_lists_on_box_change", 1 if on else 0)

    NHC_STATE_SIZE = 13

    def nhc_init(self, temperature, t_coup, dt, chain_state):
        """Ensemble_NHC constructor: chain_state = NHC_STATE_SIZE doubles of device memory."""
        self._ck(self.lib.nepmi_nhc_init(self.handle, self.n, float(temperature), float(t_coup), float(dt),
                                         self._ptr(chain_state)))

    def nhc_half_step(self, temperature, dt, thermo8, chain_state, velocity):
        self._ck(self.lib.nepmi_nhc_half_step(self.handle, self.n, float(temperature), float(dt),
                                              self._ptr(thermo8), self._ptr(chain_state), self._ptr(velocity)))

    def run_nvt_nhc(self, box, type, mass, dt, nsteps, t1, t2, t_coup, position, velocity, potential, force,
                    virial, thermo_every=0):
        """`ensemble nvt_nhc T1 T2 T_coup` (Ensemble_NHC) -> thermo array like run_nve."""
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        nrec = (nsteps // thermo_every) if thermo_every > 0 else 0
        th = np.zeros((max(nrec, 1), 8))
        self._ck(self.lib.nepmi_run_nvt_nhc(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(mass), float(dt), int(nsteps), float(t1),
            float(t2), float(t_coup), self._ptr(position), self._ptr(velocity), self._ptr(potential),
            self._ptr(force), self._ptr(virial), int(thermo_every), th.ctypes.data_as(_capi.c_dp)))
        return th[:nrec]

    def bdp_seed(self, seed):
        self._ck(self.lib.nepmi_bdp_seed(self.handle, int(seed)))

    def bdp_scale(self, temperature, t_coup, thermo8, velocity):
        self._ck(self.lib.nepmi_bdp_scale(self.handle, self.n, float(temperature), float(t_coup),
                                          self._ptr(thermo8), self._ptr(velocity)))

    def run_nvt_bdp(self, box, type, mass, dt, nsteps, t1, t2, t_coup, position, velocity, potential, force,
                    virial, thermo_every=0):
        """`ensemble nvt_bdp T1 T2 T_coup` (Ensemble_BDP) -> thermo array like run_nve."""
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        nrec = (nsteps // thermo_every) if thermo_every > 0 else 0
        th = np.zeros((max(nrec, 1), 8))
        self._ck(self.lib.nepmi_run_nvt_bdp(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(mass), float(dt), int(nsteps), float(t1),
            float(t2), float(t_coup), self._ptr(position), self._ptr(velocity), self._ptr(potential),
            self._ptr(force), self._ptr(virial), int(thermo_every), th.ctypes.data_as(_capi.c_dp)))
        return th[:nrec]

    def lan_seed(self, seed):
        """seed of the per-atom Langevin generators (the reference takes rand()); the next half-step initialises them"""
        self._ck(self.lib.nepmi_lan_seed(self.handle, int(seed)))

    def lan_half_step(self, temperature, t_coup, mass, velocity):
        """integrate_nvt_lan_half (Ensemble_LAN): Langevin kick of every atom + removal of the centre-of-mass velocity"""
        self._ck(self.lib.nepmi_lan_half_step(self.handle, self.n, float(temperature), float(t_coup), self._ptr(mass),
                                              self._ptr(velocity)))

    def run_nvt_lan(self, box, type, mass, dt, nsteps, t1, t2, t_coup, position, velocity, potential, force,
                    virial, thermo_every=0):
        """`ensemble nvt_lan T1 T2 T_coup` (Ensemble_LAN) -> thermo array like run_nve."""
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        nrec = (nsteps // thermo_every) if thermo_every > 0 else 0
        th = np.zeros((max(nrec, 1), 8))
        self._ck(self.lib.nepmi_run_nvt_lan(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(mass), float(dt), int(nsteps), float(t1),
            float(t2), float(t_coup), self._ptr(position), self._ptr(velocity), self._ptr(potential),
            self._ptr(force), self._ptr(virial), int(thermo_every), th.ctypes.data_as(_capi.c_dp)))
        return th[:nrec]

    def run_nvt_bao(self, box, type, mass, dt, nsteps, t1, t2, t_coup, position, velocity, potential, force,
                    virial, thermo_every=0):
        """`ensemble nvt_bao T1 T2 T_coup` (Ensemble_BAO, BAOAB Langevin) -> thermo array like run_nve."""
        _, hp = _h9(box)
        _, pp = _pbc3(self.pbc)
        nrec = (nsteps // thermo_every) if thermo_every > 0 else 0
        th = np.zeros((max(nrec, 1), 8))
        self._ck(self.lib.nepmi_run_nvt_bao(
            self.handle, hp, pp, self.n, self._ptr(type), self._ptr(mass), float(dt), int(nsteps), float(t1),
            float(t2), float(t_coup), self._ptr(position), self._ptr(velocity), self._ptr(potential),
            self._ptr(force), self._ptr(virial), int(thermo_every), th.ctypes.data_as(_capi.c_dp)))
        return th[:nrec]

    # -- diagnostics ---------------------------------------------------------------------------
    def neighbors(self, which, nn, nl, ld):
        return self._ck(self.lib.nepmi_neighbors_export(self.handle, int(which), self._ptr(nn), self._ptr(nl), int(ld)))

    def descriptors(self, q, fp):
        self._ck(self.lib.nepmi_descriptors_export(self.handle, self._ptr(q), self._ptr(fp)))

    def stats(self, with_lists=False):
        st = _capi.NepmiStats()
        self._ck(self.lib.nepmi_engine_stats(self.handle, 1 if with_lists else 0, C.byref(st)))
        return st

    def set_timing(self, on=True):
        """False/0 off, True/1 every kernel, 2 the force-assembly kernel only (see include/nepmi.h)."""
        self._ck(self.lib.nepmi_engine_set_timing(self.handle, int(on)))

    def set_option(self, name, value):
        """experiment / test switches by name (nepmi_engine_set_option; include/nepmi.h lists them)"""
        self._ck(self.lib.nepmi_engine_set_option(self.handle, name.encode(), float(value)))

    def set_tiles(self, mode=-1):
        """0/False: no LDS-window kernels; 1: radial pass only; 2/True: radial pass + force assembly;
        -1: chosen by the engine (times modes 2 and 1 once)."""
        mode = 2 if mode is True else 0 if mode is False else int(mode)
        self.set_option("tiles", mode)

    def set_win_lanes(self, lanes=0):
        """lanes per atom of the LDS-window kernels: 0 = by the number of bricks, or 1 / 2 / 4"""
        self.set_option("win_lanes", int(lanes))

    def set_force_form(self, mode=-1):
        """force assembly: -1 run loops scatter / per-call gather (default), 0 gather everywhere, 1 scatter wherever it applies
        (nepmi_engine_set_force_form)"""
        self._ck(self.lib.nepmi_engine_set_force_form(self.handle, int(mode)))

    def set_radial_mask(self, on=True):
        """scatter-form loop steps: inside bits over the packed Verlet words instead of a compacted radial list
        (option "radial_mask")"""
        self.set_option("radial_mask", 1 if on else 0)

    def set_radial_sync(self, on=True):
        """scatter-form loop steps: the radial list as wave-synchronous words (default) or the slot-major compact list
        (option "radial_sync")"""
        self.set_option("radial_sync", 1 if on else 0)

    def set_scatter_guard(self, ev_per_angstrom=64.0, hard_factor=0.0):
        """guard band of the scatter-form force assembly per pair half (test hook: options "scatter_guard", "scatter_guard_hard")"""
        self.set_option("scatter_guard", float(ev_per_angstrom))
        self.set_option("scatter_guard_hard", float(hard_factor))

    def set_virial_mode(self, mode=0):
        """per-call evaluations: 0 per-atom virials in the reference's attribution (default), 1 only the total has to be right
        (the scatter form of the force assembly where it applies): nepmi_engine_set_virial_mode"""
        self._ck(self.lib.nepmi_engine_set_virial_mode(self.handle, int(mode)))

    def set_brick_force(self, on=True):
        """fused angular kernel + scatter-form force assembly as ONE kernel per brick (default where it applies) or separately
        (option "brick_force")"""
        self.set_option("brick_force", 1 if on else 0)

    def set_angular_fused(self, on=True):
        """angular descriptor + ANN + partial angular forces in one kernel (default) or as separate kernels
        (option "angular_fused")"""
        self.set_option("angular_fused", 1 if on else 0)

    def set_angular_pair_trip(self, on=True):
        """record loops of the fused angular kernel in trips of two records, one radial evaluation per record and lane pair
        (default), or one record per trip on both lanes (option "angular_pair_trip"); bit-identical results"""
        self.set_option("angular_pair_trip", 1 if on else 0)

    def set_angular_flat_tables(self, on=True):
        """per-atom phases of the fused angular kernel on the flat-table LDS image (default: bias and output weight as one
        read, radial coefficient rows in whole 16-byte groups per lane) or on the first image (option "angular_flat_tables");
        bit-identical results"""
        self.set_option("angular_flat_tables", 1 if on else 0)

    def set_lean_list_walks(self, on=True):
        """the per-step radial list walked without work its sums never use (default: list A of two-type shapes evaluated once
        per candidate in the radial pass, no weights or control flow for the padding places of the wave-synchronous words in
        the scatter form) or by the former bodies (option "lean_list_walks"); bit-identical results"""
        self.set_option("lean_list_walks", 1 if on else 0)

    def set_angular_only_list_a(self, on=True):
        """two-type shapes: the members of list A stand in the two type-pure streams of the static window layout as well and
        the radial pass walks list A for the angular membership alone (default), or list A carries its own radial work
        (option "angular_only_list_a"); radial sums, energies and forces bit-identical, the scatter form's float virial to
        its last bits (the per-step compact list leaves in another order).  Takes effect at the next list rebuild, which it
        asks for."""
        self.set_option("angular_only_list_a", 1 if on else 0)

    def set_rebuild_fast_pack(self, on=True):
        """the list rebuild with the neighbours' types handed from the list builder to the packing of the list words, the
        bricks' statistics by a wavefront per brick and one host look behind the builder (default), or the former kernels and
        looks (option "rebuild_fast_pack"); the same list words, bit-identical results.  Takes effect at the next rebuild."""
        self.set_option("rebuild_fast_pack", 1 if on else 0)

    def set_fold_seam(self, on=True):
        """single-domain NVE run loops in the scatter form: the fold of the window sums inside the integrator pass behind it
        (default), or as a launch of its own (option "fold_seam"); bit-identical results (a window sum too large for the seam
        sends a step back to the separate kernels without a list rebuild: include/nepmi.h)"""
        self.set_option("fold_seam", 1 if on else 0)

    def describe(self):
        """the kernel forms the last force evaluation ran (counted rules of the engine, as text)"""
        import ctypes as C
        buf = C.create_string_buffer(1024)
        n = self.lib.nepmi_engine_describe(self.handle, buf, 1024)
        if n < 0:
            self._ck(n)
        return buf.value.decode()

    def set_stepwise_loops(self, on=True):
        """test hook: run_nvt_lan / run_nvt_bao as the stepwise sequence on the caller's arrays"""
        self.set_option("stepwise_loops", int(bool(on)))

    def set_win_static(self, on=True):
        """static window layout of the one-lane window kernels (default on); False = the scanned layout"""
        self.set_option("win_static", int(bool(on)))

    def set_mfma(self, on=True):
        """False / 0: per-atom ANN kernel; True / 1 (default): descriptor + ANN fused where the shape allows it, else the
        matrix-core ANN kernel; 2: the matrix-core kernel wherever it applies (no fusion)"""
        self.set_option("mfma", int(on))

    def set_temperature(self, temperature):
        """The `temperature` argument of NEP::compute(temperature, ...) for nep4[_zbl]_temperature models (no effect on
        plain models); stays in force for later compute / run calls."""
        self._ck(self.lib.nepmi_engine_set_temperature(self.handle, float(temperature)))

    def set_angular_recompute(self, mode=-1):
        self.set_option("angular_recompute", int(mode))

    def set_generic(self, on=True):
        self.set_option("generic", 1 if on else 0)


def dos_from_mvac(lib, sums, group_size, dt_ps, omega_max, num_dos_points=None):
    """nepmi_dos_from_mvac on host arrays: sums [G, 3, Nc], group_size [G] -> (omega [Np], mvac [G, 3, Nc], dos [G, 3, Np])"""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    ng, _, nc = sums.shape
    npts = nc if num_dos_points is None else int(num_dos_points)
    size = np.ascontiguousarray(group_size, dtype=np.int64)
    if sums.shape[1] != 3 or size.shape != (ng,):
        raise ValueError("sums: [G, 3, Nc], group_size: [G]")
    mvac, dos = np.zeros((ng, 3, nc)), np.zeros((ng, 3, max(npts, 0)))
    _capi.check(lib, lib.nepmi_dos_from_mvac(sums.ctypes.data_as(_capi.c_dp), ng, nc, size.ctypes.data_as(C.POINTER(_capi.c_i64)),
                                             float(dt_ps), float(omega_max), npts, mvac.ctypes.data_as(_capi.c_dp),
                                             dos.ctypes.data_as(_capi.c_dp)))
    d_omega = float(omega_max) / npts
    return d_omega + np.arange(npts) * d_omega, mvac, dos  # (as find_dos forms omega_k)


class Correlator:
    """Time-correlation sums (nepmi_corr_*): quantity "msd" (unwrapped positions), "vac" (velocities) or "mvac" (velocities, every
    atom weighted by `weights`: n floats in the caller's atom order, the masses), `num_corr` lags of `interval` steps, optionally per
    group (`group_of_atom`: n ints in the caller's atom order, -1 = not sampled).

    Attach it to the engine (`engine.attach(c)`) and the run_* methods sample it on the device; a host that steps by hand calls
    `sample(q)` with q = [3N] f64 on the device.  `read()` -> (sums [num_groups, 3, num_corr], num_origins, num_samples); the
    reader normalises: MSD_l = sums / (atoms * origins).  An "mvac" correlator also has `dos(dt_ps, omega_max)`."""
    QUANTITIES = {"msd": 0, "vac": 1, "mvac": 2}

    def __init__(self, engine, quantity, interval, num_corr, group_of_atom=None, num_groups=1, weights=None):
        self.engine = engine
        self.lib = engine.lib
        self.quantity = self.QUANTITIES[quantity] if isinstance(quantity, str) else int(quantity)
        self.interval, self.num_corr, self.num_groups = int(interval), int(num_corr), int(num_groups)
        gp = None
        if group_of_atom is not None:
            g = np.ascontiguousarray(np.asarray(group_of_atom), dtype=np.int32)
            if g.shape != (engine.n,):
                raise ValueError("group_of_atom: one int per atom")
            gp = g.ctypes.data_as(_capi.c_ip)
            self.group_size = np.array([(g == k).sum() for k in range(self.num_groups)], dtype=np.int64)
        else:
            self.group_size = np.array([engine.n] + [0] * (self.num_groups - 1), dtype=np.int64)
        out = C.c_void_p()
        if weights is None:  # (quantity 2 without weights: the library's refusal)
            _capi.check(self.lib, self.lib.nepmi_corr_create(engine.handle, self.quantity, engine.n, self.interval, self.num_corr, gp,
                                                             self.num_groups, C.byref(out)))
        else:
            w = np.ascontiguousarray(np.asarray(weights), dtype=np.float64)
            if w.shape != (engine.n,):
                raise ValueError("weights: one float per atom")
            _capi.check(self.lib, self.lib.nepmi_corr_create_weighted(engine.handle, self.quantity, engine.n, self.interval,
                                                                      self.num_corr, gp, self.num_groups,
                                                                      w.ctypes.data_as(_capi.c_dp), C.byref(out)))
        self.handle = out
        if not hasattr(engine, "_correlators"):
            engine._correlators = weakref.WeakSet()
        engine._correlators.add(self)

    def sample(self, q):
        _capi.check(self.lib, self.lib.nepmi_corr_sample(self.handle, NEP._ptr(q)))

    def read(self):
        sums = np.zeros((self.num_groups, 3, self.num_corr))
        no, ns = C.c_int64(0), C.c_int64(0)
        _capi.check(self.lib, self.lib.nepmi_corr_read(self.handle, sums.ctypes.data_as(_capi.c_dp), C.byref(no), C.byref(ns)))
        return sums, int(no.value), int(ns.value)

    def dos(self, dt_ps, omega_max, num_dos_points=None):
        """"mvac" only: -> (omega [Np], mvac [num_groups, 3, num_corr] normalised to lag 0, dos [num_groups, 3, Np]) from the sums so
        far (nepmi_dos_from_mvac); dt_ps = the time between two samples in ps, Np = num_dos_points or num_corr."""
        if self.quantity != 2:
            raise ValueError("dos: an \"mvac\" correlator only")
        sums = self.read()[0]
        return dos_from_mvac(self.lib, sums, self.group_size, dt_ps, omega_max, num_dos_points)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nepmi_corr_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


class RDF:
    """Radial distribution function as integer pair counts (nepmi_rdf_*): `num_bins` bins up to `rc`, one row per type pair
    (a <= b; a outer, b from a), `type_of_atom`: n ints in the caller's atom order, 0 .. num_types - 1.

    Attach it to the engine (`engine.attach(r)`) and the run_* methods sample it on the device every `interval` steps; a host
    that steps by hand calls `sample(pos, h, pbc)` with pos = [3N] f64 on the device.  `read()` -> (counts [P, num_bins] uint64,
    vsum [P, num_bins] = sum over the samples of count * volume, num_samples); `g()` normalises as the reference's rdf.out.
    `lds_budget` (bytes) moves the threshold between the two forms of the pair kernel; `form` is 1 (tables in LDS) or 2."""

    def __init__(self, engine, rc, num_bins, interval, type_of_atom, num_types, lds_budget=None):
        self.engine = engine
        self.lib = engine.lib
        self.rc, self.num_bins, self.interval, self.num_types = float(rc), int(num_bins), int(interval), int(num_types)
        self.num_pairs = self.num_types * (self.num_types + 1) // 2
        t = np.ascontiguousarray(np.asarray(type_of_atom), dtype=np.int32)
        if t.shape != (engine.n,):
            raise ValueError("type_of_atom: one int per atom")
        out = C.c_void_p()
        _capi.check(self.lib, self.lib.nepmi_rdf_create(engine.handle, engine.n, self.rc, self.num_bins, self.interval,
                                                        t.ctypes.data_as(_capi.c_ip), self.num_types, C.byref(out)))
        self.handle = out
        if not hasattr(engine, "_correlators"):
            engine._correlators = weakref.WeakSet()
        engine._correlators.add(self)
        if lds_budget is not None:
            _capi.check(self.lib, self.lib.nepmi_rdf_set_lds_budget(self.handle, int(lds_budget)))

    @property
    def form(self):
        return _capi.check(self.lib, self.lib.nepmi_rdf_form(self.handle))

    def sample(self, pos, h, pbc):
        _, hp = _h9(h)
        _, pp = _pbc3(pbc)
        _capi.check(self.lib, self.lib.nepmi_rdf_sample(self.handle, NEP._ptr(pos), hp, pp))

    def read(self):
        counts = np.zeros((self.num_pairs, self.num_bins), dtype=np.uint64)
        vsum = np.zeros((self.num_pairs, self.num_bins))
        ns = C.c_int64(0)
        _capi.check(self.lib, self.lib.nepmi_rdf_read(self.handle, counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      vsum.ctypes.data_as(_capi.c_dp), C.byref(ns)))
        return counts, vsum, int(ns.value)

    def g(self, num_atoms_of_type, num_repeats=None):
        """-> (r [num_bins], total [num_bins], partial [P, num_bins]), rdf.cu:107-112 and :236-243 on the integer sums;
        num_repeats defaults to the samples taken."""
        _, vsum, ns = self.read()
        return rdf_normalise(vsum, self.rc, num_atoms_of_type, ns if num_repeats is None else num_repeats)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nepmi_rdf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


class ARDF:
    """Angular-resolved RDF as integer pair counts (nepmi_ardf_*): `num_r_bins` bins up to `rc`, `num_theta_bins` bins of the
    azimuth of the pair vector in the xy plane; column 0 is the total, then one column per ordered type pair of `pairs`
    (up to six (a, b)).  `type_of_atom`: n ints in the caller's atom order, 0 .. num_types - 1 (not needed without pairs).

    `attach()` and the engine's run_* methods sample it on the device every `interval` steps; a host that steps by hand calls
    `sample(pos, h, pbc)` with pos = [3N] f64 on the device.  `read()` -> (counts [C, R, T] uint64, vsum [C, R, T] = sum over
    the samples of count * volume, num_samples); `g(n_of_type)` normalises as the reference's angular_rdf.out.
    `set_lds_budget(bytes)` moves the threshold between the two forms of the pair kernel; `form` is 1 (tables in LDS) or 2."""

    def __init__(self, engine, rc, num_r_bins, num_theta_bins, interval, type_of_atom=None, num_types=1, pairs=()):
        self.engine = engine
        self.lib = engine.lib
        self.rc, self.num_r_bins, self.num_theta_bins = float(rc), int(num_r_bins), int(num_theta_bins)
        self.interval, self.num_types = int(interval), int(num_types)
        self.pairs = [(int(a), int(b)) for a, b in pairs]
        self.num_columns = 1 + len(self.pairs)
        tp = None
        if type_of_atom is not None:
            t = np.ascontiguousarray(np.asarray(type_of_atom), dtype=np.int32)
            if t.shape != (engine.n,):
                raise ValueError("type_of_atom: one int per atom")
            tp = t.ctypes.data_as(_capi.c_ip)
        pt = np.ascontiguousarray(np.asarray(self.pairs, dtype=np.int32).reshape(-1))
        out = C.c_void_p()
        _capi.check(self.lib, self.lib.nepmi_ardf_create(engine.handle, engine.n, self.rc, self.num_r_bins, self.num_theta_bins,
                                                         self.interval, tp, self.num_types, len(self.pairs),
                                                         pt.ctypes.data_as(_capi.c_ip) if len(self.pairs) else None, C.byref(out)))
        self.handle = out
        if not hasattr(engine, "_correlators"):
            engine._correlators = weakref.WeakSet()
        engine._correlators.add(self)

    @property
    def form(self):
        return _capi.check(self.lib, self.lib.nepmi_ardf_form(self.handle))

    def set_lds_budget(self, nbytes):
        _capi.check(self.lib, self.lib.nepmi_ardf_set_lds_budget(self.handle, int(nbytes)))

    def attach(self):
        self.engine.attach(self)

    def detach(self):
        self.engine.detach(self)

    def sample(self, pos, h, pbc):
        _, hp = _h9(h)
        _, pp = _pbc3(pbc)
        _capi.check(self.lib, self.lib.nepmi_ardf_sample(self.handle, NEP._ptr(pos), hp, pp))

    def read(self):
        shape = (self.num_columns, self.num_r_bins, self.num_theta_bins)
        counts = np.zeros(shape, dtype=np.uint64)
        vsum = np.zeros(shape)
        ns = C.c_int64(0)
        _capi.check(self.lib, self.lib.nepmi_ardf_read(self.handle, counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       vsum.ctypes.data_as(_capi.c_dp), C.byref(ns)))
        return counts, vsum, int(ns.value)

    def g(self, num_atoms_of_type, num_repeats=None):
        """-> (r [R], theta [T], g [C, R, T]): angular_rdf.cu:124-129 and :605-644 on the integer sums; num_repeats defaults to
        the samples taken."""
        _, vsum, ns = self.read()
        return ardf_normalise(vsum, self.rc, self.pairs, num_atoms_of_type, ns if num_repeats is None else num_repeats)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nepmi_ardf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


ARDF_PI = 3.14159265358979  # the reference's PI (utilities/common.cuh): the bin edges and the printed angles are formed with it


def ardf_edges(rc, num_r_bins, num_theta_bins):
    """-> (r, lo, up [R], theta, theta_up [T]): the bin centres and edges as the reference forms them (angular_rdf.cu:116-121,
    :459-478)"""
    dr = rc / num_r_bins
    r = np.array([w * dr + dr / 2 for w in range(num_r_bins)])
    step = 2 * ARDF_PI / num_theta_bins
    th = np.array([-ARDF_PI + t * step + step / 2 for t in range(num_theta_bins)])
    return r, r - dr / 2, r + dr / 2, th, th + step / 2


def ardf_normalise(vsum, rc, pairs, num_atoms_of_type, num_repeats):
    """The one normalisation of the angular-RDF sums: bv = D / (2 pi) * 4 pi / 3 (up^3 - lo^3); total = vsum / (N^2 bv S),
    (a, a) = vsum / (N_a^2 bv S), (a, b) = vsum / (N_a N_b bv S)."""
    vsum = np.asarray(vsum, dtype=np.float64)
    na = np.asarray(num_atoms_of_type, dtype=np.float64)
    _, R, T = vsum.shape
    r, lo, up, th, _ = ardf_edges(rc, R, T)
    bv = (1.0 / T) * (4.0 / 3.0 * np.pi * (up ** 3 - lo ** 3))
    g = np.zeros_like(vsum)
    S = float(num_repeats)
    for c in range(vsum.shape[0]):
        w = na.sum() ** 2 if c == 0 else na[pairs[c - 1][0]] * na[pairs[c - 1][1]]
        with np.errstate(divide="ignore", invalid="ignore"):
            g[c] = vsum[c] / (w * bv[:, None] * S)
    return r, th, g


class AdfRow(C.Structure):
    _fields_ = [("itype", C.c_int), ("jtype", C.c_int), ("ktype", C.c_int),
                ("rmin_j", C.c_double), ("rmax_j", C.c_double), ("rmin_k", C.c_double), ("rmax_k", C.c_double)]


class ADF:
    """Angular distribution function as integer triplet counts (nepmi_adf_*): `num_bins` bins over 0 .. 180 degrees, one row of
    counts per entry of `rows`.  A row is (itype, jtype, ktype, rmin_j, rmax_j, rmin_k, rmax_k) with the types all -1 (any) or all
    >= 0; (rmin, rmax) alone is the global form: any types, both ranges equal.  `type_of_atom`: n ints in the caller's atom
    order, 0 .. num_types - 1; not needed when every row is "any".

    Attach it to the engine (`engine.attach(a)`) and the run_* methods sample it on the device every `interval` steps; a host
    that steps by hand calls `sample(pos, h, pbc)` with pos = [3N] f64 on the device.  `read()` -> (counts [M, num_bins] uint64,
    cumulative over the samples, num_samples); `density()` normalises as the reference's adf.out.  A centre atom with more than
    `capacity` neighbours in range voids the sample: `sample` and every later `read` raise with code -6.
    `lds_budget` (bytes) moves the threshold between the two forms of the triplet kernel; `form` is 1 (tables in LDS) or 2."""

    def __init__(self, engine, rows, num_bins, interval, type_of_atom=None, num_types=0, lds_budget=None):
        self.engine = engine
        self.lib = engine.lib
        self.num_bins, self.interval, self.num_types = int(num_bins), int(interval), int(num_types)
        rows = list(rows)
        if len(rows) == 2 and not hasattr(rows[0], "__len__"):
            rows = [(-1, -1, -1, rows[0], rows[1], rows[0], rows[1])]
        self.rows = [tuple(r) for r in rows]
        self.num_rows = len(self.rows)
        arr = (AdfRow * max(1, self.num_rows))()
        for m, r in enumerate(self.rows):
            arr[m] = AdfRow(int(r[0]), int(r[1]), int(r[2]), float(r[3]), float(r[4]), float(r[5]), float(r[6]))
        tp = None
        if type_of_atom is not None:
            t = np.ascontiguousarray(np.asarray(type_of_atom), dtype=np.int32)
            if t.shape != (engine.n,):
                raise ValueError("type_of_atom: one int per atom")
            tp = t.ctypes.data_as(_capi.c_ip)
        out = C.c_void_p()
        _capi.check(self.lib, self.lib.nepmi_adf_create(engine.handle, engine.n, self.num_bins, self.interval,
                                                        C.cast(arr, C.c_void_p), self.num_rows, tp, self.num_types, C.byref(out)))
        self.handle = out
        if not hasattr(engine, "_correlators"):
            engine._correlators = weakref.WeakSet()
        engine._correlators.add(self)
        if lds_budget is not None:
            _capi.check(self.lib, self.lib.nepmi_adf_set_lds_budget(self.handle, int(lds_budget)))

    @property
    def form(self):
        return _capi.check(self.lib, self.lib.nepmi_adf_form(self.handle))

    @property
    def capacity(self):
        return int(self.lib.nepmi_adf_capacity())

    def sample(self, pos, h, pbc):
        _, hp = _h9(h)
        _, pp = _pbc3(pbc)
        _capi.check(self.lib, self.lib.nepmi_adf_sample(self.handle, NEP._ptr(pos), hp, pp))

    def read(self):
        counts = np.zeros((self.num_rows, self.num_bins), dtype=np.uint64)
        ns = C.c_int64(0)
        _capi.check(self.lib, self.lib.nepmi_adf_read(self.handle, counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ns)))
        return counts, int(ns.value)

    def density(self):
        """-> (angle [num_bins] in degrees, the bin centres; density [M, num_bins]): adf.cu:315-350 on the integer sums"""
        counts, _ = self.read()
        return adf_normalise(counts)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nepmi_adf_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


class OrientOrder:
    """Steinhardt bond-orientational order per atom (nepmi_orient_*): `mode` is "cutoff" (`value` = the radius) or "nnn" (`value` =
    the number of nearest neighbours, searched inside `rc_search`); `degrees`: 1 .. 8 values of l in 0 .. 12.  The columns of an
    atom are ql[nd], then wl[nd] if `wl`, then wlhat[nd] if `wlhat`; `average` replaces q_lm by its mean over the atom and its
    members (Lechner-Dellago) first.

    Attach it to the engine (`engine.attach(o)`) and the run_* methods sample it on the device every `interval` steps; a host
    that steps by hand calls `sample(pos, h, pbc)` with pos = [3N] f64 on the device.  `read()` -> (last [n, ncol], sum [n, ncol],
    nn [n], num_samples), all in the caller's atom order.  A centre atom with more than `capacity` members inside the radius voids
    the sample: `sample` and every later `read` raise with code -6."""

    def __init__(self, engine, mode, value, degrees, average=False, wl=False, wlhat=False, interval=1, rc_search=6.0):
        self.engine = engine
        self.lib = engine.lib
        if mode not in ("cutoff", "nnn"):
            raise ValueError("mode: 'cutoff' or 'nnn'")
        self.mode = mode
        self.degrees = [int(l) for l in degrees]
        self.nd = len(self.degrees)
        self.average, self.wl, self.wlhat, self.interval = bool(average), bool(wl), bool(wlhat), int(interval)
        self.ncol = self.nd * (1 + int(self.wl) + int(self.wlhat))
        self.n = engine.n
        rc = float(value) if mode == "cutoff" else float(rc_search)
        nnn = 0 if mode == "cutoff" else int(value)
        deg = (C.c_int * max(1, self.nd))(*self.degrees)
        out = C.c_void_p()
        _capi.check(self.lib, self.lib.nepmi_orient_create(engine.handle, engine.n, 0 if mode == "cutoff" else 1, rc, nnn, deg, self.nd,
                                                           int(self.average), int(self.wl), int(self.wlhat), self.interval, C.byref(out)))
        self.handle = out
        if not hasattr(engine, "_correlators"):
            engine._correlators = weakref.WeakSet()
        engine._correlators.add(self)

    @property
    def capacity(self):
        return int(self.lib.nepmi_orient_capacity())

    def sample(self, pos, h, pbc):
        _, hp = _h9(h)
        _, pp = _pbc3(pbc)
        _capi.check(self.lib, self.lib.nepmi_orient_sample(self.handle, NEP._ptr(pos), hp, pp))

    def read(self):
        last = np.zeros((self.n, self.ncol), dtype=np.float64)
        total = np.zeros((self.n, self.ncol), dtype=np.float64)
        nn = np.zeros(self.n, dtype=np.int32)
        ns = C.c_int64(0)
        _capi.check(self.lib, self.lib.nepmi_orient_read(self.handle, last.ctypes.data_as(_capi.c_dp), total.ctypes.data_as(_capi.c_dp),
                                                         nn.ctypes.data_as(_capi.c_ip), C.byref(ns)))
        return last, total, nn, int(ns.value)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nepmi_orient_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


def adf_normalise(counts):
    """The one normalisation of the ADF sums: every row divided by its own total x the bin width in degrees, or by the bin width
    alone when the total is 0; the angles are the bin centres."""
    counts = np.asarray(counts)
    nb = counts.shape[1]
    edges = np.arange(nb + 1) * (180.0 / nb)
    angle = (edges[1:] + edges[:-1]) / 2
    delta = angle[1] - angle[0] if nb > 1 else 180.0
    total = counts.sum(axis=1, dtype=np.uint64).astype(np.float64)
    return angle, counts.astype(np.float64) / (np.where(total > 0, total, 1.0) * delta)[:, None]


def rdf_normalise(vsum, rc, num_atoms_of_type, num_repeats):
    """The one normalisation of the RDF sums: dV_w = 4 pi ((w + 0.5) dr)^2 dr, total = 2 sum_p vsum_p / (N^2 dV R),
    partial(a, a) = 2 vsum / (N_a^2 dV R), partial(a < b) = vsum / (N_a N_b dV R)."""
    vsum = np.asarray(vsum, dtype=np.float64)
    na = np.asarray(num_atoms_of_type, dtype=np.float64)
    T, nb = len(na), vsum.shape[1]
    dr = rc / nb
    r = (np.arange(nb) + 0.5) * dr
    dV = 4.0 * np.pi * r * r * dr
    R = float(num_repeats)
    total = 2.0 * vsum.sum(axis=0) / (na.sum() ** 2 * dV * R)
    partial = np.zeros_like(vsum)
    p = 0
    for a in range(T):
        for b in range(a, T):
            partial[p] = (2.0 if a == b else 1.0) * vsum[p] / (na[a] * na[b] * dV * R)
            p += 1
    return r, total, partial
