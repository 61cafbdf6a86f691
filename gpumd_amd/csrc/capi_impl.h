// C ABI (include/nepmi.h) on top of EngineT<NEPMI_BACKEND>.  Included exactly once by
// engine.hip (NEPMI_BACKEND = HipBackend, the product) and by tests/emu/emu.cpp (host loops, test
// infrastructure only).  The including file defines:
//   using NepmiBackend = ...;   NepmiBackend nepmi_make_backend(void* stream);
#pragma once
#include "../../include/nepmi.h"
#include "engine_impl.h"

#include <exception>
#include <string>

// Every handle starts with the function table of the library that created it (capi_dispatch.inc: a model whose shape is not
// among this library's compiled ones is served by a JIT core, capi_jit.h, and calls on its handles are forwarded there);
// nullptr in builds without the dispatch layer (tests/emu).
struct nepmi_api;
#if defined(NEPMI_CAPI_DISPATCH)
extern "C" const nepmi_api nepmi_self_api;
#define NEPMI_SELF_API (&nepmi_self_api)
#else
#define NEPMI_SELF_API nullptr
#endif

struct nepmi_model {
  const nepmi_api* api;
  nepmi::NepModel m;
};

struct nepmi_engine {
  const nepmi_api* api;
  nepmi::EngineT<NepmiBackend>* e;
};

struct nepmi_corr {
  const nepmi_api* api;
  nepmi::CorrelatorT<NepmiBackend>* c;
};

struct nepmi_rdf {
  const nepmi_api* api;
  nepmi::RdfT<NepmiBackend>* r;
};

struct nepmi_ardf {
  const nepmi_api* api;
  nepmi::ArdfT<NepmiBackend>* r;
};

struct nepmi_adf {
  const nepmi_api* api;
  nepmi::AdfT<NepmiBackend>* a;
};

struct nepmi_orient {
  const nepmi_api* api;
  nepmi::OrientT<NepmiBackend>* o;
};

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg)
{
  g_last_error = msg;
  return code;
}

template <class F>
int guarded(F&& f)
{
  try {
    f();
    return NEPMI_OK;
  } catch (const nepmi::EngineError& e) {
    return fail(e.code, e.msg);
  } catch (const std::exception& e) {
    return fail(NEPMI_ERR_HIP, e.what());
  }
}

} // namespace

extern "C" {

const char* nepmi_last_error(void) { return g_last_error.c_str(); }
int nepmi_version(void) { return NEPMI_VERSION; }

nepmi_model* nepmi_model_load(const char* path)
{
  if (!path) {
    fail(NEPMI_ERR_ARG, "null path");
    return nullptr;
  }
  nepmi_model* m = new nepmi_model();
  m->api = NEPMI_SELF_API;
  bool unsupported = false;
  const std::string err = nepmi::load_nep_model(path, m->m, &unsupported);
  if (!err.empty()) {
    g_last_error = err;
    delete m;
    return nullptr;
  }
#if !defined(NEPMI_JIT_CORE)
  // A model whose shape has no compiled kernels here (and no JIT core took it: the public nepmi_model_load asks for one
  // first) is zero-padded into the smallest COVER shape that holds it (nep_model.h: embed_model) -- compiled kernels at the
  // price of the padded work -- instead of the run-time-shape kernels.  NEPMI_JIT=0 or NEPMI_COVER=0: the run-time-shape
  // kernels; NEPMI_FORCE_COVER=1 (measurements): pad even a model of a compiled shape.
  {
    const char* jit = std::getenv("NEPMI_JIT");
    const char* cov = std::getenv("NEPMI_COVER");
    const char* force = std::getenv("NEPMI_FORCE_COVER");
    const bool forced = force && force[0] == '1';
    const bool allowed = !(jit && jit[0] == '0') && !(cov && cov[0] == '0');
    int c[4];
    const int builtin = nepmi::builtin_shape_of(m->m);
    if (m->m.kind == 0 && (forced || (allowed && builtin == 0)) && builtin != 7 && builtin != 8 && builtin != 9 && nepmi::cover_shape_for(m->m, c)) {
      const int f[5] = {m->m.n_max_radial, m->m.basis_size_radial, m->m.n_max_angular, m->m.basis_size_angular, m->m.num_L};
      if (!nepmi::embed_model(m->m, c[0], c[1], c[2], c[3]))
        std::fprintf(stderr, "nepmi: the run-time-shape kernels serve this model, several times slower than compiled ones\n");
      else if (!forced)
        std::fprintf(stderr, "nepmi: no kernels compiled for this model's shape (n_max %d %d, basis_size %d %d, %d invariant rows): it is served, "
                             "zero-padded, by the kernels of the compiled shape (n_max %d %d, basis_size %d %d, 6 rows)\n",
                     f[0], f[2], f[1], f[3], f[4], c[0], c[2], c[1], c[3]);
    } else if (m->m.kind == 0 && builtin == 0 && !(jit && jit[0] == '0')) {
      std::fprintf(stderr, "nepmi: the run-time-shape kernels serve this model (no compiled shape holds it), several times slower than compiled ones\n");
    }
  }
#endif
  return m;
}

void nepmi_model_free(nepmi_model* m) { delete m; }

int nepmi_model_info(const nepmi_model* mm, nepmi_info* o)
{
  if (!mm || !o)
    return fail(NEPMI_ERR_ARG, "null argument");
  const nepmi::NepModel& m = mm->m;
  o->version = m.version;
  o->num_types = m.num_types;
  o->zbl_enabled = m.zbl_enabled;
  o->zbl_flexible = m.zbl_flexible;
  o->zbl_rc_inner = m.zbl_rc_inner;
  o->zbl_rc_outer = m.zbl_rc_outer;
  o->rc_radial = m.rc_radial_max;
  o->rc_angular = m.rc_angular_max;
  o->MN_radial = m.MN_radial;
  o->MN_angular = m.MN_angular;
  o->n_max_radial = m.embedded() ? m.file_n_max_radial : m.n_max_radial;
  o->n_max_angular = m.embedded() ? m.file_n_max_angular : m.n_max_angular;
  o->basis_size_radial = m.embedded() ? m.file_basis_size_radial : m.basis_size_radial;
  o->basis_size_angular = m.embedded() ? m.file_basis_size_angular : m.basis_size_angular;
  o->L_max = m.embedded() ? m.file_L_max : m.L_max;
  o->has_q_222 = m.embedded() ? m.file_has_q_222 : m.has_q_222;
  o->has_q_1111 = m.embedded() ? m.file_has_q_1111 : m.has_q_1111;
  o->num_L = m.embedded() ? m.file_num_L : m.num_L;
  o->dim = m.embedded() ? m.file_dim : m.dim;
  o->num_neurons = m.num_neurons;
  o->num_para = m.num_para;
  o->has_q_112 = m.has_q_112;
  o->has_q_123 = m.has_q_123;
  o->has_q_233 = m.has_q_233;
  o->has_q_134 = m.has_q_134;
  o->model_type = m.temperature_model ? 3 : 0;
  return NEPMI_OK;
}

const char* nepmi_model_symbol(const nepmi_model* m, int type)
{
  if (!m || type < 0 || type >= m->m.num_types)
    return "";
  return m->m.symbols[type].c_str();
}

nepmi_engine* nepmi_engine_create(const nepmi_model* m, int64_t n_atoms, void* stream)
{
  if (!m) {
    fail(NEPMI_ERR_ARG, "null model");
    return nullptr;
  }
  nepmi_engine* e = new nepmi_engine();
  e->api = NEPMI_SELF_API;
  e->e = nullptr;
  const int st = guarded([&] { e->e = new nepmi::EngineT<NepmiBackend>(m->m, n_atoms, nepmi_make_backend(stream)); });
  if (st != NEPMI_OK) {
    delete e;
    return nullptr;
  }
  return e;
}

void nepmi_engine_destroy(nepmi_engine* e)
{
  if (e) {
    delete e->e;
    delete e;
  }
}

int nepmi_force_compute(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, double* pos, double* pe,
  double* force, double* virial)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] {
    e->e->apply_pbc(h, pbc, n, pos);
    e->e->zero_properties(n, pe, force, virial);
    e->e->potential_compute(h, pbc, n, type, pos, pe, force, virial);
  });
}

int nepmi_potential_compute(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* pos,
  double* pe, double* force, double* virial)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->potential_compute(h, pbc, n, type, pos, pe, force, virial); });
}

int nepmi_potential_compute_levels(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* pos,
  const signed char* level, double* pe, double* force, double* virial)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->potential_compute_levels(h, pbc, n, type, pos, level, pe, force, virial); });
}

int nepmi_potential_compute_levels_begin(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* pos,
  const signed char* level, double* pe, double* force, double* virial)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  bool started = false;
  const int st = guarded([&] { started = e->e->potential_compute_levels_begin(h, pbc, n, type, pos, level, pe, force, virial); });
  return st != NEPMI_OK ? st : (started ? 1 : 0);
}

int nepmi_potential_compute_levels_end(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* pos,
  const signed char* level, double* pe, double* force, double* virial)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->potential_compute_levels_end(h, pbc, n, type, pos, level, pe, force, virial); });
}

int nepmi_engine_invalidate(nepmi_engine* e)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  e->e->invalidate();
  return NEPMI_OK;
}

int nepmi_apply_pbc(nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, double* pos)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->apply_pbc(h, pbc, n, pos); });
}

int nepmi_zero_properties(nepmi_engine* e, int64_t n, double* pe, double* force, double* virial)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->zero_properties(n, pe, force, virial); });
}

int nepmi_average_properties(
  nepmi_engine* e, int64_t n, double denominator, double* pe, double* force, double* virial)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (!(denominator > 0.0))
    return fail(NEPMI_ERR_ARG, "average_properties: denominator should be positive");
  return guarded([&] { e->e->average_properties(n, denominator, pe, force, virial); });
}

int nepmi_vv_step1(
  nepmi_engine* e, int64_t n, double dt, const double* mass, const double* force, double* pos, double* vel)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->velocity_verlet(true, n, dt, mass, force, pos, vel, nullptr); });
}

int nepmi_vv_step2(nepmi_engine* e, int64_t n, double dt, const double* mass, const double* force, double* vel)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->velocity_verlet(false, n, dt, mass, force, nullptr, vel, nullptr); });
}

int nepmi_find_thermo(
  nepmi_engine* e, int64_t n, double volume, const double* mass, const double* pe, const double* vel,
  const double* virial, double* thermo8)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->find_thermo(n, volume, mass, pe, vel, virial, thermo8); });
}

int nepmi_run_nve(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* mass,
  double dt, int64_t nsteps, double* pos, double* vel, double* pe, double* force, double* virial,
  int64_t thermo_every, double* thermo_host)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] {
    e->e->run_md(e->e->kNve, h, pbc, n, type, mass, dt, nsteps, 0.0, 0.0, 1.0, pos, vel, pe, force, virial, thermo_every,
                 thermo_host);
  });
}

int nepmi_berendsen_scale(
  nepmi_engine* e, int64_t n, double temperature, double coupling, const double* thermo8, double* vel)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->berendsen(n, temperature, coupling, thermo8, vel); });
}

int nepmi_run_nvt_ber(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* mass,
  double dt, int64_t nsteps, double t1, double t2, double t_coup, double* pos, double* vel, double* pe,
  double* force, double* virial, int64_t thermo_every, double* thermo_host)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] {
    e->e->run_md(e->e->kBer, h, pbc, n, type, mass, dt, nsteps, t1, t2, t_coup, pos, vel, pe, force, virial, thermo_every,
                 thermo_host);
  });
}

// the refusals of Integrate::parse_ensemble for `npt_ber` (integrate.cu:649-692), with its messages
static int npt_check(const double h[9], const int pbc[3], int num_p, const double* p_target, const double* p_coupling, nepmi::NptSpec& s)
{
  if (!h || !pbc || !p_target || !p_coupling)
    return fail(NEPMI_ERR_ARG, "null argument");
  if (num_p != 1 && num_p != 3 && num_p != 6)
    return fail(NEPMI_ERR_ARG, "npt_ber: the number of target pressure components should be 1, 3 or 6");
  const bool triclinic = h[1] != 0 || h[2] != 0 || h[3] != 0 || h[5] != 0 || h[6] != 0 || h[7] != 0;
  const bool open_dir = pbc[0] == 0 || pbc[1] == 0 || pbc[2] == 0;
  if (num_p == 3 && triclinic)
    return fail(NEPMI_ERR_ARG, "Cannot use triclinic box with only 3 target pressure components.");
  if (num_p == 1 && triclinic)
    return fail(NEPMI_ERR_ARG, "Cannot use triclinic box with only 1 target pressure component.");
  if (num_p == 1 && open_dir)
    return fail(NEPMI_ERR_ARG, "Cannot use isotropic pressure with non-periodic boundary in any direction.");
  if (num_p == 6 && open_dir)
    return fail(NEPMI_ERR_ARG, "Cannot use 6 pressure components with non-periodic boundary in any direction.");
  std::memset(&s, 0, sizeof(s));
  s.num_p = num_p;
  for (int k = 0; k < num_p; ++k) {
    if (!(p_coupling[k] >= 0.0))
      return fail(NEPMI_ERR_ARG, "npt_ber: pressure coupling should be >= 0");
    s.p0[k] = p_target[k];
    s.pc[k] = p_coupling[k];
  }
  return NEPMI_OK;
}

int nepmi_berendsen_pressure(
  nepmi_engine* e, int64_t n, int num_p, const double p_target[6], const double p_coupling[6], const double* thermo8,
  double h[9], double* pos)
{
  if (!e || !thermo8 || !pos)
    return fail(NEPMI_ERR_ARG, "bad argument");
  // open directions: those of the engine's last force evaluation (all periodic before the first)
  int pbc[3] = {1, 1, 1};
  if (e->e->num_compute > 0)
    for (int d = 0; d < 3; ++d)
      pbc[d] = e->e->box().pbc[d];
  nepmi::NptSpec s;
  const int st = npt_check(h, pbc, num_p, p_target, p_coupling, s);
  if (st != NEPMI_OK)
    return st;
  return guarded([&] { e->e->berendsen_pressure(n, s, pbc, thermo8, h, pos); });
}

int nepmi_run_npt_ber(
  nepmi_engine* e, double h[9], const int pbc[3], int64_t n, const int* type, const double* mass, double dt,
  int64_t nsteps, double t1, double t2, double t_coup, int num_p, const double p_target[6], const double p_coupling[6],
  double* pos, double* vel, double* pe, double* force, double* virial, int64_t thermo_every, double* thermo_host,
  double* box_host)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  nepmi::NptSpec s;
  const int st = npt_check(h, pbc, num_p, p_target, p_coupling, s);
  if (st != NEPMI_OK)
    return st;
  double h_out[9];
  s.h_out = h_out;
  s.box_host = box_host;
  const int rc = guarded([&] {
    e->e->run_md(e->e->kBer, h, pbc, n, type, mass, dt, nsteps, t1, t2, t_coup, pos, vel, pe, force, virial, thermo_every,
                 thermo_host, &s);
  });
  if (rc == NEPMI_OK)
    for (int k = 0; k < 9; ++k)
      h[k] = h_out[k];
  return rc;
}

int nepmi_nhc_init(nepmi_engine* e, int64_t n, double temperature, double t_coup, double dt, double* chain_state)
{
  if (!e || !chain_state)
    return fail(NEPMI_ERR_ARG, "bad argument");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] { e->e->nhc_init(n, temperature, t_coup, dt, chain_state); });
}

int nepmi_nhc_half_step(
  nepmi_engine* e, int64_t n, double temperature, double dt, const double* thermo8, double* chain_state,
  double* vel)
{
  if (!e || !chain_state || !thermo8 || !vel)
    return fail(NEPMI_ERR_ARG, "bad argument");
  return guarded([&] { e->e->nhc_half_step(n, temperature, dt, thermo8, chain_state, vel); });
}

int nepmi_run_nvt_nhc(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* mass,
  double dt, int64_t nsteps, double t1, double t2, double t_coup, double* pos, double* vel, double* pe,
  double* force, double* virial, int64_t thermo_every, double* thermo_host)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] {
    e->e->run_md(e->e->kNhc, h, pbc, n, type, mass, dt, nsteps, t1, t2, t_coup, pos, vel, pe, force, virial, thermo_every,
                 thermo_host);
  });
}

int nepmi_engine_reset_thermostat(nepmi_engine* e)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  e->e->reset_thermostat();
  return NEPMI_OK;
}

int nepmi_bdp_seed(nepmi_engine* e, uint64_t seed)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  e->e->bdp_seed(seed);
  return NEPMI_OK;
}

int nepmi_bdp_scale(nepmi_engine* e, int64_t n, double temperature, double t_coup, const double* thermo8, double* vel)
{
  if (!e || !thermo8 || !vel)
    return fail(NEPMI_ERR_ARG, "bad argument");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] { e->e->bdp_scale(n, temperature, t_coup, thermo8, vel); });
}

int nepmi_run_nvt_bdp(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* mass,
  double dt, int64_t nsteps, double t1, double t2, double t_coup, double* pos, double* vel, double* pe,
  double* force, double* virial, int64_t thermo_every, double* thermo_host)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] {
    e->e->run_md(e->e->kBdp, h, pbc, n, type, mass, dt, nsteps, t1, t2, t_coup, pos, vel, pe, force, virial, thermo_every,
                 thermo_host);
  });
}

int nepmi_lan_seed(nepmi_engine* e, int seed)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  e->e->lan_seed(seed);
  return NEPMI_OK;
}

int nepmi_lan_half_step(nepmi_engine* e, int64_t n, double temperature, double t_coup, const double* mass, double* vel)
{
  if (!e || !mass || !vel)
    return fail(NEPMI_ERR_ARG, "bad argument");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] { e->e->lan_half_step(n, temperature, t_coup, mass, vel); });
}

int nepmi_run_nvt_lan(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* mass,
  double dt, int64_t nsteps, double t1, double t2, double t_coup, double* pos, double* vel, double* pe,
  double* force, double* virial, int64_t thermo_every, double* thermo_host)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] {
    e->e->run_md(e->e->kLan, h, pbc, n, type, mass, dt, nsteps, t1, t2, t_coup, pos, vel, pe, force, virial, thermo_every,
                 thermo_host);
  });
}

int nepmi_run_nvt_bao(
  nepmi_engine* e, const double h[9], const int pbc[3], int64_t n, const int* type, const double* mass,
  double dt, int64_t nsteps, double t1, double t2, double t_coup, double* pos, double* vel, double* pe,
  double* force, double* virial, int64_t thermo_every, double* thermo_host)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (t_coup < 1.0)
    return fail(NEPMI_ERR_ARG, "Temperature coupling should >= 1.");
  return guarded([&] {
    e->e->run_md(e->e->kBao, h, pbc, n, type, mass, dt, nsteps, t1, t2, t_coup, pos, vel, pe, force, virial, thermo_every,
                 thermo_host);
  });
}

int nepmi_neighbors_export(nepmi_engine* e, int which, int* nn, int* nl, int64_t ld)
{
  if (!e || which < 0 || which > 2 || !nn || !nl)
    return fail(NEPMI_ERR_ARG, "bad argument");
  int mx = -1;
  const int st = guarded([&] { e->e->export_lists(which, nn, nl, ld, &mx); });
  if (st != NEPMI_OK)
    return st;
  int ms, mr, ma;
  double ar, aa;
  const int st2 = guarded([&] { e->e->list_stats(ms, mr, ma, ar, aa); });
  if (st2 != NEPMI_OK)
    return st2;
  return which == 0 ? mr : which == 1 ? ma : ms;
}

int nepmi_descriptors_export(nepmi_engine* e, float* q, float* fp)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->export_descriptors(q, fp); });
}

int nepmi_engine_stats(nepmi_engine* e, int with_lists, nepmi_stats* out)
{
  if (!e || !out)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] {
    auto& eng = *e->e;
    eng.backend().sync();
    if (eng.num_compute > 0)
      eng.check_flags_now(); // overflow flags of the force calls since the last read-back
    std::memset(out, 0, sizeof(*out));
    out->num_compute = eng.num_compute;
    out->num_rebuild = eng.num_rebuild;
    if (with_lists && eng.num_compute > 0)
      eng.list_stats(out->max_nn_skin, out->max_nn_radial, out->max_nn_angular, out->mean_nn_radial, out->mean_nn_angular);
    out->ms_force_last = eng.backend().region_ms(nepmi::kRegionForce);
    const int slots[7] = {nepmi::kSlotGather, nepmi::kSlotRadial, nepmi::kSlotAngular, nepmi::kSlotAnn,
                          nepmi::kSlotAngForce, nepmi::kSlotForce, nepmi::kSlotVV};
    for (int k = 0; k < 7; ++k) {
      out->ms_kernel[k] = eng.backend().slot_ms(slots[k]);
      out->ms_kernel_sum[k] = eng.backend().slot_sum(slots[k]);
      out->launches[k] = eng.backend().slot_count(slots[k]);
    }
    out->radial_tiles = eng.tile_mode_in_use();
    out->discarded_steps = eng.num_discarded;
    out->ms_kernel_sum[7] = eng.backend().region_sum(nepmi::kRegionRebuild);
    out->launches[7] = eng.backend().region_count(nepmi::kRegionRebuild);
    out->ms_kernel[7] = eng.backend().region_ms(nepmi::kRegionRebuild);
  });
}

int nepmi_engine_describe(nepmi_engine* e, char* buf, int len)
{
  if (!e || !buf || len < 1)
    return fail(NEPMI_ERR_ARG, "bad argument");
  const std::string s = e->e->describe();
  const int n = (int)s.size() < len - 1 ? (int)s.size() : len - 1;
  std::memcpy(buf, s.data(), (size_t)n);
  buf[n] = 0;
  return n;
}

int nepmi_engine_set_timing(nepmi_engine* e, int on)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  e->e->backend().set_timing(on < 0 ? 0 : ((on >= 16 && on < 32) ? on : (on > 2 ? 1 : on)));
  e->e->num_discarded = 0; // counted over the same window as the kernel sums
  return NEPMI_OK;
}

int nepmi_engine_set_force_form(nepmi_engine* e, int mode)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (mode < -1 || mode > 1)
    return fail(NEPMI_ERR_ARG, "force form: -1 (by caller), 0 (gather), 1 (scatter)");
  e->e->set_force_form(mode);
  return NEPMI_OK;
}

int nepmi_engine_set_virial_mode(nepmi_engine* e, int mode)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  if (mode != 0 && mode != 1)
    return fail(NEPMI_ERR_ARG, "virial mode: 0 (per-atom, the reference's attribution), 1 (totals)");
  e->e->set_loop_context(mode == 1);
  return NEPMI_OK;
}

int nepmi_engine_set_temperature(nepmi_engine* e, double temperature)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  return guarded([&] { e->e->set_temperature(temperature); });
}

int nepmi_engine_set_external_skin(nepmi_engine* e, int on)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  e->e->set_external_skin(on != 0);
  return NEPMI_OK;
}

int nepmi_engine_set_unwrapped(nepmi_engine* e, double* d_unwrapped)
{
  if (!e)
    return fail(NEPMI_ERR_ARG, "null engine");
  e->e->set_unwrapped(d_unwrapped);
  return NEPMI_OK;
}

namespace {
int corr_create_common(
  nepmi_engine* e, int quantity, int64_t n, int64_t sample_interval, int num_corr, const int* group_of_atom, int num_groups,
  const double* weight_host, nepmi_corr** out)
{
  *out = nullptr;
  nepmi_corr* c = new nepmi_corr();
  c->api = NEPMI_SELF_API;
  c->c = nullptr;
  const int st = guarded([&] {
    if (n != e->e->num_atoms())
      throw nepmi::EngineError{NEPMI_ERR_ARG, "correlator: n is not the engine's number of atoms"};
    c->c = new nepmi::CorrelatorT<NepmiBackend>(e->e->backend(), quantity, n, sample_interval, num_corr, group_of_atom, num_groups,
                                                weight_host);
  });
  if (st != NEPMI_OK) {
    delete c;
    return st;
  }
  *out = c;
  return NEPMI_OK;
}
} // namespace

int nepmi_corr_create(
  nepmi_engine* e, int quantity, int64_t n, int64_t sample_interval, int num_corr, const int* group_of_atom, int num_groups,
  nepmi_corr** out)
{
  if (!e || !out)
    return fail(NEPMI_ERR_ARG, "null argument");
  return corr_create_common(e, quantity, n, sample_interval, num_corr, group_of_atom, num_groups, nullptr, out);
}

int nepmi_corr_create_weighted(
  nepmi_engine* e, int quantity, int64_t n, int64_t sample_interval, int num_corr, const int* group_of_atom, int num_groups,
  const double* weight_host, nepmi_corr** out)
{
  if (!e || !out)
    return fail(NEPMI_ERR_ARG, "null argument");
  *out = nullptr;
  if (quantity == 0 || quantity == 1)
    return fail(NEPMI_ERR_ARG, "correlator: weights belong to quantity 2 (MVAC)");
  if (quantity != 2)
    return fail(NEPMI_ERR_ARG, "correlator: the weighted quantity should be 2 (MVAC)");
  if (!weight_host)
    return fail(NEPMI_ERR_ARG, "correlator: quantity 2 (MVAC) needs the weight array");
  return corr_create_common(e, quantity, n, sample_interval, num_corr, group_of_atom, num_groups, weight_host, out);
}

// normalize_vac and find_dos, src/measure/dos.cu:414-427 and 450-481 (host only)
int nepmi_dos_from_mvac(
  const double* sums, int num_groups, int num_corr, const int64_t* group_size, double dt_ps, double omega_max, int num_dos_points,
  double* mvac_out, double* dos_out)
{
  if (!sums || !group_size || !mvac_out || !dos_out)
    return fail(NEPMI_ERR_ARG, "null argument");
  if (num_groups < 1 || num_corr < 1 || num_dos_points < 1)
    return fail(NEPMI_ERR_ARG, "dos: number of groups, of correlation steps and of DOS points should be positive");
  if (!(dt_ps > 0.0) || !(omega_max > 0.0))
    return fail(NEPMI_ERR_ARG, "dos: sampling time and maximal angular frequency should be positive");
  const double pi = 3.14159265358979323846;
  const double d_omega = omega_max / num_dos_points;
  std::vector<double> windowed((size_t)num_corr);
  for (int g = 0; g < num_groups; ++g)
    for (int d = 0; d < 3; ++d) {
      const double* s = sums + ((size_t)g * 3 + d) * num_corr;
      double* mvac = mvac_out + ((size_t)g * 3 + d) * num_corr;
      double* dos = dos_out + ((size_t)g * 3 + d) * num_dos_points;
      const double s0 = s[0];
      if (s0 == 0.0) { // an empty group (the reference prints 0 / 0 there)
        std::fill(mvac, mvac + num_corr, 0.0);
        std::fill(dos, dos + num_dos_points, 0.0);
        continue;
      }
      for (int l = 0; l < num_corr; ++l) {
        mvac[l] = s[l] / s0;
        const double hann = (std::cos((pi * l) / num_corr) + 1.0) * 0.5;
        windowed[l] = mvac[l] * (l == 0 ? hann : 2.0 * hann);
      }
      for (int k = 0; k < num_dos_points; ++k) {
        const double omega = d_omega + k * d_omega;
        double sum = 0.0;
        for (int l = 0; l < num_corr; ++l)
          sum += windowed[l] * std::cos(omega * l * dt_ps);
        dos[k] = sum * (dt_ps * 2.0 * (double)group_size[g]);
      }
    }
  return NEPMI_OK;
}

void nepmi_corr_destroy(nepmi_corr* c)
{
  if (!c)
    return;
  if (c->c && c->c->attached_to)
    guarded([&] { static_cast<nepmi::EngineT<NepmiBackend>*>(c->c->attached_to)->corr_detach(c->c); });
  guarded([&] { delete c->c; });
  delete c;
}

int nepmi_corr_sample(nepmi_corr* c, const double* q)
{
  if (!c || !q)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] { c->c->sample_now(q); });
}

int nepmi_corr_attach(nepmi_engine* e, nepmi_corr* c)
{
  if (!e || !c)
    return fail(NEPMI_ERR_ARG, "null argument");
  if (c->api != e->api)
    return fail(NEPMI_ERR_ARG, "correlator: created from an engine of another kernel library");
  return guarded([&] { e->e->corr_attach(c->c); });
}

int nepmi_corr_detach(nepmi_engine* e, nepmi_corr* c)
{
  if (!e || !c)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] { e->e->corr_detach(c->c); });
}

int nepmi_corr_read(nepmi_corr* c, double* sums_host, int64_t* num_origins, int64_t* num_samples)
{
  if (!c)
    return fail(NEPMI_ERR_ARG, "null correlator");
  return guarded([&] { c->c->read(sums_host, num_origins, num_samples); });
}

int nepmi_rdf_create(
  nepmi_engine* e, int64_t n, double rc, int num_bins, int64_t sample_interval, const int* type_of_atom, int num_types,
  nepmi_rdf** out)
{
  if (!e || !out)
    return fail(NEPMI_ERR_ARG, "null argument");
  *out = nullptr;
  nepmi_rdf* r = new nepmi_rdf();
  r->api = NEPMI_SELF_API;
  r->r = nullptr;
  const int st = guarded([&] {
    if (n != e->e->num_atoms())
      throw nepmi::EngineError{NEPMI_ERR_ARG, "rdf: n is not the engine's number of atoms"};
    r->r = new nepmi::RdfT<NepmiBackend>(e->e->backend(), n, rc, num_bins, sample_interval, type_of_atom, num_types);
  });
  if (st != NEPMI_OK) {
    delete r;
    return st;
  }
  *out = r;
  return NEPMI_OK;
}

void nepmi_rdf_destroy(nepmi_rdf* r)
{
  if (!r)
    return;
  if (r->r && r->r->attached_to)
    guarded([&] { static_cast<nepmi::EngineT<NepmiBackend>*>(r->r->attached_to)->rdf_detach(r->r); });
  guarded([&] { delete r->r; });
  delete r;
}

int nepmi_rdf_sample(nepmi_rdf* r, const double* pos, const double* h9, const int* pbc3)
{
  if (!r || !pos || !h9 || !pbc3)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] {
    nepmi::BoxD box;
    nepmi::box_from_h9(h9, pbc3, box);
    r->r->sample_now(pos, box);
  });
}

int nepmi_rdf_attach(nepmi_engine* e, nepmi_rdf* r)
{
  if (!e || !r)
    return fail(NEPMI_ERR_ARG, "null argument");
  if (r->api != e->api)
    return fail(NEPMI_ERR_ARG, "rdf: created from an engine of another kernel library");
  return guarded([&] { e->e->rdf_attach(r->r); });
}

int nepmi_rdf_detach(nepmi_engine* e, nepmi_rdf* r)
{
  if (!e || !r)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] { e->e->rdf_detach(r->r); });
}

int nepmi_rdf_read(nepmi_rdf* r, uint64_t* counts_host, double* vsum_host, int64_t* num_samples)
{
  if (!r)
    return fail(NEPMI_ERR_ARG, "null rdf handle");
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counts are 64-bit");
  return guarded([&] { r->r->read(reinterpret_cast<unsigned long long*>(counts_host), vsum_host, num_samples); });
}

int nepmi_rdf_set_lds_budget(nepmi_rdf* r, int64_t bytes)
{
  if (!r)
    return fail(NEPMI_ERR_ARG, "null rdf handle");
  r->r->set_lds_budget(bytes);
  return NEPMI_OK;
}

int nepmi_rdf_form(nepmi_rdf* r)
{
  if (!r)
    return fail(NEPMI_ERR_ARG, "null rdf handle");
  return r->r->form();
}

int nepmi_ardf_create(
  nepmi_engine* e, int64_t n, double rc, int num_r_bins, int num_theta_bins, int64_t sample_interval, const int* type_of_atom,
  int num_types, int num_pairs, const int* pair_types, nepmi_ardf** out)
{
  if (!e || !out)
    return fail(NEPMI_ERR_ARG, "null argument");
  *out = nullptr;
  nepmi_ardf* r = new nepmi_ardf();
  r->api = NEPMI_SELF_API;
  r->r = nullptr;
  const int st = guarded([&] {
    if (n != e->e->num_atoms())
      throw nepmi::EngineError{NEPMI_ERR_ARG, "ardf: n is not the engine's number of atoms"};
    r->r = new nepmi::ArdfT<NepmiBackend>(e->e->backend(), n, rc, num_r_bins, num_theta_bins, sample_interval, type_of_atom, num_types,
                                          num_pairs, pair_types);
  });
  if (st != NEPMI_OK) {
    delete r;
    return st;
  }
  *out = r;
  return NEPMI_OK;
}

void nepmi_ardf_destroy(nepmi_ardf* r)
{
  if (!r)
    return;
  if (r->r && r->r->attached_to)
    guarded([&] { static_cast<nepmi::EngineT<NepmiBackend>*>(r->r->attached_to)->ardf_detach(r->r); });
  guarded([&] { delete r->r; });
  delete r;
}

int nepmi_ardf_sample(nepmi_ardf* r, const double* pos, const double* h9, const int* pbc3)
{
  if (!r || !pos || !h9 || !pbc3)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] {
    nepmi::BoxD box;
    nepmi::box_from_h9(h9, pbc3, box);
    r->r->sample_now(pos, box);
  });
}

int nepmi_ardf_attach(nepmi_engine* e, nepmi_ardf* r)
{
  if (!e || !r)
    return fail(NEPMI_ERR_ARG, "null argument");
  if (r->api != e->api)
    return fail(NEPMI_ERR_ARG, "ardf: created from an engine of another kernel library");
  return guarded([&] { e->e->ardf_attach(r->r); });
}

int nepmi_ardf_detach(nepmi_engine* e, nepmi_ardf* r)
{
  if (!e || !r)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] { e->e->ardf_detach(r->r); });
}

int nepmi_ardf_read(nepmi_ardf* r, uint64_t* counts_host, double* vsum_host, int64_t* num_samples)
{
  if (!r)
    return fail(NEPMI_ERR_ARG, "null ardf handle");
  return guarded([&] { r->r->read(reinterpret_cast<unsigned long long*>(counts_host), vsum_host, num_samples); });
}

int nepmi_ardf_set_lds_budget(nepmi_ardf* r, int64_t bytes)
{
  if (!r)
    return fail(NEPMI_ERR_ARG, "null ardf handle");
  r->r->set_lds_budget(bytes);
  return NEPMI_OK;
}

int nepmi_ardf_form(nepmi_ardf* r)
{
  if (!r)
    return fail(NEPMI_ERR_ARG, "null ardf handle");
  return r->r->form();
}

int nepmi_adf_create(
  nepmi_engine* e, int64_t n, int num_bins, int64_t sample_interval, const nepmi_adf_row* rows, int num_rows,
  const int* type_of_atom, int num_types, nepmi_adf** out)
{
  if (!e || !out)
    return fail(NEPMI_ERR_ARG, "null argument");
  *out = nullptr;
  nepmi_adf* a = new nepmi_adf();
  a->api = NEPMI_SELF_API;
  a->a = nullptr;
  const int st = guarded([&] {
    if (n != e->e->num_atoms())
      throw nepmi::EngineError{NEPMI_ERR_ARG, "adf: n is not the engine's number of atoms"};
    std::vector<nepmi::AdfRowIn> in;
    if (rows)
      for (int m = 0; m < num_rows && m < nepmi::kAdfMaxRows; ++m)
        in.push_back(nepmi::AdfRowIn{rows[m].itype, rows[m].jtype, rows[m].ktype, rows[m].rmin_j, rows[m].rmax_j, rows[m].rmin_k, rows[m].rmax_k});
    a->a = new nepmi::AdfT<NepmiBackend>(e->e->backend(), n, num_bins, sample_interval, rows ? in.data() : nullptr, num_rows, type_of_atom, num_types);
  });
  if (st != NEPMI_OK) {
    delete a;
    return st;
  }
  *out = a;
  return NEPMI_OK;
}

void nepmi_adf_destroy(nepmi_adf* a)
{
  if (!a)
    return;
  if (a->a && a->a->attached_to)
    guarded([&] { static_cast<nepmi::EngineT<NepmiBackend>*>(a->a->attached_to)->adf_detach(a->a); });
  guarded([&] { delete a->a; });
  delete a;
}

int nepmi_adf_sample(nepmi_adf* a, const double* pos, const double* h9, const int* pbc3)
{
  if (!a || !pos || !h9 || !pbc3)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] {
    nepmi::BoxD box;
    nepmi::box_from_h9(h9, pbc3, box);
    a->a->sample_now(pos, box);
  });
}

int nepmi_adf_attach(nepmi_engine* e, nepmi_adf* a)
{
  if (!e || !a)
    return fail(NEPMI_ERR_ARG, "null argument");
  if (a->api != e->api)
    return fail(NEPMI_ERR_ARG, "adf: created from an engine of another kernel library");
  return guarded([&] { e->e->adf_attach(a->a); });
}

int nepmi_adf_detach(nepmi_engine* e, nepmi_adf* a)
{
  if (!e || !a)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] { e->e->adf_detach(a->a); });
}

int nepmi_adf_read(nepmi_adf* a, uint64_t* counts_host, int64_t* num_samples)
{
  if (!a)
    return fail(NEPMI_ERR_ARG, "null adf handle");
  return guarded([&] { a->a->read(reinterpret_cast<unsigned long long*>(counts_host), num_samples); });
}

int nepmi_adf_set_lds_budget(nepmi_adf* a, int64_t bytes)
{
  if (!a)
    return fail(NEPMI_ERR_ARG, "null adf handle");
  a->a->set_lds_budget(bytes);
  return NEPMI_OK;
}

int nepmi_adf_form(nepmi_adf* a)
{
  if (!a)
    return fail(NEPMI_ERR_ARG, "null adf handle");
  return a->a->form();
}

int nepmi_adf_capacity(void) { return nepmi::kAdfMaxNeighbours; }

int nepmi_orient_create(
  nepmi_engine* e, int64_t n, int mode, double rc, int nnn, const int* degrees, int num_degrees, int average, int wl, int wlhat,
  int64_t sample_interval, nepmi_orient** out)
{
  if (!e || !out)
    return fail(NEPMI_ERR_ARG, "null argument");
  *out = nullptr;
  nepmi_orient* o = new nepmi_orient();
  o->api = NEPMI_SELF_API;
  o->o = nullptr;
  const int st = guarded([&] {
    if (n != e->e->num_atoms())
      throw nepmi::EngineError{NEPMI_ERR_ARG, "orient: n is not the engine's number of atoms"};
    o->o = new nepmi::OrientT<NepmiBackend>(e->e->backend(), n, mode, rc, nnn, degrees, num_degrees, average, wl, wlhat, sample_interval);
  });
  if (st != NEPMI_OK) {
    delete o;
    return st;
  }
  *out = o;
  return NEPMI_OK;
}

void nepmi_orient_destroy(nepmi_orient* o)
{
  if (!o)
    return;
  if (o->o && o->o->attached_to)
    guarded([&] { static_cast<nepmi::EngineT<NepmiBackend>*>(o->o->attached_to)->orient_detach(o->o); });
  guarded([&] { delete o->o; });
  delete o;
}

int nepmi_orient_sample(nepmi_orient* o, const double* pos, const double* h9, const int* pbc3)
{
  if (!o || !pos || !h9 || !pbc3)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] {
    nepmi::BoxD box;
    nepmi::box_from_h9(h9, pbc3, box);
    o->o->sample_now(pos, box);
  });
}

int nepmi_orient_attach(nepmi_engine* e, nepmi_orient* o)
{
  if (!e || !o)
    return fail(NEPMI_ERR_ARG, "null argument");
  if (o->api != e->api)
    return fail(NEPMI_ERR_ARG, "orient: created from an engine of another kernel library");
  return guarded([&] { e->e->orient_attach(o->o); });
}

int nepmi_orient_detach(nepmi_engine* e, nepmi_orient* o)
{
  if (!e || !o)
    return fail(NEPMI_ERR_ARG, "null argument");
  return guarded([&] { e->e->orient_detach(o->o); });
}

int nepmi_orient_read(nepmi_orient* o, double* last_host, double* sum_host, int* nn_host, int64_t* num_samples)
{
  if (!o)
    return fail(NEPMI_ERR_ARG, "null orient handle");
  return guarded([&] { o->o->read(last_host, sum_host, nn_host, num_samples); });
}

int nepmi_orient_capacity(void) { return nepmi::kOrientMaxNeighbours; }

int nepmi_engine_set_option(nepmi_engine* e, const char* name, double value)
{
  if (!e || !name)
    return fail(NEPMI_ERR_ARG, "null engine or option name");
  const std::string n(name);
  const int iv = (int)value;
  auto& eng = *e->e;
  if (n == "generic")
    return guarded([&] { eng.set_force_generic(iv != 0); });
  if (n == "tiles")
    eng.set_tile_mode(iv < 0 ? -1 : iv > 2 ? 2 : iv);
  else if (n == "win_lanes")
    eng.set_win_lanes(iv);
  else if (n == "win_max_atoms")
    eng.set_win_max_atoms(iv);
  else if (n == "scatter_guard")
    eng.set_scatter_guard_delayed(value, eng.take_guard_delay());
  else if (n == "scatter_guard_hard")
    eng.set_scatter_guard(-1.0, value);
  else if (n == "scatter_guard_delay") // the NEXT "scatter_guard" applies from the value-th force assembly after it on
    eng.set_guard_delay(iv);
  else if (n == "radial_mask")
    eng.set_radial_mask(iv != 0);
  else if (n == "radial_sync")
    eng.set_radial_sync(iv != 0);
  else if (n == "angular_fused")
    eng.set_angular_fused(iv != 0);
  else if (n == "angular_pair_trip")
    eng.set_angular_pair_trip(iv != 0);
  else if (n == "angular_flat_tables")
    eng.set_angular_flat_tables(iv != 0);
  else if (n == "lean_list_walks")
    eng.set_lean_list_walks(iv != 0);
  else if (n == "angular_only_list_a")
    eng.set_angular_only_list_a(iv != 0);
  else if (n == "rebuild_fast_pack")
    eng.set_rebuild_fast_pack(iv != 0);
  else if (n == "fold_seam")
    eng.set_fold_seam(iv != 0);
  else if (n == "brick_force") {
    if (iv != 0 && !eng.has_brick_force())
      return fail(NEPMI_ERR_ARG, "option 'brick_force': the per-brick force kernel is not part of this build (make BRICK=1)");
    eng.set_brick_force(iv != 0);
  }
  else if (n == "win_static")
    eng.set_win2(iv != 0);
  else if (n == "keep_lists_on_box_change")
    eng.set_keep_lists(iv != 0);
  else if (n == "stepwise_loops")
    eng.set_stepwise_loops(iv != 0);
  else if (n == "mfma")
    eng.set_use_mfma(iv);
  else if (n == "angular_recompute")
    eng.set_angular_recompute(iv);
  else
    return fail(NEPMI_ERR_ARG, "unknown engine option '" + n + "'");
  return NEPMI_OK;
}

} // extern "C"
