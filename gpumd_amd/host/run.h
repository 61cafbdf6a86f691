// Run: the run.in interpreter and the MD loop (src/main_gpumd/run.{cu,cuh}), restricted to the
// keywords of the hot path: potential, replicate, velocity, ensemble nve, time_step, dump_thermo,
// dump_xyz (all options but the NEP-charge quantities), dump_restart, run.
#pragma once
#include "force.h"

namespace gmi {

struct DumpXyz {
  int interval = 0;
  std::string filename;
  int precision = 1; // 1 single (%.9g, the default: dump_xyz.cuh:67), 2 double (%.17g)   -- dump_xyz.cu:163-165
  bool has_mass = false, has_charge = false, has_velocity = false, has_force = false, has_potential = false,
       has_unwrapped_position = false, has_virial = false, has_group_labels = false; // parse_utilities.cu:97-147
  bool separated = false;   // file name ended in '*': one file per frame, <name><step>  (dump_xyz.cu:104-110)
  int grouping_method = -1; // `group <method> <id>`: only that group's atoms are written (dump_xyz.cu:368-372)
  int group_id = 0;
  FILE* fid = nullptr;
};

// Dump_Observer (src/measure/dump_observer.cuh): `dump_observer <mode> <thermo> <exyz> <has_vel> <has_force>`
struct DumpObserver {
  bool active = false;
  std::string mode = "observe"; // observe: every potential re-evaluated at the output steps; average: the run's own
  int interval_thermo = 1, interval_exyz = 1, has_velocity = 0, has_force = 0;
  std::vector<FILE*> exyz_files, thermo_files; // observer<i>.xyz / observer<i>.out (no index when there is one)
};

// Active (src/measure/active.cuh): `active <interval> <has_velocity> <has_force> <has_uncertainty> <threshold>` -- committee
// uncertainty over the `potential` lines of run.in, the run itself follows the first one
struct ActiveLearning {
  bool active = false;
  int interval = 1, has_velocity = 0, has_force = 0, has_uncertainty = 0;
  double threshold = 0.0;
  FILE* exyz_file = nullptr; // active.xyz
  FILE* out_file = nullptr;  // active.out
};

// MSD (src/measure/msd.cuh) and SDC (src/measure/sdc.cuh): `compute_msd <interval> <Nc> [group <method> <id> | all_groups <method>]
// [save_every <k>]`, `compute_sdc <interval> <Nc> [group <method> <id>]`.  The sums are libnepmi's (nepmi_corr_*), sampled inside
// the run loops; normalisation, finite difference / trapezoid and the files are the host's.
struct ComputeCorr {
  bool active = false;
  int interval = 0, num_corr = 0;
  int grouping_method = -1, group_id = -1;
  bool all_groups = false;
  int save_every = 0;
  // of the run in progress
  nepmi_corr* handle = nullptr;
  int num_atoms = 0, num_groups = 1;
  std::vector<int> atoms_per_group;
  double cell[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}; // MSD::preprocess keeps the box of the run's start
  // DOS (src/measure/dos.cuh): `compute_dos <interval> <Nc> <omega_max> [group <method> <id>] [num_dos_points <n>]`, a negative
  // group id = every group of the method.  The mass-weighted sums are libnepmi's (quantity 2 of nepmi_corr_*, the weights from
  // atom.cpu_mass), the normalisation and the transform nepmi_dos_from_mvac; mvac.out and dos.out are the host's.
  double omega_max = 0.0;
  int num_dos_points = -1;
};

// RDF (src/measure/rdf.cuh): `compute_rdf <rc> <num_bins> <interval>`.  The pair counts are libnepmi's (nepmi_rdf_*), sampled inside
// the run loops; the normalisation and rdf.out are the host's.
struct ComputeRdf {
  bool active = false;
  double rc = 0.0;
  int num_bins = 0, interval = 0;
  int num_types = 0;                 // types that have atoms (RDF::parse, rdf.cu:316-323)
  std::vector<int> type_index;       // their indices in the potential's order
  std::vector<int> num_atoms;        // and their atom counts
  nepmi_rdf* handle = nullptr;       // of the run in progress
};

// Angular RDF (src/measure/angular_rdf.cuh): `compute_angular_rdf <rc> <r_bins> <theta_bins> <interval> [atom <i> <j>]...`, up to
// six `atom` groups.  The pair counts are libnepmi's (nepmi_ardf_*), sampled inside the run loops; the normalisation and
// angular_rdf.out are the host's.
struct ComputeArdf {
  bool active = false;
  double rc = 0.0;
  int num_r_bins = 0, num_theta_bins = 0, interval = 0;
  std::vector<int> pair_types;       // [pairs][2], types in the potential's order
  nepmi_ardf* handle = nullptr;      // of the run in progress
};

// ADF (src/measure/adf.cuh): `compute_adf <interval> <num_bins> <rc_min> <rc_max>` or `compute_adf <interval> <num_bins>
// (<itype> <jtype> <ktype> <rc_min_j> <rc_max_j> <rc_min_k> <rc_max_k>)+`.  The triplet counts are libnepmi's (nepmi_adf_*),
// sampled inside the run loops; the run is cut at the sample steps, where the host appends a block to adf.out.
struct ComputeAdf {
  bool active = false;
  bool global = true;
  int interval = 0, num_bins = 0;
  std::vector<nepmi_adf_row> rows;
  nepmi_adf* handle = nullptr;       // of the run in progress
};

// OrientOrder (src/measure/orientorder.cuh): `compute_orientorder <interval> cutoff <rc> | nnn <k> <ndegrees> <l...> <average>
// [<wl> [<wlhat>]]`.  The columns are libnepmi's (nepmi_orient_*), sampled inside the run loops; the run is cut at the sample
// steps, where the host appends a block of the last sample to orientorder.out.
struct ComputeOrient {
  bool active = false;
  int interval = 0, mode = 0, nnn = 0;
  double rc = 6.0;
  std::vector<int> degrees;
  bool average = false, wl = false, wlhat = false;
  nepmi_orient* handle = nullptr;    // of the run in progress
};

// One process per GPU (torchrun / mpirun style launch: RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR, MASTER_PORT or
// OMPI_COMM_WORLD_*): the run is domain-decomposed by libnepmi's nepmi_dist_* driver (RCCL over xGMI when every
// rank has its own GPU, TCP sockets otherwise); rank 0 writes the output files.
struct Parallel {
  int rank = 0, world = 1, local_rank = 0;
  bool use_rccl = false;
  std::string master_addr = "127.0.0.1";
  int master_port = 29400;
};

class Run
{
public:
  Run(bool check_only, const Parallel& par);
  ~Run();
  void execute_run_in();

private:
  void parse_one_keyword(const std::vector<std::string>& tokens);
  void perform_a_run();
  void perform_a_run_dist();
  void run_segment(int steps, double t_a, double t_b);
  void correct_velocity_now();
  void setup_dist(const std::vector<std::string>& potential_line);
  void dist_setup_atoms();
  void find_thermo();
  void dump_thermo(int step);
  void dump_xyz(DumpXyz& d, int step);
  void dump_restart(int step);
  void dump_observer_open();
  void dump_observer_process(int step);
  void dump_observer_write(int step, int file_index);
  void dump_observer_close();
  void active_open();
  void active_process(int step);
  void active_close();
  void parse_compute_corr(const std::vector<std::string>& p, bool msd);
  void corr_open(ComputeCorr& c, int quantity, const char* name);
  void corr_close(ComputeCorr& c);
  void corr_sample_stepwise();
  void write_msd(const char* filename);
  void write_sdc();
  void parse_compute_dos(const std::vector<std::string>& p);
  void write_dos();
  void parse_compute_rdf(const std::vector<std::string>& p);
  void rdf_open();
  void rdf_close();
  void write_rdf();
  void parse_compute_angular_rdf(const std::vector<std::string>& p);
  void ardf_open();
  void ardf_close();
  void write_angular_rdf();
  void parse_compute_adf(const std::vector<std::string>& p);
  void adf_open();
  void adf_close();
  void write_adf(int step);
  void parse_compute_orientorder(const std::vector<std::string>& p);
  void orient_open();
  void orient_close();
  void write_orient(int step);

  bool check_only_;
  Parallel par_;
  nepmi_transport boot_{};      // TCP: the rendezvous, and the transport itself when RCCL is not used
  nepmi_transport rccl_{};
  bool have_boot_ = false, have_rccl_ = false;
  nepmi_model* dist_model_ = nullptr;
  nepmi_dist* dist_ = nullptr;
  bool dist_ready_ = false;
  double* nhc_state_ = nullptr; // stepwise path (several potentials averaged): the chain of this run
  int correct_interval_ = 0, correct_group_method_ = -1; // correct_velocity (run.cu:610-647)
  Box box;
  Atom atom;
  std::vector<Group> groups;
  Force force;
  bool has_velocity_in_xyz = false;
  bool gpu_allocated = false;
  std::string ensemble = "nve";
  double temperature1 = 300.0, temperature2 = 300.0, temperature_coupling = 100.0; // nvt_ber, nvt_nhc
  // npt_ber (Integrate::parse_ensemble, integrate.cu:631-715): natural units after parsing, Voigt order xx yy zz yz xz xy for 6
  int num_target_pressure_components = 0;
  double target_pressure[6] = {0, 0, 0, 0, 0, 0}, pressure_coupling[6] = {0, 0, 0, 0, 0, 0};
  double time_step = 1.0 / TIME_UNIT_CONVERSION;
  double global_time = 0.0;
  int number_of_steps = 0;
  double initial_temperature = 300.0;
  int dump_thermo_interval = 0;
  int dump_restart_interval = 0;
  std::vector<DumpXyz> dump_xyzs;
  DumpObserver observer;
  ActiveLearning active_;
  ComputeCorr msd_, sdc_, dos_;
  ComputeRdf rdf_;
  ComputeArdf ardf_;
  ComputeAdf adf_;
  ComputeOrient orient_;
  int corr_steps_ = 0; // finished steps of the run in progress (the paths that step by hand sample on it)
  GPU_Vector<double> thermo; // 8 doubles
  std::vector<std::string> elements;
  std::string potential_file;
};

} // namespace gmi
