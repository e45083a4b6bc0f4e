// fpx_engine.hip -- the host side of the library: EngineBase, Engine<R> (one process drives one GPU through one handle; all
// particle state and all met fields stay resident in HBM between calls), the factory of the fp32 engine, the dispatchers
// to the step kernels' tables, and the C ABI of include/flexpart_amd.h.  No device code lives here: every kernel sits in
// the header of its feature (fpx_fields.hpp, fpx_sort.hpp, fpx_particles.hpp, fpx_outgrid.hpp, fpx_probes.hpp, the
// headers of the newer features), and the three kernels of the particle step are translation units of their own
// (fpx_step_prep.hip, fpx_step_loop.hip; fpx_tu.hpp).
#define FPX_TU_PART 0
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <rccl/rccl.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/flexpart_amd.h"
#include "fpx_tu.hpp"
#include "fpx_device.hpp"
#include "fpx_verttransform.hpp"
#include "fpx_verttransform_gfs.hpp"
#include "fpx_calcpar.hpp"
#include "fpx_calcpar_gfs.hpp"
#include "fpx_getvdep.hpp"
#include "fpx_calcpv.hpp"
#include "fpx_calcfluxes.hpp"
#include "fpx_partavg.hpp"
#include "fpx_initcond.hpp"
#include "fpx_ohreaction.hpp"
#include "fpx_plumetraj.hpp"
#include "fpx_domainfill.hpp"
#include "fpx_convect.hpp"
#include "fpx_convect_gfs.hpp"
#include "fpx_step_common.hpp"
#include "fpx_fields.hpp"
#include "fpx_sort.hpp"
#include "fpx_particles.hpp"
#include "fpx_outgrid.hpp"
#include "fpx_probes.hpp"
#include "fpx_rng_host.hpp"
#include "fpx_host_res.hpp"
#include "fpx_recfile.hpp"

namespace fpx {

// shared by the translation units (fpx_tu.hpp): the message behind fpx_last_error()
#if FPX_TU_REAL == 4
extern thread_local std::string g_err;
#else
thread_local std::string g_err;
#endif
static int fail(int code, const std::string &msg) { g_err = msg; return code; }

#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(FPX_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// ---------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------
// one type for all translation units
struct EngineBase {
  virtual ~EngineBase() {}
  virtual int set_height(const void *h, int n) = 0;
  virtual int upload_fields(int slot, const fpx_fields *f) = 0;
  virtual int verttransform(int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out) = 0;
  virtual int verttransform_nest(int nest, int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out) = 0;
  virtual int verttransform_gfs(int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out, void *pplev_out) = 0;
  virtual int calcpar(int slot, const fpx_calcpar_in *c, const fpx_calcpar_out *out) = 0;
  virtual int calcpar_nest(int nest, int slot, const fpx_calcpar_in *c, const fpx_calcpar_out *out) = 0;
  virtual int calcpar_gfs(int slot, const fpx_calcpar_gfs_in *c, const fpx_calcpar_out *out) = 0;
  virtual double cp_ms() = 0;
  virtual int getvdep_init(const fpx_getvdep_tables *t) = 0;
  virtual int getvdep(int slot, const fpx_getvdep_in *g, void *vdep_out) = 0;
  virtual int getvdep_nest_init(int nest, const void *xlandusen) = 0;
  virtual int getvdep_nest(int nest, int slot, const fpx_getvdep_in *g, void *vdep_out) = 0;
  virtual double gv_ms() = 0;
  virtual int calcpv_init(const fpx_calcpv_cfg *c) = 0;
  virtual int get_pvh(int nest, void *pvh_out) = 0;
  virtual double pv_ms() = 0;
  virtual int set_windtime(const int32_t mt[2], const int32_t mi[2]) = 0;
  virtual int rng_fill_table() = 0;
  virtual int rng_set_table(const void *t, int n) = 0;
  virtual int rng_get_table(void *t, int n) = 0;
  virtual int upload_particles(long long first, long long count, const fpx_particles *p) = 0;
  virtual int download_particles(long long first, long long count, const fpx_particles *p) = 0;
  virtual int set_numpart(long long n) = 0;
  virtual int set_release_points(int numpoint, const void *xmass, const int32_t *npart) = 0;
  virtual int set_release_heights(int numpoint, const void *zpoint1, const void *zpoint2) = 0;
  virtual int release_init(const fpx_release *r) = 0;
  virtual int releaseparticles(int itime, int64_t *numpart, int32_t *numparticlecount, void *xmasssave, void *rho_rel, int64_t *nreleased) = 0;
  virtual int split_particles(int itime, int64_t *numpart) = 0;
  virtual size_t redist_bytes(int64_t num_trans) = 0;
  virtual int redist_pack(int itime, int64_t num_trans, void *buf, size_t buf_bytes, int64_t *numpart) = 0;
  virtual int redist_unpack(int itime, int64_t num_trans, const void *buf, size_t buf_bytes, int64_t *numpart) = 0;
  virtual int step(int itime, fpx_step_stats *st, bool async) = 0;
  virtual int sync() = 0;
  virtual int counters(fpx_step_stats *out, int reset) = 0;
  virtual int kernel_time(double *ms, long long *launches, int reset, double *parts) = 0;
  virtual int sort_particles() = 0;
  virtual int seed_particles(long long n, unsigned long long seed, double frac_pbl, double zmax, double lat_margin,
                             int itime0) = 0;
  virtual int outgrid_init(const fpx_outgrid *g, const void *outheight) = 0;
  virtual int set_output_times(int loutnext, int loutstep) = 0;
  virtual int conccalc(int itime, double weight) = 0;
  virtual int get_grids(void *gridunc, void *drygridunc, int allreduce, int clear) = 0;
  virtual int get_flux(void *flux, int allreduce, int clear) = 0;
  virtual int fluxoutput(int itime, const fpx_fluxout *f, const char *prefix, int reduced) = 0;
  virtual int calcfluxes_time(double *ms, long long *launches, int reset) = 0;
  virtual int get_partavg(long long first, long long count, int32_t *npart_av, void *const *sums) = 0;
  virtual int partoutput_average(int itime, const char *prefix, int64_t *nrecords) = 0;
  virtual int partavg_time(double *ms, long long *launches, int reset) = 0;
  virtual int initcond_finish(int itime) = 0;
  virtual int get_initcond(void *init_cond, int allreduce, int clear) = 0;
  virtual int initial_cond_output(int itime, const fpx_initout *o, const char *prefix, int reduced) = 0;
  virtual int initcond_time(double *ms, long long *launches, int reset) = 0;
  virtual int plumetraj_init(const fpx_plumetraj_cfg *c) = 0;
  virtual int plumetraj(int itime, const char *path, int32_t *nrecords) = 0;
  virtual int get_plumetraj(int max_records, int32_t *jpoint, int32_t *npart, int32_t *iterations, int32_t *numb, void *values, int ld) = 0;
  virtual double plumetraj_ms() = 0;
  virtual int domainfill_init(const fpx_domainfill_cfg *c) = 0;
  virtual int boundcond_domainfill(int itime, int64_t *numpart, int32_t *numparticlecount, fpx_domainfill_stats *out) = 0;
  virtual int domainfill_acc(void *we, void *sn, const void *we_in, const void *sn_in) = 0;
  virtual int boundcond_output(const char *path) = 0;
  virtual double domainfill_ms() = 0;
  virtual int count_particles(int64_t *local, int64_t *total, int allreduce) = 0;
  virtual int lane_stats(uint64_t *out, int n, int reset) = 0;
  virtual int set_option(const char *name, const char *value) = 0;
  virtual int get_info(const char *name, int64_t *value) = 0;
  virtual int comm_init(const void *id, int nbytes, int nranks, int rank) = 0;
  virtual int comm_init_host(int nranks, int rank, fpx_allreduce_fn fn, void *user) = 0;
  virtual int nests_init(const fpx_nests *n) = 0;
  virtual int upload_nest_fields(int nest, int slot, const fpx_fields *f) = 0;
  virtual int wet_init(const fpx_wet_config *w) = 0;
  virtual int upload_wet_fields(int slot, const fpx_wet_fields *f) = 0;
  virtual int upload_wet_nest_fields(int nest, int slot, const fpx_wet_fields *f, int readclouds_nest) = 0;
  virtual int wetdepo(int itime, int ltsample, int loutnext) = 0;
  virtual int get_wetgrid(void *wetgridunc, int allreduce) = 0;
  virtual int oh_init(const fpx_oh_config *c) = 0;
  virtual int gethourlyOH(int itime) = 0;
  virtual int ohreaction(int itime, int ltsample, int loutnext) = 0;
  virtual int get_oh_hourly(void *oh_hourly, void *memohtime) = 0;
  virtual int set_oh_hourly(const void *oh_hourly, const void *memohtime) = 0;
  virtual int ohreaction_ms(double *ms) = 0;
  virtual int outgrid_nest_init(const fpx_outgrid_nest *g) = 0;
  virtual int get_grids_nest(void *griduncn, void *drygriduncn, void *wetgriduncn, int allreduce, int clear) = 0;
  virtual int receptors_init(int n, const void *x, const void *y, const void *area) = 0;
  virtual int get_receptors(void *creceptor, int ld, int allreduce, int clear) = 0;
  virtual void *stream_ptr() = 0;
  virtual double vt_ms() = 0;
  virtual double po_ms() = 0;
  virtual int upload_diag_fields(int slot, const fpx_diag_fields *f) = 0;
  virtual int upload_diag_nest_fields(int nest, int slot, const fpx_diag_fields *f) = 0;
  virtual int partoutput(int itime, const char *path, int64_t *nrec) = 0;
  virtual int concoutput(int itime, const fpx_concout *c, const char *prefix, int clear) = 0;
  virtual int readpartpositions(const char *path, const fpx_restart *r, int64_t *numpart_out, int32_t *numparticlecount, int32_t *itimein) = 0;
  virtual int conv_init(const fpx_conv_config *c) = 0;
  virtual int upload_conv_fields(int slot, const fpx_conv_fields *f) = 0;
  virtual int convmix(int itime, int64_t *nmoved) = 0;
  virtual int cbaseflux_io(void *host, bool set) = 0;
  virtual int upload_conv_nest_fields(int nest, int slot, const fpx_conv_fields *f) = 0;
  virtual int cbaseflux_nest_io(int nest, void *host, bool set) = 0;
  virtual double conv_ms() = 0;
  virtual int conv_columns(const int32_t *col, int ncol, int32_t *lconv, int32_t *nconvtop, void *fmassfrac, void *uvzlev) = 0;
  virtual int conv_init_gfs(const fpx_conv_gfs_config *c) = 0;
  virtual int upload_conv_gfs_fields(int slot, const fpx_conv_gfs_fields *f) = 0;
  virtual int conv_soundings(const int32_t *col, int ncol, void *psconv, void *pconv, void *phconv, void *dpr, void *tconv, void *qconv) = 0;
  virtual int checkpoint_write(const char *path, int itime, int numparticlecount) = 0;
  virtual int checkpoint_read(const char *path, int32_t *itime, int64_t *numpart_out, int32_t *numparticlecount) = 0;
};
EngineBase *make_engine_f32(const fpx_config *cfg, int *rc);   // defined by the unit that holds Engine<float>
// The three kernels of the step are compiled in units of their own (fpx_step_prep.hip, fpx_step_loop.hip) and reach the
// engine as untyped host-stub addresses; the engine casts them to the kernel's signature (same headers, same layout).
// real_bytes 8|4 picks the arithmetic type.
const void *step_kernel_prep(int real_bytes, bool drydep, bool init, bool polar, bool nest);
const void *step_kernel_loop(int real_bytes, bool lean, int turbswitch, int cblflag, int rng_mode, bool susp, bool *is_lean);
const void *step_kernel_finish(int real_bytes, bool drydep, bool polar, bool nest);
FPX_TU_OPEN

template <typename R>
struct Engine : EngineBase {
  fpx_config cfg;
  hipStream_t stream = nullptr;
  View<R> V;
  Parts<R> P;
  bool maybe_new = true;   // particles may have been released since the last step
  // A particle is initialised in the step whose time equals its itramem (timemanager.f90:553) -- normally the step after it was
  // released or uploaded (maybe_new).  A host may also hand over particles that are born LATER (itra1 = itramem in the future):
  // the instance of k_prep that can initialize() runs at every step up to the latest birth among the particles the host placed
  // (found by one reduction over the particle arrays at the first step after an upload, a warm start, a restore or a receive).
  bool births_unknown = true;
  long long birth_horizon = LLONG_MIN;   // ldirect * itramem, the latest among the live particles at the last such event
  int find_birth_horizon() {
    births_unknown = false;
    birth_horizon = LLONG_MIN;
    if (numpart == 0) return 0;
    int rc;
    if (!d_count && (rc = dalloc(&d_count, 4))) return rc;
    const long long init = LLONG_MIN;
    HIPCHK(hipMemcpyAsync(d_count, &init, sizeof(long long), hipMemcpyHostToDevice, stream));
    const int nb = (int)std::min<long long>((numpart + 255) / 256, 256 * 16);
    k_birth_max<<<nb, 256, 0, stream>>>(P.itra1, P.itramem, numpart, cfg.ldirect, d_count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&birth_horizon, d_count, sizeof(long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  bool height_set = false, window_set = false, table_set = false, slot_loaded[2] = {false, false};
  long long numpart = 0;
  // owned device memory
  std::vector<void *> owned;
  Scratch staging;
  unsigned int *slot_of_pid = nullptr;   // only after a locality sort; read it through slot_map()
  bool slot_map_dirty = false;
  // Time-blended wind packs of the step in flight (View::w3t0 / w3t1).  Worth their 0.65 GB of extra traffic per step only
  // for a large cloud.  Blended and unblended gathers round differently, so the switch is a function of the configuration
  // alone -- fpx_config.blend_mode, or in its automatic mode the run's particle count over ALL ranks (global_particles) --
  // never of what this rank or this step happens to hold: runs with different rank counts, restarted runs and runs under
  // fpx_step_async stay bitwise equal (README_PARALLEL.md:189-192).
  R *d_w3t[2] = {nullptr, nullptr}, *d_r2t = nullptr;
  static constexpr long long kBlendMinGlobal = 30000000ll;
  bool blend_on() const {
    if (cfg.blend_mode == 1) return true;
    if (cfg.blend_mode == 2) return false;
    return (cfg.global_particles > 0 ? cfg.global_particles : cfg.max_particles) >= kBlendMinGlobal;
  }
  unsigned long long blended_steps = 0;
  int blend_winds(int itime) {
    V.w3t0 = nullptr; V.w3t1 = nullptr; V.r2t0 = nullptr;
    if (!blend_on()) return 0;
    blended_steps++;
    const long long npoint = (long long)cfg.nx * cfg.ny * cfg.nz;
    int rc;
    for (int k = 0; k < 2; k++)
      if (!d_w3t[k]) { if ((rc = dalloc(&d_w3t[k], (size_t)npoint * 3))) return rc; }
    if (!d_r2t) { if ((rc = dalloc(&d_r2t, (size_t)npoint * 2))) return rc; }
    const int t1 = itime + std::abs(cfg.lsynctime) * cfg.ldirect;   // the time of advance.f90:836-841 (ldt = |lsynctime| there)
    const bool have1 = std::abs((long long)t1) <= std::abs((long long)V.memtime1);      // advance.f90:836: no Petterssen step beyond the window
    const R dt1a = (R)(itime - V.memtime0), dt2a = (R)(V.memtime1 - itime), dtta = (R)1 / (dt1a + dt2a);
    const R dt1b = (R)(t1 - V.memtime0), dt2b = (R)(V.memtime1 - t1), dttb = have1 ? (R)1 / (dt1b + dt2b) : (R)0;
    k_blend_w3<R><<<(int)((npoint + 255) / 256), 256, 0, stream>>>(V.w3, V.r2, npoint, V.m1, V.m2, dt1a, dt2a, dtta, dt1b, dt2b, dttb,
                                                                     d_w3t[0], have1 ? d_w3t[1] : (R *)nullptr, d_r2t);
    HIPCHK(hipGetLastError());
    V.w3t0 = d_w3t[0];
    V.r2t0 = d_r2t;
    V.w3t1 = have1 ? d_w3t[1] : nullptr;
    return 0;
  }
  const unsigned int *slot_map() {
    if (slot_of_pid && slot_map_dirty) {
      k_slot_map<<<(int)((P.cap + kBlock - 1) / kBlock), kBlock, 0, stream>>>(P.pid, P.cap, d_slot_of_pid);
      slot_map_dirty = false;
    }
    return slot_of_pid;
  }
  unsigned int *d_slot_of_pid = nullptr;
  Parts<R> P2;                           // second particle buffer set (sort ping-pong), allocated lazily
  bool have_p2 = false;
  unsigned int *d_keys = nullptr, *d_keys2 = nullptr, *d_vals = nullptr, *d_vals2 = nullptr;
  Scratch d_sort_tmp;
  Stats *d_stats = nullptr;
  unsigned int *d_pbl_list = nullptr, *d_pbl_ctr = nullptr;   // the counters of the work list and of the launches that go through it (layout: k_list_counts)
  unsigned int *d_surv[2] = {nullptr, nullptr};               // lists of the suspended particles (ping-pong between launches), allocated with the first sliced step
  std::vector<int> slice_caps;                                // pass budget of each launch of the Langevin kernel, the last one 0 (none)
  struct Options {                                            // fpx_set_option
    int verbose = 0, pbl_blocks_per_cu = 0, prep_lds_pad = 0, permute = 0 /* 0 auto, 1 direct, 2 staged */, vt_unfused = 0;
    long conv_scratch_mb = 0;
    int conv_one_lane = 0, conv_no_walk = 0, conv_rows_plain = 0;
    int pbl_grid_blocks = 0, finish_blocks = 0;   // tests: upper bounds on the grids of k_pbl_loop / k_pbl_finish (0 = none)
    int pbl_drain_lanes = -1;                     // -1: the engine's default (FPX_DRAIN_LANES)
    int prep_init_always = 0;                     // measurements: every step runs the instance of k_prep that can initialize() new particles
    int pbl_cost_buckets = FPX_COST_BUCKETS;      // -1: by the size of this rank's cloud
    std::vector<int> pbl_slices;
  } opt;
  int drain_lanes() const { return opt.pbl_drain_lanes >= 0 ? opt.pbl_drain_lanes : FPX_DRAIN_LANES; }
  unsigned char *d_pbl_flag = nullptr, *d_pbl_flag2 = nullptr;
  unsigned int *d_iota = nullptr;
  PblRec<R> Q;
  GridP<R> Gp;
  WetP<R> Wp;
  bool wet_on = false, wet_slot[2] = {false, false};
  WetNest<R> h_wnest[kMaxNests] = {};     // host copy of the device table Wp.nest
  WetNest<R> *d_wnest = nullptr;
  bool wet_nest_slot[kMaxNests][2] = {};
  ncclComm_t comm = nullptr;
  int comm_ranks = 1, comm_rank = 0;
  long long rel_global_count = 0;        // particles released so far by all ranks (key of the release's counter RNG)
  // host-supplied all-reduce (fpx_comm_init_host): the transport of an MPI host, or gloo in the tests
  fpx_allreduce_fn host_allreduce = nullptr;
  void *host_allreduce_user = nullptr;
  Scratch red_pin{true};                 // pinned bounce buffer of the host transport: [send | recv]
  // The output accumulators' sums over the ranks (fpx_host_res.hpp), one per accumulator: the reference's gridunc0,
  // drygridunc0, wetgridunc0, griduncn0, ... and creceptor0 (mpi_mod.f90:2451-2492,2543-2569; allocated in
  // outgrid_init.f90:220-225), and the same for flux and init_cond.  The per-rank partial sums stay untouched in Gp.*,
  // fx_flux and ic_grid: drygridunc / wetgridunc accumulate over the whole run and are reduced again at every output
  // time.  The extents are set where the accumulators are allocated (sum_grid.count() elements of gridunc, ...).
  RankSum sum_grid, sum_dry, sum_wet, sum_gridn, sum_dryn, sum_wetn, sum_rec, sum_flux, sum_ic;
  Scratch d_sel_tmp;
  int pbl_grid = 0, pbl_per_cu = 0;
  // TABLE_SEQ state
  HostRng<float> rng4;
  HostRng<double> rng8;
  std::vector<float> tab4;
  std::vector<double> tab8;
  int *d_nrand_adv = nullptr, *d_nrand_init = nullptr;
  float *d_dcas4 = nullptr, *d_dcas14 = nullptr;
  double *d_dcas8 = nullptr, *d_dcas18 = nullptr;
  unsigned char *d_flags = nullptr;
  std::vector<unsigned char> h_flags;
  std::vector<int> h_nrand_adv, h_nrand_init;
  std::vector<float> h_dcas4, h_dcas14;
  std::vector<double> h_dcas8, h_dcas18;
  // timing
  // events: before k_prep | before k_pbl_loop | after it | after k_pbl_finish | after k_prep (before the work-list sort)
  // intervals: the step | k_prep + work list | k_pbl_loop | k_pbl_finish | k_prep alone
  IntervalTimer<5> step_timer{{0, 3}, {0, 1}, {1, 2}, {2, 3}, {0, 4}};
  unsigned int step_counter = 0;

  template <typename T>
  int dalloc(T **p, size_t n) {
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T));
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    owned.push_back(q);
    *p = (T *)q;
    return 0;
  }

  int init(const fpx_config *c) {
    cfg = *c;
    if (cfg.nz > kMaxNz) return fail(FPX_ERR_ARG, "nz exceeds the engine's level limit (512)");
    if (cfg.nx < 2 || cfg.ny < 2 || cfg.nz < 2) return fail(FPX_ERR_ARG, "grid too small");
    if ((long long)cfg.nx * cfg.ny * cfg.nz > 0xFFFFFFF0ll) return fail(FPX_ERR_ARG, "grid too large: nx*ny*nz must fit 32 bits (the kernels index grid cells with 32-bit integers)");
    if (cfg.nxmax < cfg.nx || cfg.nymax < cfg.ny || cfg.nzmax < cfg.nz) return fail(FPX_ERR_ARG, "allocated extents smaller than used extents");
    if (cfg.nspec < 1 || cfg.nspec > FPX_MAXSPEC || cfg.maxspec < cfg.nspec) return fail(FPX_ERR_ARG, "bad nspec/maxspec");
    if (cfg.max_particles < 1 || cfg.max_particles > 0xFFFFFFF0ll) return fail(FPX_ERR_ARG, "bad max_particles");
    if (cfg.ifine < 1) return fail(FPX_ERR_ARG, "ifine must be >= 1");
    if (cfg.lsynctime == 0 || std::abs((long long)cfg.lsynctime) > 65535) return fail(FPX_ERR_ARG, "lsynctime must be non-zero and at most 65535 s in magnitude (the hand-over record of the Langevin kernel keeps |itimec - itime| in 16 bits)");
    if (cfg.device_partavg != 0 && cfg.device_partavg != 1) return fail(FPX_ERR_ARG, "device_partavg must be 0 or 1");
    if (cfg.device_partavg == 1 && cfg.ipout != 3) return fail(FPX_ERR_ARG, "device_partavg = 1 without ipout = 3: there are no averages to compute");
    if (cfg.ipout == 3 && !cfg.device_partavg) return fail(FPX_ERR_UNSUPPORTED, "ipout = 3: the particle loop's partpos_average (timemanager.f90:617) is not computed by this engine");
    if (cfg.device_flux != 0 && cfg.device_flux != 1) return fail(FPX_ERR_ARG, "device_flux must be 0 or 1");
    if (cfg.device_flux == 1 && cfg.iflux != 1) return fail(FPX_ERR_ARG, "device_flux = 1 without iflux = 1: there is no flux to compute");
    if (cfg.iflux == 1 && !cfg.device_flux) return fail(FPX_ERR_UNSUPPORTED, "iflux = 1: the particle loop's calcfluxes (timemanager.f90:623) is not computed by this engine");
    if (cfg.linit_cond >= 1 && !cfg.device_initcond) return fail(FPX_ERR_UNSUPPORTED, "linit_cond >= 1: the particle loop's initial_cond_calc (timemanager.f90:631,702) is not computed by this engine");
    if (cfg.device_initcond != 0 && cfg.device_initcond != 1) return fail(FPX_ERR_ARG, "device_initcond must be 0 or 1");
    if (cfg.device_initcond == 1 && cfg.linit_cond != 1 && cfg.linit_cond != 2) return fail(FPX_ERR_ARG, "device_initcond = 1 needs linit_cond = 1 or 2: there is no sensitivity to compute");
    if (cfg.device_initcond == 1 && cfg.ldirect == 1) return fail(FPX_ERR_ARG, "device_initcond = 1 with ldirect = 1: the sensitivity to initial conditions belongs to backward runs (readcommand.f90:349)");
    if (cfg.lsettling && cfg.compute_real_bytes == 4 && (long long)cfg.nx * cfg.ny > (1ll << 24)) return fail(FPX_ERR_ARG, "lsettling with the f32 engine: nx*ny must not exceed 2^24 (the Langevin kernel keeps the column index of get_settling in an f32 stash slot)");
    if (cfg.blend_mode < 0 || cfg.blend_mode > 2) return fail(FPX_ERR_ARG, "blend_mode must be 0 (automatic), 1 (on) or 2 (off)");
    if (cfg.global_particles < 0) return fail(FPX_ERR_ARG, "global_particles must not be negative");
    if (cfg.pbl_slice_passes < -1) return fail(FPX_ERR_ARG, "pbl_slice_passes must be -1 (one launch), 0 (the engine's schedule) or a pass budget");
    HIPCHK(hipSetDevice(cfg.device));
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    memset(&V, 0, sizeof(V));
    memset(&P, 0, sizeof(P));
    memset(&Gp, 0, sizeof(Gp));
    // scalars: typed exactly as the reference's default-real variables
    V.nx = cfg.nx; V.ny = cfg.ny; V.nz = cfg.nz; V.nxmin1 = cfg.nx - 1; V.nymin1 = cfg.ny - 1; V.nmixz = cfg.nmixz;
    V.dx = (R)cfg.dx; V.dy = (R)cfg.dy; V.xlon0 = (R)cfg.xlon0; V.ylat0 = (R)cfg.ylat0;
    {  // gridcheck_ecmwf.f90:311-312 with par_mod.f90:59 r_earth, pi
      const R r_earth = (R)6.371e6, pi = (R)3.14159265;
      V.dxconst = (R)180. / (V.dx * r_earth * pi);
      V.dyconst = (R)180. / (V.dy * r_earth * pi);
    }
    V.xglobal = cfg.xglobal; V.nglobal = cfg.nglobal; V.sglobal = cfg.sglobal;
    V.switchnorthg = (R)cfg.switchnorthg; V.switchsouthg = (R)cfg.switchsouthg;
    for (int i = 0; i < 9; i++) { V.northpolemap[i] = (R)cfg.northpolemap[i]; V.southpolemap[i] = (R)cfg.southpolemap[i]; }
    V.polemaps = nullptr;   // allocated below, with the other device arrays
    V.ldirect = cfg.ldirect; V.lsynctime = cfg.lsynctime; V.method = cfg.method; V.mintime = cfg.mintime;
    V.ifine = cfg.ifine; V.turbswitch = cfg.turbswitch; V.cblflag = cfg.cblflag; V.mdomainfill = cfg.mdomainfill;
    V.lsettling = cfg.lsettling; V.nspec = cfg.nspec; V.drydep = cfg.drydep;
    V.turboff = cfg.turboff != 0; V.interpolhmix = cfg.interpolhmix != 0;
    V.pbl_cost_buckets = 0;   // set per step (Engine::step)
    V.ctl = (R)cfg.ctl; V.fine = (R)1. / (R)cfg.ifine;   // readcommand.f90:271
    V.d_trop = (R)cfg.d_trop; V.d_strat = (R)cfg.d_strat; V.turbmesoscale = (R)cfg.turbmesoscale;
    for (int i = 0; i < FPX_MAXSPEC; i++) {
      V.drydepspec[i] = cfg.drydepspec[i];
      V.density[i] = (R)cfg.density[i]; V.dquer[i] = (R)cfg.dquer[i]; V.vsetaver[i] = (R)cfg.vsetaver[i];
      V.cunningham[i] = (R)cfg.cunningham[i]; V.decay[i] = (R)cfg.decay[i];
    }
    V.lage_last = cfg.lage_last; V.mquasilag = cfg.mquasilag;
    V.numpoint = 0; V.rel_xmass = nullptr; V.rel_npart = nullptr; V.rel_nsp = nullptr;
    V.rng_mode = cfg.rng_mode; V.seed = cfg.seed; V.maxrand = 1000000;
    if (cfg.particle_base < 0 || cfg.particle_base + cfg.max_particles > 0xFFFFFFF0ll) return fail(FPX_ERR_ARG, "particle_base + max_particles must fit 32 bits");
    if (cfg.particle_base != 0 && cfg.rng_mode == FPX_RNG_TABLE_SEQ) return fail(FPX_ERR_ARG, "particle_base: the serial-stream RNG mode (TABLE_SEQ) is a single-rank mode");
    V.pid_base = (unsigned int)cfg.particle_base;
    V.eps = (R)(cfg.par_nxmax > 0 ? cfg.par_nxmax : cfg.nxmax) / (R)3.e5;   // advance.f90:107
    V.numbnests = 0;
    V.nest = nullptr;

    const size_t ncol = (size_t)cfg.nx * cfg.ny, nlev = ncol * cfg.nz;
    R *p;
    int rc;
    if ((rc = dalloc(&p, cfg.nz))) return rc; V.height = p;
    {
      R maps[18];
      for (int i = 0; i < 9; i++) { maps[i] = V.northpolemap[i]; maps[9 + i] = V.southpolemap[i]; }
      if ((rc = dalloc(&p, 18))) return rc;
      HIPCHK(hipMemcpy(p, maps, sizeof(maps), hipMemcpyHostToDevice));
      V.polemaps = p;
    }
    {
      R rows[kMaxSpec][4];
      for (int i = 0; i < kMaxSpec; i++) { rows[i][0] = V.density[i]; rows[i][1] = V.dquer[i]; rows[i][2] = V.vsetaver[i]; rows[i][3] = V.cunningham[i]; }
      if ((rc = dalloc(&p, kMaxSpec * 4))) return rc;
      HIPCHK(hipMemcpy(p, rows, sizeof(rows), hipMemcpyHostToDevice));
      V.spec = p;
    }
    if ((rc = dalloc(&p, nlev * 6))) return rc; V.w3 = p;
    HIPCHK(hipMemsetAsync(p, 0, nlev * 6 * sizeof(R), stream));
    if (cfg.nglobal || cfg.sglobal) {
      if ((rc = dalloc(&p, nlev * 6))) return rc; V.w3pol = p;
      HIPCHK(hipMemsetAsync(p, 0, nlev * 6 * sizeof(R), stream));
    }
    if ((rc = dalloc(&p, nlev * 4))) return rc; V.r2 = p;
    HIPCHK(hipMemsetAsync(p, 0, nlev * 4 * sizeof(R), stream));
    if ((rc = dalloc(&p, ncol * 8))) return rc; V.sfc = p;
    HIPCHK(hipMemsetAsync(p, 0, ncol * 8 * sizeof(R), stream));
    if ((rc = dalloc(&p, ncol))) return rc; V.hcell = p;
    if ((rc = dalloc(&p, ncol))) return rc; V.tropo = p;
    if (cfg.drydep) { if ((rc = dalloc(&p, ncol * 2 * cfg.nspec))) return rc; V.vdep = p; }
    if (cfg.lsettling) { if ((rc = dalloc(&p, nlev * 2))) return rc; V.rhott = p; }
    if ((rc = dalloc(&p, V.maxrand))) return rc; V.rannumb = p;
    if ((rc = dalloc(&d_stats, 1))) return rc;
    HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(Stats), stream));

    const size_t cap = (size_t)cfg.max_particles;
    P.cap = (long long)cap;
    if ((rc = dalloc(&P.xt, cap))) return rc;
    if ((rc = dalloc(&P.yt, cap))) return rc;
    R **rs[] = {&P.zt, &P.up, &P.vp, &P.wp, &P.us, &P.vs, &P.ws};
    for (auto q : rs) if ((rc = dalloc(q, cap))) return rc;
    int **is[] = {&P.idt, &P.itra1, &P.itramem, &P.npoint, &P.nclass, &P.itrasplit};
    for (auto q : is) if ((rc = dalloc(q, cap))) return rc;
    if ((rc = dalloc(&P.cbt, cap))) return rc;
    if ((rc = dalloc(&P.xmass1, cap * cfg.nspec))) return rc;
    if (cfg.drybkdep || cfg.wetbkdep) {
      // backward runs with receptor scavenging (readcommand.f90:320-340): xscav_frac1(maxpart,maxspec), -1 = not yet scavenged
      if (cfg.ldirect != -1) return fail(FPX_ERR_ARG, "drybkdep / wetbkdep are options of backward runs (ldirect = -1)");
      if (cfg.drybkdep && cfg.wetbkdep) return fail(FPX_ERR_ARG, "drybkdep and wetbkdep exclude each other (COMMAND ind_receptor 3 or 4)");
      if ((rc = dalloc(&P.xscav, cap * cfg.nspec))) return rc;
      k_fill<R><<<(int)((cap * cfg.nspec + kBlock - 1) / kBlock), kBlock, 0, stream>>>(P.xscav, (R)-1, 0, (long long)(cap * cfg.nspec), nullptr);
    }
    if ((rc = dalloc(&P.pid, cap))) return rc;
    if (cfg.device_partavg && (rc = partavg_alloc(0))) return rc;
    if ((rc = dalloc(&d_pbl_list, cap))) return rc;
    if ((rc = dalloc(&d_pbl_ctr, kCtrWords))) return rc;
    if ((rc = dalloc(&d_pbl_flag, cap))) return rc;
    if ((rc = dalloc(&d_pbl_flag2, cap))) return rc;
    if ((rc = dalloc(&d_iota, cap))) return rc;
    memset(&Q, 0, sizeof(Q));
    {
      if ((rc = dalloc(&Q.rec, cap))) return rc;
      if (cfg.drydep && (rc = dalloc(&Q.tdep, cap))) return rc;
    }
    // every storage space starts zeroed (releaseparticles leaves the turbulent state of a space it takes as it finds it;
    // the host's arrays start from zero too), dead (FLEXPART.f90:315-317) and identity-numbered
    {
      R *rz[] = {P.zt, P.up, P.vp, P.wp, P.us, P.vs, P.ws};
      for (R *q : rz) HIPCHK(hipMemsetAsync(q, 0, cap * sizeof(R), stream));
      HIPCHK(hipMemsetAsync(P.xt, 0, cap * sizeof(double), stream));
      HIPCHK(hipMemsetAsync(P.yt, 0, cap * sizeof(double), stream));
      HIPCHK(hipMemsetAsync(P.xmass1, 0, cap * cfg.nspec * sizeof(R), stream));
      int *iz[] = {P.idt, P.itramem, P.npoint, P.nclass};
      for (int *q : iz) HIPCHK(hipMemsetAsync(q, 0, cap * sizeof(int), stream));
      HIPCHK(hipMemsetAsync(P.cbt, 0, cap * sizeof(short), stream));
    }

    const int nb = (int)((cap + kBlock - 1) / kBlock);
    k_fill<int><<<nb, kBlock, 0, stream>>>(P.itra1, kDead, 0, (long long)cap, nullptr);
    // "never split" carries the sign of the run's direction: the test is ldirect*itime >= ldirect*itrasplit (timemanager.f90:478)
    k_fill<int><<<nb, kBlock, 0, stream>>>(P.itrasplit, (cfg.ldirect < 0 ? -1 : 1) * 999999999, 0, (long long)cap, nullptr);
    k_iota_pid<<<nb, kBlock, 0, stream>>>(P.pid, 0, (long long)cap);
    k_iota_pid<<<nb, kBlock, 0, stream>>>(d_iota, 0, (long long)cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }

  ~Engine() override {
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto &e : pinned_host) (void)hipHostUnregister(const_cast<void *>(e.first));
    for (void *q : owned) (void)hipFree(q);         // (the scratch buffers and the timers' events free themselves: fpx_host_res.hpp)
    if (comm) (void)ncclCommDestroy(comm);
    if (stream) (void)hipStreamDestroy(stream);
  }

  int set_height(const void *h, int n) override {
    if (!h || n != cfg.nz) return fail(FPX_ERR_ARG, "set_height: need nz values");
    std::vector<R> tmp(n);
    for (int k = 0; k < n; k++) tmp[k] = cfg.host_real_bytes == 4 ? (R)((const float *)h)[k] : (R)((const double *)h)[k];
    for (int k = 1; k < n; k++)
      if (!(tmp[k] > tmp[k - 1])) return fail(FPX_ERR_ARG, "set_height: heights must increase strictly");
    HIPCHK(hipMemcpyAsync((void *)V.height, tmp.data(), n * sizeof(R), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    height_host.resize(n);
    for (int k = 0; k < n; k++) height_host[k] = cfg.host_real_bytes == 4 ? (double)((const float *)h)[k] : ((const double *)h)[k];
    height_set = true;
    return 0;
  }

  // ---- host arrays -> device packs ----------------------------------------------------------
  // Extents of the host arrays of grid g (0: the mother grid, l >= 1: nested grid l): nx, ny used of nxmax, nymax allocated.
  struct HostGrid { int nx, ny, nxmax, nymax; };
  HostGrid host_grid(int g) const {
    if (g == 0) return {cfg.nx, cfg.ny, cfg.nxmax, cfg.nymax};
    return {h_nest[g - 1].nx, h_nest[g - 1].ny, nest_nxmaxn, nest_nymaxn};
  }
  // n elements of T from the host through the staging buffer (or, `on_device`, where they are) into launch(), then wait:
  // staging is reused by the next array
  template <typename T, typename Launch>
  int staged_launch(const void *src, size_t n, bool on_device, Launch launch) {
    if (!on_device) {
      HIPCHK(staging.reserve(n * sizeof(T), stream));
      HIPCHK(hipMemcpyAsync(staging.as(), src, n * sizeof(T), hipMemcpyHostToDevice, stream));
      src = staging.as();
    }
    launch((const T *)src);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  // [nz][nymax][nxmax] -> component `off` of a [ny][nx][nz][stride] pack (x<->z transpose)
  template <typename H, typename O>
  int pack3(HostGrid g, const void *src, O *out, int stride, int off, bool on_device = false) {
    return staged_launch<H>(src, (size_t)g.nxmax * g.nymax * cfg.nz, on_device, [&](const H *in) {   // levels beyond nz are never read
      dim3 grid((g.nx + 31) / 32, (cfg.nz + 31) / 32, g.ny), block(32, 8);
      k_pack3<H, O><<<grid, block, 0, stream>>>(in, out, g.nx, g.ny, cfg.nz, g.nxmax, g.nymax, stride, off);
    });
  }
  // [nymax][nxmax] -> component `off` of a [ny][nx][stride] pack
  template <typename H>
  int pack2(HostGrid g, const void *host, R *out, int stride, int off) {
    return staged_launch<H>(host, (size_t)g.nxmax * g.nymax, false, [&](const H *in) {
      const int tot = g.nx * g.ny;
      k_pack2<H, R><<<(tot + kBlock - 1) / kBlock, kBlock, 0, stream>>>(in, out, g.nx, g.ny, g.nxmax, stride, off);
    });
  }
  // nlev of [nlevmax][nymax][nxmax] -> compact [nlev][ny][nx], still in the host's real kind
  template <typename H>
  int compact_t(HostGrid g, const void *host, void *out, int nlev, int nlevmax) {
    return staged_launch<H>(host, (size_t)g.nxmax * g.nymax * nlevmax, false, [&](const H *in) {
      const long long n = (long long)g.nx * g.ny * nlev;
      k_conv_pack<H, H><<<(int)((n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(in, (H *)out, g.nx, g.ny, nlev, g.nxmax, g.nymax);
    });
  }
  int p3(HostGrid g, const void *host, const R *out, int stride, int off) {
    return cfg.host_real_bytes == 4 ? pack3<float>(g, host, (R *)out, stride, off) : pack3<double>(g, host, (R *)out, stride, off);
  }
  int p2(HostGrid g, const void *host, const R *out, int stride, int off) {
    return cfg.host_real_bytes == 4 ? pack2<float>(g, host, (R *)out, stride, off) : pack2<double>(g, host, (R *)out, stride, off);
  }
  int compact(HostGrid g, const void *host, void *out, int nlev, int nlevmax) {
    return cfg.host_real_bytes == 4 ? compact_t<float>(g, host, out, nlev, nlevmax) : compact_t<double>(g, host, out, nlev, nlevmax);
  }

  // ---- wind fields of one grid and time slot ---------------------------------------------------
  struct WindDst { const R *w3, *r2, *sfc, *tropo, *vdep, *hcell, *w3pol, *rhott; };   // w3pol, rhott: the mother grid's alone
  WindDst wind_dst(int g) const {
    if (g == 0) return {V.w3, V.r2, V.sfc, V.tropo, V.vdep, V.hcell, V.w3pol, V.rhott};
    const NestDesc<R> &N = h_nest[g - 1];
    return {N.w3, N.r2, N.sfc, N.tropo, N.vdep, N.hcell, nullptr, nullptr};
  }
  // the 2-D fields (what calcpar / calcpar_nests leave on the host when the 3-D ones come from the device transform)
  int upload_wind2(int g, int slot, const fpx_fields *f) {
    const HostGrid G = host_grid(g);
    const WindDst T = wind_dst(g);
    const int s = slot - 1;
    int rc;
    if ((rc = p2(G, f->ustar, T.sfc, 8, s * 4 + 0)) || (rc = p2(G, f->wstar, T.sfc, 8, s * 4 + 1)) ||
        (rc = p2(G, f->oli, T.sfc, 8, s * 4 + 2)) || (rc = p2(G, f->hmix, T.sfc, 8, s * 4 + 3))) return rc;
    if (slot == 1 && (rc = p2(G, f->tropopause, T.tropo, 1, 0))) return rc;   // literal time index 1: advance.f90:253 (tropopausen: advance.f90:263)
    if (T.vdep) {
      const size_t plane = (size_t)G.nxmax * G.nymax * cfg.host_real_bytes;
      for (int ks = 0; ks < cfg.nspec; ks++)
        if ((rc = p2(G, (const char *)f->vdep + plane * ks, T.vdep, 2 * cfg.nspec, s * cfg.nspec + ks))) return rc;
    }
    if (g == 0 && ((rc = diag_alloc()) || (rc = diag2_from_host(diag_tropo[s], f->tropopause, DG_TROPO + s)))) return rc;   // partoutput interpolates it in time
    return 0;
  }
  int upload_wind(int g, int slot, const fpx_fields *f) {
    const HostGrid G = host_grid(g);
    const WindDst T = wind_dst(g);
    const int s = slot - 1;
    int rc;
    if ((rc = p3(G, f->uu, T.w3, 6, s * 3 + 0)) || (rc = p3(G, f->vv, T.w3, 6, s * 3 + 1)) || (rc = p3(G, f->ww, T.w3, 6, s * 3 + 2))) return rc;
    if (g == 0 && T.w3pol)
      if ((rc = p3(G, f->uupol, T.w3pol, 6, s * 3 + 0)) || (rc = p3(G, f->vvpol, T.w3pol, 6, s * 3 + 1)) || (rc = p3(G, f->ww, T.w3pol, 6, s * 3 + 2))) return rc;
    if ((rc = p3(G, f->rho, T.r2, 4, s * 2 + 0)) || (rc = p3(G, f->drhodz, T.r2, 4, s * 2 + 1))) return rc;
    if (g == 0 && slot == 1 && T.rhott)   // literal time index 1: get_settling.f90:83-84
      if ((rc = p3(G, f->rho, T.rhott, 2, 0)) || (rc = p3(G, f->tt, T.rhott, 2, 1))) return rc;
    if ((rc = upload_wind2(g, slot, f))) return rc;
    k_hcell<R><<<(G.nx * G.ny + kBlock - 1) / kBlock, kBlock, 0, stream>>>(T.sfc, (R *)T.hcell, G.nx, G.ny);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    if (g == 0) slot_loaded[s] = true; else nest_loaded[g - 1][s] = true;
    return 0;
  }
  int upload_fields(int slot, const fpx_fields *f) override {
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "upload_fields: slot must be 1 or 2");
    if (!f || !f->uu || !f->vv || !f->ww || !f->rho || !f->drhodz || !f->hmix || !f->ustar || !f->wstar || !f->oli || !f->tropopause)
      return fail(FPX_ERR_ARG, "upload_fields: uu, vv, ww, rho, drhodz, hmix, ustar, wstar, oli, tropopause are required");
    if ((cfg.nglobal || cfg.sglobal) && (!f->uupol || !f->vvpol)) return fail(FPX_ERR_ARG, "upload_fields: uupol/vvpol required on a grid with poles");
    if (cfg.drydep && !f->vdep) return fail(FPX_ERR_ARG, "upload_fields: vdep required with DRYDEP");
    if (cfg.lsettling && !f->tt) return fail(FPX_ERR_ARG, "upload_fields: tt required with lsettling");
    return upload_wind(0, slot, f);
  }
  int upload_nest_fields(int nest, int slot, const fpx_fields *f) override {
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "upload_nest_fields: nest out of range (fpx_nests_init first)");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "upload_nest_fields: slot must be 1 or 2");
    if (!f || !f->uu || !f->vv || !f->ww || !f->rho || !f->drhodz || !f->hmix || !f->ustar || !f->wstar || !f->oli || !f->tropopause)
      return fail(FPX_ERR_ARG, "upload_nest_fields: uun, vvn, wwn, rhon, drhodzn, hmixn, ustarn, wstarn, olin, tropopausen are required");
    if (cfg.drydep && !f->vdep) return fail(FPX_ERR_ARG, "upload_nest_fields: vdepn required with DRYDEP");
    return upload_wind(nest, slot, f);
  }


  // ---- verttransform_ecmwf on the device --------------------------------
  // Model-level input -> z-level fields, computed in the host's real kind H in the host's own
  // array layout on the device, then repacked like an upload (the 3-D fields never cross PCIe
  // as z-level arrays unless the host asks for them back through `out`).
  std::vector<double> height_host;     // height(nz) in the host's real kind, widened
  // host arrays registered for DMA on request (fpx_model_levels.pin_host): address -> bytes; released in the destructor
  std::vector<std::pair<const void *, size_t>> pinned_host;
  void pin_host_range(const void *p, size_t bytes) {
    for (auto &e : pinned_host) if (e.first == p && e.second >= bytes) return;
    if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterDefault) == hipSuccess) pinned_host.emplace_back(p, bytes);
    else (void)hipGetLastError();      // not fatal: the copy falls back to the pageable path
  }
  void *vt_sets[1 + kMaxNests][32] = {};   // device arrays of the transform per grid (0 = mother, l = nest l), allocated on first use
  bool vt_set_ready[1 + kMaxNests] = {};

  template <typename H>
  static H vt_ew_host(H x) {           // ew.f90:4-29
    H y = (H)373.16 / x;
    H a = (H)-7.90298 * (y - (H)1.);
    a = a + ((H)5.02808 * (H)0.43429 * std::log(y));
    H c = ((H)1. - ((H)1. / y)) * (H)11.344;
    c = (H)-1. + std::pow((H)10., c);
    c = (H)-1.3816 * c / (H)1.e7;
    H d = ((H)1. - y) * (H)3.49149;
    d = (H)-1. + std::pow((H)10., d);
    d = (H)8.1328 * d / (H)1.e3;
    y = a + c + d;
    return (H)101324.6 * std::pow((H)10., y);
  }

  // first call: z levels from the first column with ps > 1000 hPa, verttransform_ecmwf.f90:134-187
  template <typename H>
  int vt_init_height(const fpx_model_levels *m, std::vector<H> &hgt, int &nmixz) {
    const H *ps = (const H *)m->ps, *tt2 = (const H *)m->tt2, *td2 = (const H *)m->td2;
    const H *tth = (const H *)m->tth, *qvh = (const H *)m->qvh, *akz = (const H *)m->akz, *bkz = (const H *)m->bkz;
    const size_t sx = (size_t)cfg.nxmax, sxy = (size_t)cfg.nxmax * cfg.nymax;
    long long col = -1;
    for (int jy = 0; jy < cfg.ny && col < 0; jy++)
      for (int ix = 0; ix < cfg.nx; ix++)
        if (ps[ix + sx * jy] > (H)100000.) { col = (long long)(ix + sx * jy); break; }
    if (col < 0) return fail(FPX_ERR_ARG, "verttransform: no column with ps > 100000 Pa to build the z levels from");
    const H konst = (H)287.05 / (H)9.81;
    H tvold = tt2[col] * ((H)1. + (H)0.378 * vt_ew_host<H>(td2[col]) / ps[col]);
    H pold = ps[col];
    hgt.assign(cfg.nz, (H)0);
    for (int kz = 2; kz <= m->nuvz; kz++) {
      const H pint = akz[kz - 1] + bkz[kz - 1] * ps[col];
      const H tv = tth[col + sxy * (kz - 1)] * ((H)1. + (H)0.608 * qvh[col + sxy * (kz - 1)]);
      if (std::abs(tv - tvold) > (H)0.2) hgt[kz - 1] = hgt[kz - 2] + konst * std::log(pold / pint) * (tv - tvold) / std::log(tv / tvold);
      else hgt[kz - 1] = hgt[kz - 2] + konst * std::log(pold / pint) * tv;
      tvold = tv;
      pold = pint;
    }
    nmixz = cfg.nz;
    for (int kz = 1; kz <= cfg.nz; kz++)
      if (hgt[kz - 1] > (H)4500.) { nmixz = kz; break; }   // hmixmax, par_mod.f90:77
    return 0;
  }

  template <typename H>
  int verttransform_t(int nest, int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out) {
    // nest = 0: the mother grid (verttransform_ecmwf.f90); nest = l >= 1: nested grid l (verttransform_nests.f90: the same
    // algorithm on the nest's arrays -- no height initialisation, no polar caps, the nest's own dyn/ylat0n in cosf and
    // the mother's dxconst, dyconst times xresoln, yresoln in the slope term, :346,384-385)
    const int nz = cfg.nz;
    const HostGrid HG = host_grid(nest);
    const int gnx = HG.nx, gny = HG.ny, gnxmax = HG.nxmax, gnymax = HG.nymax;
    void **vt_dev = vt_sets[nest];
    bool &vt_ready = vt_set_ready[nest];
    const size_t n2 = (size_t)gnxmax * gnymax, n3 = n2 * nz;
    int rc;
    enum { UUH, VVH, PVH, WWH, TTH, QVH, PS, TT2, TD2, AKZ, BKZ, AKN, BKN, HGT,
           UU, VV, WW, TT, QV, PV, RHO, DRHO, UPOL, VPOL, UVZ, WZ, RHOH, PINM, KUV, KW, NBUF };
    if (!vt_ready) {
      for (int i = 0; i < NBUF; i++) {
        const size_t n = (i >= PS && i <= TD2) ? n2 : (i >= AKZ && i <= HGT) ? (size_t)nz : n3;
        H *q = nullptr;
        if ((rc = dalloc(&q, n))) return rc;
        HIPCHK(hipMemsetAsync(q, 0, n * sizeof(H), stream));
        vt_dev[i] = q;
      }
      vt_ready = true;
    }
    auto D = [&](int i) { return (H *)vt_dev[i]; };
    // z levels: derived on the first call (or on request), else the ones the host has set
    if (!nest && (m->init || !height_set)) {
      std::vector<H> hgt;
      int nmixz = 0;
      if ((rc = vt_init_height<H>(m, hgt, nmixz))) return rc;
      if ((rc = set_height(hgt.data(), nz))) return rc;
      V.nmixz = nmixz;
      cfg.nmixz = nmixz;
    }
    {
      std::vector<H> hh(nz);
      for (int k = 0; k < nz; k++) hh[k] = (H)height_host[k];
      HIPCHK(hipMemcpyAsync(D(HGT), hh.data(), nz * sizeof(H), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    const void *src[13] = {m->uuh, m->vvh, m->pvh, m->wwh, m->tth, m->qvh, m->ps, m->tt2, m->td2, m->akz, m->bkz, m->aknew, m->bknew};
    for (int i = 0; i < 13; i++) {
      if (i == PVH && !m->pvh) continue;                                  // computed below, on the device
      const size_t n = (i >= PS && i <= TD2) ? n2 : (i >= AKZ) ? (size_t)nz : n3;
      if (m->pin_host && n >= n2) pin_host_range(src[i], n * sizeof(H));
      HIPCHK(hipMemcpyAsync(D(i), src[i], n * sizeof(H), hipMemcpyHostToDevice, stream));
    }
    vt::Geo<H> G;
    G.nx = gnx; G.ny = gny; G.nz = nz; G.nuvz = m->nuvz; G.nwz = m->nwz; G.nxmax = gnxmax; G.nymax = gnymax;
    G.dx = (H)cfg.dx; G.dy = (H)cfg.dy; G.xlon0 = (H)cfg.xlon0; G.ylat0 = (H)cfg.ylat0;
    {   // gridcheck_ecmwf.f90:311-312, in the host's real kind
      const H pi = (H)3.14159265, r_earth = (H)6.371e6;
      G.dxconst = (H)180. / (G.dx * r_earth * pi);
      G.dyconst = (H)180. / (G.dy * r_earth * pi);
    }
    G.xres = (H)1.; G.yres = (H)1.;
    if (nest) {   // after dxconst, dyconst (the mother's): the nest's own spacing and origin for cosf
      G.dy = (H)m->nest_dy; G.ylat0 = (H)m->nest_ylat0;
      G.xres = (H)h_nest[nest - 1].xres; G.yres = (H)h_nest[nest - 1].yres;
    }
    G.nglobal = nest ? 0 : cfg.nglobal; G.sglobal = nest ? 0 : cfg.sglobal;
    G.switchnorthg = (H)cfg.switchnorthg; G.switchsouthg = (H)cfg.switchsouthg;
    for (int i = 0; i < 9; i++) { G.northpolemap[i] = (H)cfg.northpolemap[i]; G.southpolemap[i] = (H)cfg.southpolemap[i]; }
    vt::In<H> I{D(UUH), D(VVH), D(PVH), D(WWH), D(TTH), D(QVH), D(PS), D(TT2), D(TD2), D(AKZ), D(BKZ), D(AKN), D(BKN), D(HGT)};
    vt::Out<H> O{D(UU), D(VV), D(WW), D(TT), D(QV), D(PV), D(RHO), D(DRHO), D(UPOL), D(VPOL), D(UVZ), D(WZ), D(RHOH), D(PINM)};
    // pvh = NULL: calcpv.f90 / calcpv_nests.f90 on the arrays just uploaded, into D(PVH), under an event pair of its own.
    // ppml and theta go to UVZ and WZ, which the transform below overwrites anyway.
    Events<2> pev, ev;
    if (!m->pvh) {
      pv::Args<H> P;
      P.nx = gnx; P.ny = gny; P.nuvz = m->nuvz; P.nxmax = gnxmax; P.nymax = gnymax;
      P.xglobal = nest ? 0 : cfg.xglobal; P.nglobal = nest ? 0 : cfg.nglobal; P.sglobal = nest ? 0 : cfg.sglobal;
      P.dx = nest ? (H)pv_dxn[nest - 1] : (H)cfg.dx; P.dy = G.dy; P.ylat0 = G.ylat0;
      P.uuh = D(UUH); P.vvh = D(VVH); P.tth = D(TTH); P.ps = D(PS); P.akz = D(AKZ); P.bkz = D(BKZ);
      P.ppml = D(UVZ); P.theta = D(WZ); P.pvh = D(PVH);
      HIPCHK(pev.create());
      HIPCHK(hipEventRecord(pev[0], stream));
      const dim3 gp((gnx * gny + 255) / 256, m->nuvz);
      pv::k_theta<H><<<gp, 256, 0, stream>>>(P);
      pv::k_pv<H><<<gp, 256, 0, stream>>>(P);
      if (P.nglobal || P.sglobal) pv::k_pole<H><<<dim3((m->nuvz + 63) / 64, 2), 64, 0, stream>>>(P);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(pev[1], stream));
    }
    HIPCHK(ev.create());
    HIPCHK(hipEventRecord(ev[0], stream));
    const int ncol = gnx * gny, nb = (ncol + 255) / 256;
    const size_t sm = (size_t)nz * sizeof(H);
    const dim3 g3(nb, nz);
    unsigned short *kuv = (unsigned short *)vt_dev[KUV], *kw = (unsigned short *)vt_dev[KW];
    // fused path: the ECMWF level structure (nuvz = nwz = nz) and a tile's uvzlev fits the LDS of a CU twice
    constexpr int kVtWaves = FPX_VT_WAVES;
    const size_t sm_lev = (size_t)nz * vt::kVtCols * sizeof(H), sm_fused = sm_lev + (size_t)5 * nz * sizeof(H);
    const bool fused = m->nuvz == nz && m->nwz == nz && nz >= 3 && sm_fused <= (size_t)80 * 1024 && n3 < ((size_t)1 << 31) && !opt.vt_unfused;
    if (fused) {
      vt::Tiles T;
      T.tiles_y = (gny + vt::kVtTy - 1) / vt::kVtTy;
      T.ntiles = T.tiles_y * ((gnx + vt::kVtTx - 1) / vt::kVtTx);
      T.tiles_per_xcd = (T.ntiles + 7) / 8;
      static bool attr_set = false;
      if (!attr_set) {
        HIPCHK(hipFuncSetAttribute((const void *)vt::k_vt_levels<H>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        HIPCHK(hipFuncSetAttribute((const void *)vt::k_vt_fused<H, kVtWaves>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        attr_set = true;
      }
      vt::k_vt_levels<H><<<8 * T.tiles_per_xcd, 512, sm_lev, stream>>>(G, I, O, T);
      vt::k_vt_fused<H, kVtWaves><<<8 * T.tiles_per_xcd, kVtWaves * 64, sm_fused, stream>>>(G, I, O, T);
    } else {
      vt::k_vt_inc<H><<<g3, 256, 0, stream>>>(G, I, O);
      vt::k_vt_column<H><<<nb, 256, 0, stream>>>(G, I, O);
      vt::k_vt_search<H><<<dim3(nb, 2), 256, sm, stream>>>(G, I, O, kuv, kw);
      vt::k_vt_fill<H><<<g3, 256, 0, stream>>>(G, I, O, kuv, kw);
      vt::k_vt_post<H><<<g3, 256, 0, stream>>>(G, I, O, kuv);
    }
    const size_t smrow = (size_t)(gnx + 3) * sizeof(H);
    if (G.nglobal) {
      const int jy0 = std::max(0, (int)G.switchnorthg - 2), jy1 = cfg.ny - 1;
      if (jy1 >= jy0) vt::k_vt_polar<H><<<dim3((cfg.nx + 255) / 256, jy1 - jy0 + 1, nz), 256, 0, stream>>>(G, O, jy0, jy1, 0);
      vt::k_vt_polerow<H><<<nz, 64, smrow, stream>>>(G, O, 0);
    }
    if (G.sglobal) {
      const int jy0 = 0, jy1 = std::min(cfg.ny - 1, (int)G.switchsouthg + 3);
      if (jy1 >= jy0) vt::k_vt_polar<H><<<dim3((cfg.nx + 255) / 256, jy1 - jy0 + 1, nz), 256, 0, stream>>>(G, O, jy0, jy1, 1);
      vt::k_vt_polerow<H><<<nz, 64, smrow, stream>>>(G, O, 1);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], stream));
    // repack into the gather layout, as upload_fields / upload_nest_fields do from the staged host arrays
    const int s = slot - 1;
    auto pk = [&](const H *in, const R *outp, int stride, int off) -> int {
      dim3 grid((gnx + 31) / 32, (nz + 31) / 32, gny), block(32, 8);
      k_pack3<H, R><<<grid, block, 0, stream>>>(in, (R *)outp, gnx, gny, nz, gnxmax, gnymax, stride, off);
      HIPCHK(hipGetLastError());
      return 0;
    };
    const WindDst T = wind_dst(nest);
    if ((rc = pk(D(UU), T.w3, 6, s * 3 + 0)) || (rc = pk(D(VV), T.w3, 6, s * 3 + 1)) || (rc = pk(D(WW), T.w3, 6, s * 3 + 2))) return rc;
    if (!nest && T.w3pol)
      if ((rc = pk(D(UPOL), T.w3pol, 6, s * 3 + 0)) || (rc = pk(D(VPOL), T.w3pol, 6, s * 3 + 1)) || (rc = pk(D(WW), T.w3pol, 6, s * 3 + 2))) return rc;
    if ((rc = pk(D(RHO), T.r2, 4, s * 2 + 0)) || (rc = pk(D(DRHO), T.r2, 4, s * 2 + 1))) return rc;
    if (!nest && slot == 1 && T.rhott)
      if ((rc = pk(D(RHO), T.rhott, 2, 0)) || (rc = pk(D(TT), T.rhott, 2, 1))) return rc;
    if (!nest && wet_on && Wp.ttw) { if ((rc = pk(D(TT), Wp.ttw, 2, s))) return rc; }
    if (sfc && (rc = upload_wind2(nest, slot, sfc))) return rc;
    if (!nest) {   // pv, qv, tt of this slot stay on the device for partoutput
      if ((rc = diag_alloc())) return rc;
      if ((rc = diag3(D(PV), true, 0, s)) || (rc = diag3(D(QV), true, 1, s)) || (rc = diag3(D(TT), true, 2, s))) return rc;
    }
    if (sfc) k_hcell<R><<<(gnx * gny + kBlock - 1) / kBlock, kBlock, 0, stream>>>(T.sfc, (R *)T.hcell, gnx, gny);
    HIPCHK(hipGetLastError());
    if (out) {   // z-level arrays the host still wants (partoutput, convection, cloud diagnostics ...)
      void *dst[10] = {out->uu, out->vv, out->ww, out->tt, out->qv, out->pv, out->rho, out->drhodz, out->uupol, out->vvpol};
      for (int i = 0; i < 10; i++)
        if (dst[i]) HIPCHK(hipMemcpyAsync(dst[i], D(UU + i), n3 * sizeof(H), hipMemcpyDeviceToHost, stream));
      if (out->height) for (int k = 0; k < nz; k++) ((H *)out->height)[k] = (H)height_host[k];
      if (out->nmixz) *out->nmixz = V.nmixz;
    }
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    vt_last_ms = ms;
    pv_last_ms = 0;
    if (!m->pvh) {
      HIPCHK(hipEventElapsedTime(&ms, pev[0], pev[1]));
      pv_last_ms = ms;
    }
    pvh_on_device[nest] = true;
    // without sfc the slot's 2-D fields are still those of the previous wind field until fpx_calcpar has run: not loaded
    if (nest) { nest_loaded[nest - 1][s] = sfc != nullptr; nest_vdep_pending[nest - 1][s] = false; }   // sfc = NULL: until fpx_calcpar_nest
    else { slot_loaded[s] = sfc != nullptr; vdep_pending[s] = false; }
    vt_slot_on_device[nest] = slot;           // whose model-level arrays the grid's buffers hold (fpx_calcpar, fpx_calcpar_nest)
    if (nest) { nest_dyn[nest - 1] = m->nest_dy; nest_ylat0n[nest - 1] = m->nest_ylat0; }   // calcpar_nests.f90:73
    return 0;
  }
  int vt_slot_on_device[1 + kMaxNests] = {};
  double nest_dyn[kMaxNests] = {}, nest_ylat0n[kMaxNests] = {};

  // ---- calcpv / calcpv_nests on the device (fpx_calcpv.hpp; launched by verttransform_t when pvh = NULL) ----------
  double pv_dxn[kMaxNests] = {};       // com_mod's dxn(l): calcpv_nests.f90:168,171 divides by it (dx/xresoln need not round to it)
  bool pv_ready = false;
  bool pvh_on_device[1 + kMaxNests] = {};
  double pv_last_ms = 0;
  int calcpv_init(const fpx_calcpv_cfg *c) override {
    if (!c || c->struct_bytes != (int32_t)sizeof(fpx_calcpv_cfg)) return fail(FPX_ERR_ARG, "calcpv_init: null or fpx_calcpv_cfg size mismatch (ABI)");
    for (int l = 0; l < kMaxNests; l++) pv_dxn[l] = c->dxn[l];
    pv_ready = true;
    return 0;
  }
  int get_pvh(int nest, void *pvh_out) override {
    if (nest < 0 || nest > V.numbnests) return fail(FPX_ERR_ARG, "get_pvh: nest out of range (0 = the mother grid)");
    if (!pvh_out) return fail(FPX_ERR_ARG, "get_pvh: null");
    if (!vt_set_ready[nest] || !pvh_on_device[nest]) return fail(FPX_ERR_STATE, "get_pvh: no transform of this grid has run yet");
    const HostGrid HG = host_grid(nest);
    const size_t bytes = (size_t)HG.nxmax * HG.nymax * cfg.nz * cfg.host_real_bytes;
    HIPCHK(hipMemcpyAsync(pvh_out, vt_sets[nest][2], bytes, hipMemcpyDeviceToHost, stream));   // [2]: PVH of verttransform_t
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  double pv_ms() override { return pv_last_ms; }

  // ---- calcpar on the device ----------------------------------------------------------
  // g = 0: the mother grid (calcpar.f90); g = l >= 1: nested grid l (one iteration l of calcpar_nests.f90:63-225): the same
  // kernel on the nest's arrays, extents and latitudes, with buffers and gather packs of the nest's own
  // The buffers of a grid's calcpar (cp_begin) and what follows the kernel (cp_finish) are shared by calcpar_t and
  // calcpar_gfs_t: gather packs, hcell, the copies into `out`, the timing and the slot's state.
  template <typename H>
  struct CpDev { H *str, *shf, *exc, *ust, *wst, *oli, *hmix, *akm, *bkm, *trop; };
  template <typename H>
  int cp_begin(int g, int s, CpDev<H> &d) {
    const HostGrid HG = host_grid(g);
    const int nz = cfg.nz;
    const size_t n2 = (size_t)HG.nxmax * HG.nymax;
    int rc;
    if (!cp_buf[g]) {
      H *q = nullptr;
      if ((rc = dalloc(&q, 8 * n2 + 2 * (size_t)nz))) return rc;       // surfstr, sshf, excessoro, ustar, wstar, oli, hmix, tropopause | akm, bkm
      HIPCHK(hipMemsetAsync(q, 0, (8 * n2 + 2 * (size_t)nz) * sizeof(H), stream));
      cp_buf[g] = q;
    }
    H *B = (H *)cp_buf[g];
    d.str = B; d.shf = B + n2; d.exc = B + 2 * n2; d.ust = B + 3 * n2; d.wst = B + 4 * n2; d.oli = B + 5 * n2; d.hmix = B + 6 * n2;
    d.akm = B + 8 * n2; d.bkm = d.akm + nz;
    // the slot's tropopause in the host's layout (the mother grid's is kept for partoutput): it starts at zero and stale values
    // persist as in the reference -- the kernel writes a column only where the criterion fires (calcpar_nests.f90:201-214)
    if (g == 0) {
      if ((rc = diag_alloc())) return rc;
      d.trop = (H *)diag_tropo[s];
    } else {
      if (!nest_tropo[g - 1][s]) {
        H *q = nullptr;
        if ((rc = dalloc(&q, n2))) return rc;
        HIPCHK(hipMemsetAsync(q, 0, n2 * sizeof(H), stream));
        nest_tropo[g - 1][s] = q;
      }
      d.trop = (H *)nest_tropo[g - 1][s];
    }
    return 0;
  }
  template <typename H>
  int cp_finish(int g, int slot, const CpDev<H> &d, const void *vdep, const fpx_calcpar_out *out, Events<2> &ev) {
    const HostGrid HG = host_grid(g);
    const WindDst T = wind_dst(g);
    const int s = slot - 1;
    const size_t n2 = (size_t)HG.nxmax * HG.nymax;
    int rc;
    // into the gather packs, as upload_fields / upload_nest_fields do from the host's arrays
    auto pk2 = [&](const H *in, const R *outp, int stride, int off) -> int {
      const int tot = HG.nx * HG.ny;
      k_pack2<H, R><<<(tot + kBlock - 1) / kBlock, kBlock, 0, stream>>>(in, (R *)outp, HG.nx, HG.ny, HG.nxmax, stride, off);
      HIPCHK(hipGetLastError());
      return 0;
    };
    if ((rc = pk2(d.ust, T.sfc, 8, s * 4 + 0)) || (rc = pk2(d.wst, T.sfc, 8, s * 4 + 1)) || (rc = pk2(d.oli, T.sfc, 8, s * 4 + 2)) || (rc = pk2(d.hmix, T.sfc, 8, s * 4 + 3))) return rc;
    if (slot == 1 && (rc = pk2(d.trop, T.tropo, 1, 0))) return rc;        // literal time index 1, advance.f90:253 (tropopausen: :263)
    if (g == 0) diag_have[DG_TROPO + s] = true;
    if (T.vdep && vdep) {
      const size_t plane = n2 * cfg.host_real_bytes;
      for (int ks = 0; ks < cfg.nspec; ks++)
        if ((rc = p2(HG, (const char *)vdep + plane * ks, T.vdep, 2 * cfg.nspec, s * cfg.nspec + ks))) return rc;
    }
    k_hcell<R><<<(HG.nx * HG.ny + kBlock - 1) / kBlock, kBlock, 0, stream>>>(T.sfc, (R *)T.hcell, HG.nx, HG.ny);
    HIPCHK(hipGetLastError());
    if (out) {
      void *dst[5] = {out->ustar, out->wstar, out->oli, out->hmix, out->tropopause};
      const H *src[5] = {d.ust, d.wst, d.oli, d.hmix, d.trop};
      for (int i = 0; i < 5; i++)
        if (dst[i]) HIPCHK(hipMemcpyAsync(dst[i], src[i], n2 * sizeof(H), hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    cp_last_ms = ms;
    cp_slot_on_device[g] = slot;               // whose ustar, oli the grid's buffer holds (fpx_getvdep, fpx_getvdep_nest)
    // device_vdep with DRYDEP: the slot's vdep is still the previous wind field's until fpx_getvdep has run: not loaded
    const bool pending = T.vdep && !vdep;
    if (g == 0) { vdep_pending[s] = pending; slot_loaded[s] = !pending; }
    else { nest_vdep_pending[g - 1][s] = pending; nest_loaded[g - 1][s] = !pending; }
    return 0;
  }
  template <typename H>
  int calcpar_t(int g, int slot, const fpx_calcpar_in *c, const fpx_calcpar_out *out) {
    enum { UUH, VVH, PVH, WWH, TTH, QVH, PS, TT2, TD2, AKZ, BKZ, AKN, BKN, HGT,
           UU, VV, WW, TT, QV, PV, RHO, DRHO, UPOL, VPOL, UVZ, WZ, RHOH, PINM, KUV, KW, NBUF };
    void **vt_dev = vt_sets[g];
    auto D = [&](int i) { return (H *)vt_dev[i]; };
    const HostGrid HG = host_grid(g);
    const int nz = cfg.nz, s = slot - 1;
    const size_t n2 = (size_t)HG.nxmax * HG.nymax;
    int rc;
    CpDev<H> d;
    if ((rc = cp_begin<H>(g, s, d))) return rc;
    HIPCHK(hipMemcpyAsync(d.str, c->surfstr, n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d.shf, c->sshf, n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    if (c->lsubgrid == 1) HIPCHK(hipMemcpyAsync(d.exc, c->excessoro, n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d.akm, c->akm, (size_t)nz * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d.bkm, c->bkm, (size_t)nz * sizeof(H), hipMemcpyHostToDevice, stream));
    cp::Args<H> A;
    A.G.nx = HG.nx; A.G.ny = HG.ny; A.G.nz = nz; A.G.nuvz = nz; A.G.nwz = nz; A.G.nxmax = HG.nxmax; A.G.nymax = HG.nymax;
    A.G.dx = (H)cfg.dx; A.G.dy = (H)cfg.dy; A.G.xlon0 = (H)cfg.xlon0; A.G.ylat0 = (H)cfg.ylat0;
    if (g) { A.G.dy = (H)nest_dyn[g - 1]; A.G.ylat0 = (H)nest_ylat0n[g - 1]; }   // altmin: ylat0n(l) + jy*dyn(l), calcpar_nests.f90:73
    A.I = vt::In<H>{D(UUH), D(VVH), D(PVH), D(WWH), D(TTH), D(QVH), D(PS), D(TT2), D(TD2), D(AKZ), D(BKZ), D(AKN), D(BKN), D(HGT)};
    A.surfstr = d.str; A.sshf = d.shf; A.excessoro = d.exc; A.akm = d.akm; A.bkm = d.bkm; A.lsubgrid = c->lsubgrid;
    A.zlev = D(RHOH);                          // scratch of the grid's transform, free between calls
    A.ustar = d.ust; A.wstar = d.wst; A.oli = d.oli; A.hmix = d.hmix; A.tropopause = d.trop;
    Events<2> ev;
    HIPCHK(ev.create());
    HIPCHK(hipEventRecord(ev[0], stream));
    cp::k_calcpar<H><<<(HG.nx * HG.ny + 255) / 256, 256, 0, stream>>>(A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], stream));
    return cp_finish<H>(g, slot, d, c->vdep, out, ev);
  }
  // fpx_calcpar_gfs: the NCEP branch (fpx_calcpar_gfs.hpp) on the arrays fpx_verttransform_gfs left; the host's raw hmix goes
  // into the hmix plane, which the kernel reads and overwrites column by column
  template <typename H>
  int calcpar_gfs_t(int slot, const fpx_calcpar_gfs_in *c, const fpx_calcpar_out *out) {
    enum { UUH, VVH, PVH, WWH, TTH, QVH, PS, TT2, TD2, AKZ, BKZ, AKN, BKN, HGT,
           UU, VV, WW, TT, QV, PV, RHO, DRHO, UPOL, VPOL, UVZ, WZ, RHOH, PINM, KUV, KW, NBUF };
    void **vt_dev = vt_sets[0];
    auto D = [&](int i) { return (H *)vt_dev[i]; };
    const HostGrid HG = host_grid(0);
    const int nz = cfg.nz, s = slot - 1;
    const size_t n2 = (size_t)HG.nxmax * HG.nymax;
    int rc;
    CpDev<H> d;
    if ((rc = cp_begin<H>(0, s, d))) return rc;
    HIPCHK(hipMemcpyAsync(d.str, c->surfstr, n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d.shf, c->sshf, n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d.hmix, c->hmix, n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    if (c->lsubgrid == 1) HIPCHK(hipMemcpyAsync(d.exc, c->excessoro, n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    cpg::Args<H> A;
    A.G = vt::Geo<H>{};
    A.G.nx = HG.nx; A.G.ny = HG.ny; A.G.nz = nz; A.G.nuvz = nz; A.G.nwz = nz; A.G.nxmax = HG.nxmax; A.G.nymax = HG.nymax;
    A.G.dx = (H)cfg.dx; A.G.dy = (H)cfg.dy; A.G.xlon0 = (H)cfg.xlon0; A.G.ylat0 = (H)cfg.ylat0;
    A.I = vt::In<H>{D(UUH), D(VVH), D(PVH), D(WWH), D(TTH), D(QVH), D(PS), D(TT2), D(TD2), D(AKZ), D(BKZ), D(AKN), D(BKN), D(HGT)};
    A.surfstr = d.str; A.sshf = d.shf; A.excessoro = d.exc; A.lsubgrid = c->lsubgrid;
    A.zlev = D(RHOH);                          // scratch of the transform, free between calls
    A.ustar = d.ust; A.wstar = d.wst; A.oli = d.oli; A.hmix = d.hmix; A.tropopause = d.trop;
    Events<2> ev;
    HIPCHK(ev.create());
    HIPCHK(hipEventRecord(ev[0], stream));
    cpg::k_calcpar_gfs<H><<<(HG.nx * HG.ny + 255) / 256, 256, 0, stream>>>(A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], stream));
    return cp_finish<H>(0, slot, d, c->vdep, out, ev);
  }
  void *cp_buf[1 + kMaxNests] = {};          // one per grid, sized by it: calls for the mother grid and the nests may interleave
  void *nest_tropo[kMaxNests][2] = {};       // tropopausen(:,:,1,n,l) in the host's layout and real kind, allocated on first use
  double cp_last_ms = 0;
  int cp_slot_on_device[1 + kMaxNests] = {};
  bool vdep_pending[2] = {false, false};
  bool nest_vdep_pending[kMaxNests][2] = {};
  int calcpar(int slot, const fpx_calcpar_in *c, const fpx_calcpar_out *out) override {
    if (met_format == MET_GFS) return fail(FPX_ERR_UNSUPPORTED, "calcpar: NCEP GFS fields: the NCEP branch of calcpar.f90:109-121,145-149 (first level above ground, mixing height from the GRIB file) is not computed by this call: fpx_calcpar_gfs computes it");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "calcpar: slot must be 1 or 2");
    if (!c || !c->surfstr || !c->sshf || !c->akm || !c->bkm) return fail(FPX_ERR_ARG, "calcpar: surfstr, sshf, akm, bkm are required");
    if (c->lsubgrid == 1 && !c->excessoro) return fail(FPX_ERR_ARG, "calcpar: excessoro required with lsubgrid = 1");
    if (cfg.drydep && !c->vdep && !c->device_vdep) return fail(FPX_ERR_ARG, "calcpar: vdep (the host's getvdep) required with DRYDEP");
    if (!vt_set_ready[0] || vt_slot_on_device[0] != slot) return fail(FPX_ERR_STATE, "calcpar: fpx_verttransform_ecmwf of this slot first (its model-level arrays are read on the device)");
    return cfg.host_real_bytes == 4 ? calcpar_t<float>(0, slot, c, out) : calcpar_t<double>(0, slot, c, out);
  }
  int calcpar_nest(int nest, int slot, const fpx_calcpar_in *c, const fpx_calcpar_out *out) override {
    if (met_format == MET_GFS) return fail(FPX_ERR_UNSUPPORTED, "calcpar_nest: NCEP GFS fields: the NCEP branch of calcpar.f90:109-121,145-149 is computed by fpx_calcpar_gfs for the mother grid, and the reference has no GFS nests");
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "calcpar_nest: nest out of range (fpx_nests_init first)");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "calcpar_nest: slot must be 1 or 2");
    if (!c || !c->surfstr || !c->sshf || !c->akm || !c->bkm) return fail(FPX_ERR_ARG, "calcpar_nest: surfstrn, sshfn, akm, bkm are required");
    if (c->lsubgrid == 1 && !c->excessoro) return fail(FPX_ERR_ARG, "calcpar_nest: excessoron required with lsubgrid = 1");
    if (cfg.drydep && !c->vdep && !c->device_vdep) return fail(FPX_ERR_ARG, "calcpar_nest: vdepn (the host's getvdep_nests) required with DRYDEP");
    if (!vt_set_ready[nest] || vt_slot_on_device[nest] != slot)
      return fail(FPX_ERR_STATE, "calcpar_nest: fpx_verttransform_nest of this nest and slot first (its model-level arrays are read on the device)");
    return cfg.host_real_bytes == 4 ? calcpar_t<float>(nest, slot, c, out) : calcpar_t<double>(nest, slot, c, out);
  }
  int calcpar_gfs(int slot, const fpx_calcpar_gfs_in *c, const fpx_calcpar_out *out) override {
    if (met_format != MET_GFS) return fail(FPX_ERR_UNSUPPORTED, "calcpar_gfs: this handle does not take NCEP GFS fields (no fpx_verttransform_gfs has run on it): fpx_calcpar computes the ECMWF branch");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "calcpar_gfs: slot must be 1 or 2");
    if (!c || c->struct_bytes != (int32_t)sizeof(fpx_calcpar_gfs_in)) return fail(FPX_ERR_ARG, "calcpar_gfs: null or fpx_calcpar_gfs_in size mismatch (ABI)");
    if (!c->surfstr || !c->sshf || !c->hmix) return fail(FPX_ERR_ARG, "calcpar_gfs: surfstr, sshf, hmix (the GRIB file's mixing height) are required");
    if (c->lsubgrid == 1 && !c->excessoro) return fail(FPX_ERR_ARG, "calcpar_gfs: excessoro required with lsubgrid = 1");
    if (cfg.drydep && !c->vdep && !c->device_vdep) return fail(FPX_ERR_ARG, "calcpar_gfs: vdep (the host's getvdep) required with DRYDEP");
    if (!vt_set_ready[0] || vt_slot_on_device[0] != slot) return fail(FPX_ERR_STATE, "calcpar_gfs: fpx_verttransform_gfs of this slot first (its pressure-level arrays are read on the device)");
    return cfg.host_real_bytes == 4 ? calcpar_gfs_t<float>(slot, c, out) : calcpar_gfs_t<double>(slot, c, out);
  }
  // ---- getvdep on the device (calcpar.f90:171-189) ------------------------------------------------------------
  void *gv_tab = nullptr;                      // the resistance and species tables: shared by the mother grid and the nests
  void *gv_land[1 + kMaxNests] = {}, *gv_buf[1 + kMaxNests] = {};   // per grid (0 = mother, l = nest l): xlanduse / xlandusen(:,:,:,l); inputs and vdep planes
  unsigned char *gv_season[1 + kMaxNests] = {};
  int gv_land_classes[1 + kMaxNests] = {};    // numclass the grid's gv_land was sized for
  gv::Layout gv_lay{0, 0, 0};
  double gv_bdate = 0, gv_last_ms = 0;
  bool gv_ready = false, gv_nest_ready[kMaxNests] = {};

  template <typename H>
  int getvdep_init_t(const fpx_getvdep_tables *t) {
    const gv::Layout Ly{t->numclass, t->ni, t->maxspec};
    const size_t n2 = (size_t)cfg.nxmax * cfg.nymax;
    int rc;
    gv_ready = false;
    for (int l = 0; l < kMaxNests; l++) gv_nest_ready[l] = false;    // xlandusen follows the tables: fpx_getvdep_nest_init again
    if (!gv_tab || Ly.numclass != gv_lay.numclass || Ly.ni != gv_lay.ni || Ly.maxspec != gv_lay.maxspec) {
      H *q = nullptr;
      if ((rc = dalloc(&q, (size_t)Ly.total()))) return rc;
      gv_tab = q;
      if ((rc = dalloc(&q, n2 * Ly.numclass))) return rc;
      gv_land[0] = q;
    }
    std::vector<H> pk((size_t)Ly.total());
    auto put = [&](int off, const void *src, size_t n) { memcpy(pk.data() + off, src, n * sizeof(H)); };
    const int ms = Ly.maxspec, nc = Ly.numclass;
    put(Ly.z0(), t->z0, nc); put(Ly.ri(), t->ri, 5 * nc); put(Ly.rac(), t->rac, 5 * nc);
    put(Ly.rcl(), t->rcl, (size_t)ms * 5 * nc); put(Ly.rgs(), t->rgs, (size_t)ms * 5 * nc); put(Ly.rlu(), t->rlu, (size_t)ms * 5 * nc);
    const void *sp[6] = {t->rm, t->reldiff, t->henry, t->f0, t->density, t->dryvel};
    for (int i = 0; i < 6; i++) put(Ly.spec() + i * ms, sp[i], ms);
    put(Ly.vset(), t->vset, (size_t)ms * Ly.ni); put(Ly.vset() + ms * Ly.ni, t->schmi, (size_t)ms * Ly.ni); put(Ly.vset() + 2 * ms * Ly.ni, t->fract, (size_t)ms * Ly.ni);
    HIPCHK(hipMemcpyAsync(gv_tab, pk.data(), pk.size() * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(gv_land[0], t->xlanduse, n2 * nc * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    gv_lay = Ly;
    gv_bdate = t->bdate;
    gv_ready = true;
    return 0;
  }
  int getvdep_init(const fpx_getvdep_tables *t) override {
    static_assert(gv::kMaxSpec == FPX_MAXSPEC, "the lane-private species arrays of k_getvdep");
    if (!t || !t->xlanduse || !t->z0 || !t->ri || !t->rac || !t->rcl || !t->rgs || !t->rlu || !t->rm || !t->reldiff || !t->henry ||
        !t->f0 || !t->density || !t->dryvel || !t->vset || !t->schmi || !t->fract)
      return fail(FPX_ERR_ARG, "getvdep_init: xlanduse, z0, ri, rac, rcl, rgs, rlu, rm, reldiff, henry, f0, density, dryvel, vset, schmi, fract are required");
    if (!cfg.drydep) return fail(FPX_ERR_ARG, "getvdep_init: the run has no dry deposition (DRYDEP)");
    if (t->numclass < 1 || t->numclass > 255 || t->ni < 1 || t->ni > 4096 || t->maxspec < cfg.nspec || t->maxspec > 64)
      return fail(FPX_ERR_ARG, "getvdep_init: 1 <= numclass <= 255, 1 <= ni <= 4096, nspec <= maxspec <= 64 expected");
    const gv::Layout Ly{t->numclass, t->ni, t->maxspec};
    if ((size_t)Ly.total() * cfg.host_real_bytes > (size_t)60 * 1024) return fail(FPX_ERR_ARG, "getvdep_init: the resistance tables do not fit the LDS of a block (60 KiB)");
    return cfg.host_real_bytes == 4 ? getvdep_init_t<float>(t) : getvdep_init_t<double>(t);
  }
  // xlandusen(0:nxmaxn-1,0:nymaxn-1,numclass,l) of nested grid `nest`; the resistance and species tables are fpx_getvdep_init's
  int getvdep_nest_init(int nest, const void *xlandusen) override {
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "getvdep_nest_init: nest out of range (fpx_nests_init first)");
    if (!xlandusen) return fail(FPX_ERR_ARG, "getvdep_nest_init: xlandusen is required");
    if (!cfg.drydep) return fail(FPX_ERR_ARG, "getvdep_nest_init: the run has no dry deposition (DRYDEP)");
    if (!gv_ready) return fail(FPX_ERR_STATE, "getvdep_nest_init: fpx_getvdep_init first (numclass and the resistance tables are shared)");
    const size_t bytes = (size_t)nest_nxmaxn * nest_nymaxn * gv_lay.numclass * cfg.host_real_bytes;
    int rc;
    if (!gv_land[nest] || gv_land_classes[nest] != gv_lay.numclass) {
      char *q = nullptr;
      if ((rc = dalloc(&q, bytes))) return rc;
      gv_land[nest] = q;
      gv_land_classes[nest] = gv_lay.numclass;
    }
    HIPCHK(hipMemcpyAsync(gv_land[nest], xlandusen, bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    gv_nest_ready[nest - 1] = true;
    return 0;
  }

  // caldate.f90:42-65 (the date part), its default-real literals in the host's real kind H
  template <typename H>
  static int gv_caldate(double juldate, int *hhmiss = nullptr) {
#pragma clang fp contract(off)
    int julday = (int)juldate;
    if ((juldate - julday) * 86400. >= 86399.5) {
      juldate = juldate + juldate - julday - 86399.5 / 86400.;
      julday = (int)juldate;
    }
    int ja;
    if (julday >= 2299161) {
      const int jalpha = (int)(((H)(julday - 1867216) - (H)0.25) / (H)36524.25);
      ja = julday + 1 + jalpha - (int)((H)0.25 * (H)jalpha);
    } else ja = julday;
    const int jb = ja + 1524;
    const int jc = (int)((H)6680. + ((H)(jb - 2439870) - (H)122.1) / (H)365.25);
    const int jd = 365 * jc + (int)((H)0.25 * (H)jc);
    const int je = (int)((H)(jb - jd) / (H)30.6001);
    const int dd = jb - jd - (int)((H)30.6001 * (H)je);
    int mm = je - 1;
    if (mm > 12) mm = mm - 12;
    int yyyy = jc - 4715;
    if (mm > 2) yyyy = yyyy - 1;
    if (yyyy <= 0) yyyy = yyyy - 1;
    if (hhmiss) {   // caldate.f90:66-78
      int hh = (int)(24. * (juldate - (double)julday));
      int mi = (int)(1440. * (juldate - (double)julday) - 60. * (double)hh);
      int ss = (int)std::lround(86400. * (juldate - (double)julday) - 3600. * (double)hh - 60. * (double)mi);
      if (ss == 60) { ss = 0; mi = mi + 1; }
      if (mi == 60) { mi = 0; hh = hh + 1; }
      *hhmiss = 10000 * hh + 100 * mi + ss;
    }
    return 10000 * yyyy + 100 * mm + dd;
  }
  // getvdep.f90:51-77: the seasonal category of every grid row at wind-field time wftime.  The rows of a nest go through
  // the very same formula, ylat = jy*dy + ylat0 with the MOTHER grid's dy, ylat0 (getvdep_nests.f90:54), over its nyn rows
  template <typename H>
  void gv_seasons(int wftime, std::vector<unsigned char> &ls, int ny) {
#pragma clang fp contract(off)
    ls.resize(ny);
    for (int jy = 0; jy < ny; jy++) {
      double jul = gv_bdate + (double)wftime / 86400.;
      const H ylat = (H)jy * (H)cfg.dy + (H)cfg.ylat0;
      if (ylat < (H)0) jul = jul + (double)(365 / 2);
      const int yyyymmdd = gv_caldate<H>(jul);
      const int yyyy = yyyymmdd / 10000;
      int mmdd = yyyymmdd - 10000 * yyyy;
      if (ylat > (H)-20 && ylat < (H)20) mmdd = 600;
      int lseason;
      if (mmdd >= 1201 || mmdd <= 301) lseason = 4;
      else if (mmdd >= 1101 || mmdd <= 331) lseason = 3;
      else if (mmdd >= 401 && mmdd <= 515) lseason = 5;
      else if (mmdd >= 516 && mmdd <= 915) lseason = 1;
      else lseason = 2;
      ls[jy] = (unsigned char)lseason;
    }
  }

  // gr = 0: the mother grid (calcpar.f90:171-189 with getvdep.f90); gr = l >= 1: nested grid l (calcpar_nests.f90:139-157 with
  // getvdep_nests.f90): the same kernel on the nest's arrays and xlandusen(:,:,:,l), with buffers and a gather pack of the nest's own
  template <typename H>
  int getvdep_t(int gr, int slot, const fpx_getvdep_in *g, void *vdep_out) {
    const HostGrid HG = host_grid(gr);
    const WindDst T = wind_dst(gr);
    const int s = slot - 1, nspec = cfg.nspec;
    const size_t n2 = (size_t)HG.nxmax * HG.nymax;
    int rc;
    if (!gv_buf[gr]) {
      H *q = nullptr;
      if ((rc = dalloc(&q, (9 + (size_t)FPX_MAXSPEC) * n2))) return rc;      // ssr, lsprec, convprec, sd, ustar, oli, ps, tt2, td2 | vdep planes
      HIPCHK(hipMemsetAsync(q, 0, (9 + (size_t)FPX_MAXSPEC) * n2 * sizeof(H), stream));
      gv_buf[gr] = q;
      if ((rc = dalloc(&gv_season[gr], (size_t)HG.ny))) return rc;
    }
    H *B = (H *)gv_buf[gr];
    const void *host[9] = {g->ssr, g->lsprec, g->convprec, g->sd, g->ustar, g->oli, g->ps, g->tt2, g->td2};
    const H *dev[9];
    for (int i = 0; i < 9; i++) {
      dev[i] = B + i * n2;
      if (host[i]) HIPCHK(hipMemcpyAsync(B + i * n2, host[i], n2 * sizeof(H), hipMemcpyHostToDevice, stream));
    }
    if (!g->ustar) dev[4] = (const H *)cp_buf[gr] + 3 * n2;                    // what fpx_calcpar / fpx_calcpar_nest of this grid left (calcpar_t)
    if (!g->oli) dev[5] = (const H *)cp_buf[gr] + 5 * n2;
    for (int i = 6; i < 9; i++)
      if (!host[i]) dev[i] = (const H *)vt_sets[gr][i];                        // PS, TT2, TD2 of the grid's transform (verttransform_t)
    std::vector<unsigned char> ls;
    gv_seasons<H>(g->wftime, ls, HG.ny);
    HIPCHK(hipMemcpyAsync(gv_season[gr], ls.data(), ls.size(), hipMemcpyHostToDevice, stream));
    gv::Args<H> A;
    A.nx = HG.nx; A.ny = HG.ny; A.nxmax = HG.nxmax; A.nymax = HG.nymax; A.nspec = nspec;
    A.T = gv_lay; A.tables = (const H *)gv_tab; A.xlanduse = (const H *)gv_land[gr];
    A.ssr = dev[0]; A.lsprec = dev[1]; A.convprec = dev[2]; A.sd = dev[3]; A.ustar = dev[4]; A.oli = dev[5]; A.ps = dev[6]; A.tt2 = dev[7]; A.td2 = dev[8];
    A.lseason = gv_season[gr];
    H *d_vdep = B + 9 * n2;
    A.vdep = d_vdep;
    Events<2> ev;
    HIPCHK(ev.create());
    HIPCHK(hipEventRecord(ev[0], stream));
    gv::k_getvdep<H><<<(HG.nx * HG.ny + 255) / 256, 256, (size_t)gv_lay.total() * sizeof(H), stream>>>(A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], stream));
    // into the gather pack, as upload_fields / upload_nest_fields do from the host's vdep(0,0,1,n) planes
    const int tot = HG.nx * HG.ny;
    for (int ks = 0; ks < nspec; ks++) {
      k_pack2<H, R><<<(tot + kBlock - 1) / kBlock, kBlock, 0, stream>>>(d_vdep + n2 * ks, (R *)T.vdep, HG.nx, HG.ny, HG.nxmax, 2 * nspec, s * nspec + ks);
      HIPCHK(hipGetLastError());
    }
    if (vdep_out) HIPCHK(hipMemcpyAsync(vdep_out, d_vdep, n2 * nspec * sizeof(H), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    gv_last_ms = ms;
    // fpx_calcpar / fpx_calcpar_nest (device_vdep = 1) was waiting for this
    if (gr == 0) { if (vdep_pending[s]) { vdep_pending[s] = false; slot_loaded[s] = true; } }
    else if (nest_vdep_pending[gr - 1][s]) { nest_vdep_pending[gr - 1][s] = false; nest_loaded[gr - 1][s] = true; }
    return 0;
  }
  int getvdep(int slot, const fpx_getvdep_in *g, void *vdep_out) override {
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "getvdep: slot must be 1 or 2");
    if (!cfg.drydep || !V.vdep) return fail(FPX_ERR_ARG, "getvdep: the run has no dry deposition (DRYDEP)");
    if (!gv_ready) return fail(FPX_ERR_STATE, "getvdep: fpx_getvdep_init first (the land-use inventory and the resistance tables)");
    if (!g || !g->ssr || !g->lsprec || !g->convprec || !g->sd) return fail(FPX_ERR_ARG, "getvdep: ssr, lsprec, convprec, sd are required");
    if ((!g->ustar || !g->oli) && (!cp_buf[0] || cp_slot_on_device[0] != slot))
      return fail(FPX_ERR_ARG, "getvdep: ustar / oli = NULL means the ones fpx_calcpar / fpx_calcpar_gfs left on the device: that call for this slot first");
    if ((!g->ps || !g->tt2 || !g->td2) && (!vt_set_ready[0] || vt_slot_on_device[0] != slot))
      return fail(FPX_ERR_ARG, "getvdep: ps / tt2 / td2 = NULL means the ones of fpx_verttransform_ecmwf / fpx_verttransform_gfs: transform this slot first");
    return cfg.host_real_bytes == 4 ? getvdep_t<float>(0, slot, g, vdep_out) : getvdep_t<double>(0, slot, g, vdep_out);
  }
  int getvdep_nest(int nest, int slot, const fpx_getvdep_in *g, void *vdep_out) override {
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "getvdep_nest: nest out of range (fpx_nests_init first)");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "getvdep_nest: slot must be 1 or 2");
    if (!cfg.drydep || !h_nest[nest - 1].vdep) return fail(FPX_ERR_ARG, "getvdep_nest: the run has no dry deposition (DRYDEP)");
    if (!gv_ready || !gv_nest_ready[nest - 1]) return fail(FPX_ERR_STATE, "getvdep_nest: fpx_getvdep_init, then fpx_getvdep_nest_init of this nest first (the tables and the nest's land-use inventory)");
    if (!g || !g->ssr || !g->lsprec || !g->convprec || !g->sd) return fail(FPX_ERR_ARG, "getvdep_nest: ssrn, lsprecn, convprecn, sdn are required");
    if ((!g->ustar || !g->oli) && (!cp_buf[nest] || cp_slot_on_device[nest] != slot))
      return fail(FPX_ERR_ARG, "getvdep_nest: ustarn / olin = NULL means the ones fpx_calcpar_nest left on the device: fpx_calcpar_nest of this nest and slot first");
    if ((!g->ps || !g->tt2 || !g->td2) && (!vt_set_ready[nest] || vt_slot_on_device[nest] != slot))
      return fail(FPX_ERR_ARG, "getvdep_nest: psn / tt2n / td2n = NULL means the ones of fpx_verttransform_nest: transform this nest and slot first");
    return cfg.host_real_bytes == 4 ? getvdep_t<float>(nest, slot, g, vdep_out) : getvdep_t<double>(nest, slot, g, vdep_out);
  }
  double gv_ms() override { return gv_last_ms; }
  double vt_last_ms = 0, po_last_ms = 0;
  double po_ms() override { return po_last_ms; }
  double vt_ms() override { return vt_last_ms; }
  double cp_ms() override { return cp_last_ms; }

  // ---- verttransform_gfs on the device (fpx_verttransform_gfs.hpp) ----------------------------------------------
  // NCEP GFS pressure-level input -> z-level fields.  The same buffers, calcpv launch and repacking as verttransform_t;
  // the kernels, the per-slot persistent ww and pplev are its own.
  enum { MET_NONE = 0, MET_ECMWF = 1, MET_GFS = 2 };
  int met_format = MET_NONE;              // set by the first successful transform of the handle
  void *gfs_ww[2] = {nullptr, nullptr};   // ww(:,:,:,n) of com_mod in the host's layout and kind: zero at first use, cells the
  void *gfs_pplev = nullptr;              // routine does not write keep their content (verttransform_gfs.f90:271-285); pplev of the last call
  template <typename H>
  int verttransform_gfs_t(int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out, void *pplev_out) {
    const int nz = cfg.nz;
    const HostGrid HG = host_grid(0);
    const int gnx = HG.nx, gny = HG.ny, gnxmax = HG.nxmax, gnymax = HG.nymax;
    void **vt_dev = vt_sets[0];
    const size_t n2 = (size_t)gnxmax * gnymax, n3 = n2 * nz;
    int rc;
    enum { UUH, VVH, PVH, WWH, TTH, QVH, PS, TT2, TD2, AKZ, BKZ, AKN, BKN, HGT,
           UU, VV, WW, TT, QV, PV, RHO, DRHO, UPOL, VPOL, UVZ, WZ, RHOH, PINM, KUV, KW, NBUF };
    if (!vt_set_ready[0]) {               // the buffer set of verttransform_t (fpx_get_pvh reads its PVH)
      for (int i = 0; i < NBUF; i++) {
        const size_t n = (i >= PS && i <= TD2) ? n2 : (i >= AKZ && i <= HGT) ? (size_t)nz : n3;
        H *q = nullptr;
        if ((rc = dalloc(&q, n))) return rc;
        HIPCHK(hipMemsetAsync(q, 0, n * sizeof(H), stream));
        vt_dev[i] = q;
      }
      vt_set_ready[0] = true;
    }
    for (int i = 0; i < 3; i++) {
      void *&dst = i < 2 ? gfs_ww[i] : gfs_pplev;
      if (dst) continue;
      H *q = nullptr;
      if ((rc = dalloc(&q, n3))) return rc;
      HIPCHK(hipMemsetAsync(q, 0, n3 * sizeof(H), stream));
      dst = q;
    }
    auto D = [&](int i) { return (H *)vt_dev[i]; };
    const int s = slot - 1;
    H *d_ww = (H *)gfs_ww[s], *d_pplev = (H *)gfs_pplev;
    if (m->init || !height_set) {         // verttransform_gfs.f90:84-139: the same code as the ECMWF routine's
      std::vector<H> hgt;
      int nmixz = 0;
      if ((rc = vt_init_height<H>(m, hgt, nmixz))) return rc;
      if ((rc = set_height(hgt.data(), nz))) return rc;
      V.nmixz = nmixz;
      cfg.nmixz = nmixz;
    }
    {
      std::vector<H> hh(nz);
      for (int k = 0; k < nz; k++) hh[k] = (H)height_host[k];
      HIPCHK(hipMemcpyAsync(D(HGT), hh.data(), nz * sizeof(H), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    const void *src[13] = {m->uuh, m->vvh, m->pvh, m->wwh, m->tth, m->qvh, m->ps, m->tt2, m->td2, m->akz, m->bkz, m->aknew, m->bknew};
    for (int i = 0; i < 13; i++) {
      if (i == PVH && !m->pvh) continue;
      const size_t n = (i >= PS && i <= TD2) ? n2 : (i >= AKZ) ? (size_t)nz : n3;
      if (m->pin_host && n >= n2) pin_host_range(src[i], n * sizeof(H));
      HIPCHK(hipMemcpyAsync(D(i), src[i], n * sizeof(H), hipMemcpyHostToDevice, stream));
    }
    vt::Geo<H> G;
    G.nx = gnx; G.ny = gny; G.nz = nz; G.nuvz = nz; G.nwz = nz; G.nxmax = gnxmax; G.nymax = gnymax;
    G.dx = (H)cfg.dx; G.dy = (H)cfg.dy; G.xlon0 = (H)cfg.xlon0; G.ylat0 = (H)cfg.ylat0;
    {   // gridcheck_gfs.f90:241-242
      const H pi = (H)3.14159265, r_earth = (H)6.371e6;
      G.dxconst = (H)180. / (G.dx * r_earth * pi);
      G.dyconst = (H)180. / (G.dy * r_earth * pi);
    }
    G.xres = (H)1.; G.yres = (H)1.;
    G.nglobal = cfg.nglobal; G.sglobal = cfg.sglobal;
    G.switchnorthg = (H)cfg.switchnorthg; G.switchsouthg = (H)cfg.switchsouthg;
    for (int i = 0; i < 9; i++) { G.northpolemap[i] = (H)cfg.northpolemap[i]; G.southpolemap[i] = (H)cfg.southpolemap[i]; }
    vt::In<H> I{D(UUH), D(VVH), D(PVH), D(WWH), D(TTH), D(QVH), D(PS), D(TT2), D(TD2), D(AKZ), D(BKZ), D(AKN), D(BKN), D(HGT)};
    vt::Out<H> O{D(UU), D(VV), d_ww, D(TT), D(QV), D(PV), D(RHO), D(DRHO), D(UPOL), D(VPOL), D(UVZ), D(WZ), D(RHOH), D(PINM)};
    Events<2> pev, ev;
    if (!m->pvh) {                        // calcpv.f90 has no format branch: ppml = akz + bkz*ps
      pv::Args<H> P;
      P.nx = gnx; P.ny = gny; P.nuvz = nz; P.nxmax = gnxmax; P.nymax = gnymax;
      P.xglobal = cfg.xglobal; P.nglobal = cfg.nglobal; P.sglobal = cfg.sglobal;
      P.dx = (H)cfg.dx; P.dy = G.dy; P.ylat0 = G.ylat0;
      P.uuh = D(UUH); P.vvh = D(VVH); P.tth = D(TTH); P.ps = D(PS); P.akz = D(AKZ); P.bkz = D(BKZ);
      P.ppml = D(UVZ); P.theta = D(WZ); P.pvh = D(PVH);
      HIPCHK(pev.create());
      HIPCHK(hipEventRecord(pev[0], stream));
      const dim3 gp((gnx * gny + 255) / 256, nz);
      pv::k_theta<H><<<gp, 256, 0, stream>>>(P);
      pv::k_pv<H><<<gp, 256, 0, stream>>>(P);
      if (P.nglobal || P.sglobal) pv::k_pole<H><<<dim3((nz + 63) / 64, 2), 64, 0, stream>>>(P);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(pev[1], stream));
    }
    HIPCHK(ev.create());
    HIPCHK(hipEventRecord(ev[0], stream));
    const int nb = (gnx * gny + 255) / 256;
    vt::k_vg_levels<H><<<nb, 256, 0, stream>>>(G, I, O);
    vt::k_vg_column<H><<<nb, 256, (size_t)5 * nz * sizeof(H), stream>>>(G, I, O, d_pplev);
    const size_t smrow = (size_t)(gnx + 3) * sizeof(H);
    if (G.nglobal) {
      const int jy0 = std::max(0, (int)G.switchnorthg - 2), jy1 = cfg.ny - 1;
      if (jy1 >= jy0) vt::k_vt_polar<H><<<dim3((cfg.nx + 255) / 256, jy1 - jy0 + 1, nz), 256, 0, stream>>>(G, O, jy0, jy1, 0);
      vt::k_vg_polerow<H><<<nz, 64, smrow, stream>>>(G, O, 0);
    }
    if (G.sglobal) {
      const int jy0 = 0, jy1 = std::min(cfg.ny - 1, (int)G.switchsouthg + 3);
      if (jy1 >= jy0) vt::k_vt_polar<H><<<dim3((cfg.nx + 255) / 256, jy1 - jy0 + 1, nz), 256, 0, stream>>>(G, O, jy0, jy1, 1);
      vt::k_vg_polerow<H><<<nz, 64, smrow, stream>>>(G, O, 1);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev[1], stream));
    // repack into the gather layout, as verttransform_t does
    auto pk = [&](const H *in, const R *outp, int stride, int off) -> int {
      dim3 grid((gnx + 31) / 32, (nz + 31) / 32, gny), block(32, 8);
      k_pack3<H, R><<<grid, block, 0, stream>>>(in, (R *)outp, gnx, gny, nz, gnxmax, gnymax, stride, off);
      HIPCHK(hipGetLastError());
      return 0;
    };
    const WindDst T = wind_dst(0);
    if ((rc = pk(D(UU), T.w3, 6, s * 3 + 0)) || (rc = pk(D(VV), T.w3, 6, s * 3 + 1)) || (rc = pk(d_ww, T.w3, 6, s * 3 + 2))) return rc;
    if (T.w3pol)
      if ((rc = pk(D(UPOL), T.w3pol, 6, s * 3 + 0)) || (rc = pk(D(VPOL), T.w3pol, 6, s * 3 + 1)) || (rc = pk(d_ww, T.w3pol, 6, s * 3 + 2))) return rc;
    if ((rc = pk(D(RHO), T.r2, 4, s * 2 + 0)) || (rc = pk(D(DRHO), T.r2, 4, s * 2 + 1))) return rc;
    if (slot == 1 && T.rhott)
      if ((rc = pk(D(RHO), T.rhott, 2, 0)) || (rc = pk(D(TT), T.rhott, 2, 1))) return rc;
    if (wet_on && Wp.ttw) { if ((rc = pk(D(TT), Wp.ttw, 2, s))) return rc; }
    const bool have2d = sfc->hmix != nullptr;       // all five or none (checked by the caller); none: fpx_calcpar_gfs follows
    if (have2d && (rc = upload_wind2(0, slot, sfc))) return rc;
    if ((rc = diag_alloc())) return rc;
    if ((rc = diag3(D(PV), true, 0, s)) || (rc = diag3(D(QV), true, 1, s)) || (rc = diag3(D(TT), true, 2, s))) return rc;
    if (have2d) k_hcell<R><<<(gnx * gny + kBlock - 1) / kBlock, kBlock, 0, stream>>>(T.sfc, (R *)T.hcell, gnx, gny);
    HIPCHK(hipGetLastError());
    if (out) {
      void *dst[10] = {out->uu, out->vv, out->ww, out->tt, out->qv, out->pv, out->rho, out->drhodz, out->uupol, out->vvpol};
      for (int i = 0; i < 10; i++)
        if (dst[i]) HIPCHK(hipMemcpyAsync(dst[i], i == 2 ? d_ww : D(UU + i), n3 * sizeof(H), hipMemcpyDeviceToHost, stream));
      if (out->height) for (int k = 0; k < nz; k++) ((H *)out->height)[k] = (H)height_host[k];
      if (out->nmixz) *out->nmixz = V.nmixz;
    }
    if (pplev_out) HIPCHK(hipMemcpyAsync(pplev_out, d_pplev, n3 * sizeof(H), hipMemcpyDeviceToHost, stream));
    if (conv_gfs && (rc = conv_keep_gfs<H>(slot, D(PS), D(TT2), D(TD2), D(TT), D(QV), d_pplev))) return rc;
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    vt_last_ms = ms;
    pv_last_ms = 0;
    if (!m->pvh) {
      HIPCHK(hipEventElapsedTime(&ms, pev[0], pev[1]));
      pv_last_ms = ms;
    }
    pvh_on_device[0] = true;
    // without the 2-D fields the slot still holds those of the previous wind field until fpx_calcpar_gfs has run: not loaded
    slot_loaded[s] = have2d; vdep_pending[s] = false;
    vt_slot_on_device[0] = slot;
    return 0;
  }
  int verttransform_gfs(int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out, void *pplev_out) override {
    if (met_format == MET_ECMWF) return fail(FPX_ERR_UNSUPPORTED, "verttransform_gfs: this handle has run an ECMWF transform (fpx_verttransform_ecmwf / fpx_verttransform_nest): GFS fields are refused on it");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "verttransform_gfs: slot must be 1 or 2");
    if (!m || !m->uuh || !m->vvh || !m->wwh || !m->tth || !m->qvh || !m->ps || !m->tt2 || !m->td2 || !m->akz || !m->bkz || !m->aknew || !m->bknew)
      return fail(FPX_ERR_ARG, "verttransform_gfs: uuh, vvh, wwh, tth, qvh, ps, tt2, td2, akz, bkz, aknew, bknew are required (pvh = NULL: calcpv on the device)");
    if (m->nuvz != cfg.nz || m->nwz != cfg.nz) return fail(FPX_ERR_ARG, "verttransform_gfs: nuvz = nwz = nz expected (gridcheck_gfs.f90:439-491 sets them equal)");
    if (cfg.nz < 4 || cfg.nz > 65535 || cfg.ny > 65535) return fail(FPX_ERR_ARG, "verttransform_gfs: 4 <= nz <= 65535, ny <= 65535");
    if (!sfc) return fail(FPX_ERR_UNSUPPORTED, "verttransform_gfs: sfc = NULL: the NCEP branch of calcpar.f90:109-121,145-149 is not computed by this engine; pass the host's hmix, ustar, wstar, oli, tropopause");
    const int n2d = (sfc->hmix != nullptr) + (sfc->ustar != nullptr) + (sfc->wstar != nullptr) + (sfc->oli != nullptr) + (sfc->tropopause != nullptr);
    if (n2d != 0 && n2d != 5) return fail(FPX_ERR_ARG, "verttransform_gfs: the 2-D fields hmix, ustar, wstar, oli, tropopause are required (or all five NULL and fpx_calcpar_gfs)");
    if (n2d == 5 && cfg.drydep && !sfc->vdep) return fail(FPX_ERR_ARG, "verttransform_gfs: vdep required with DRYDEP");
    if (!m->pvh && (cfg.nx < 3 || cfg.ny < 4)) return fail(FPX_ERR_ARG, "verttransform_gfs: calcpv on the device (pvh = NULL) needs nx >= 3, ny >= 4");
    const int rc = cfg.host_real_bytes == 4 ? verttransform_gfs_t<float>(slot, m, sfc, out, pplev_out) : verttransform_gfs_t<double>(slot, m, sfc, out, pplev_out);
    if (!rc) met_format = MET_GFS;
    return rc;
  }

  int verttransform(int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out) override {
    if (met_format == MET_GFS) return fail(FPX_ERR_UNSUPPORTED, "verttransform: this handle takes NCEP GFS fields (fpx_verttransform_gfs has run): the ECMWF transform is refused on it");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "verttransform: slot must be 1 or 2");
    if (!m || !m->uuh || !m->vvh || !m->wwh || !m->tth || !m->qvh || !m->ps || !m->tt2 || !m->td2 || !m->akz || !m->bkz || !m->aknew || !m->bknew)
      return fail(FPX_ERR_ARG, "verttransform: uuh, vvh, wwh, tth, qvh, ps, tt2, td2, akz, bkz, aknew, bknew are required (pvh = NULL: calcpv on the device)");
    if (m->nuvz != cfg.nz || m->nwz != cfg.nz) return fail(FPX_ERR_ARG, "verttransform: nuvz = nwz = nz expected (gridcheck_ecmwf.f90 sets them equal)");
    if (cfg.nz < 3 || cfg.nz > 65535 || cfg.ny > 65535) return fail(FPX_ERR_ARG, "verttransform: 3 <= nz <= 65535, ny <= 65535");
    if (sfc && (!sfc->hmix || !sfc->ustar || !sfc->wstar || !sfc->oli || !sfc->tropopause)) return fail(FPX_ERR_ARG, "verttransform: the 2-D fields hmix, ustar, wstar, oli, tropopause are required (or sfc = NULL and fpx_calcpar)");
    if (sfc && cfg.drydep && !sfc->vdep) return fail(FPX_ERR_ARG, "verttransform: vdep required with DRYDEP");
    if (!m->pvh && (cfg.nx < 3 || cfg.ny < 4)) return fail(FPX_ERR_ARG, "verttransform: calcpv on the device (pvh = NULL) needs nx >= 3, ny >= 4");
    const int rc = cfg.host_real_bytes == 4 ? verttransform_t<float>(0, slot, m, sfc, out) : verttransform_t<double>(0, slot, m, sfc, out);
    if (!rc) met_format = MET_ECMWF;
    return rc;
  }
  int verttransform_nest(int nest, int slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out) override {
    if (met_format == MET_GFS) return fail(FPX_ERR_UNSUPPORTED, "verttransform_nest: this handle takes NCEP GFS fields (fpx_verttransform_gfs has run): the reference has no GFS nests");
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "verttransform_nest: nest out of range (fpx_nests_init first)");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "verttransform_nest: slot must be 1 or 2");
    if (!height_set) return fail(FPX_ERR_STATE, "verttransform_nest: the z levels come from the mother grid's first transform (or fpx_set_height)");
    if (!m || !m->uuh || !m->vvh || !m->wwh || !m->tth || !m->qvh || !m->ps || !m->tt2 || !m->td2 || !m->akz || !m->bkz || !m->aknew || !m->bknew)
      return fail(FPX_ERR_ARG, "verttransform_nest: uuhn, vvhn, wwhn, tthn, qvhn, psn, tt2n, td2n, akz, bkz, aknew, bknew are required (pvhn = NULL: calcpv_nests on the device)");
    if (m->nuvz != cfg.nz || m->nwz != cfg.nz) return fail(FPX_ERR_ARG, "verttransform_nest: nuvz = nwz = nz expected");
    if (!(m->nest_dy > 0)) return fail(FPX_ERR_ARG, "verttransform_nest: nest_dy (dyn) and nest_ylat0 (ylat0n) of fpx_model_levels are required");
    if (sfc && (!sfc->hmix || !sfc->ustar || !sfc->wstar || !sfc->oli || !sfc->tropopause)) return fail(FPX_ERR_ARG, "verttransform_nest: hmixn, ustarn, wstarn, olin, tropopausen are required (or sfc = NULL and fpx_calcpar_nest)");
    if (sfc && cfg.drydep && !sfc->vdep) return fail(FPX_ERR_ARG, "verttransform_nest: vdepn required with DRYDEP");
    if (!m->pvh) {
      if (!pv_ready) return fail(FPX_ERR_STATE, "verttransform_nest: fpx_calcpv_init first (dxn of the nests) to compute pvhn on the device");
      if (!(pv_dxn[nest - 1] > 0)) return fail(FPX_ERR_ARG, "verttransform_nest: dxn of this nest (fpx_calcpv_init) must be positive");
      if (h_nest[nest - 1].nx < 3 || h_nest[nest - 1].ny < 4) return fail(FPX_ERR_ARG, "verttransform_nest: calcpv_nests on the device (pvhn = NULL) needs nxn >= 3, nyn >= 4");
    }
    return cfg.host_real_bytes == 4 ? verttransform_t<float>(nest, slot, m, sfc, out) : verttransform_t<double>(nest, slot, m, sfc, out);
  }


  // ---- partoutput -------------------------------------------------------
  void *diag_oro = nullptr, *diag_tropo[2] = {nullptr, nullptr}, *diag_d3 = nullptr;   // in the host's real kind
  bool diag_have[9] = {};          // oro | pv, qv, tt of slot 1, 2 | tropopause of slot 1, 2
  enum { DG_ORO = 0, DG_PV = 1, DG_QV = 3, DG_TT = 5, DG_TROPO = 7 };
  int diag_alloc() {
    int rc;
    const size_t n2 = (size_t)cfg.nxmax * cfg.nymax * cfg.host_real_bytes;
    char *p = nullptr;
    if (!diag_oro) { if ((rc = dalloc(&p, n2))) return rc; diag_oro = p; HIPCHK(hipMemsetAsync(p, 0, n2, stream)); }
    for (int m = 0; m < 2; m++)
      if (!diag_tropo[m]) { if ((rc = dalloc(&p, n2))) return rc; diag_tropo[m] = p; HIPCHK(hipMemsetAsync(p, 0, n2, stream)); }
    if (!diag_d3) {
      const size_t n = (size_t)cfg.nx * cfg.ny * cfg.nz * 6 * cfg.host_real_bytes;
      if ((rc = dalloc(&p, n))) return rc;
      diag_d3 = p;
      HIPCHK(hipMemsetAsync(p, 0, n, stream));
    }
    return 0;
  }
  int diag2_from_host(void *dev, const void *host, int have) {
    HIPCHK(hipMemcpyAsync(dev, host, (size_t)cfg.nxmax * cfg.nymax * cfg.host_real_bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    diag_have[have] = true;
    return 0;
  }
  // one 3-D field in the host's layout (host memory, or device memory when `on_device`) -> component c of slot s of d3
  int diag3(const void *src, bool on_device, int c, int s) {
    const int rc = cfg.host_real_bytes == 4 ? pack3<float>(host_grid(0), src, (float *)diag_d3, 6, s * 3 + c, on_device)
                                            : pack3<double>(host_grid(0), src, (double *)diag_d3, 6, s * 3 + c, on_device);
    if (!rc) diag_have[DG_PV + 2 * c + s] = true;
    return rc;
  }
  // oron and ttn of a nested wind field for releaseparticles (:216-273): compact copies in the host's real kind
  void *rel_nest_oro[kMaxNests] = {}, *rel_nest_tt2[kMaxNests] = {};
  int upload_diag_nest_fields(int nest, int slot, const fpx_diag_fields *f) override {
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "upload_diag_nest_fields: nest out of range (fpx_nests_init first)");
    if (!f || slot < 0 || slot > 2) return fail(FPX_ERR_ARG, "upload_diag_nest_fields: slot 0 (oron only), 1 or 2");
    const HostGrid G = host_grid(nest);
    const size_t n2 = (size_t)G.nx * G.ny * cfg.host_real_bytes;
    const int l = nest - 1;
    int rc;
    if (f->oro) {
      if (!rel_nest_oro[l]) { char *q = nullptr; if ((rc = dalloc(&q, n2))) return rc; rel_nest_oro[l] = q; }
      if ((rc = compact(G, f->oro, rel_nest_oro[l], 1, 1))) return rc;
    }
    if (slot == 2 && f->tt) {
      if (!rel_nest_tt2[l]) { char *q = nullptr; if ((rc = dalloc(&q, n2 * cfg.nz))) return rc; rel_nest_tt2[l] = q; }
      if ((rc = compact(G, f->tt, rel_nest_tt2[l], cfg.nz, cfg.nz))) return rc;
    }
    return 0;
  }

  int upload_diag_fields(int slot, const fpx_diag_fields *f) override {
    if (!f || slot < 0 || slot > 2) return fail(FPX_ERR_ARG, "upload_diag_fields: slot 0 (oro only), 1 or 2");
    int rc;
    if ((rc = diag_alloc())) return rc;
    if (f->oro && (rc = diag2_from_host(diag_oro, f->oro, DG_ORO))) return rc;
    if (slot == 0) return 0;
    const int s = slot - 1;
    if (f->pv && (rc = diag3(f->pv, false, 0, s))) return rc;
    if (f->qv && (rc = diag3(f->qv, false, 1, s))) return rc;
    if (f->tt && (rc = diag3(f->tt, false, 2, s))) return rc;
    return 0;
  }

  template <typename H>
  int partoutput_t(int itime, const char *path, int64_t *nrec) {
    const long long n = numpart;
    const int reclen = 8 + (10 + cfg.nspec) * (int)sizeof(H);
    const size_t recwords = (size_t)reclen / 4 + 2;
    Scratch b_flags, b_idx, b_out, b_tmp;
    RecFile file(path);
    if (!file.is_open()) return fail(FPX_ERR_ARG, std::string("partoutput: cannot open ") + path);
    unsigned int count = 0;
    file.scalar((int32_t)itime);                         // write(unitpartout) itime, partoutput.f90:90
    if (n > 0) {
      hipError_t e;
      if ((e = b_flags.reserve(n * sizeof(unsigned int), stream)) != hipSuccess || (e = b_idx.reserve(n * sizeof(unsigned int), stream)) != hipSuccess)
        return fail(FPX_ERR_NOMEM, std::string("partoutput: ") + hipGetErrorString(e));
      unsigned int *flags = b_flags.as<unsigned int>(), *idx = b_idx.as<unsigned int>();
      const int nb = (int)((n + kBlock - 1) / kBlock);
      Events<2> ev;
      (void)ev.create();
      (void)hipEventRecord(ev[0], stream);
      k_po_flags<R><<<nb, kBlock, 0, stream>>>(P, n, itime, flags);
      size_t tb = 0;
      (void)rocprim::exclusive_scan(nullptr, tb, flags, idx, 0u, (size_t)n, rocprim::plus<unsigned int>(), stream);
      if ((e = b_tmp.reserve(tb, stream)) != hipSuccess) return fail(FPX_ERR_NOMEM, "partoutput: scan storage");
      e = rocprim::exclusive_scan(b_tmp.as(), tb, flags, idx, 0u, (size_t)n, rocprim::plus<unsigned int>(), stream);
      unsigned int last_idx = 0, last_flag = 0;
      if (e == hipSuccess) e = hipMemcpyAsync(&last_idx, idx + (n - 1), 4, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess) e = hipMemcpyAsync(&last_flag, flags + (n - 1), 4, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("partoutput: ") + hipGetErrorString(e));
      count = last_idx + last_flag;
      if (count > 0) {
        const size_t words = (size_t)count * recwords;
        if ((e = b_out.reserve(words * 4, stream)) != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("partoutput: record buffer: ") + hipGetErrorString(e));
        unsigned int *out = b_out.as<unsigned int>();
        const DiagP<H> D = diag_args<H>();
        k_partoutput<R, H><<<nb, kBlock, 0, stream>>>(V, P, D, idx, n, itime, out);
        e = hipGetLastError();
        (void)hipEventRecord(ev[1], stream);
        if (e == hipSuccess && hipEventSynchronize(ev[1]) == hipSuccess) {
          float ms = 0;
          if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) po_last_ms = ms;
        }
        // stream the record bytes to the file through two pinned bounce buffers: the copy of chunk k+1 runs while
        // chunk k is written (the call is bound by the host's write, about 4 GB/s into tmpfs)
        const size_t chunk = (size_t)64 << 20, total = words * 4;
        Scratch pin(true);
        Events<2> done;
        if (e == hipSuccess) e = pin.reserve(2 * std::min(chunk, total), stream);
        if (e == hipSuccess) e = done.create();
        const size_t bufsz = std::min(chunk, total);
        auto issue = [&](size_t k) -> hipError_t {
          const size_t off = k * chunk, nbytes = std::min(chunk, total - off);
          hipError_t r = hipMemcpyAsync(pin.as<char>() + (k & 1) * bufsz, (const char *)out + off, nbytes, hipMemcpyDeviceToHost, stream);
          return r == hipSuccess ? hipEventRecord(done[k & 1], stream) : r;
        };
        const size_t nchunks = (total + chunk - 1) / chunk;
        if (e == hipSuccess) e = issue(0);
        for (size_t k = 0; e == hipSuccess && file.ok() && k < nchunks; k++) {
          e = hipEventSynchronize(done[k & 1]);
          if (e == hipSuccess && k + 1 < nchunks) e = issue(k + 1);
          const size_t nbytes = std::min(chunk, total - k * chunk);
          if (e == hipSuccess) file.write(pin.as<char>() + (k & 1) * bufsz, nbytes);   // the kernel has framed the records
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream); else (void)hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("partoutput: ") + hipGetErrorString(e));
      }
    }
    {   // the closing record, partoutput.f90:182-184
      const int32_t m5 = -99999;
      const H m4 = (H)-9999.9;
      file.put(m5);
      for (int j = 0; j < 3; j++) file.put(m4);
      file.put(m5);
      for (int j = 0; j < 7 + cfg.nspec; j++) file.put(m4);
      file.end();                                        // reclen bytes, as every record of the kernel
    }
    if (!file.close()) return fail(FPX_ERR_ARG, std::string("partoutput: write error on ") + path);
    if (nrec) *nrec = count;
    return 0;
  }

  int partoutput(int itime, const char *path, int64_t *nrec) override {
    if (!path) return fail(FPX_ERR_ARG, "partoutput: null path");
    if (!height_set || !window_set || !slot_loaded[0] || !slot_loaded[1]) return fail(FPX_ERR_STATE, "partoutput: height, both field slots and the wind-time window must be set first");
    for (int i = 0; i < 9; i++)
      if (!diag_have[i]) return fail(FPX_ERR_STATE, "partoutput: oro, pv, qv, tt (fpx_upload_diag_fields or fpx_verttransform_ecmwf) and tropopause of both slots are needed");
    return cfg.host_real_bytes == 4 ? partoutput_t<float>(itime, path, nrec) : partoutput_t<double>(itime, path, nrec);
  }


  // ---- readpartpositions (warm start from the dump) -----------------------
  // random_mod.f90:12-42 (ran1), for nclass when nclassunc > 1: one serial stream, seed -8
  struct Ran1 {
    int iv[32] = {}, iy = 0, idum = -8;
    template <typename H>
    H next() {
      const int ia = 16807, im = 2147483647, iq = 127773, ir = 2836, ntab = 32, ndiv = 1 + (im - 1) / ntab;
      const H am = (H)1. / (H)im, rnmx = (H)1. - (H)1.2e-7;
      if (idum <= 0 || iy == 0) {
        idum = std::max(-idum, 1);
        for (int j = ntab + 8; j >= 1; j--) {
          const int k = idum / iq;
          idum = ia * (idum - k * iq) - ir * k;
          if (idum < 0) idum += im;
          if (j <= ntab) iv[j - 1] = idum;
        }
        iy = iv[0];
      }
      const int k = idum / iq;
      idum = ia * (idum - k * iq) - ir * k;
      if (idum < 0) idum += im;
      const int j = 1 + iy / ndiv;
      iy = iv[j - 1];
      iv[j - 1] = idum;
      return std::min(am * (H)iy, rnmx);
    }
  };

  template <typename H>
  int readpart_t(const char *path, const fpx_restart *r, int64_t *numpart_out, int32_t *numparticlecount, int32_t *itimein_out) {
    FILE *fh = fopen(path, "rb");
    if (!fh) return fail(FPX_ERR_ARG, std::string("readpartpositions: cannot open ") + path);
    FileCloser closer(fh);
    if (fseek(fh, 0, SEEK_END) != 0) return fail(FPX_ERR_ARG, "readpartpositions: seek");
    const long long size = ftell(fh);
    rewind(fh);
    const int reclen = 8 + (10 + cfg.nspec) * (int)sizeof(H);
    const long long recbytes = reclen + 8;
    int32_t hdr[3];
    if (size < 12 + recbytes || fread(hdr, 4, 3, fh) != 3 || hdr[0] != 4 || hdr[2] != 4 || (size - 12) % recbytes != 0)
      return fail(FPX_ERR_ARG, "readpartpositions: not a partposit dump of this build (record length = 8 + (10+nspec) reals)");
    const int itimein = hdr[1];
    const long long n = (size - 12) / recbytes - 1;
    {   // the last record must be the closing one (xlonin = -9999.9, readpartpositions.f90:120)
      std::vector<unsigned char> last((size_t)recbytes);
      H xl;
      if (fseek(fh, (long)(size - recbytes), SEEK_SET) != 0 || fread(last.data(), 1, (size_t)recbytes, fh) != (size_t)recbytes)
        return fail(FPX_ERR_ARG, "readpartpositions: short read");
      memcpy(&xl, last.data() + 8, sizeof(H));
      if (!(xl == (H)-9999.9)) return fail(FPX_ERR_ARG, "readpartpositions: the file does not end with the closing record");
      if (fseek(fh, 12, SEEK_SET) != 0) return fail(FPX_ERR_ARG, "readpartpositions: seek");
    }
    if (n > P.cap) return fail(FPX_ERR_ARG, "readpartpositions: more particles in the dump than the engine holds (maxpart)");
    // readpartpositions.f90:133-134: the previous run must end where this one starts
    if (std::abs(r->jul_header + (double)itimein / 86400. - r->bdate) > 1.e-5)
      return fail(FPX_ERR_ARG, "readpartpositions: ending time of the previous run does not agree with the start of this run");
    Scratch b_status, b_nclass, b_raw, pin(true);
    hipError_t e = b_status.reserve(2 * sizeof(int), stream);
    int *d_status = b_status.as<int>();
    if (e == hipSuccess) e = hipMemsetAsync(d_status, 0, 2 * sizeof(int), stream);
    int status[2] = {0, 0};
    if (n > 0 && e == hipSuccess) {
      const size_t bytes = (size_t)(n + 1) * recbytes;
      e = b_raw.reserve(bytes, stream);
      unsigned int *raw = b_raw.as<unsigned int>();
      const size_t chunk = (size_t)64 << 20;
      if (e == hipSuccess) e = pin.reserve(std::min(chunk, bytes), stream);
      for (size_t off = 0; e == hipSuccess && off < bytes; off += chunk) {
        const size_t nb = std::min(chunk, bytes - off);
        if (fread(pin.as(), 1, nb, fh) != nb) return fail(FPX_ERR_ARG, "readpartpositions: short read");
        e = hipMemcpyAsync((char *)raw + off, pin.as(), nb, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
      }
      if (e == hipSuccess && r->nclassunc > 1) {      // nclass(i)=min(int(ran1(idummy)*real(nclassunc))+1,nclassunc), :142-143
        std::vector<int> nc((size_t)n);
        Ran1 g;
        for (long long i = 0; i < n; i++) nc[i] = std::min((int)(g.template next<H>() * (H)r->nclassunc) + 1, r->nclassunc);
        e = b_nclass.reserve((size_t)n * sizeof(int), stream);
        if (e == hipSuccess) e = hipMemcpyAsync(b_nclass.as(), nc.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
      }
      if (e == hipSuccess) {
        k_readpart<R, H><<<(int)((n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(P, raw, n, cfg.nspec, (H)cfg.dx, (H)cfg.dy, (H)cfg.xlon0, (H)cfg.ylat0,
                                                                                r->jul_header, r->bdate, r->mintime, r->itrasplit, b_nclass.as<int>(), d_status);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipMemcpyAsync(status, d_status, sizeof status, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
    }
    if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("readpartpositions: ") + hipGetErrorString(e));
    if (status[0] != 0) return fail(FPX_ERR_ARG, status[0] == 1 ? "readpartpositions: record markers do not match this build's record length"
                                                  : "readpartpositions: the file does not hold exactly one dump (header, records, closing record)");
    numpart = n;
    slot_of_pid = nullptr;
    maybe_new = true; births_unknown = true;
    if (numpart_out) *numpart_out = n;
    if (numparticlecount) *numparticlecount = status[1];
    if (itimein_out) *itimein_out = itimein;
    return 0;
  }
  int readpartpositions(const char *path, const fpx_restart *r, int64_t *numpart_out, int32_t *numparticlecount, int32_t *itimein) override {
    if (!path || !r) return fail(FPX_ERR_ARG, "readpartpositions: null argument");
    if (r->nclassunc < 1) return fail(FPX_ERR_ARG, "readpartpositions: nclassunc >= 1");
    return cfg.host_real_bytes == 4 ? readpart_t<float>(path, r, numpart_out, numparticlecount, itimein)
                                    : readpart_t<double>(path, r, numpart_out, numparticlecount, itimein);
  }


  // ---- releaseparticles + splitting ------------------------------------------------
  struct ReleaseTables {
    bool set = false;
    int numpoint = 0, itsplit = 0, ind_rel = 0, nclassunc = 1;
    double bdate = 0;
    std::vector<int> start, end;
    std::vector<short> kindz;
    std::vector<double> xp1, xp2, yp1, yp2, zp1, zp2;          // values of the host's real kind, widened
    std::vector<double> point_hour, area_hour, point_dow, area_dow;   // [24|7][nspec]
  } rel;
  std::vector<double> rel_xmass_h;       // [nspec][numpoint], host copy of the table of fpx_set_release_points
  std::vector<int> rel_npart_h;
  Ran1 rel_ran1 = [] { Ran1 r; r.idum = -7; return r; }();   // releaseparticles.f90:59: integer :: idummy = -7 (SAVE'd): the stream persists between calls

  int release_init(const fpx_release *r) override {
    if (!r || r->struct_bytes != (int32_t)sizeof(fpx_release)) return fail(FPX_ERR_ARG, "release_init: null or fpx_release size mismatch (ABI)");
    if (r->numpoint < 1 || r->numpoint != V.numpoint) return fail(FPX_ERR_ARG, "release_init: numpoint must equal that of fpx_set_release_points (call it first)");
    if (!r->ireleasestart || !r->ireleaseend || !r->kindz || !r->xpoint1 || !r->xpoint2 || !r->ypoint1 || !r->ypoint2 || !r->zpoint1 || !r->zpoint2)
      return fail(FPX_ERR_ARG, "release_init: the release-point arrays are required");
    if (r->nclassunc < 1) return fail(FPX_ERR_ARG, "release_init: nclassunc >= 1");
    const int np = r->numpoint, ms = cfg.maxspec, ns = cfg.nspec;
    auto rd = [&](const void *p, size_t i) -> double { return cfg.host_real_bytes == 4 ? (double)((const float *)p)[i] : ((const double *)p)[i]; };
    rel.numpoint = np; rel.itsplit = r->itsplit; rel.ind_rel = r->ind_rel; rel.nclassunc = r->nclassunc; rel.bdate = r->bdate;
    rel.start.assign(r->ireleasestart, r->ireleasestart + np); rel.end.assign(r->ireleaseend, r->ireleaseend + np);
    rel.kindz.assign(r->kindz, r->kindz + np);
    std::vector<double> *dst[6] = {&rel.xp1, &rel.xp2, &rel.yp1, &rel.yp2, &rel.zp1, &rel.zp2};
    const void *src[6] = {r->xpoint1, r->xpoint2, r->ypoint1, r->ypoint2, r->zpoint1, r->zpoint2};
    for (int a = 0; a < 6; a++) { dst[a]->resize(np); for (int i = 0; i < np; i++) (*dst[a])[i] = rd(src[a], i); }
    // (maxspec, 24|7) column-major -> [hour|day][species]; absent tables mean "no variation" (factor 1)
    auto table = [&](const void *p, int n2, std::vector<double> &out) {
      out.assign((size_t)n2 * ns, 1.0);
      if (p) for (int k = 0; k < n2; k++) for (int sp = 0; sp < ns; sp++) out[(size_t)k * ns + sp] = rd(p, (size_t)k * ms + sp);
    };
    table(r->point_hour, 24, rel.point_hour); table(r->area_hour, 24, rel.area_hour);
    table(r->point_dow, 7, rel.point_dow); table(r->area_dow, 7, rel.area_dow);
    rel.set = true;
    if (cfg.wetbkdep) {   // the height range of every point, which WETBKDEP needs in the particle loop (timemanager.f90:590-591)
      int rc = set_release_heights(np, r->zpoint1, r->zpoint2);
      if (rc) return rc;
    }
    return 0;
  }

  // juldate.f90 / caldate.f90 (the date part) in the host's real kind H
  template <typename H>
  static double jul_of(int yyyymmdd, int hhmiss) {
    const int igreg = 15 + 31 * (10 + 12 * 1582);
    int yyyy = yyyymmdd / 10000, mm = (yyyymmdd - 10000 * yyyy) / 100, dd = yyyymmdd - 10000 * yyyy - 100 * mm;
    const int hh = hhmiss / 10000, mi = (hhmiss - 10000 * hh) / 100, ss = hhmiss - 10000 * hh - 100 * mi;
    int jy, jm;
    if (yyyy < 0) yyyy = yyyy + 1;
    if (mm > 2) { jy = yyyy; jm = mm + 1; } else { jy = yyyy - 1; jm = mm + 13; }
    int julday = (int)((H)365.25 * (H)jy) + (int)((H)30.6001 * (H)jm) + dd + 1720995;
    if (dd + 31 * (mm + 12 * yyyy) >= igreg) {
      const int ja = (int)((H)0.01 * (H)jy);
      julday = julday + 2 - ja + (int)((H)0.25 * (H)ja);
    }
    return (double)julday + (double)hh / 24. + (double)mi / 1440. + (double)ss / 86400.;
  }
  template <typename H>
  static int month_of(double juldate) {
    const int igreg = 2299161;
    int julday = (int)juldate, ja;
    if ((juldate - julday) * 86400. >= 86399.5) { juldate = juldate + juldate - julday - 86399.5 / 86400.; julday = (int)juldate; }
    if (julday >= igreg) {
      const int jalpha = (int)((((H)(julday - 1867216)) - (H)0.25) / (H)36524.25);
      ja = julday + 1 + jalpha - (int)((H)0.25 * (H)jalpha);
    } else ja = julday;
    const int jb = ja + 1524;
    const int jc = (int)((H)6680. + (((H)(jb - 2439870)) - (H)122.1) / (H)365.25);
    const int jd = 365 * jc + (int)((H)0.25 * (H)jc);
    const int je = (int)((H)(jb - jd) / (H)30.6001);
    int mm = je - 1;
    if (mm > 12) mm = mm - 12;
    return mm;
  }

  template <typename H>
  int release_t(int itime, int64_t *numpart_io, int32_t *npc_io, H *xmasssave, H *rho_rel, int64_t *nreleased) {
    const int np = rel.numpoint, ns = cfg.nspec;
    // ---- releaseparticles.f90:63-131 on the host, in the host's real kind -------------------------------
    const double julmonday = jul_of<H>(19000101, 0);
    double jul = rel.bdate + (double)itime / 86400.;
    { const int mm = month_of<H>(jul); if (mm >= 4 && mm <= 9) jul = jul + 1. / 24.; }
    std::vector<long long> first(np + 1, 0), gfirst(np, 0);
    long long gcount = rel_global_count;
    std::vector<H> mass((size_t)ns * np, (H)0), xp1(np), xaux(np), yp1(np), yaux(np), zp1(np), zaux(np);
    // the fractional carry of every release point advances in a copy: the host's xmasssave is written only when the call
    // succeeds ("nothing is released" on error -- a corrected retry must release what the reference would)
    std::vector<H> xsave(xmasssave, xmasssave + np);
    auto commit_carry = [&]() { for (int i = 0; i < np; i++) xmasssave[i] = xsave[i]; };
    bool any_p3 = false;
    for (int i = 0; i < np; i++) {
      long long numrel = 0;
      xp1[i] = (H)rel.xp1[i]; yp1[i] = (H)rel.yp1[i]; zp1[i] = (H)rel.zp1[i];
      xaux[i] = (H)rel.xp2[i] - (H)rel.xp1[i]; yaux[i] = (H)rel.yp2[i] - (H)rel.yp1[i]; zaux[i] = (H)rel.zp2[i] - (H)rel.zp1[i];
      if (itime >= rel.start[i] && itime <= rel.end[i]) {
        H xlonav = (H)cfg.xlon0 + ((H)rel.xp2[i] + (H)rel.xp1[i]) / (H)2. * (H)cfg.dx;
        if (xlonav < (H)-180.) xlonav = xlonav + (H)360.;
        if (xlonav > (H)180.) xlonav = xlonav - (H)360.;
        const double jullocal = jul + (double)xlonav / 360.;
        double juldiff = jullocal - julmonday;
        const int nweeks = (int)(juldiff / 7.);
        juldiff = juldiff - (double)nweeks * 7.;
        int ndayofweek = (int)juldiff + 1;
        int nhour = (int)std::lround((juldiff - (double)(ndayofweek - 1)) * 24.);
        if (nhour == 0) { nhour = 24; ndayofweek = ndayofweek - 1; if (ndayofweek == 0) ndayofweek = 7; }
        const bool point_source = std::fabs((double)((H)rel.xp2[i] - (H)rel.xp1[i])) < 1.e-4 && std::fabs((double)((H)rel.yp2[i] - (H)rel.yp1[i])) < 1.e-4;
        std::vector<H> tc(ns);
        H avg = (H)0;
        for (int k = 0; k < ns; k++) {
          tc[k] = point_source ? (H)rel.point_hour[(size_t)(nhour - 1) * ns + k] * (H)rel.point_dow[(size_t)(ndayofweek - 1) * ns + k]
                               : (H)rel.area_hour[(size_t)(nhour - 1) * ns + k] * (H)rel.area_dow[(size_t)(ndayofweek - 1) * ns + k];
          avg = avg + tc[k];
        }
        avg = avg / (H)ns;
        if (rel.start[i] != rel.end[i]) {
          H rfraction = (H)std::fabs((double)((H)rel_npart_h[i] * (H)cfg.lsynctime / (H)(rel.end[i] - rel.start[i])));
          if (itime == rel.start[i] || itime == rel.end[i]) rfraction = rfraction / (H)2.;
          rfraction = rfraction * avg;
          rfraction = rfraction + xsave[i];
          numrel = (long long)(int)rfraction;
          xsave[i] = rfraction - (H)(int)numrel;
        } else numrel = rel_npart_h[i];
        for (int k = 0; k < ns; k++) mass[(size_t)k * np + i] = (H)rel_xmass_h[(size_t)k * np + i] / (H)rel_npart_h[i] * tc[k] / avg;
        if (numrel > 0 && rel.kindz[i] == 3) any_p3 = true;
      }
      // several ranks (releaseparticles_mpi.f90:139-162): every rank takes numrel / nranks particles of the point, the first
      // mod(numrel, nranks) ranks one more; the particles of all ranks together are those of the single-rank run (the counter
      // RNG is keyed on the particle's number in the release count of the whole run)
      long long numrel_all = std::max<long long>(numrel, 0), roff = 0;
      numrel = numrel_all;
      if (comm_ranks > 1) {
        const long long base = numrel_all / comm_ranks, rem = numrel_all % comm_ranks;
        numrel = base + (comm_rank < rem ? 1 : 0);
        roff = (long long)comm_rank * base + std::min<long long>(comm_rank, rem);
      }
      gfirst[i] = gcount + roff;
      gcount += numrel_all;
      first[i + 1] = first[i] + numrel;
    }
    const long long ntotal = first[np];
    if (nreleased) *nreleased = ntotal;
    if (ntotal == 0) { rel_global_count = gcount; commit_carry(); return 0; }
    const bool dens = rel.ind_rel == 1 || rel.ind_rel == 3 || rel.ind_rel == 4;
    for (int l = 0; l < V.numbnests; l++) {
      if (!rel_nest_oro[l]) return fail(FPX_ERR_STATE, "releaseparticles: oron of every nest is needed (fpx_upload_diag_nest_fields slot 0)");
      if ((any_p3 || dens) && !nest_loaded[l][1]) return fail(FPX_ERR_STATE, "releaseparticles: rhon of time slot 2 is needed (fpx_upload_nest_fields)");
      if (any_p3 && !rel_nest_tt2[l]) return fail(FPX_ERR_STATE, "releaseparticles: ttn of time slot 2 is needed for kindz = 3 (fpx_upload_diag_nest_fields slot 2)");
    }
    if (!height_set || !diag_have[DG_ORO]) return fail(FPX_ERR_STATE, "releaseparticles: height and oro (fpx_upload_diag_fields slot 0) are needed");
    if ((any_p3 || dens) && !slot_loaded[1]) return fail(FPX_ERR_STATE, "releaseparticles: rho of time slot 2 is needed (kindz = 3 or ind_rel = 1, 3, 4)");
    if (any_p3 && !diag_have[DG_TT + 1]) return fail(FPX_ERR_STATE, "releaseparticles: tt of time slot 2 is needed for kindz = 3 (fpx_upload_diag_fields slot 2)");
    numpart = *numpart_io;
    // ---- the k-th particle takes the k-th vacant storage space in particle-number order (:133-137) --------
    const long long cap = P.cap;
    std::vector<Scratch> mine;       // this call's buffers
    auto mal = [&](auto **q, size_t n) -> hipError_t { mine.emplace_back(); const hipError_t e = mine.back().reserve(n * sizeof(**q), stream); *q = (decltype(*q + 0))mine.back().as(); return e; };
    unsigned int *flags = nullptr, *rank = nullptr, *target = nullptr, *d_max = nullptr;
    long long *d_first = nullptr, *d_gfirst = nullptr;
    H *d_pts = nullptr, *d_mass = nullptr, *d_uni = nullptr, *d_rho = nullptr;
    short *d_kindz = nullptr;
    void *tmp = nullptr;
    // the capacity-sized work arrays are kept between calls (grow-only): hipFree is a device-wide synchronisation, and at
    // the bench size they are 0.8 GB per call
    hipError_t e = rel_scratch((size_t)cap, &flags, &rank) ? hipErrorOutOfMemory : hipSuccess;
    if (e == hipSuccess) e = mal(&target, (size_t)ntotal);
    if (e == hipSuccess) e = mal(&d_max, 1);
    if (e == hipSuccess) e = mal(&d_first, (size_t)np + 1);
    if (e == hipSuccess) e = mal(&d_gfirst, (size_t)np);
    if (e == hipSuccess) e = mal(&d_pts, (size_t)6 * np);
    if (e == hipSuccess) e = mal(&d_mass, (size_t)ns * np);
    if (e == hipSuccess) e = mal(&d_kindz, (size_t)np);
    if (e == hipSuccess) e = mal(&d_rho, (size_t)np);
    // the vacancies are looked for in the storage spaces 1 .. numpart + ntotal only: the spaces behind numpart are vacant, so
    // the first ntotal vacancies lie in there (or, past the capacity, do not exist) -- not a scan of the whole capacity per call
    const long long scan_n = std::min<long long>(cap, numpart + ntotal);
    size_t tb = 0;
    if (e == hipSuccess) {
      (void)rocprim::exclusive_scan(nullptr, tb, flags, rank, 0u, (size_t)scan_n, rocprim::plus<unsigned int>(), stream);
      e = rel_scan_tmp(tb, &tmp) ? hipErrorOutOfMemory : hipSuccess;
    }
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("releaseparticles: ") + hipGetErrorString(e));
    const int nbc = (int)((scan_n + kBlock - 1) / kBlock);
    k_rel_flags<R><<<nbc, kBlock, 0, stream>>>(P, slot_map(), scan_n, itime, flags);
    e = rocprim::exclusive_scan(tmp, tb, flags, rank, 0u, (size_t)scan_n, rocprim::plus<unsigned int>(), stream);
    unsigned int last[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&last[0], rank + (scan_n - 1), 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[1], flags + (scan_n - 1), 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("releaseparticles: ") + hipGetErrorString(e));
    if ((long long)last[0] + last[1] < ntotal)
      return fail(FPX_ERR_NOMEM, "releaseparticles: total number of particles required exceeds the maximum allowed number (releaseparticles.f90:369-378)");
    k_rel_targets<<<nbc, kBlock, 0, stream>>>(flags, rank, scan_n, ntotal, target);
    // ---- the four uniforms of every particle: serial ran1 stream (x, y, class, z per particle) or counter RNG ----
    std::vector<H> uni;
    if (cfg.rng_mode == FPX_RNG_TABLE_SEQ) {
      uni.resize((size_t)4 * ntotal);
      for (long long k = 0; k < ntotal; k++)
        for (int d = 0; d < 4; d++) uni[(size_t)d * ntotal + k] = rel_ran1.template next<H>();
      e = mal(&d_uni, (size_t)4 * ntotal);
      if (e == hipSuccess) e = hipMemcpyAsync(d_uni, uni.data(), uni.size() * sizeof(H), hipMemcpyHostToDevice, stream);
    }
    std::vector<H> pts((size_t)6 * np);
    for (int i = 0; i < np; i++) { pts[i] = xp1[i]; pts[np + i] = xaux[i]; pts[2 * np + i] = yp1[i]; pts[3 * np + i] = yaux[i]; pts[4 * np + i] = zp1[i]; pts[5 * np + i] = zaux[i]; }
    std::vector<H> rho_h(np, (H)0);
    if (rho_rel) for (int i = 0; i < np; i++) rho_h[i] = rho_rel[i];
    if (e == hipSuccess) e = hipMemcpyAsync(d_first, first.data(), (np + 1) * sizeof(long long), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_gfirst, gfirst.data(), np * sizeof(long long), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pts, pts.data(), pts.size() * sizeof(H), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_mass, mass.data(), mass.size() * sizeof(H), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_kindz, rel.kindz.data(), np * sizeof(short), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rho, rho_h.data(), np * sizeof(H), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_max, 0, 4, stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(stream); return fail(FPX_ERR_DEVICE, std::string("releaseparticles: ") + hipGetErrorString(e)); }
    RelPoints<H> RP{d_first, d_gfirst, d_pts, d_pts + np, d_pts + 2 * np, d_pts + 3 * np, d_pts + 4 * np, d_pts + 5 * np, d_mass, d_kindz, np};
    DiagP<H> D;
    D.oro = (const H *)diag_oro; D.tropo[0] = (const H *)diag_tropo[0]; D.tropo[1] = (const H *)diag_tropo[1]; D.d3 = (const H *)diag_d3;
    D.nxmax = cfg.nxmax; D.nymax = cfg.nymax; D.dx = (H)cfg.dx; D.dy = (H)cfg.dy; D.xlon0 = (H)cfg.xlon0; D.ylat0 = (H)cfg.ylat0;
    RelNests<R, H> NS;
    NS.n = V.numbnests;
    NS.eps = (H)cfg.par_nxmax / (H)3.e5;
    for (int l = 0; l < V.numbnests; l++) {
      const NestDesc<R> &N = h_nest[l];
      NS.g[l].nx = N.nx; NS.g[l].ny = N.ny;
      NS.g[l].xl = (H)N.xl; NS.g[l].yl = (H)N.yl; NS.g[l].xr = (H)N.xr; NS.g[l].yr = (H)N.yr; NS.g[l].xres = (H)N.xres; NS.g[l].yres = (H)N.yres;
      NS.g[l].oro = (const H *)rel_nest_oro[l]; NS.g[l].tt2 = (const H *)rel_nest_tt2[l]; NS.g[l].r2 = N.r2;
    }
    k_release<R, H><<<(int)((ntotal + kBlock - 1) / kBlock), kBlock, 0, stream>>>(V, P, D, NS, RP, target, slot_map(), ntotal, itime, d_uni, (int)*npc_io,
                                                                                  cfg.mintime, rel.itsplit, rel.ind_rel, rel.nclassunc, cfg.mquasilag,
                                                                                  dens ? d_rho : (H *)nullptr, d_max);
    e = hipGetLastError();
    unsigned int maxpid = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&maxpid, d_max, 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && rho_rel && dens) e = hipMemcpyAsync(rho_h.data(), d_rho, np * sizeof(H), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream); else (void)hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("releaseparticles: ") + hipGetErrorString(e));
    if (rho_rel && dens) for (int i = 0; i < np; i++) rho_rel[i] = rho_h[i];
    numpart = std::max<long long>(numpart, (long long)maxpid + 1);          // :362
    *numpart_io = numpart;
    *npc_io = (int32_t)(*npc_io + ntotal);
    rel_global_count = gcount;
    commit_carry();
    maybe_new = true;
    return 0;
  }
  // grow-only scratch of fpx_releaseparticles / fpx_split_particles: two unsigned arrays of n elements and the scan's temporary
  Scratch rel_flags_buf, rel_rank_buf, rel_tmp_buf;
  int rel_scratch(size_t n, unsigned int **flags, unsigned int **rank) {
    if (rel_flags_buf.reserve(n * 4, stream) != hipSuccess || rel_rank_buf.reserve(n * 4, stream) != hipSuccess) return 1;
    *flags = rel_flags_buf.as<unsigned int>(); *rank = rel_rank_buf.as<unsigned int>();
    return 0;
  }
  int rel_scan_tmp(size_t bytes, void **tmp) {
    if (rel_tmp_buf.reserve(bytes, stream) != hipSuccess) return 1;
    *tmp = rel_tmp_buf.as();
    return 0;
  }
  int releaseparticles(int itime, int64_t *numpart_io, int32_t *npc_io, void *xmasssave, void *rho_rel, int64_t *nreleased) override {
    if (!rel.set) return fail(FPX_ERR_STATE, "releaseparticles: fpx_release_init first");
    if (!numpart_io || !npc_io || !xmasssave) return fail(FPX_ERR_ARG, "releaseparticles: numpart, numparticlecount and xmasssave are required");
    if (*numpart_io < 0 || *numpart_io > P.cap) return fail(FPX_ERR_ARG, "releaseparticles: numpart outside capacity");
    return cfg.host_real_bytes == 4 ? release_t<float>(itime, numpart_io, npc_io, (float *)xmasssave, (float *)rho_rel, nreleased)
                                    : release_t<double>(itime, numpart_io, npc_io, (double *)xmasssave, (double *)rho_rel, nreleased);
  }
  int split_particles(int itime, int64_t *numpart_io) override {
    if (!rel.set) return fail(FPX_ERR_STATE, "split_particles: fpx_release_init first (itsplit)");
    if (!numpart_io || *numpart_io < 0 || *numpart_io > P.cap) return fail(FPX_ERR_ARG, "split_particles: numpart outside capacity");
    numpart = *numpart_io;
    if (!(cfg.ldirect * itime >= cfg.ldirect * rel.itsplit) || numpart == 0 || numpart == P.cap) return 0;   // timemanager.f90:473
    const long long n = numpart, room = P.cap - n;
    unsigned int *flags = nullptr, *rank = nullptr;
    void *tmp = nullptr;
    hipError_t e = rel_scratch((size_t)n, &flags, &rank) ? hipErrorOutOfMemory : hipSuccess;
    size_t tb = 0;
    if (e == hipSuccess) {
      (void)rocprim::exclusive_scan(nullptr, tb, flags, rank, 0u, (size_t)n, rocprim::plus<unsigned int>(), stream);
      e = rel_scan_tmp(tb, &tmp) ? hipErrorOutOfMemory : hipSuccess;
    }
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("split_particles: ") + hipGetErrorString(e));
    const int nb = (int)((n + kBlock - 1) / kBlock);
    k_split_flags<R><<<nb, kBlock, 0, stream>>>(P, slot_map(), n, itime, cfg.ldirect, flags);
    e = rocprim::exclusive_scan(tmp, tb, flags, rank, 0u, (size_t)n, rocprim::plus<unsigned int>(), stream);
    unsigned int last[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&last[0], rank + (n - 1), 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&last[1], flags + (n - 1), 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) {
      k_split<R><<<nb, kBlock, 0, stream>>>(P, slot_map(), flags, rank, n, room, cfg.nspec);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream); else (void)hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("split_particles: ") + hipGetErrorString(e));
    numpart = n + std::min<long long>((long long)last[0] + last[1], room);
    *numpart_io = numpart;
    return 0;
  }

  // ---- particle redistribution between ranks, mpi_mod.f90:661-856 ------------------------------
  // The host keeps the transport (its MPI_Send / MPI_Recv, one message instead of the reference's 9 + nspec); the engine
  // packs and places.  buf may be host or device memory (hipMemcpyDefault).
  Scratch redist_dev;
  size_t redist_bytes(int64_t num_trans) override { return num_trans > 0 ? RedistBuf<R>::bytes(num_trans, cfg.nspec) : 0; }
  int redist_pack(int itime, int64_t num_trans, void *buf, size_t buf_bytes, int64_t *numpart_io) override {
    (void)itime;
    if (!numpart_io || *numpart_io < 0 || *numpart_io > P.cap) return fail(FPX_ERR_ARG, "redist_pack: numpart outside capacity");
    if (num_trans < 0 || num_trans > *numpart_io) return fail(FPX_ERR_ARG, "redist_pack: num_trans must be between 0 and numpart");
    if (num_trans == 0) return 0;
    const size_t need = redist_bytes(num_trans);
    if (!buf || buf_bytes < need) return fail(FPX_ERR_ARG, "redist_pack: buffer smaller than fpx_redist_bytes(num_trans)");
    if (redist_dev.reserve(need, stream) != hipSuccess) return fail(FPX_ERR_NOMEM, "redist_pack: staging buffer");
    // first back into particle-number order over the extent the engine itself holds (the extent of the last locality sort:
    // its slots are a permutation of exactly those numbers), then the host's count -- as set_numpart does; the other order
    // would sort a range whose numbers are not a permutation and lose live particles
    { const int rc = restore_particle_order(); if (rc) return rc; }   // numpart shrinks below
    numpart = *numpart_io;
    const RedistBuf<R> B = RedistBuf<R>::at(redist_dev.as(), num_trans, cfg.nspec);
    k_redist_pack<R><<<(int)((num_trans + kBlock - 1) / kBlock), kBlock, 0, stream>>>(P, slot_map(), numpart - num_trans, B, cfg.nspec);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(buf, redist_dev.as(), need, hipMemcpyDefault, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream); else (void)hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("redist_pack: ") + hipGetErrorString(e));
    numpart -= num_trans;                                 // :746
    *numpart_io = numpart;
    return 0;
  }
  int redist_unpack(int itime, int64_t num_trans, const void *buf, size_t buf_bytes, int64_t *numpart_io) override {
    if (!numpart_io || *numpart_io < 0 || *numpart_io > P.cap) return fail(FPX_ERR_ARG, "redist_unpack: numpart outside capacity");
    if (num_trans < 0) return fail(FPX_ERR_ARG, "redist_unpack: num_trans < 0");
    if (num_trans == 0) return 0;
    const long long maxnumpart = *numpart_io + num_trans;   // :811
    if (maxnumpart > P.cap) return fail(FPX_ERR_NOMEM, "redist_unpack: numpart + num_trans exceeds the particle capacity (the reference would write past maxpart)");
    const size_t need = redist_bytes(num_trans);
    if (!buf || buf_bytes < need) return fail(FPX_ERR_ARG, "redist_unpack: buffer smaller than fpx_redist_bytes(num_trans)");
    // work arrays: vacancy flags + ranks over 1..maxnumpart, validity flags + ranks and the targets over the message
    unsigned int *flags = nullptr, *rank = nullptr;
    void *tmp = nullptr;
    const size_t nwork = (size_t)maxnumpart + 3 * (size_t)num_trans + 1;
    if (redist_dev.reserve(need, stream) != hipSuccess) return fail(FPX_ERR_NOMEM, "redist_unpack: staging buffer");
    if (rel_scratch(nwork, &flags, &rank)) return fail(FPX_ERR_NOMEM, "redist_unpack: work arrays");
    unsigned int *valid = flags + maxnumpart, *vrank = rank + maxnumpart;
    unsigned int *target = flags + maxnumpart + num_trans, *d_max = rank + maxnumpart + num_trans;
    size_t tb1 = 0, tb2 = 0;
    (void)rocprim::exclusive_scan(nullptr, tb1, flags, rank, 0u, (size_t)maxnumpart, rocprim::plus<unsigned int>(), stream);
    (void)rocprim::exclusive_scan(nullptr, tb2, valid, vrank, 0u, (size_t)num_trans, rocprim::plus<unsigned int>(), stream);
    if (rel_scan_tmp(std::max(tb1, tb2), &tmp)) return fail(FPX_ERR_NOMEM, "redist_unpack: scan storage");
    numpart = *numpart_io;
    hipError_t e = hipMemcpyAsync(redist_dev.as(), buf, need, hipMemcpyDefault, stream);
    const RedistBuf<R> B = RedistBuf<R>::at(redist_dev.as(), num_trans, cfg.nspec);
    const int nbm = (int)((maxnumpart + kBlock - 1) / kBlock), nbt = (int)((num_trans + kBlock - 1) / kBlock);
    if (e == hipSuccess) {
      k_rel_flags<R><<<nbm, kBlock, 0, stream>>>(P, slot_map(), maxnumpart, itime, flags);          // vacant: itra1 /= itime (:818)
      k_redist_valid<<<nbt, kBlock, 0, stream>>>(B.itra1, num_trans, itime, valid);                  // :816
      e = rocprim::exclusive_scan(tmp, tb1, flags, rank, 0u, (size_t)maxnumpart, rocprim::plus<unsigned int>(), stream);
    }
    if (e == hipSuccess) e = rocprim::exclusive_scan(tmp, tb2, valid, vrank, 0u, (size_t)num_trans, rocprim::plus<unsigned int>(), stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_max, 0, 4, stream);
    if (e == hipSuccess) {
      // the spaces numpart+1 .. maxnumpart are vacant, so there are at least num_trans targets
      k_rel_targets<<<nbm, kBlock, 0, stream>>>(flags, rank, maxnumpart, num_trans, target);
      k_redist_unpack<R><<<nbt, kBlock, 0, stream>>>(P, slot_map(), B, cfg.nspec, valid, vrank, target, d_max);
      e = hipGetLastError();
    }
    unsigned int maxpid = 0, nvalid[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(&maxpid, d_max, 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&nvalid[0], vrank + (num_trans - 1), 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&nvalid[1], valid + (num_trans - 1), 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream); else (void)hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("redist_unpack: ") + hipGetErrorString(e));
    if (nvalid[0] + nvalid[1] > 0) numpart = std::max<long long>(numpart, (long long)maxpid + 1);   // numpart=max(numpart,ipart), :836
    *numpart_io = numpart;
    maybe_new = true; births_unknown = true;
    return 0;
  }

  // ---- concoutput: the grid_conc files ------------------------------------
  int concoutput(int itime, const fpx_concout *c, const char *prefix, int clear) override {
    if (!Gp.on) return fail(FPX_ERR_STATE, "concoutput: fpx_outgrid_init first");
    if (!c || !c->area || !c->volume || !prefix) return fail(FPX_ERR_ARG, "concoutput: area, volume and the file name prefix are required");
    if (cfg.host_real_bytes != 4) return fail(FPX_ERR_ARG, "concoutput: only for hosts with a 4-byte default real (the reference's concoutput.f90 does not compile with 8)");
    if (cfg.ldirect != 1) return fail(FPX_ERR_ARG, "concoutput: forward runs only (ldirect = 1)");
    if (!(c->outnum > 0)) return fail(FPX_ERR_ARG, "concoutput: outnum > 0");
    const int iout = c->iout ? c->iout : 1;
    if (iout < 1 || iout > 3) return fail(FPX_ERR_ARG, "concoutput: iout 1 (concentration), 2 (mixing ratio) or 3 (both)");
    const bool want_conc = iout == 1 || iout == 3, want_ppt = iout == 2 || iout == 3;
    if (want_ppt && (!c->prefix_pptv || !c->outheight)) return fail(FPX_ERR_ARG, "concoutput: prefix_pptv and outheight are required for iout 2, 3");
    if (want_ppt && (!slot_loaded[0] || !slot_loaded[1] || !window_set || !height_set)) return fail(FPX_ERR_STATE, "concoutput: mixing ratios need the met fields and the wind-time window");
    if (c->nest && !Gp.nested) return fail(FPX_ERR_STATE, "concoutput: nested output grid requested without fpx_outgrid_nest_init");
    // nest = 1: the nested output grid (concoutput_nest.f90: the same algorithm on griduncn, wetgriduncn, drygriduncn, arean, volumen)
    const long long n2 = c->nest ? (long long)Gp.numxgridn * Gp.numygridn : (long long)Gp.numxgrid * Gp.numygrid, n3 = n2 * Gp.numzgrid;
    R *g3 = c->nest ? Gp.griduncn : Gp.gridunc;            // the rank's own partial sums (zeroed afterwards with clear = 1)
    // What is written: with reduced = 1 the sums over all ranks that fpx_get_grids / fpx_get_wetgrid / fpx_get_grids_nest
    // (allreduce = 1) left in the receive buffers -- concoutput_mpi.f90:279,298 writes from gridunc0 / drygridunc0 /
    // wetgridunc0 -- of the grids this call writes
    const void *s3v = nullptr, *sdry = nullptr, *swet = nullptr;
    {
      const char *getters = "fpx_get_grids / fpx_get_wetgrid / fpx_get_grids_nest";
      int rc;
      if ((rc = source(c->nest ? sum_gridn : sum_grid, g3, c->reduced, "concoutput", getters, &s3v))) return rc;
      if (c->drydep && (rc = source(c->nest ? sum_dryn : sum_dry, c->nest ? Gp.drygriduncn : Gp.drygridunc, c->reduced, "concoutput", getters, &sdry))) return rc;
      if (c->wetdep && (rc = source(c->nest ? sum_wetn : sum_wet, c->nest ? Gp.wetgriduncn : Gp.wetgridunc, c->reduced, "concoutput", getters, &swet))) return rc;
    }
    const R *s3 = (const R *)s3v;
    const float *gdry = (const float *)sdry, *gwet = (const float *)swet;
    float *d_area = nullptr, *d_vol = nullptr, *val = nullptr, *wr = nullptr;
    unsigned int *nz = nullptr, *rs = nullptr, *rpos = nullptr, *runid = nullptr;
    int *wi = nullptr;
    Scratch tmp;
    std::vector<Scratch> mine;       // this call's buffers
    auto mal = [&](auto **q, size_t bytes) -> hipError_t { mine.emplace_back(); const hipError_t e = mine.back().reserve(bytes, stream); *q = (decltype(*q + 0))mine.back().as(); return e; };
    float *d_dens = nullptr, *d_outh = nullptr;
    hipError_t e = mal(&d_area, n2 * 4);
    if (e == hipSuccess) e = mal(&d_vol, n3 * 4);
    if (e == hipSuccess && want_ppt) e = mal(&d_dens, n3 * 4);
    if (e == hipSuccess && want_ppt) e = mal(&d_outh, (size_t)Gp.numzgrid * 4);
    if (e == hipSuccess) e = mal(&val, n3 * 4);
    if (e == hipSuccess) e = mal(&wr, n3 * 4);
    if (e == hipSuccess) e = mal(&nz, n3 * 4);
    if (e == hipSuccess) e = mal(&rs, n3 * 4);
    if (e == hipSuccess) e = mal(&rpos, n3 * 4);
    if (e == hipSuccess) e = mal(&runid, n3 * 4);
    if (e == hipSuccess) e = mal(&wi, n3 * 4);
    size_t tb = 0;
    if (e == hipSuccess) {
      (void)rocprim::exclusive_scan(nullptr, tb, nz, rpos, 0u, (size_t)n3, rocprim::plus<unsigned int>(), stream);
      size_t tb2 = 0;
      (void)rocprim::inclusive_scan(nullptr, tb2, rs, runid, (size_t)n3, rocprim::plus<unsigned int>(), stream);
      tb = std::max(tb, tb2);
      e = tmp.reserve(tb, stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(d_area, c->area, n2 * 4, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_vol, c->volume, n3 * 4, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && want_ppt) {
      e = hipMemcpyAsync(d_outh, c->outheight, (size_t)Gp.numzgrid * 4, hipMemcpyHostToDevice, stream);
      if (e == hipSuccess) {
        k_co_density<R><<<(int)((n3 + kBlock - 1) / kBlock), kBlock, 0, stream>>>(V, c->nest ? Gp.numxgridn : Gp.numxgrid, c->nest ? Gp.numygridn : Gp.numygrid, Gp.numzgrid, d_outh,
                                                                                (float)(c->nest ? Gp.dxoutn : Gp.dxout), (float)(c->nest ? Gp.dyoutn : Gp.dyout),
                                                                                (float)c->outlon0, (float)c->outlat0, (float)cfg.dx, (float)cfg.dy, (float)cfg.xlon0, (float)cfg.ylat0, d_dens);
        e = hipGetLastError();
      }
    }
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("concoutput: ") + hipGetErrorString(e));
    std::vector<int> h_wi((size_t)n3);
    std::vector<float> h_wr((size_t)n3);
    // one compressed dump: device work, then the four records (count, indices, count, values)
    auto dump = [&](auto *grid, size_t class_stride, long long n, const float *scale, int conc, int idx0, RecFile &file, float wm = 1.f) -> int {
      const int nb = (int)((n + kBlock - 1) / kBlock);
      int32_t ci = 0, cr = 0;
      if (grid) {
        k_co_values<<<nb, kBlock, 0, stream>>>(grid, class_stride, Gp.nclassunc, n, val, nz, rs);
        size_t t1 = tb;
        hipError_t e2 = rocprim::exclusive_scan(tmp.as(), t1, nz, rpos, 0u, (size_t)n, rocprim::plus<unsigned int>(), stream);
        t1 = tb;
        if (e2 == hipSuccess) e2 = rocprim::inclusive_scan(tmp.as(), t1, rs, runid, (size_t)n, rocprim::plus<unsigned int>(), stream);
        k_co_write<<<nb, kBlock, 0, stream>>>(val, nz, rs, rpos, runid, n, scale, conc, (float)c->outnum, 1.f, idx0, wi, wr, d_dens, wm);
        unsigned int last[3] = {0, 0, 0};
        if (e2 == hipSuccess) e2 = hipMemcpyAsync(&last[0], rpos + (n - 1), 4, hipMemcpyDeviceToHost, stream);
        if (e2 == hipSuccess) e2 = hipMemcpyAsync(&last[1], nz + (n - 1), 4, hipMemcpyDeviceToHost, stream);
        if (e2 == hipSuccess) e2 = hipMemcpyAsync(&last[2], runid + (n - 1), 4, hipMemcpyDeviceToHost, stream);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(stream);
        cr = (int32_t)(last[0] + last[1]); ci = (int32_t)last[2];
        if (e2 == hipSuccess && ci > 0) e2 = hipMemcpyAsync(h_wi.data(), wi, (size_t)ci * 4, hipMemcpyDeviceToHost, stream);
        if (e2 == hipSuccess && cr > 0) e2 = hipMemcpyAsync(h_wr.data(), wr, (size_t)cr * 4, hipMemcpyDeviceToHost, stream);
        if (e2 == hipSuccess) e2 = hipStreamSynchronize(stream);
        if (e2 != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("concoutput: ") + hipGetErrorString(e2));
      }
      file.scalar(ci);
      file.record(h_wi.data(), (size_t)ci * 4);
      file.scalar(cr);
      file.record(h_wr.data(), (size_t)cr * 4);
      return file.ok() ? 0 : fail(FPX_ERR_ARG, "concoutput: write error");
    };
    int rc = 0;
    for (int ks = 0; ks < cfg.nspec && !rc; ks++)
      for (int pass = 0; pass < 2 && !rc; pass++) {          // 0: grid_conc (:349-447), 1: grid_pptv (:482-590)
        if ((pass == 0 && !want_conc) || (pass == 1 && !want_ppt)) continue;
        char name[1024];
        snprintf(name, sizeof name, "%s%03d", pass == 0 ? prefix : c->prefix_pptv, ks + 1);
        RecFile file(name);
        if (!file.is_open()) { rc = fail(FPX_ERR_ARG, std::string("concoutput: cannot open ") + name); break; }
        file.scalar((int32_t)itime);
        if (!file.ok()) rc = fail(FPX_ERR_ARG, "concoutput: write error");
        for (int kp = 0; kp < Gp.maxpointspec_act && !rc; kp++)
          for (int nage = 0; nage < Gp.nageclass && !rc; nage++) {
            // element (0,0,[1,]ks,kp,class 0,nage) of the 6-D / 7-D arrays; consecutive classes are class_stride apart
            const size_t o2 = ((((size_t)nage * Gp.nclassunc) * Gp.maxpointspec_act + kp) * Gp.maxspec + ks) * (size_t)n2;
            const size_t cs2 = (size_t)Gp.maxpointspec_act * Gp.maxspec * (size_t)n2;
            const size_t o3 = o2 * Gp.numzgrid, cs3 = cs2 * Gp.numzgrid;
            rc = dump(gwet ? gwet + o2 : (const float *)nullptr, cs2, n2, d_area, 0, 0, file);
            if (!rc) rc = dump(gdry ? gdry + o2 : (const float *)nullptr, cs2, n2, d_area, 0, 0, file);
            if (!rc) rc = dump(s3 + o3, cs3, n3, d_vol, pass == 0 ? 1 : 2, (int)n2 /* kz is 1-based in the index, :425 */, file,
                               pass == 1 ? (float)c->weightmolar[ks] : 1.f);
          }
        if (!file.close() && !rc) rc = fail(FPX_ERR_ARG, "concoutput: write error");
      }
    if (rc) return rc;
    if (clear) {   // gridunc(:,:,:,:,:,:,:)=0., concoutput.f90:714 / griduncn, concoutput_nest.f90 (the deposition grids keep accumulating)
      HIPCHK(hipMemsetAsync(g3, 0, (c->nest ? sum_gridn : sum_grid).bytes(), stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    return 0;
  }

  int set_windtime(const int32_t mt[2], const int32_t mi[2]) override {
    if (!mt || !mi) return fail(FPX_ERR_ARG, "set_windtime: null");
    if ((mi[0] != 1 && mi[0] != 2) || (mi[1] != 1 && mi[1] != 2) || mi[0] == mi[1]) return fail(FPX_ERR_ARG, "set_windtime: memind must be a permutation of (1,2)");
    if (mt[0] == mt[1]) return fail(FPX_ERR_ARG, "set_windtime: memtime(1) == memtime(2)");
    V.memtime0 = mt[0]; V.memtime1 = mt[1]; V.m1 = mi[0] - 1; V.m2 = mi[1] - 1;
    V.lwindinterv = std::abs(mt[1] - mt[0]);
    {   // mesoscale autocorrelation, advance.f90:728-729: the same two numbers for every particle of a step
      const R r = sizeof(R) == 4 ? (R)expf(-2.0f * (float)std::abs(cfg.lsynctime) / (float)V.lwindinterv)
                                 : (R)exp(-2.0 * (double)std::abs(cfg.lsynctime) / (double)V.lwindinterv);
      V.meso_r = r;
      V.meso_rs = sizeof(R) == 4 ? (R)sqrtf(1.0f - (float)r * (float)r) : (R)sqrt(1.0 - (double)r * (double)r);
    }
    window_set = true;
    return 0;
  }

  // ---- RNG -----------------------------------------------------------------
  int rng_fill_table() override {
    const int n = V.maxrand;
    std::vector<R> t(n);
    if (cfg.host_real_bytes == 4) { rng4 = HostRng<float>(); rng4.fill_table(tab4, n); for (int i = 0; i < n; i++) t[i] = (R)tab4[i]; }
    else { rng8 = HostRng<double>(); rng8.fill_table(tab8, n); for (int i = 0; i < n; i++) t[i] = (R)tab8[i]; }
    HIPCHK(hipMemcpyAsync((void *)V.rannumb, t.data(), n * sizeof(R), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    table_set = true;
    return 0;
  }
  int rng_set_table(const void *tab, int n) override {
    if (!tab || n != V.maxrand) return fail(FPX_ERR_ARG, "rng_set_table: need maxrand = 1000000 values");
    std::vector<R> t(n);
    tab4.clear(); tab8.clear();
    if (cfg.host_real_bytes == 4) { tab4.assign((const float *)tab, (const float *)tab + n); for (int i = 0; i < n; i++) t[i] = (R)tab4[i]; }
    else { tab8.assign((const double *)tab, (const double *)tab + n); for (int i = 0; i < n; i++) t[i] = (R)tab8[i]; }
    HIPCHK(hipMemcpyAsync((void *)V.rannumb, t.data(), n * sizeof(R), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    table_set = true;
    return 0;
  }
  int rng_get_table(void *out, int n) override {
    if (!out || n != V.maxrand || !table_set) return fail(FPX_ERR_ARG, "rng_get_table: no table / bad size");
    if (cfg.host_real_bytes == 4) memcpy(out, tab4.data(), n * sizeof(float));
    else memcpy(out, tab8.data(), n * sizeof(double));
    return 0;
  }

  // ---- particles -----------------------------------------------------------
  template <typename H, typename D>
  int put(const H *host, D *dev, long long first, long long count) {
    HIPCHK(staging.reserve((size_t)count * sizeof(H), stream));
    HIPCHK(hipMemcpyAsync(staging.as(), host, (size_t)count * sizeof(H), hipMemcpyHostToDevice, stream));
    k_scatter_in<H, D><<<(int)((count + kBlock - 1) / kBlock), kBlock, 0, stream>>>(staging.as<const H>(), dev, slot_map(), first, count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  template <typename H, typename D>
  int get(H *host, const D *dev, long long first, long long count) {
    HIPCHK(staging.reserve((size_t)count * sizeof(H), stream));
    k_gather_out<D, H><<<(int)((count + kBlock - 1) / kBlock), kBlock, 0, stream>>>(dev, staging.as<H>(), slot_map(), first, count);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host, staging.as(), (size_t)count * sizeof(H), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  template <typename D>
  int fill(D *dev, D val, long long first, long long count) {
    k_fill<D><<<(int)((count + kBlock - 1) / kBlock), kBlock, 0, stream>>>(dev, val, first, count, slot_map());
    HIPCHK(hipGetLastError());
    return 0;
  }
  int put_real(const void *host, R *dev, long long first, long long count) {
    if (!host) return fill<R>(dev, (R)0, first, count);
    return cfg.host_real_bytes == 4 ? put<float, R>((const float *)host, dev, first, count) : put<double, R>((const double *)host, dev, first, count);
  }
  int get_real(void *host, const R *dev, long long first, long long count) {
    if (!host) return 0;
    return cfg.host_real_bytes == 4 ? get<float, R>((float *)host, dev, first, count) : get<double, R>((double *)host, dev, first, count);
  }

  int upload_particles(long long first, long long count, const fpx_particles *p) override {
    if (!p || first < 0 || count < 0 || first + count > P.cap) return fail(FPX_ERR_ARG, "upload_particles: range outside capacity");
    if (count == 0) return 0;
    if (!p->xtra1 || !p->ytra1 || !p->ztra1 || !p->itra1) return fail(FPX_ERR_ARG, "upload_particles: xtra1, ytra1, ztra1, itra1 are required");
    int rc;
    if ((rc = put<double, double>(p->xtra1, P.xt, first, count))) return rc;
    if ((rc = put<double, double>(p->ytra1, P.yt, first, count))) return rc;
    if ((rc = put_real(p->ztra1, P.zt, first, count))) return rc;
    if ((rc = put_real(p->uap, P.up, first, count))) return rc;
    if ((rc = put_real(p->ucp, P.vp, first, count))) return rc;
    if ((rc = put_real(p->uzp, P.wp, first, count))) return rc;
    if ((rc = put_real(p->us, P.us, first, count))) return rc;
    if ((rc = put_real(p->vs, P.vs, first, count))) return rc;
    if ((rc = put_real(p->ws, P.ws, first, count))) return rc;
    if ((rc = put<int, int>(p->itra1, P.itra1, first, count))) return rc;
    if (p->itramem) { if ((rc = put<int, int>(p->itramem, P.itramem, first, count))) return rc; } else if ((rc = fill<int>(P.itramem, 0, first, count))) return rc;
    if (p->idt) { if ((rc = put<int, int>(p->idt, P.idt, first, count))) return rc; } else if ((rc = fill<int>(P.idt, 0, first, count))) return rc;
    if (p->npoint) { if ((rc = put<int, int>(p->npoint, P.npoint, first, count))) return rc; } else if ((rc = fill<int>(P.npoint, 1, first, count))) return rc;
    if (p->nclass) { if ((rc = put<int, int>(p->nclass, P.nclass, first, count))) return rc; } else if ((rc = fill<int>(P.nclass, 1, first, count))) return rc;
    if (p->itrasplit) { if ((rc = put<int, int>(p->itrasplit, P.itrasplit, first, count))) return rc; }
    else if ((rc = fill<int>(P.itrasplit, (cfg.ldirect < 0 ? -1 : 1) * 999999999, first, count))) return rc;   // "never", in the run's direction
    if (p->cbt) { if ((rc = put<short, short>(p->cbt, P.cbt, first, count))) return rc; } else if ((rc = fill<short>(P.cbt, (short)1, first, count))) return rc;
    for (int ks = 0; ks < cfg.nspec; ks++) {
      R *dst = P.xmass1 + (size_t)ks * P.cap;
      if (p->xmass1) {
        const char *src = (const char *)p->xmass1 + (size_t)ks * p->xmass1_ld * cfg.host_real_bytes;
        if ((rc = put_real(src, dst, first, count))) return rc;
      } else if ((rc = fill<R>(dst, (R)1, first, count))) return rc;
    }
    if (P.xscav)
      for (int ks = 0; ks < cfg.nspec; ks++) {
        R *dst = P.xscav + (size_t)ks * P.cap;
        if (p->xscav_frac1) {
          const char *src = (const char *)p->xscav_frac1 + (size_t)ks * p->xmass1_ld * cfg.host_real_bytes;
          if ((rc = put_real(src, dst, first, count))) return rc;
        } else if ((rc = fill<R>(dst, (R)-1, first, count))) return rc;     // as releaseparticles.f90:167-171 leaves a new particle
      }
    HIPCHK(hipStreamSynchronize(stream));
    numpart = std::max(numpart, first + count);
    maybe_new = true; births_unknown = true;
    return 0;
  }

  int download_particles(long long first, long long count, const fpx_particles *p) override {
    if (!p || first < 0 || count < 0 || first + count > P.cap) return fail(FPX_ERR_ARG, "download_particles: range outside capacity");
    if (count == 0) return 0;
    int rc;
    if (p->xtra1 && (rc = get<double, double>(p->xtra1, P.xt, first, count))) return rc;
    if (p->ytra1 && (rc = get<double, double>(p->ytra1, P.yt, first, count))) return rc;
    if ((rc = get_real(p->ztra1, P.zt, first, count))) return rc;
    if ((rc = get_real(p->uap, P.up, first, count))) return rc;
    if ((rc = get_real(p->ucp, P.vp, first, count))) return rc;
    if ((rc = get_real(p->uzp, P.wp, first, count))) return rc;
    if ((rc = get_real(p->us, P.us, first, count))) return rc;
    if ((rc = get_real(p->vs, P.vs, first, count))) return rc;
    if ((rc = get_real(p->ws, P.ws, first, count))) return rc;
    if (p->itra1 && (rc = get<int, int>(p->itra1, P.itra1, first, count))) return rc;
    if (p->itramem && (rc = get<int, int>(p->itramem, P.itramem, first, count))) return rc;
    if (p->idt && (rc = get<int, int>(p->idt, P.idt, first, count))) return rc;
    if (p->npoint && (rc = get<int, int>(p->npoint, P.npoint, first, count))) return rc;
    if (p->nclass && (rc = get<int, int>(p->nclass, P.nclass, first, count))) return rc;
    if (p->itrasplit && (rc = get<int, int>(p->itrasplit, P.itrasplit, first, count))) return rc;
    if (p->cbt && (rc = get<short, short>(p->cbt, P.cbt, first, count))) return rc;
    if (p->xmass1)
      for (int ks = 0; ks < cfg.nspec; ks++) {
        char *dst = (char *)p->xmass1 + (size_t)ks * p->xmass1_ld * cfg.host_real_bytes;
        if ((rc = get_real(dst, P.xmass1 + (size_t)ks * P.cap, first, count))) return rc;
      }
    if (p->xscav_frac1 && P.xscav)
      for (int ks = 0; ks < cfg.nspec; ks++) {
        char *dst = (char *)p->xscav_frac1 + (size_t)ks * p->xmass1_ld * cfg.host_real_bytes;
        if ((rc = get_real(dst, P.xscav + (size_t)ks * P.cap, first, count))) return rc;
      }
    return 0;
  }

  // ---- convective mixing -------------------------------------------------------------------------
  bool conv_on = false;
  int conv_nuvz = 0, conv_nconvlev = 0;
  // per wind-field grid (0: the mother grid, l: nested grid l; a nest's arrays are allocated with its first upload)
  void *conv_fld[1 + kMaxNests][5][2] = {};  // ps, tt2, td2, tth, qvh of the two slots, compact [ny][nx], host real kind
  bool conv_slot[1 + kMaxNests][2] = {};
  void *conv_cb[1 + kMaxNests] = {};         // cbaseflux [ny][nx], cbasefluxn(:,:,l)
  void *conv_tab[4] = {};                    // akz, bkz, akm, bkm
  size_t conv_cb_bytes(int g) const { const HostGrid G = host_grid(g); return (size_t)G.nx * G.ny * cfg.host_real_bytes; }
  int conv_alloc(int g) {
    const size_t n2 = conv_cb_bytes(g);
    unsigned char *q = nullptr;
    int rc;
    for (int f = 0; f < 5; f++)
      for (int sl = 0; sl < 2; sl++) {
        if ((rc = dalloc(&q, f < 3 ? n2 : n2 * conv_nuvz))) return rc;
        conv_fld[g][f][sl] = q;
      }
    if ((rc = dalloc(&q, n2))) return rc;
    HIPCHK(hipMemsetAsync(q, 0, n2, stream));
    conv_cb[g] = q;
    return 0;
  }
  size_t conv_ncol_alloc = 0;                // columns (all domains) the per-column arrays are sized for
  int *conv_pcol = nullptr, *conv_act = nullptr, *conv_lconv = nullptr, *conv_ntop = nullptr, *conv_cflag = nullptr, *conv_ntop_raw = nullptr;
  int4 *conv_colslot = nullptr;
  unsigned int *conv_flag = nullptr, *conv_rank = nullptr;
  unsigned char *conv_draws = nullptr;
  void *conv_rn = nullptr;
  Scratch conv_scr, conv_scan_tmp;
  unsigned long long *conv_nmoved = nullptr;
  double conv_last_ms = 0;
  double conv_ms() override { return conv_last_ms; }

  int conv_init(const fpx_conv_config *c) override {
    if (met_format == MET_GFS || conv_gfs) return fail(FPX_ERR_UNSUPPORTED, "conv_init: NCEP GFS fields: convmix.f90:100-116,173-189 (pplev-based columns) and the NCEP branch of calcmatrix.f90 are not computed by this call: fpx_conv_init_gfs sets them up");
    if (!c || c->struct_bytes != (int32_t)sizeof(fpx_conv_config)) return fail(FPX_ERR_ARG, "conv_init: null or fpx_conv_config size mismatch (ABI)");
    if (c->nuvz < 4 || c->nconvlev < 2 || c->nconvlev > c->nuvz - 2) return fail(FPX_ERR_ARG, "conv_init: need 2 <= nconvlev <= nuvz - 2");
    if (!c->akz || !c->bkz || !c->akm || !c->bkm) return fail(FPX_ERR_ARG, "conv_init: akz, bkz, akm, bkm are required");
    if (conv_on) return fail(FPX_ERR_STATE, "conv_init: already initialised");
    if (cfg.device_flux) return fail(FPX_ERR_UNSUPPORTED, "conv_init: device_flux = 1: the calcfluxes calls of the convective displacement (convmix.f90:208-220,284-296) are not computed by this engine");
    const size_t hb = (size_t)cfg.host_real_bytes;
    int rc;
    const void *tabs[4] = {c->akz, c->bkz, c->akm, c->bkm};
    for (int i = 0; i < 4; i++) {
      unsigned char *q = nullptr;
      if ((rc = dalloc(&q, (size_t)c->nuvz * hb))) return rc;
      HIPCHK(hipMemcpyAsync(q, tabs[i], (size_t)c->nuvz * hb, hipMemcpyHostToDevice, stream));
      conv_tab[i] = q;
    }
    conv_nuvz = c->nuvz; conv_nconvlev = c->nconvlev;
    if ((rc = conv_alloc(0))) return rc;
    if ((rc = dalloc(&conv_pcol, (size_t)P.cap)) || (rc = dalloc(&conv_draws, (size_t)P.cap))) return rc;
    if ((rc = dalloc(&conv_nmoved, (size_t)1))) return rc;
    {
      unsigned char *q = nullptr;
      if ((rc = dalloc(&q, (size_t)P.cap * hb))) return rc;
      conv_rn = q;
    }
    HIPCHK(hipStreamSynchronize(stream));
    conv_on = true;
    return 0;
  }

  int upload_conv(int g, int slot, const fpx_conv_fields *f) {
    int rc;
    if (g > 0 && !conv_cb[g] && (rc = conv_alloc(g))) return rc;
    const void *src[5] = {f->ps, f->tt2, f->td2, f->tth, f->qvh};
    for (int i = 0; i < 5; i++)
      if ((rc = compact(host_grid(g), src[i], conv_fld[g][i][slot - 1], i < 3 ? 1 : conv_nuvz, i < 3 ? 1 : f->nuvzmax))) return rc;
    conv_slot[g][slot - 1] = true;
    return 0;
  }
  int upload_conv_fields(int slot, const fpx_conv_fields *f) override {
    if (!conv_on) return fail(FPX_ERR_STATE, "upload_conv_fields: fpx_conv_init first");
    if (conv_gfs) return fail(FPX_ERR_UNSUPPORTED, "upload_conv_fields: fpx_conv_init_gfs has run on this handle: its slots take ps, tt2, td2, tt, qv, pplev (fpx_upload_conv_gfs_fields), not the model-level tth, qvh");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "upload_conv_fields: slot must be 1 or 2");
    if (!f || !f->ps || !f->tt2 || !f->td2 || !f->tth || !f->qvh) return fail(FPX_ERR_ARG, "upload_conv_fields: ps, tt2, td2, tth, qvh are required");
    if (f->nuvzmax < conv_nuvz) return fail(FPX_ERR_ARG, "upload_conv_fields: nuvzmax < nuvz");
    return upload_conv(0, slot, f);
  }
  int upload_conv_nest_fields(int nest, int slot, const fpx_conv_fields *f) override {
    if (!conv_on) return fail(FPX_ERR_STATE, "upload_conv_nest_fields: fpx_conv_init first");
    if (conv_gfs) return fail(FPX_ERR_UNSUPPORTED, "upload_conv_nest_fields: fpx_conv_init_gfs has run on this handle: the reference has no GFS nests");
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "upload_conv_nest_fields: nest out of range (fpx_nests_init first)");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "upload_conv_nest_fields: slot must be 1 or 2");
    if (!f || !f->ps || !f->tt2 || !f->td2 || !f->tth || !f->qvh) return fail(FPX_ERR_ARG, "upload_conv_nest_fields: ps, tt2, td2, tth, qvh are required");
    if (f->nuvzmax < conv_nuvz) return fail(FPX_ERR_ARG, "upload_conv_nest_fields: nuvzmax < nuvz");
    return upload_conv(nest, slot, f);
  }
  // cbaseflux of grid g <-> host, for the entry point `who`
  int cbaseflux_copy(int g, void *host, bool set, const char *who) {
    if (!conv_on) return fail(FPX_ERR_STATE, std::string(who) + ": fpx_conv_init first");
    if (g > 0 && (g > V.numbnests || !conv_cb[g])) return fail(FPX_ERR_STATE, std::string(who) + ": fpx_upload_conv_nest_fields of this nest first");
    if (!host) return fail(FPX_ERR_ARG, std::string(who) + ": null");
    if (set) HIPCHK(hipMemcpyAsync(conv_cb[g], host, conv_cb_bytes(g), hipMemcpyHostToDevice, stream));
    else HIPCHK(hipMemcpyAsync(host, conv_cb[g], conv_cb_bytes(g), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  int cbaseflux_io(void *host, bool set) override { return cbaseflux_copy(0, host, set, "cbaseflux"); }
  int cbaseflux_nest_io(int nest, void *host, bool set) override {   // (an index below 1 is no nest: kMaxNests + 1 fails the same check)
    return cbaseflux_copy(nest < 1 ? kMaxNests + 1 : nest, host, set, "cbaseflux_nest");
  }

  // sort2.f90 (the reference's quicksort with insertion sort below 7 elements; not stable): the order in which convmix
  // visits the particles, hence the order of redist's draws from the shared ran3 stream.  Host side of the parity mode.
  static void conv_sort2(int n, int *arr, int *brr) {     // 1-based [1..n]
    const int M = 7, NSTACK = 50;
    int i, ir, j, jstack = 0, k, l = 1, istack[51], a, b;
    ir = n;
    for (;;) {
      if (ir - l < M) {
        for (j = l + 1; j <= ir; j++) {
          a = arr[j]; b = brr[j];
          for (i = j - 1; i >= 1; i--) {
            if (arr[i] <= a) break;
            arr[i + 1] = arr[i]; brr[i + 1] = brr[i];
          }
          if (i < 1) i = 0;
          arr[i + 1] = a; brr[i + 1] = b;
        }
        if (jstack == 0) return;
        ir = istack[jstack]; l = istack[jstack - 1]; jstack -= 2;
      } else {
        k = (l + ir) / 2;
        std::swap(arr[k], arr[l + 1]); std::swap(brr[k], brr[l + 1]);
        if (arr[l + 1] > arr[ir]) { std::swap(arr[l + 1], arr[ir]); std::swap(brr[l + 1], brr[ir]); }
        if (arr[l] > arr[ir]) { std::swap(arr[l], arr[ir]); std::swap(brr[l], brr[ir]); }
        if (arr[l + 1] > arr[l]) { std::swap(arr[l + 1], arr[l]); std::swap(brr[l + 1], brr[l]); }
        i = l + 1; j = ir; a = arr[l]; b = brr[l];
        for (;;) {
          do i++; while (arr[i] < a);
          do j--; while (arr[j] > a);
          if (j < i) break;
          std::swap(arr[i], arr[j]); std::swap(brr[i], brr[j]);
        }
        arr[l] = arr[j]; arr[j] = a; brr[l] = brr[j]; brr[j] = b;
        jstack += 2;
        if (jstack > NSTACK) return;
        if (ir - i + 1 >= j - l) { istack[jstack] = ir; istack[jstack - 1] = i; ir = j - 1; }
        else { istack[jstack] = j - 1; istack[jstack - 1] = l; l = i; }
      }
    }
  }

  // replay of the serial stream: particles by particle number, igrid as convmix builds it, the reference's sort2, ran3 for
  // the particles the probe pass found drawing
  template <typename H>
  int conv_replay(long long n, int ndom, const int *off) {
    std::vector<unsigned char> h_draws((size_t)n);
    std::vector<int> h_pcol((size_t)n);
    std::vector<unsigned int> h_pid((size_t)n);
    HIPCHK(hipMemcpyAsync(h_draws.data(), conv_draws, (size_t)n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_pcol.data(), conv_pcol, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(h_pid.data(), P.pid, (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    std::vector<int> col_by_pid((size_t)n, -1), igrid((size_t)n + 1), ipoint((size_t)n + 1);
    std::vector<unsigned char> draws_by_pid((size_t)n, 0);
    for (long long s = 0; s < n; s++) {
      const unsigned int p = h_pid[(size_t)s];
      if (p >= (unsigned int)n) return fail(FPX_ERR_STATE, "convmix: particle numbers beyond numpart");
      col_by_pid[p] = h_pcol[(size_t)s];
      draws_by_pid[p] = h_draws[(size_t)s];
    }
    std::vector<H> rn((size_t)n, (H)-1);
    for (int d = 0; d < ndom; d++) {          // the mother grid first, then nest by nest (convmix.f90:139-196, 198-250)
      for (long long p = 1; p <= n; p++) {
        const int c = col_by_pid[(size_t)p - 1];
        igrid[(size_t)p] = (c >= off[d] && c < off[d + 1]) ? 1 + c - off[d] : -1;
        ipoint[(size_t)p] = (int)p;
      }
      conv_sort2((int)n, igrid.data(), ipoint.data());
      for (long long k = 1; k <= n; k++) {
        if (igrid[(size_t)k] == -1) continue;
        const int p = ipoint[(size_t)k] - 1;
        if (!draws_by_pid[(size_t)p]) continue;
        rn[(size_t)p] = sizeof(H) == 4 ? (H)rng4.ran3(rng4.idummy_redist) : (H)rng8.ran3(rng8.idummy_redist);
      }
    }
    HIPCHK(hipMemcpyAsync(conv_rn, rn.data(), (size_t)n * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  Scratch conv_alive;
  int conv_last_active = 0, conv_last_survivors = 0;
  // what fpx_conv_columns needs to know of the last call of fpx_convmix, whose scratch stays as that call left it
  struct ConvLast {
    bool valid = false;
    int ncol = 0, nact = 0, Bm = 0, batches = 0;
    int form = 0;                            // of the stored matrices: 0 interleaved, 1 walk-major (forward), 2 transposed walk-major (backward)
  } conv_last;

  template <typename H>
  int convmix_t(int itime, int64_t *nmoved_out) {
    const long long n = numpart;
    const int nx = cfg.nx, ny = cfg.ny;
    const int nv = conv_nuvz + 2;
    conv_last = ConvLast{};
    // wind-field domains: the mother grid and the nests (fpx_nests_init); columns numbered through all of them
    conv::Fields<H> F;
    int off[conv::kConvMaxDom + 1];
    F.ndom = 1 + V.numbnests;
    off[0] = 0;
    for (int d = 0; d < F.ndom; d++) {
      conv::Dom<H> &D = F.dom[d];
      void *(*fld)[2] = conv_fld[d];
      for (int sl = 0; sl < 2; sl++) {
        D.ps[sl] = (const H *)fld[0][sl]; D.tt2[sl] = (const H *)fld[1][sl]; D.td2[sl] = (const H *)fld[2][sl];
        D.tth[sl] = (const H *)fld[3][sl]; D.qvh[sl] = (const H *)fld[4][sl];
      }
      D.cb = (H *)conv_cb[d];
      D.nx = host_grid(d).nx; D.ny = host_grid(d).ny;
      D.off = off[d];
      off[d + 1] = off[d] + D.nx * D.ny;
      if (d > 0) {
        const NestDesc<R> &N = h_nest[d - 1];
        D.xl = (H)N.xl; D.yl = (H)N.yl; D.xr = (H)N.xr; D.yr = (H)N.yr; D.xres = (H)N.xres; D.yres = (H)N.yres;
      } else { D.xl = D.yl = D.xr = D.yr = (H)0; D.xres = D.yres = (H)1; }
    }
    const int ncol = off[F.ndom];
    F.akz = (const H *)conv_tab[0]; F.bkz = (const H *)conv_tab[1]; F.akm = (const H *)conv_tab[2]; F.bkm = (const H *)conv_tab[3];
    F.nuvz = conv_nuvz; F.nconvlev = conv_nconvlev;
    F.m1 = V.m1; F.m2 = V.m2;
    F.dt1 = (H)(itime - V.memtime0); F.dt2 = (H)(V.memtime1 - itime);
    F.dtt = (H)1. / (F.dt1 + F.dt2);
    F.delt = (H)std::abs(cfg.lsynctime);
    F.eps = (H)cfg.par_nxmax / (H)3.e5;
    if ((size_t)ncol > conv_ncol_alloc) {
      int rc2;
      if ((rc2 = dalloc(&conv_flag, (size_t)ncol)) || (rc2 = dalloc(&conv_rank, (size_t)ncol)) || (rc2 = dalloc(&conv_act, (size_t)ncol)) ||
          (rc2 = dalloc(&conv_lconv, (size_t)ncol)) || (rc2 = dalloc(&conv_ntop, (size_t)ncol)) || (rc2 = dalloc(&conv_cflag, (size_t)ncol)) ||
          (rc2 = dalloc(&conv_ntop_raw, (size_t)ncol)) || (rc2 = dalloc(&conv_colslot, (size_t)ncol))) return rc2;
      conv_ncol_alloc = (size_t)ncol;
    }
    const int nb = (int)((n + kBlock - 1) / kBlock), nbc = (ncol + kBlock - 1) / kBlock;
    Events<2> ev;
    HIPCHK(ev.create());
    HIPCHK(hipEventRecord(ev[0], stream));
    HIPCHK(hipMemsetAsync(conv_flag, 0, (size_t)ncol * sizeof(unsigned int), stream));
    HIPCHK(hipMemsetAsync(conv_nmoved, 0, sizeof(unsigned long long), stream));
    conv::k_conv_mark<R, H><<<nb, kBlock, 0, stream>>>(F, P.xt, P.yt, P.itra1, n, itime, conv_pcol, conv_flag);
    HIPCHK(hipGetLastError());
    size_t tb = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, tb, conv_flag, conv_rank, 0u, (size_t)ncol, rocprim::plus<unsigned int>(), stream));
    HIPCHK(conv_scan_tmp.reserve(tb, stream));
    HIPCHK(rocprim::exclusive_scan(conv_scan_tmp.as(), tb, conv_flag, conv_rank, 0u, (size_t)ncol, rocprim::plus<unsigned int>(), stream));
    unsigned int last_rank = 0, last_flag = 0;
    HIPCHK(hipMemcpyAsync(&last_rank, conv_rank + (ncol - 1), 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&last_flag, conv_flag + (ncol - 1), 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const int nact = (int)(last_rank + last_flag);
    if (nact == 0) { if (nmoved_out) *nmoved_out = 0; conv_last_ms = 0; conv_last.valid = true; conv_last.ncol = ncol; return 0; }
    conv::k_conv_list<<<nbc, kBlock, 0, stream>>>(conv_flag, conv_rank, ncol, conv_act);
    HIPCHK(hipGetLastError());
    // scratch: the vectors of every column that holds particles; the matrices only for the columns that get past CONVECT's
    // early exits, in batches that fit the budget (default: a quarter of the free device memory)
    const size_t vec_elems = conv::vec_elems_per_column<H>(nv) * conv::group_round((size_t)nact);
    const size_t cst_elems = conv::group_round((size_t)conv::C_COUNT * nact);
    const size_t vec_bytes = (vec_elems + cst_elems) * sizeof(H);
    const size_t per_mat = conv::mat_elems_per_column<H>(nv) * sizeof(H);
    size_t budget;
    {
      size_t free_b = 0, total_b = 0;
      HIPCHK(hipMemGetInfo(&free_b, &total_b));
      budget = (free_b + conv_scr.bytes()) / 4;
      if (opt.conv_scratch_mb > 0) budget = (size_t)opt.conv_scratch_mb << 20;
    }
    HIPCHK(conv_alive.reserve((size_t)nact * 3 * sizeof(unsigned int), stream));
    unsigned int *alive = conv_alive.as<unsigned int>(), *srank = alive + nact;
    int *surv = (int *)(alive + 2 * (size_t)nact);
    // upper bound of the matrix batch before the survivors are known: all active columns, capped by the budget
    int Bm_cap = (int)std::min<size_t>(conv::group_round((size_t)nact), std::max<size_t>(64, budget / per_mat / conv::kGroup * conv::kGroup));
    {
      const hipError_t e = conv_scr.reserve(vec_bytes + (size_t)Bm_cap * per_mat, stream);
      if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("convmix: scratch: ") + hipGetErrorString(e));
    }
    H *vbuf = conv_scr.as<H>(), *cst = vbuf + vec_elems, *mbuf = cst + cst_elems;
    const H height_nz = (H)height_host[cfg.nz - 1];
    const bool seq = cfg.rng_mode == FPX_RNG_TABLE_SEQ;
    const bool conv_one_lane = opt.conv_one_lane != 0;     // the one-lane-per-column kernel (kept as the check of the level-parallel ones)
    // fmassfrac stored along the rows (forward runs) / columns (backward) the particles walk (k_conv_matrix_walk, _walk_t);
    // fpx_set_option "conv_no_walk": the interleaved form
    const bool conv_walk = !conv_one_lane && !opt.conv_no_walk;
    const bool conv_rows_plain = opt.conv_rows_plain != 0;  // k_conv_rows without the LDS staging of its operands
    if (conv_gfs) cvg::k_conv_column_a_gfs<H><<<conv::serial_grid(nact), 64, 0, stream>>>(F, (const H *)conv_pplev[F.m1], (const H *)conv_pplev[F.m2], vbuf, cst, nv, conv_act, nact, alive);
    else conv::k_conv_column_a<H><<<conv::serial_grid(nact), 64, 0, stream>>>(F, vbuf, cst, nv, conv_act, nact, alive);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(conv_lconv, 0, (size_t)nact * sizeof(int), stream));
    HIPCHK(hipMemsetAsync(conv_ntop, 0, (size_t)nact * sizeof(int), stream));
    tb = conv_scan_tmp.bytes();
    HIPCHK(rocprim::exclusive_scan(conv_scan_tmp.as(), tb, alive, srank, 0u, (size_t)nact, rocprim::plus<unsigned int>(), stream));
    HIPCHK(hipMemcpyAsync(&last_rank, srank + (nact - 1), 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&last_flag, alive + (nact - 1), 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const int nsurv = (int)(last_rank + last_flag);
    conv_last_active = nact; conv_last_survivors = nsurv;
    if (nsurv > 0) {
      conv::k_conv_survivors<<<(nact + kBlock - 1) / kBlock, kBlock, 0, stream>>>(alive, srank, nact, surv);
      HIPCHK(hipGetLastError());
      const int Bm = std::min(nsurv, Bm_cap);
      if (seq && nsurv > Bm) return fail(FPX_ERR_UNSUPPORTED, "convmix: the serial-stream parity mode needs all convective columns in one scratch batch (raise the option \"conv_scratch_mb\" of fpx_set_option)");
      // parity mode: the random numbers come from the shared serial stream in the reference's visiting order, which needs to
      // know who draws -- a probe pass records that, the host replays the stream, then the particles are moved
      conv_last.Bm = Bm;
      for (int m0 = 0; m0 < nsurv; m0 += Bm) {
        conv_last.batches++;
        if (conv_one_lane) {
          conv::k_conv_column_b<H><<<(Bm + 63) / 64, 64, 0, stream>>>(F, vbuf, mbuf, cst, nv, nact, conv_act, surv, m0, Bm, nsurv, conv_lconv, conv_ntop);
        } else {
          const int nlev = F.nconvlev + 1;
          const unsigned int gl = conv::level_grid(Bm, nlev);
          conv::k_conv_prelude<H><<<conv::serial_grid(Bm), 64, 0, stream>>>(F, vbuf, mbuf, cst, nv, nact, surv, m0, Bm, nsurv, conv_cflag, conv_ntop_raw);
          if (conv_rows_plain) conv::k_conv_rows<H><<<gl, 64, 0, stream>>>(vbuf, mbuf, cst, nv, nact, surv, m0, Bm, nsurv, nlev);
          else conv::k_conv_rows_lds<H><<<conv::level_grid(Bm, (nlev + conv::kRowsPerBlock - 1) / conv::kRowsPerBlock), dim3(64, conv::kRowsPerBlock), 0, stream>>>(
                   vbuf, mbuf, cst, nv, nact, surv, m0, Bm, nsurv, nlev);
          conv::k_conv_cols<H><<<gl, 64, 0, stream>>>(vbuf, mbuf, cst, nv, nact, surv, m0, Bm, nsurv, nlev, conv_ntop_raw);
          conv::k_conv_flux<H><<<gl, 64, 0, stream>>>(F, vbuf, mbuf, cst, nv, nact, surv, m0, Bm, nsurv, nlev, conv_cflag);
          if (conv_walk && cfg.ldirect == 1) conv::k_conv_matrix_walk<H><<<gl, 64, 0, stream>>>(F, vbuf, mbuf, cst, nv, nact, conv_act, surv, m0, Bm, nsurv, nlev, conv_cflag, conv_ntop_raw, conv_lconv, conv_ntop);
          else if (conv_walk) conv::k_conv_matrix_walk_t<H><<<conv::level_grid(Bm, (nlev + conv::kWalkRows - 1) / conv::kWalkRows), dim3(64, conv::kWalkRows), 0, stream>>>(
                                  F, vbuf, mbuf, cst, nv, nact, conv_act, surv, m0, Bm, nsurv, nlev, conv_cflag, conv_ntop_raw, conv_lconv, conv_ntop);
          else conv::k_conv_matrix<H><<<gl, 64, 0, stream>>>(F, vbuf, mbuf, cst, nv, nact, conv_act, surv, m0, Bm, nsurv, nlev, conv_cflag, conv_ntop_raw, conv_lconv, conv_ntop);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(conv_colslot, 0, (size_t)ncol * sizeof(int4), stream));
        conv::k_conv_slots<<<(nact + kBlock - 1) / kBlock, kBlock, 0, stream>>>(conv_act, alive, srank, conv_lconv, conv_ntop, nact, m0, Bm, conv_colslot);
        if (seq) {
          HIPCHK(hipMemsetAsync(conv_draws, 0, (size_t)n, stream));
          conv::k_conv_redist<R, H, ConvRngSeq<H>><<<nb, kBlock, 0, stream>>>(conv_pcol, conv_colslot, P.zt, n, vbuf, mbuf, nv, nact, Bm,
                                                                          cfg.ldirect, cfg.lsynctime, height_nz, ConvRngSeq<H>{(const H *)conv_rn, P.pid},
                                                                          conv_draws, 1, nullptr, conv_walk ? 1 : 0);
          HIPCHK(hipGetLastError());
          int rrc = conv_replay<H>(n, F.ndom, off);
          if (rrc) return rrc;
          conv::k_conv_redist<R, H, ConvRngSeq<H>><<<nb, kBlock, 0, stream>>>(conv_pcol, conv_colslot, P.zt, n, vbuf, mbuf, nv, nact, Bm,
                                                                          cfg.ldirect, cfg.lsynctime, height_nz, ConvRngSeq<H>{(const H *)conv_rn, P.pid},
                                                                          conv_draws, 0, conv_nmoved, conv_walk ? 1 : 0);
        } else {
          conv::k_conv_redist<R, H, ConvRngCtr<R, H>><<<nb, kBlock, 0, stream>>>(conv_pcol, conv_colslot, P.zt, n, vbuf, mbuf, nv, nact, Bm,
                                                                             cfg.ldirect, cfg.lsynctime, height_nz, ConvRngCtr<R, H>{V, P.pid, step_counter},
                                                                             conv_draws, 0, conv_nmoved, conv_walk ? 1 : 0);
        }
        HIPCHK(hipGetLastError());
      }
    }
    HIPCHK(hipEventRecord(ev[1], stream));
    unsigned long long moved = 0;
    HIPCHK(hipMemcpyAsync(&moved, conv_nmoved, sizeof(moved), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) conv_last_ms = ms;
    if (nmoved_out) *nmoved_out = (int64_t)moved;
    conv_last.ncol = ncol; conv_last.nact = nact;
    conv_last.form = !conv_walk ? 0 : cfg.ldirect == 1 ? 1 : 2;
    conv_last.valid = true;
    return 0;
  }

  // fpx_conv_columns: one gather kernel over the scratch of the last call; nothing of fpx_convmix runs
  template <typename H>
  int conv_columns_t(const int32_t *col, int ncol_req, int32_t *lconv, int32_t *nconvtop, void *fmassfrac, void *uvzlev) {
    const int nl = conv_nconvlev + 1, nv = conv_nuvz + 2;      // nconvtop <= nconvlev + 1 (CONVECT's inb <= nconvlev), uvzlev(nconvtop + 1) < nv
    const ConvLast &L = conv_last;
    const size_t nfm = (size_t)ncol_req * nl * nl, nuz = (size_t)ncol_req * (nl + 1);
    Scratch ibuf, rbuf;
    hipError_t e = ibuf.reserve((size_t)ncol_req * 3 * sizeof(int), stream);
    if (e == hipSuccess) e = rbuf.reserve((nfm + nuz) * sizeof(H), stream);
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("conv_columns: ") + hipGetErrorString(e));
    int *d_col = ibuf.as<int>(), *d_lconv = d_col + ncol_req, *d_ntop = d_lconv + ncol_req;
    H *d_fm = rbuf.as<H>(), *d_uz = d_fm + nfm;
    HIPCHK(hipMemcpyAsync(d_col, col, (size_t)ncol_req * sizeof(int), hipMemcpyHostToDevice, stream));
    H *vbuf = nullptr, *mbuf = nullptr;
    const unsigned int *srank = nullptr;
    if (L.nact > 0) {                                      // the layout of convmix_t's scratch
      const size_t vec_elems = conv::vec_elems_per_column<H>(nv) * conv::group_round((size_t)L.nact);
      const size_t cst_elems = conv::group_round((size_t)conv::C_COUNT * L.nact);
      vbuf = conv_scr.as<H>(); mbuf = vbuf + vec_elems + cst_elems;
      srank = conv_alive.as<unsigned int>() + L.nact;
    }
    conv::k_conv_columns<H><<<ncol_req, 64, 0, stream>>>(d_col, L.ncol, conv_flag, conv_rank, srank, conv_lconv, conv_ntop, vbuf, mbuf, nv, L.nact,
                                                        L.Bm, nl, L.form, d_lconv, d_ntop, d_fm, d_uz);
    HIPCHK(hipGetLastError());
    if (lconv) HIPCHK(hipMemcpyAsync(lconv, d_lconv, (size_t)ncol_req * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (nconvtop) HIPCHK(hipMemcpyAsync(nconvtop, d_ntop, (size_t)ncol_req * sizeof(int), hipMemcpyDeviceToHost, stream));
    if (fmassfrac) HIPCHK(hipMemcpyAsync(fmassfrac, d_fm, nfm * sizeof(H), hipMemcpyDeviceToHost, stream));
    if (uvzlev) HIPCHK(hipMemcpyAsync(uvzlev, d_uz, nuz * sizeof(H), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  int conv_columns(const int32_t *col, int ncol_req, int32_t *lconv, int32_t *nconvtop, void *fmassfrac, void *uvzlev) override {
    if (!conv_on) return fail(FPX_ERR_STATE, "conv_columns: fpx_conv_init first");
    if (!conv_last.valid) return fail(FPX_ERR_STATE, "conv_columns: no completed call of fpx_convmix to report");
    if (conv_last.batches > 1) return fail(FPX_ERR_STATE, "conv_columns: the last call of fpx_convmix ran " + std::to_string(conv_last.batches) + " matrix batches; only the matrices of the last one exist (raise the option \"conv_scratch_mb\" of fpx_set_option)");
    if (ncol_req < 0 || (ncol_req > 0 && !col)) return fail(FPX_ERR_ARG, "conv_columns: ncol < 0 or col is null");
    for (int i = 0; i < ncol_req; i++)
      if (col[i] < 0 || col[i] >= conv_last.ncol) return fail(FPX_ERR_ARG, "conv_columns: column out of range (mother grid first, then the nests)");
    if (ncol_req == 0) return 0;
    return cfg.host_real_bytes == 4 ? conv_columns_t<float>(col, ncol_req, lconv, nconvtop, fmassfrac, uvzlev)
                                    : conv_columns_t<double>(col, ncol_req, lconv, nconvtop, fmassfrac, uvzlev);
  }

  // ---- the NCEP GFS branch (fpx_convect_gfs.hpp) ------------------------------------------------------------------
  // conv_fld[0][0..4] hold ps, tt2, td2 and the z-level tt, qv (in the places of tth, qvh); pplev has buffers of its own.
  bool conv_gfs = false;
  void *conv_pplev[2] = {nullptr, nullptr};
  int conv_init_gfs(const fpx_conv_gfs_config *c) override {
    if (!c || c->struct_bytes != (int32_t)sizeof(fpx_conv_gfs_config)) return fail(FPX_ERR_ARG, "conv_init_gfs: null or fpx_conv_gfs_config size mismatch (ABI)");
    if (met_format == MET_ECMWF) return fail(FPX_ERR_UNSUPPORTED, "conv_init_gfs: this handle has run an ECMWF transform: fpx_conv_init is its convection set-up");
    if (V.numbnests) return fail(FPX_ERR_UNSUPPORTED, "conv_init_gfs: fpx_nests_init has run: the reference has no GFS nests (the eps-free nest test of convmix.f90:108-116 is never reached)");
    if (conv_on) return fail(FPX_ERR_STATE, "conv_init_gfs: convection is already initialised");
    if (cfg.device_flux) return fail(FPX_ERR_UNSUPPORTED, "conv_init_gfs: device_flux = 1: the calcfluxes calls of the convective displacement (convmix.f90:208-220,284-296) are not computed by this engine");
    if (c->nuvz != cfg.nz) return fail(FPX_ERR_ARG, "conv_init_gfs: nuvz = nz expected (gridcheck_gfs.f90:439-491 sets them equal)");
    if (c->nuvz < 4 || c->nconvlev < 2 || c->nconvlev > c->nuvz - 2) return fail(FPX_ERR_ARG, "conv_init_gfs: need 2 <= nconvlev <= nuvz - 2");
    const size_t hb = (size_t)cfg.host_real_bytes;
    int rc;
    conv_nuvz = c->nuvz; conv_nconvlev = c->nconvlev;
    if ((rc = conv_alloc(0))) return rc;
    for (int sl = 0; sl < 2; sl++) {
      unsigned char *q = nullptr;
      if ((rc = dalloc(&q, conv_cb_bytes(0) * conv_nuvz))) return rc;
      conv_pplev[sl] = q;
    }
    if ((rc = dalloc(&conv_pcol, (size_t)P.cap)) || (rc = dalloc(&conv_draws, (size_t)P.cap))) return rc;
    if ((rc = dalloc(&conv_nmoved, (size_t)1))) return rc;
    {
      unsigned char *q = nullptr;
      if ((rc = dalloc(&q, (size_t)P.cap * hb))) return rc;
      conv_rn = q;
    }
    HIPCHK(hipStreamSynchronize(stream));
    conv_on = true; conv_gfs = true;
    met_format = MET_GFS;
    return 0;
  }
  int upload_conv_gfs_fields(int slot, const fpx_conv_gfs_fields *f) override {
    if (!conv_gfs) return fail(FPX_ERR_STATE, "upload_conv_gfs_fields: fpx_conv_init_gfs first");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "upload_conv_gfs_fields: slot must be 1 or 2");
    if (!f || !f->ps || !f->tt2 || !f->td2 || !f->tt || !f->qv || !f->pplev) return fail(FPX_ERR_ARG, "upload_conv_gfs_fields: ps, tt2, td2, tt, qv, pplev are required");
    if (f->nzmax < conv_nuvz) return fail(FPX_ERR_ARG, "upload_conv_gfs_fields: nzmax < nuvz");
    int rc;
    const void *src[6] = {f->ps, f->tt2, f->td2, f->tt, f->qv, f->pplev};
    for (int i = 0; i < 6; i++)
      if ((rc = compact(host_grid(0), src[i], i < 5 ? conv_fld[0][i][slot - 1] : conv_pplev[slot - 1], i < 3 ? 1 : conv_nuvz, i < 3 ? 1 : f->nzmax))) return rc;
    conv_slot[0][slot - 1] = true;
    return 0;
  }
  // fpx_verttransform_gfs after fpx_conv_init_gfs: the slot's ps, tt2, td2, tt, qv, pplev stay on the device for the convection
  // (device to device; the transform's buffers are in the host's kind and layout)
  template <typename H>
  int conv_keep_gfs(int slot, const H *ps, const H *tt2, const H *td2, const H *tt, const H *qv, const H *pplev) {
    const HostGrid g = host_grid(0);
    const H *src[6] = {ps, tt2, td2, tt, qv, pplev};
    for (int i = 0; i < 6; i++) {
      const int nlev = i < 3 ? 1 : conv_nuvz;
      const dim3 grid((g.nx + 31) / 32, (nlev + 7) / 8, g.ny), block(32, 8);
      cvg::k_cvg_compact<H><<<grid, block, 0, stream>>>(src[i], (H *)(i < 5 ? conv_fld[0][i][slot - 1] : conv_pplev[slot - 1]), g.nx, g.ny, nlev, g.nxmax, g.nymax);
    }
    HIPCHK(hipGetLastError());
    conv_slot[0][slot - 1] = true;
    return 0;
  }
  // fpx_conv_soundings: one gather kernel over the vectors of the last call's scratch; nothing of fpx_convmix runs
  template <typename H>
  int conv_soundings_t(const int32_t *col, int nreq, void *psconv, void *pconv, void *phconv, void *dpr, void *tconv, void *qconv) {
    const int nuvz = conv_nuvz, nv = conv_nuvz + 2;
    const ConvLast &L = conv_last;
    const size_t n1 = (size_t)nreq * (nuvz - 1), nh = (size_t)nreq * nuvz;
    Scratch ibuf, rbuf;
    hipError_t e = ibuf.reserve((size_t)nreq * sizeof(int), stream);
    if (e == hipSuccess) e = rbuf.reserve(((size_t)nreq + 4 * n1 + nh) * sizeof(H), stream);
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("conv_soundings: ") + hipGetErrorString(e));
    int *d_col = ibuf.as<int>();
    H *d_ps = rbuf.as<H>(), *d_pc = d_ps + nreq, *d_ph = d_pc + n1, *d_dpr = d_ph + nh, *d_tc = d_dpr + n1, *d_qc = d_tc + n1;
    HIPCHK(hipMemcpyAsync(d_col, col, (size_t)nreq * sizeof(int), hipMemcpyHostToDevice, stream));
    H *vbuf = nullptr, *cst = nullptr;
    if (L.nact > 0) {                                      // the layout of convmix_t's scratch
      vbuf = conv_scr.as<H>();
      cst = vbuf + conv::vec_elems_per_column<H>(nv) * conv::group_round((size_t)L.nact);
    }
    cvg::k_conv_soundings<H><<<nreq, 64, 0, stream>>>(d_col, L.ncol, conv_flag, conv_rank, vbuf, cst, nv, L.nact, nuvz, d_ps, d_pc, d_ph, d_dpr, d_tc, d_qc);
    HIPCHK(hipGetLastError());
    if (psconv) HIPCHK(hipMemcpyAsync(psconv, d_ps, (size_t)nreq * sizeof(H), hipMemcpyDeviceToHost, stream));
    if (pconv) HIPCHK(hipMemcpyAsync(pconv, d_pc, n1 * sizeof(H), hipMemcpyDeviceToHost, stream));
    if (phconv) HIPCHK(hipMemcpyAsync(phconv, d_ph, nh * sizeof(H), hipMemcpyDeviceToHost, stream));
    if (dpr) HIPCHK(hipMemcpyAsync(dpr, d_dpr, n1 * sizeof(H), hipMemcpyDeviceToHost, stream));
    if (tconv) HIPCHK(hipMemcpyAsync(tconv, d_tc, n1 * sizeof(H), hipMemcpyDeviceToHost, stream));
    if (qconv) HIPCHK(hipMemcpyAsync(qconv, d_qc, n1 * sizeof(H), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  int conv_soundings(const int32_t *col, int nreq, void *psconv, void *pconv, void *phconv, void *dpr, void *tconv, void *qconv) override {
    if (!conv_on) return fail(FPX_ERR_STATE, "conv_soundings: fpx_conv_init or fpx_conv_init_gfs first");
    if (!conv_last.valid) return fail(FPX_ERR_STATE, "conv_soundings: no completed call of fpx_convmix to report");
    if (nreq < 0 || (nreq > 0 && !col)) return fail(FPX_ERR_ARG, "conv_soundings: ncol < 0 or col is null");
    for (int i = 0; i < nreq; i++)
      if (col[i] < 0 || col[i] >= conv_last.ncol) return fail(FPX_ERR_ARG, "conv_soundings: column out of range (mother grid first, then the nests)");
    if (nreq == 0) return 0;
    return cfg.host_real_bytes == 4 ? conv_soundings_t<float>(col, nreq, psconv, pconv, phconv, dpr, tconv, qconv)
                                    : conv_soundings_t<double>(col, nreq, psconv, pconv, phconv, dpr, tconv, qconv);
  }

  int convmix(int itime, int64_t *nmoved) override {
    if (met_format == MET_GFS && !conv_gfs) return fail(FPX_ERR_UNSUPPORTED, "convmix: NCEP GFS fields: convmix.f90:100-116,173-189 (pplev-based columns) and the NCEP branch of calcmatrix.f90 need fpx_conv_init_gfs on this handle");
    if (!conv_on) return fail(FPX_ERR_STATE, "convmix: fpx_conv_init first");
    if (conv_gfs && V.numbnests) return fail(FPX_ERR_UNSUPPORTED, "convmix: NCEP GFS fields with nested wind fields: the reference has no GFS nests");
    if (conv_gfs && (!conv_slot[0][0] || !conv_slot[0][1])) return fail(FPX_ERR_STATE, "convmix: fpx_upload_conv_gfs_fields or fpx_verttransform_gfs of both slots first");
    if (!conv_slot[0][0] || !conv_slot[0][1]) return fail(FPX_ERR_STATE, "convmix: fpx_upload_conv_fields of both slots first");
    for (int l = 1; l <= V.numbnests; l++)
      if (!conv_slot[l][0] || !conv_slot[l][1]) return fail(FPX_ERR_STATE, "convmix: fpx_upload_conv_nest_fields of both slots of every nest first");
    if (1 + V.numbnests > conv::kConvMaxDom) return fail(FPX_ERR_UNSUPPORTED, "convmix: too many nests");
    if (!window_set) return fail(FPX_ERR_STATE, "convmix: fpx_set_windtime first");
    if (!height_set) return fail(FPX_ERR_STATE, "convmix: set_height first");
    if (numpart == 0) { if (nmoved) *nmoved = 0; conv_last = ConvLast{}; return 0; }
    return cfg.host_real_bytes == 4 ? convmix_t<float>(itime, nmoved) : convmix_t<double>(itime, nmoved);
  }

  // ---- lossless checkpoint (last clause) ------------------------------------------------------
  // partoutput / readpartpositions keep position, mass and age of a particle, rounded to the dump's real kind; the
  // turbulent velocity memory (up, vp, wp), the mesoscale components (us, vs, ws), cbt, idt, itramem, itrasplit,
  // nclass are re-initialised by a warm start (readpartpositions.f90:118-148), so the reference's restart is a
  // different realisation of the run.  This pair writes and reads everything the loop carries: all particle arrays in
  // the compute precision and in particle-number order, the step counter the counter RNG is keyed on, the state of
  // the serial ran3 / ran1 streams of the parity mode, and the accumulating output grids.  A run continued from it
  // is the run that was never interrupted, bit for bit.
  struct CkptHeader {
    char magic[8];
    int32_t version, real_bytes, nspec, rng_mode;
    int64_t numpart, particle_base;
    uint64_t seed;
    uint32_t step_counter;
    int32_t itime, numparticlecount, reserved;
    uint64_t n_grid3, n_grid2, n_grid3n, n_grid2n, n_receptor, rng_bytes;
    uint64_t cbase_bytes;        // conv_mod cbaseflux (the convection scheme relaxes it from call to call)
    int64_t rel_global_count;    // particles released so far by all ranks
    // version 2: what the arrays were sized with, and the length of the whole file (checked before anything is restored)
    int32_t nx, ny, nz, maxspec, numbnests, nxn[kMaxNests], nyn[kMaxNests], pad;
    uint64_t total_bytes;
  };
  void ckpt_describe_grid(CkptHeader &h) const {
    h.nx = cfg.nx; h.ny = cfg.ny; h.nz = cfg.nz; h.maxspec = cfg.maxspec; h.numbnests = V.numbnests;
    for (int l = 0; l < kMaxNests; l++) { h.nxn[l] = l < V.numbnests ? h_nest[l].nx : 0; h.nyn[l] = l < V.numbnests ? h_nest[l].ny : 0; }
    h.pad = P.xscav ? 1 : 0;      // the file carries xscav_frac1 (backward runs with DRYBKDEP / WETBKDEP)
  }
  // file length that goes with a header: header + RNG state + particle arrays + grids + receptors + cbaseflux
  static uint64_t ckpt_total_bytes(const CkptHeader &h) {
    const uint64_t per_particle = 2 * 8 + 7 * sizeof(R) + 6 * 4 + 2 + (uint64_t)h.nspec * sizeof(R) * (h.pad ? 2 : 1);   // pad = 1: xscav_frac1 follows xmass1
    return sizeof(CkptHeader) + h.rng_bytes + (uint64_t)h.numpart * per_particle + h.n_grid3 * sizeof(R) + 2 * h.n_grid2 * sizeof(float) +
           h.n_grid3n * sizeof(R) + 2 * h.n_grid2n * sizeof(float) + h.n_receptor * sizeof(R) + h.cbase_bytes;
  }
  // a restore replaces the partial sums of every output grid and of the receptors: whatever was reduced before is stale
  void invalidate_grid_sums() {
    for (RankSum *s : {&sum_grid, &sum_dry, &sum_wet, &sum_gridn, &sum_dryn, &sum_wetn, &sum_rec}) s->invalidate();
  }
  // a restore that failed half-way leaves no usable state behind: no particles, no valid reductions
  int ckpt_invalidate(int rc) {
    numpart = 0;
    maybe_new = true; births_unknown = true;
    invalidate_grid_sums();
    (void)hipStreamSynchronize(stream);
    const int nb = (int)((P.cap + kBlock - 1) / kBlock);
    k_fill<int><<<nb, kBlock, 0, stream>>>(P.itra1, kDead, 0, P.cap, nullptr);
    (void)hipStreamSynchronize(stream);
    g_err += " -- the engine holds no particles now (numpart = 0); restore from a complete checkpoint or release again";
    return rc;
  }
  static constexpr long long kCkptChunk = 1ll << 22;
  template <typename T>
  int ckpt_put_array(FILE *fh, const T *dev, long long n, std::vector<unsigned char> &buf) {
    for (long long f = 0; f < n; f += kCkptChunk) {
      const long long c = std::min(kCkptChunk, n - f);
      int rc = get<T, T>((T *)buf.data(), dev, f, c);
      if (rc) return rc;
      if (fwrite(buf.data(), sizeof(T), (size_t)c, fh) != (size_t)c) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
    }
    return 0;
  }
  template <typename T>
  int ckpt_get_array(FILE *fh, T *dev, long long n, std::vector<unsigned char> &buf) {
    for (long long f = 0; f < n; f += kCkptChunk) {
      const long long c = std::min(kCkptChunk, n - f);
      if (fread(buf.data(), sizeof(T), (size_t)c, fh) != (size_t)c) return fail(FPX_ERR_ARG, "checkpoint_read: file too short");
      int rc = put<T, T>((const T *)buf.data(), dev, f, c);
      if (rc) return rc;
    }
    return 0;
  }
  template <typename T>
  int ckpt_put_plain(FILE *fh, const T *dev, size_t n, std::vector<unsigned char> &buf) {
    for (size_t f = 0; f < n; f += (size_t)kCkptChunk) {
      const size_t c = std::min((size_t)kCkptChunk, n - f);
      HIPCHK(hipMemcpyAsync(buf.data(), dev + f, c * sizeof(T), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      if (fwrite(buf.data(), sizeof(T), c, fh) != c) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
    }
    return 0;
  }
  template <typename T>
  int ckpt_get_plain(FILE *fh, T *dev, size_t n, std::vector<unsigned char> &buf) {
    for (size_t f = 0; f < n; f += (size_t)kCkptChunk) {
      const size_t c = std::min((size_t)kCkptChunk, n - f);
      if (fread(buf.data(), sizeof(T), c, fh) != c) return fail(FPX_ERR_ARG, "checkpoint_read: file too short");
      HIPCHK(hipMemcpyAsync(dev + f, buf.data(), c * sizeof(T), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
    }
    return 0;
  }
  // header.reserved, bit 0: the file ends with the flux grid of a run with device_flux (uint64 count, then the values in the
  // host's real kind); a file without fluxes has reserved = 0 and is what it always was
  static constexpr int32_t kCkptFlux = 1;
  // bit 1: after that (or after cbaseflux) follow the interval averages of a run with device_partavg: uint64 numpart, then
  // npart_av (int32) and the fourteen sums in the host's real kind, each [numpart] in particle-number order
  static constexpr int32_t kCkptPartavg = 2;
  uint64_t ckpt_partavg_bytes(const CkptHeader &h) const { return (h.reserved & kCkptPartavg) ? 8 + (uint64_t)h.numpart * (4 + (uint64_t)pa::kSums * cfg.host_real_bytes) : 0; }
  template <typename H>
  int ckpt_put_partavg(FILE *fh, long long n, std::vector<unsigned char> &buf) {
    const pa::State<H> S = partavg_state<H>(pa_cur);
    int rc;
    if ((rc = ckpt_put_array(fh, S.npart_av, n, buf))) return rc;
    for (int k = 0; k < pa::kSums; k++) if ((rc = ckpt_put_array(fh, S.sum + (size_t)k * S.cap, n, buf))) return rc;
    return 0;
  }
  template <typename H>
  int ckpt_get_partavg(FILE *fh, long long n, std::vector<unsigned char> &buf) {
    const pa::State<H> S = partavg_state<H>(pa_cur);
    HIPCHK(hipMemsetAsync(S.npart_av, 0, (size_t)S.cap * sizeof(int), stream));
    HIPCHK(hipMemsetAsync(S.sum, 0, (size_t)S.cap * pa::kSums * sizeof(H), stream));
    int rc;
    if ((rc = ckpt_get_array(fh, S.npart_av, n, buf))) return rc;
    for (int k = 0; k < pa::kSums; k++) if ((rc = ckpt_get_array(fh, S.sum + (size_t)k * S.cap, n, buf))) return rc;
    return 0;
  }
  // bit 2: last, init_cond of a run with device_initcond (uint64 count, then the values in the host's real kind)
  static constexpr int32_t kCkptInitcond = 4;
  uint64_t ckpt_initcond_bytes(const CkptHeader &h) const { return (h.reserved & kCkptInitcond) ? 8 + (uint64_t)n_initcond * cfg.host_real_bytes : 0; }
  uint64_t ckpt_flux_bytes(const CkptHeader &h) const { return (h.reserved & kCkptFlux) ? 8 + (uint64_t)n_flux * cfg.host_real_bytes : 0; }
  struct CkptRng { HostRng<float> r4; HostRng<double> r8; Ran1 rel; };
  uint64_t conv_cbase_bytes() const {      // cbaseflux of the mother grid and of every nest that has convection fields
    if (!conv_on) return 0;
    uint64_t b = 0;
    for (int g = 0; g <= V.numbnests; g++)
      if (conv_cb[g]) b += conv_cb_bytes(g);
    return b;
  }

  int checkpoint_write(const char *path, int itime, int numparticlecount) override {
    if (!path) return fail(FPX_ERR_ARG, "checkpoint_write: path is required");
    if (dfl_on) return fail(FPX_ERR_UNSUPPORTED, "checkpoint_write: the checkpoint does not carry acc_mass_we / acc_mass_sn of fpx_domainfill_init (boundcond.bin does: fpx_boundcond_output)");
    FILE *fh = fopen(path, "wb");
    if (!fh) return fail(FPX_ERR_ARG, std::string("checkpoint_write: cannot open ") + path);
    FileCloser closer(fh);
    const size_t n_grid3 = sum_grid.count(), n_grid2 = sum_dry.count(), n_grid3n = sum_gridn.count(), n_grid2n = sum_dryn.count();
    CkptHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "FPXCKPT1", 8);
    h.version = 2; h.real_bytes = (int)sizeof(R); h.nspec = cfg.nspec; h.rng_mode = cfg.rng_mode;
    h.numpart = numpart; h.particle_base = cfg.particle_base; h.seed = V.seed; h.step_counter = step_counter;
    h.itime = itime; h.numparticlecount = numparticlecount;
    h.n_grid3 = Gp.on ? n_grid3 : 0; h.n_grid2 = Gp.on ? n_grid2 : 0;
    h.n_grid3n = Gp.on && Gp.nested ? n_grid3n : 0; h.n_grid2n = Gp.on && Gp.nested ? n_grid2n : 0;
    h.n_receptor = Gp.creceptor ? (uint64_t)Gp.numreceptor * cfg.maxspec : 0;
    h.rng_bytes = sizeof(CkptRng);
    h.cbase_bytes = conv_cbase_bytes();
    h.rel_global_count = rel_global_count;
    ckpt_describe_grid(h);
    h.reserved = cfg.device_flux && fx_flux ? kCkptFlux : 0;      // the flux section follows cbaseflux: a count and the values
    if (cfg.device_partavg) h.reserved |= kCkptPartavg;
    if (cfg.device_initcond && ic_grid) h.reserved |= kCkptInitcond;
    if (oh_on) h.reserved |= kCkptOh;
    h.total_bytes = ckpt_total_bytes(h) + ckpt_flux_bytes(h) + ckpt_partavg_bytes(h) + ckpt_initcond_bytes(h) + ckpt_oh_bytes(h);
    if (fwrite(&h, sizeof(h), 1, fh) != 1) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
    CkptRng rs{rng4, rng8, rel_ran1};
    if (fwrite(&rs, sizeof(rs), 1, fh) != 1) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
    std::vector<unsigned char> buf((size_t)kCkptChunk * 8);
    const long long n = numpart;
    int rc;
    if ((rc = ckpt_put_array(fh, P.xt, n, buf)) || (rc = ckpt_put_array(fh, P.yt, n, buf))) return rc;
    for (R *a : {P.zt, P.up, P.vp, P.wp, P.us, P.vs, P.ws}) if ((rc = ckpt_put_array(fh, a, n, buf))) return rc;
    for (int *a : {P.idt, P.itra1, P.itramem, P.npoint, P.nclass, P.itrasplit}) if ((rc = ckpt_put_array(fh, a, n, buf))) return rc;
    if ((rc = ckpt_put_array(fh, P.cbt, n, buf))) return rc;
    for (int ks = 0; ks < cfg.nspec; ks++) if ((rc = ckpt_put_array(fh, P.xmass1 + (size_t)ks * P.cap, n, buf))) return rc;
    if (P.xscav) for (int ks = 0; ks < cfg.nspec; ks++) if ((rc = ckpt_put_array(fh, P.xscav + (size_t)ks * P.cap, n, buf))) return rc;
    if (h.n_grid3 && ((rc = ckpt_put_plain(fh, Gp.gridunc, n_grid3, buf)) || (rc = ckpt_put_plain(fh, Gp.drygridunc, n_grid2, buf)) ||
                      (rc = ckpt_put_plain(fh, Gp.wetgridunc, n_grid2, buf)))) return rc;
    if (h.n_grid3n && ((rc = ckpt_put_plain(fh, Gp.griduncn, n_grid3n, buf)) || (rc = ckpt_put_plain(fh, Gp.drygriduncn, n_grid2n, buf)) ||
                       (rc = ckpt_put_plain(fh, Gp.wetgriduncn, n_grid2n, buf)))) return rc;
    if (h.n_receptor && (rc = ckpt_put_plain(fh, Gp.creceptor, (size_t)h.n_receptor, buf))) return rc;
    if (h.cbase_bytes)
      for (int g = 0; g <= V.numbnests; g++)
        if (conv_cb[g] && (rc = ckpt_put_plain(fh, (const unsigned char *)conv_cb[g], conv_cb_bytes(g), buf))) return rc;
    if (h.reserved & kCkptFlux) {
      const uint64_t cnt = n_flux;
      if (fwrite(&cnt, 8, 1, fh) != 1) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
      if ((rc = ckpt_put_plain(fh, (const unsigned char *)fx_flux, n_flux * cfg.host_real_bytes, buf))) return rc;
    }
    if (h.reserved & kCkptPartavg) {
      const uint64_t cnt = (uint64_t)n;
      if (fwrite(&cnt, 8, 1, fh) != 1) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
      if ((rc = cfg.host_real_bytes == 4 ? ckpt_put_partavg<float>(fh, n, buf) : ckpt_put_partavg<double>(fh, n, buf))) return rc;
    }
    if (h.reserved & kCkptInitcond) {
      const uint64_t cnt = n_initcond;
      if (fwrite(&cnt, 8, 1, fh) != 1) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
      if ((rc = ckpt_put_plain(fh, (const unsigned char *)ic_grid, n_initcond * cfg.host_real_bytes, buf))) return rc;
    }
    if ((h.reserved & kCkptOh) && (rc = cfg.host_real_bytes == 4 ? ckpt_put_oh<float>(fh) : ckpt_put_oh<double>(fh))) return rc;
    if (closer.close() != 0) return fail(FPX_ERR_ARG, std::string("checkpoint_write: write error on ") + path);
    return 0;
  }

  int checkpoint_read(const char *path, int32_t *itime, int64_t *numpart_out, int32_t *numparticlecount) override {
    if (!path) return fail(FPX_ERR_ARG, "checkpoint_read: path is required");
    FILE *fh = fopen(path, "rb");
    if (!fh) return fail(FPX_ERR_ARG, std::string("checkpoint_read: cannot open ") + path);
    FileCloser closer(fh);
    CkptHeader h;
    if (fread(&h, sizeof(h), 1, fh) != 1 || memcmp(h.magic, "FPXCKPT1", 8) != 0 || h.version != 2)
      return fail(FPX_ERR_ARG, "checkpoint_read: not a checkpoint of this engine (version 2)");
    if (h.real_bytes != (int)sizeof(R) || h.nspec != cfg.nspec || h.rng_mode != cfg.rng_mode || h.rng_bytes != sizeof(CkptRng))
      return fail(FPX_ERR_ARG, "checkpoint_read: written with another precision, species count or random-number mode");
    if (h.numpart < 0 || h.numpart > P.cap) return fail(FPX_ERR_ARG, "checkpoint_read: more particles than storage spaces");
    if (h.particle_base != cfg.particle_base || h.seed != V.seed) return fail(FPX_ERR_ARG, "checkpoint_read: another shard or seed");
    const size_t n_grid3 = sum_grid.count(), n_grid2 = sum_dry.count(), n_grid3n = sum_gridn.count(), n_grid2n = sum_dryn.count();
    const uint64_t g3 = Gp.on ? n_grid3 : 0, g2 = Gp.on ? n_grid2 : 0, g3n = Gp.on && Gp.nested ? n_grid3n : 0, g2n = Gp.on && Gp.nested ? n_grid2n : 0;
    const uint64_t nr = Gp.creceptor ? (uint64_t)Gp.numreceptor * cfg.maxspec : 0;
    if (h.n_grid3 != g3 || h.n_grid2 != g2 || h.n_grid3n != g3n || h.n_grid2n != g2n || h.n_receptor != nr)
      return fail(FPX_ERR_STATE, "checkpoint_read: the output grids of the checkpoint are not the ones configured (call fpx_outgrid_init ... first)");
    if (h.cbase_bytes != conv_cbase_bytes())
      return fail(FPX_ERR_STATE, "checkpoint_read: the checkpoint was written with (without) convection; call fpx_conv_init first (or not at all)");
    {
      CkptHeader mine = h;
      ckpt_describe_grid(mine);
      if (memcmp(&mine.nx, &h.nx, (const char *)&h.pad - (const char *)&h.nx) != 0)
        return fail(FPX_ERR_ARG, "checkpoint_read: written on another grid (nx, ny, nz, maxspec or the nest extents differ)");
      if (mine.pad != h.pad) return fail(FPX_ERR_ARG, "checkpoint_read: written with (without) DRYBKDEP / WETBKDEP");
      // the whole file must be there before a single array is touched
      if ((h.reserved & ~(kCkptFlux | kCkptPartavg | kCkptInitcond | kCkptOh)) != 0) return fail(FPX_ERR_ARG, "checkpoint_read: unknown sections in the file");
      if (((h.reserved & kCkptInitcond) != 0) != (cfg.device_initcond && ic_grid))
        return fail(FPX_ERR_STATE, "checkpoint_read: the checkpoint was written with (without) device_initcond; create the engine alike and call fpx_outgrid_init first");
      if (((h.reserved & kCkptOh) != 0) != oh_on)
        return fail(FPX_ERR_STATE, "checkpoint_read: the checkpoint was written with (without) OH chemistry; call fpx_oh_init first (or not at all)");
      if (((h.reserved & kCkptPartavg) != 0) != (cfg.device_partavg != 0))
        return fail(FPX_ERR_STATE, "checkpoint_read: the checkpoint was written with (without) device_partavg; create the engine alike");
      if (((h.reserved & kCkptFlux) != 0) != (cfg.device_flux && fx_flux))
        return fail(FPX_ERR_STATE, "checkpoint_read: the checkpoint was written with (without) device_flux; create the engine alike and call fpx_outgrid_init first");
      if (h.total_bytes != ckpt_total_bytes(h) + ckpt_flux_bytes(h) + ckpt_partavg_bytes(h) + ckpt_initcond_bytes(h) + ckpt_oh_bytes(h))
        return fail((h.reserved & kCkptOh) ? FPX_ERR_STATE : FPX_ERR_ARG, (h.reserved & kCkptOh) ? "checkpoint_read: inconsistent header, or the OH grid of the checkpoint is not the one of fpx_oh_init" : "checkpoint_read: inconsistent header");
      if (fseek(fh, 0, SEEK_END) != 0) return fail(FPX_ERR_ARG, "checkpoint_read: cannot seek");
      const long long len = (long long)ftell(fh);
      if (len < 0 || (uint64_t)len != h.total_bytes)
        return fail(FPX_ERR_ARG, "checkpoint_read: the file is truncated or has trailing bytes (" + std::to_string(len) + " bytes, header says " + std::to_string(h.total_bytes) + "); nothing was restored");
      if (h.reserved & kCkptFlux) {
        uint64_t cnt = 0;
        if (fseek(fh, (long)ckpt_total_bytes(h), SEEK_SET) != 0 || fread(&cnt, 8, 1, fh) != 1) return fail(FPX_ERR_ARG, "checkpoint_read: cannot read the flux section");
        if (cnt != (uint64_t)n_flux) return fail(FPX_ERR_STATE, "checkpoint_read: the flux grid of the checkpoint is not the one configured");
      }
      if (fseek(fh, (long)sizeof(h), SEEK_SET) != 0) return fail(FPX_ERR_ARG, "checkpoint_read: cannot seek");
    }
    CkptRng rs;
    if (fread(&rs, sizeof(rs), 1, fh) != 1) return fail(FPX_ERR_ARG, "checkpoint_read: file too short");
    // storage spaces in particle-number order again
    HIPCHK(hipStreamSynchronize(stream));
    slot_of_pid = nullptr;
    slot_map_dirty = false;
    {
      const int nb = (int)((P.cap + kBlock - 1) / kBlock);
      k_iota_pid<<<nb, kBlock, 0, stream>>>(P.pid, 0, P.cap);
      k_fill<int><<<nb, kBlock, 0, stream>>>(P.itra1, kDead, 0, P.cap, nullptr);
      HIPCHK(hipGetLastError());
    }
    std::vector<unsigned char> buf((size_t)kCkptChunk * 8);
    const long long n = h.numpart;
    int rc;
    if ((rc = ckpt_get_array(fh, P.xt, n, buf)) || (rc = ckpt_get_array(fh, P.yt, n, buf))) return ckpt_invalidate(rc);
    for (R *a : {P.zt, P.up, P.vp, P.wp, P.us, P.vs, P.ws}) if ((rc = ckpt_get_array(fh, a, n, buf))) return ckpt_invalidate(rc);
    for (int *a : {P.idt, P.itra1, P.itramem, P.npoint, P.nclass, P.itrasplit}) if ((rc = ckpt_get_array(fh, a, n, buf))) return ckpt_invalidate(rc);
    if ((rc = ckpt_get_array(fh, P.cbt, n, buf))) return ckpt_invalidate(rc);
    for (int ks = 0; ks < cfg.nspec; ks++) if ((rc = ckpt_get_array(fh, P.xmass1 + (size_t)ks * P.cap, n, buf))) return ckpt_invalidate(rc);
    if (P.xscav) for (int ks = 0; ks < cfg.nspec; ks++) if ((rc = ckpt_get_array(fh, P.xscav + (size_t)ks * P.cap, n, buf))) return ckpt_invalidate(rc);
    if (g3 && ((rc = ckpt_get_plain(fh, Gp.gridunc, n_grid3, buf)) || (rc = ckpt_get_plain(fh, Gp.drygridunc, n_grid2, buf)) ||
               (rc = ckpt_get_plain(fh, Gp.wetgridunc, n_grid2, buf)))) return ckpt_invalidate(rc);
    if (g3n && ((rc = ckpt_get_plain(fh, Gp.griduncn, n_grid3n, buf)) || (rc = ckpt_get_plain(fh, Gp.drygriduncn, n_grid2n, buf)) ||
                (rc = ckpt_get_plain(fh, Gp.wetgriduncn, n_grid2n, buf)))) return ckpt_invalidate(rc);
    if (nr && (rc = ckpt_get_plain(fh, Gp.creceptor, (size_t)nr, buf))) return ckpt_invalidate(rc);
    if (h.cbase_bytes)
      for (int g = 0; g <= V.numbnests; g++)
        if (conv_cb[g] && (rc = ckpt_get_plain(fh, (unsigned char *)conv_cb[g], conv_cb_bytes(g), buf))) return ckpt_invalidate(rc);
    if (h.reserved & kCkptFlux) {
      uint64_t cnt = 0;
      if (fread(&cnt, 8, 1, fh) != 1) return ckpt_invalidate(fail(FPX_ERR_ARG, "checkpoint_read: file too short"));
      if ((rc = ckpt_get_plain(fh, (unsigned char *)fx_flux, n_flux * cfg.host_real_bytes, buf))) return ckpt_invalidate(rc);
      sum_flux.invalidate();                 // flux is the file's now
    }
    if (h.reserved & kCkptPartavg) {
      uint64_t cnt = 0;
      if (fread(&cnt, 8, 1, fh) != 1 || cnt != (uint64_t)n) return ckpt_invalidate(fail(FPX_ERR_ARG, "checkpoint_read: the section of the interval averages does not match the particle count"));
      if ((rc = cfg.host_real_bytes == 4 ? ckpt_get_partavg<float>(fh, n, buf) : ckpt_get_partavg<double>(fh, n, buf))) return ckpt_invalidate(rc);
    }
    if (h.reserved & kCkptInitcond) {
      uint64_t cnt = 0;
      if (fread(&cnt, 8, 1, fh) != 1 || cnt != (uint64_t)n_initcond) return ckpt_invalidate(fail(FPX_ERR_ARG, "checkpoint_read: the init_cond grid of the checkpoint is not the one configured"));
      if ((rc = ckpt_get_plain(fh, (unsigned char *)ic_grid, n_initcond * cfg.host_real_bytes, buf))) return ckpt_invalidate(rc);
      sum_ic.invalidate();                   // init_cond is the file's now
    }
    if ((h.reserved & kCkptOh) && (rc = cfg.host_real_bytes == 4 ? ckpt_get_oh<float>(fh) : ckpt_get_oh<double>(fh))) return ckpt_invalidate(rc);
    invalidate_grid_sums();
    rng4 = rs.r4; rng8 = rs.r8; rel_ran1 = rs.rel;
    step_counter = h.step_counter;
    rel_global_count = h.rel_global_count;
    numpart = n;
    maybe_new = true; births_unknown = true;
    if (itime) *itime = h.itime;
    if (numpart_out) *numpart_out = n;
    if (numparticlecount) *numparticlecount = h.numparticlecount;
    return 0;
  }

  // point_mod zpoint1, zpoint2(numpoint): the height range of a release, which WETBKDEP multiplies the scavenging
  // coefficient with (timemanager.f90:590-591)
  R *d_zspan = nullptr;
  int zspan_n = 0;
  int set_release_heights(int numpoint, const void *zpoint1, const void *zpoint2) override {
    if (numpoint < 1 || !zpoint1 || !zpoint2) return fail(FPX_ERR_ARG, "set_release_heights: numpoint >= 1, zpoint1 and zpoint2 are required");
    std::vector<R> z((size_t)numpoint);
    for (int i = 0; i < numpoint; i++)
      z[i] = cfg.host_real_bytes == 4 ? (R)(((const float *)zpoint2)[i] - ((const float *)zpoint1)[i]) : (R)(((const double *)zpoint2)[i] - ((const double *)zpoint1)[i]);
    int rc;
    if (numpoint > zspan_n) { if ((rc = dalloc(&d_zspan, (size_t)numpoint))) return rc; zspan_n = numpoint; }
    HIPCHK(hipMemcpyAsync(d_zspan, z.data(), (size_t)numpoint * sizeof(R), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  // point_mod xmass(numpoint,maxspec), npart(numpoint): device tables indexed by npoint(j)
  int set_release_points(int numpoint, const void *xmass, const int32_t *npart) override {
    if (numpoint < 1 || !xmass || !npart) return fail(FPX_ERR_ARG, "set_release_points: numpoint >= 1, xmass and npart are required");
    std::vector<R> xm((size_t)numpoint * cfg.nspec);
    std::vector<signed char> nsp((size_t)numpoint);
    for (int kp = 0; kp < numpoint; kp++) {
      // advance.f90:518-524: first species with xmass(nrelpoint,nsp) > eps3 = tiny(1.0) of the host's real kind, else nspec
      int pick = cfg.nspec - 1;
      for (int ks = cfg.nspec - 1; ks >= 0; ks--) {
        const size_t i = (size_t)ks * numpoint + kp;
        bool above;
        if (cfg.host_real_bytes == 4) { const float v = ((const float *)xmass)[i]; xm[i] = (R)v; above = v > 1.17549435e-38f; }
        else { const double v = ((const double *)xmass)[i]; xm[i] = (R)v; above = v > 2.2250738585072014e-308; }
        if (above) pick = ks;
      }
      nsp[kp] = (signed char)pick;
    }
    HIPCHK(hipStreamSynchronize(stream));
    R *d_x; int *d_n; signed char *d_s;
    int rc;
    if ((rc = dalloc(&d_x, xm.size())) || (rc = dalloc(&d_n, (size_t)numpoint)) || (rc = dalloc(&d_s, (size_t)numpoint))) return rc;
    HIPCHK(hipMemcpyAsync(d_x, xm.data(), xm.size() * sizeof(R), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_n, npart, (size_t)numpoint * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_s, nsp.data(), (size_t)numpoint, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    V.rel_xmass = d_x; V.rel_npart = d_n; V.rel_nsp = d_s; V.numpoint = numpoint;
    rel_xmass_h.resize(xm.size());
    for (size_t i = 0; i < xm.size(); i++) rel_xmass_h[i] = cfg.host_real_bytes == 4 ? (double)((const float *)xmass)[i] : ((const double *)xmass)[i];
    rel_npart_h.assign(npart, npart + numpoint);
    rel.set = false;         // the release tables refer to these points: fpx_release_init again
    return 0;
  }

  int set_numpart(long long n) override {
    if (n < 0 || n > P.cap) return fail(FPX_ERR_ARG, "set_numpart: outside capacity");
    if (n < numpart) { const int rc = restore_particle_order(); if (rc) return rc; }
    numpart = n;
    return 0;
  }

  int seed_particles(long long n, unsigned long long seed, double frac_pbl, double zmax, double lat_margin, int itime0) override {
    if (n < 1 || n > P.cap) return fail(FPX_ERR_ARG, "seed_particles: n outside capacity");
    if (!slot_loaded[0] || !slot_loaded[1]) return fail(FPX_ERR_STATE, "seed_particles: upload both field slots first (mixing heights are needed)");
    k_seed<R><<<(int)((n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(V, P, n, seed, frac_pbl, zmax, lat_margin, itime0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    slot_of_pid = nullptr;
    numpart = n;
    maybe_new = true; births_unknown = true;
    return 0;
  }

  // ---- TABLE_SEQ: per-step start indices in the reference's serial order -----
  int prepare_seq(int itime) {
    const long long n = numpart;
    int rc;
    if (!d_flags) {
      const size_t cap = (size_t)P.cap;
      if ((rc = dalloc(&d_flags, cap))) return rc;
      if ((rc = dalloc(&d_nrand_adv, cap))) return rc;
      if ((rc = dalloc(&d_nrand_init, cap))) return rc;
      if ((rc = dalloc(&d_dcas4, cap))) return rc;
      if ((rc = dalloc(&d_dcas14, cap))) return rc;
      if ((rc = dalloc(&d_dcas8, cap))) return rc;
      if ((rc = dalloc(&d_dcas18, cap))) return rc;
    }
    h_flags.resize(n); h_nrand_adv.assign(n, 1); h_nrand_init.assign(n, 1);
    h_dcas4.assign(n, 0.f); h_dcas14.assign(n, 0.f); h_dcas8.assign(n, 0.); h_dcas18.assign(n, 0.);
    k_classify<R><<<(int)((n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(V, P, n, itime, d_flags);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_flags.data(), d_flags, n, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    // walk the particles in index order exactly as the serial loop does
    // (timemanager.f90:531-611): [initialize: ran3 -> nrand, (ran3, gasdev)] then advance: ran3 -> nrand
    const bool h4 = cfg.host_real_bytes == 4;
    for (long long j = 0; j < n; j++) {
      unsigned char f = h_flags[j];
      if (!(f & 1)) continue;
      if (f & 2) {
        if (h4) {
          h_nrand_init[j] = rng4.start_index(rng4.idummy_init, V.maxrand);
          if (f & 4) { h_dcas4[j] = rng4.ran3(rng4.idummy_init); h_dcas14[j] = rng4.gasdev(rng4.idummy_init); }
        } else {
          h_nrand_init[j] = rng8.start_index(rng8.idummy_init, V.maxrand);
          if (f & 4) { h_dcas8[j] = rng8.ran3(rng8.idummy_init); h_dcas18[j] = rng8.gasdev(rng8.idummy_init); }
        }
      }
      h_nrand_adv[j] = h4 ? rng4.start_index(rng4.idummy_adv, V.maxrand) : rng8.start_index(rng8.idummy_adv, V.maxrand);
    }
    if (h4) for (long long j = 0; j < n; j++) { h_dcas8[j] = h_dcas4[j]; h_dcas18[j] = h_dcas14[j]; }
    else for (long long j = 0; j < n; j++) { h_dcas4[j] = (float)h_dcas8[j]; h_dcas14[j] = (float)h_dcas18[j]; }
    HIPCHK(hipMemcpyAsync(d_nrand_adv, h_nrand_adv.data(), n * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_nrand_init, h_nrand_init.data(), n * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_dcas4, h_dcas4.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_dcas14, h_dcas14.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_dcas8, h_dcas8.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(d_dcas18, h_dcas18.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }

  // ---- the step --------------------------------------------------------------
  int step(int itime, fpx_step_stats *out, bool async) override {
    if (!height_set || !window_set || !slot_loaded[0] || !slot_loaded[1]) return fail(FPX_ERR_STATE, "step: height, both field slots and the wind-time window must be set first");
    if (cfg.rng_mode != FPX_RNG_PHILOX && !table_set) return fail(FPX_ERR_STATE, "step: the table RNG modes need fpx_rng_fill_table/fpx_rng_set_table");
    if (V.memtime0 == V.memtime1) return fail(FPX_ERR_STATE, "step: empty wind-time window");
    if (cfg.wetbkdep && (!wet_on || !wet_slot[0] || !wet_slot[1])) return fail(FPX_ERR_STATE, "step: WETBKDEP needs the wet-deposition set-up (fpx_wet_init, fpx_upload_wet_fields for both slots)");
    if (cfg.wetbkdep && (!d_zspan || V.numpoint > zspan_n)) return fail(FPX_ERR_STATE, "step: WETBKDEP needs the release heights zpoint1, zpoint2 (fpx_set_release_heights)");
    if (cfg.drybkdep && !cfg.drydep) return fail(FPX_ERR_STATE, "step: DRYBKDEP without DRYDEP: there is no deposition velocity to take");
    if (V.numpoint == 0 && cfg.mdomainfill == 0 && cfg.mquasilag == 0)
      return fail(FPX_ERR_STATE, "step: the release-point tables xmass, npart are needed for the mass-fraction test (fpx_set_release_points)");
    for (int l = 0; l < V.numbnests; l++)
      if (!nest_loaded[l][0] || !nest_loaded[l][1]) return fail(FPX_ERR_STATE, "step: nest fields missing (fpx_upload_nest_fields, both slots)");
    if (cfg.device_flux && !Gp.on) return fail(FPX_ERR_STATE, "step: device_flux = 1 needs the output grid the fluxes are counted on (fpx_outgrid_init)");
    if (cfg.device_initcond && !ic_grid) return fail(FPX_ERR_STATE, "step: device_initcond = 1 needs the output grid init_cond is counted on (fpx_outgrid_init)");
    if (cfg.device_partavg)
      for (int i = 0; i < 9; i++)
        if (!diag_have[i]) return fail(FPX_ERR_STATE, "step: device_partavg = 1 needs oro, pv, qv, tt of both slots on the device (fpx_upload_diag_fields or fpx_verttransform_ecmwf)");
    if (out) memset(out, 0, sizeof(*out));
    if (numpart == 0) return 0;
    if (cfg.device_flux) { const int rc = flux_prepare(); if (rc) return rc; }
    if (cfg.device_partavg) { const int rc = partavg_prepare(); if (rc) return rc; }
    if (cfg.device_initcond) HIPCHK(ic_timer.begin(stream));
    if (cfg.drydep) { sum_dry.invalidate(); sum_dryn.invalidate(); }   // the step's dry deposition adds to drygridunc / drygriduncn
    if (cfg.sort_interval > 0 && step_counter > 0 && step_counter % (unsigned)cfg.sort_interval == 0) {
      int rc = sort_particles();
      if (rc) return rc;
    }
    SeqRng S;
    memset(&S, 0, sizeof(S));
    if (cfg.rng_mode == FPX_RNG_TABLE_SEQ) {
      int rc = prepare_seq(itime);
      if (rc) return rc;
      S.nrand_adv = d_nrand_adv; S.nrand_init = d_nrand_init;
      S.cbl_dcas = d_dcas4; S.cbl_dcas1 = d_dcas14; S.cbl_dcas_d = d_dcas8; S.cbl_dcas1_d = d_dcas18;
    }
    HIPCHK(step_timer.begin(stream));
    const Events<5> &ev = step_timer.current();
    const int nb = (int)((numpart + kBlock - 1) / kBlock);
    // the pass budgets of the Langevin kernel's launches (time slices, k_pbl_loop); the last launch has none
    if (slice_caps.empty()) {
      if (!opt.pbl_slices.empty()) slice_caps = opt.pbl_slices;
      else if (cfg.pbl_slice_passes < 0) slice_caps = {0};
      else if (cfg.pbl_slice_passes > 0) slice_caps = std::vector<int>(kMaxSlices - 1, cfg.pbl_slice_passes);
      else slice_caps = {FPX_SLICE_SCHEDULE};
      if ((int)slice_caps.size() > kMaxSlices - 1) slice_caps.resize(kMaxSlices - 1);
      if (slice_caps.empty() || slice_caps.back() != 0) slice_caps.push_back(0);
      if (slice_caps.size() > 1 && !d_surv[0]) {
        int rc;
        for (int k = 0; k < 2; k++) if ((rc = dalloc(&d_surv[k], (size_t)P.cap))) return rc;
      }
    }
    if (pbl_grid == 0) {
      // persistent grid: as many blocks as the chip holds at this kernel's register budget
      hipDeviceProp_t prop;
      HIPCHK(hipGetDeviceProperties(&prop, cfg.device));
      int per_cu = 0;
      HIPCHK(hipFuncSetAttribute((const void *)loop_kernel(), hipFuncAttributeMaxDynamicSharedMemorySize, (int)loop_smem_bytes()));
      HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, loop_kernel(), kBlock, loop_smem_bytes()));
      if (opt.pbl_blocks_per_cu > 0) per_cu = std::min(per_cu, opt.pbl_blocks_per_cu);   // experiments: fewer resident waves
      pbl_grid = prop.multiProcessorCount * std::max(per_cu, 1);
      if (opt.pbl_grid_blocks > 0) pbl_grid = std::min(pbl_grid, opt.pbl_grid_blocks);   // tests: a small cloud on few waves refills like a full-size one
      pbl_per_cu = std::max(per_cu, 1);
      if (opt.verbose) fprintf(stderr, "[fpx] Langevin kernel: %d blocks per CU by the occupancy query, %zu B of dynamic LDS, grid %d\n", per_cu, loop_smem_bytes(), pbl_grid);
    }
    {
      size_t need = 0;
      HIPCHK(rocprim::radix_sort_pairs(nullptr, need, d_pbl_flag, d_pbl_flag2, d_iota, d_pbl_list, (size_t)numpart, 0u, 6u, stream));
      HIPCHK(d_sel_tmp.reserve(need, stream));
    }
    HIPCHK(hipMemsetAsync(d_pbl_ctr, 0, kCtrWords * sizeof(unsigned int), stream));
    // Cost buckets in the work list (k_prep): pure scheduling, no effect on any result, so the rank's own particle count
    // may decide.  They pay where particles per grid cell are few -- the shard one of eight GPUs runs: -4.5 % of the
    // Langevin kernel at 1.25e7 particles -- and cost locality: at 1e8 on one GPU they gain under 1 % and take the kernel's
    // HBM traffic from 1.04 to 2.4 times the algorithmic bytes (the level-pair fetches of neighbouring list entries no
    // longer share cache lines).
    V.pbl_cost_buckets = opt.pbl_cost_buckets >= 0 ? opt.pbl_cost_buckets : (numpart < 50000000ll ? 3 : 0);
    { const int rc = blend_winds(itime); if (rc) return rc; }      // its own kernel (k_blend_w3), ahead of the per-kernel events
    // device_flux: k_flux_save must follow the receptor block, and fpx_kernel_times' first interval must not hold it -- the
    // interval then opens behind both (without device_flux the order is what it always was)
    if (!cfg.device_flux) HIPCHK(hipEventRecord(ev[0], stream));
    if (P.xscav) {   // timemanager.f90:564-598, before the particle is moved
      k_bkdep<R><<<nb, kBlock, 0, stream>>>(V, Wp, P, numpart, itime, cfg.drybkdep, cfg.wetbkdep, d_zspan);
      HIPCHK(hipGetLastError());
    }
    if (cfg.device_flux) {   // timemanager.f90:560-562 -- after the receptor block, which may zero xmass1 (:578,593)
      const int rc = cfg.host_real_bytes == 4 ? flux_launch<float>(false, itime) : flux_launch<double>(false, itime);
      if (rc) return rc;
      HIPCHK(hipEventRecord(ev[0], stream));
    }
    {
      // specialised variants: dry deposition (aerosols), initialize() only when new particles can
      // exist (after an upload/seed or at itime 0), polar maps only on grids with poles
      if (births_unknown) { const int rc = find_birth_horizon(); if (rc) return rc; }
      const bool init = maybe_new || itime == 0 || (long long)cfg.ldirect * itime <= birth_horizon || opt.prep_init_always;
      const bool polar = cfg.nglobal || cfg.sglobal;
      typedef void (*prep_fn)(View<R>, GridP<R>, Parts<R>, SeqRng, PblRec<R>, long long, int, unsigned int, Stats *, unsigned char *, unsigned int *);
      const bool nest = V.numbnests > 0;
      const prep_fn f = (prep_fn)step_kernel_prep((int)sizeof(R), cfg.drydep != 0, init, polar, nest);
      const int prep_pad = opt.prep_lds_pad;   // experiments: unused dynamic LDS lowers the occupancy
      if (prep_pad > 0) HIPCHK(hipFuncSetAttribute((const void *)f, hipFuncAttributeMaxDynamicSharedMemorySize, prep_pad));
      f<<<nb, kBlock, (size_t)prep_pad, stream>>>(V, Gp, P, S, Q, numpart, itime, step_counter, d_stats, d_pbl_flag, d_pbl_ctr);
      maybe_new = false;
    }
    HIPCHK(hipEventRecord(ev[4], stream));
    {
      // work list = slots stably sorted by the 6-bit key of k_prep: class, cost bucket (non-PBL slots, keys 32 and 33, end
      // up behind the d_pbl_ctr[0] entries that are used)
      size_t need = d_sel_tmp.bytes();
      HIPCHK(rocprim::radix_sort_pairs(d_sel_tmp.as(), need, d_pbl_flag, d_pbl_flag2, d_iota, d_pbl_list, (size_t)numpart, 0u, 6u, stream));
      k_list_counts<<<1, 64, 0, stream>>>(d_pbl_flag2, numpart, d_pbl_ctr, d_stats);
    }
    // (k_pbl_finish needs every lane of its waves in the dry-deposition scatter -- wave_kernel_add: whole blocks of kBlock, no early return)
    int fin_grid = std::min(nb, 8 * 256 * 4);
    if (opt.finish_blocks > 0) fin_grid = std::min(fin_grid, opt.finish_blocks);   // tests: several tiles / strides per wave
    HIPCHK(hipEventRecord(ev[1], stream));
    for (size_t j = 0; j < slice_caps.size(); j++) {
      // launch j works through the particles launch j-1 suspended (k_pbl_loop); a launch whose list is empty ends at once;
      // the last launch suspends nothing
      const bool last = j + 1 == slice_caps.size();
      const unsigned int *list = j == 0 ? d_pbl_list : d_surv[(j - 1) & 1];
      loop_kernel()<<<pbl_grid, kBlock, loop_smem_bytes(), stream>>>(V, P, Q, itime, step_counter, d_stats, list, d_pbl_ctr + kCtrBase + kCtrStride * j, last ? 0 : slice_caps[j],
                                                                     last ? 0 : drain_lanes(), d_surv[j & 1]);
    }
    HIPCHK(hipEventRecord(ev[2], stream));
    {
      const bool polar = cfg.nglobal || cfg.sglobal, nest = V.numbnests > 0;
      typedef void (*fin_fn)(View<R>, GridP<R>, Parts<R>, PblRec<R>, int, unsigned int, Stats *, const unsigned char *, long long, const unsigned int *, const unsigned int *);
      const fin_fn f = (fin_fn)step_kernel_finish((int)sizeof(R), cfg.drydep != 0, polar, nest);
      f<<<fin_grid, kBlock, 0, stream>>>(V, Gp, P, Q, itime, step_counter, d_stats, d_pbl_flag, numpart,
                                         V.pbl_cost_buckets ? (const unsigned int *)nullptr : d_pbl_list, d_pbl_ctr);
    }
    HIPCHK(hipEventRecord(ev[3], stream));
    step_timer.commit();      // the set's last event is in the stream: from here on it counts
    HIPCHK(hipGetLastError());
    if (cfg.device_flux) {   // timemanager.f90:623
      const int rc = cfg.host_real_bytes == 4 ? flux_launch<float>(true, itime) : flux_launch<double>(true, itime);
      if (rc) return rc;
    }
    V.w3t0 = nullptr; V.w3t1 = nullptr; V.r2t0 = nullptr;      // the blended packs belong to this step's itime only
    if (cfg.device_partavg) {   // timemanager.f90:617 -- the position after advance, the particles k_prep found due (its keys outlive the step)
      const int rc = cfg.host_real_bytes == 4 ? partavg_launch<float>(itime) : partavg_launch<double>(itime);
      if (rc) return rc;
    }
    if (cfg.device_initcond) {   // timemanager.f90:631,702 -- the particles the epilogue has just terminated
      const int rc = cfg.host_real_bytes == 4 ? initcond_launch<float>() : initcond_launch<double>();
      if (rc) return rc;
    }
    if (opt.verbose > 1) {   // the lists of the launches (a synchronisation per step: diagnostics only)
      unsigned int hc[kCtrWords];
      HIPCHK(hipMemcpyAsync(hc, d_pbl_ctr, sizeof(hc), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      fprintf(stderr, "[fpx] step %u: Langevin lists (per class)", step_counter);
      for (size_t j = 0; j < slice_caps.size(); j++) {
        const unsigned int *m = hc + kCtrBase + kCtrStride * j;
        fprintf(stderr, " | %u %u %u %u", m[0], m[1], m[2], m[3]);
      }
      fprintf(stderr, "\n");
    }
    step_counter++;
    if (async) return 0;
    Stats hs;
    HIPCHK(hipMemcpyAsync(&hs, d_stats, sizeof(Stats), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (out) {
      fill_stats(out, hs, snap);
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[3]));
      out->kernel_ms = ms;
    }
    snap = hs;
    return 0;
  }

  // device counters accumulate over steps; `snap`/`base` are host snapshots
  Stats snap{}, base{};
  static void fill_stats(fpx_step_stats *out, const Stats &a, const Stats &b) {
    out->n_due = (int64_t)(a.n_due - b.n_due); out->n_initialized = (int64_t)(a.n_init - b.n_init);
    out->n_left_domain = (int64_t)(a.n_left - b.n_left); out->n_min_mass = (int64_t)(a.n_minmass - b.n_minmass);
    out->n_max_age = (int64_t)(a.n_maxage - b.n_maxage); out->nan_count = (int64_t)(a.nan_count - b.nan_count);
    out->nan_count2 = (int64_t)(a.nan_count2 - b.nan_count2); out->n_bad_position = (int64_t)(a.n_badpos - b.n_badpos);
  }
  int lane_stats(uint64_t *out, int n, int reset) override {
    Stats hs;
    HIPCHK(hipMemcpyAsync(&hs, d_stats, sizeof(Stats), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int i = 0; i < n && i < 32; i++) out[i] = hs.lanes[i / 2][i % 2];
    if (reset) HIPCHK(hipMemsetAsync((char *)d_stats + offsetof(Stats, lanes), 0, sizeof(hs.lanes), stream));
    return 0;
  }
  int set_option(const char *name, const char *value) override {
    const std::string n(name), v(value);
    char *end = nullptr;
    const long iv = strtol(value, &end, 10);
    const bool is_int = end != value && *end == 0;
    auto need_int = [&](long lo) -> bool { return is_int && iv >= lo; };
    if (n == "verbose") { if (!need_int(0)) goto bad; opt.verbose = (int)iv; return 0; }
    if (n == "pbl_blocks_per_cu") { if (!need_int(0)) goto bad; opt.pbl_blocks_per_cu = (int)iv; pbl_grid = 0; return 0; }
    if (n == "pbl_grid_blocks") { if (!need_int(0)) goto bad; opt.pbl_grid_blocks = (int)iv; pbl_grid = 0; return 0; }
    if (n == "finish_blocks") { if (!need_int(0)) goto bad; opt.finish_blocks = (int)iv; return 0; }
    if (n == "prep_lds_pad") { if (!need_int(0) || iv > 160 * 1024) goto bad; opt.prep_lds_pad = (int)iv; return 0; }
    if (n == "vt_unfused") { if (!need_int(0)) goto bad; opt.vt_unfused = iv != 0; return 0; }
    if (n == "conv_scratch_mb") { if (!need_int(0)) goto bad; opt.conv_scratch_mb = iv; return 0; }
    if (n == "conv_one_lane") { if (!need_int(0)) goto bad; opt.conv_one_lane = iv != 0; return 0; }
    if (n == "conv_no_walk") { if (!need_int(0)) goto bad; opt.conv_no_walk = iv != 0; return 0; }
    if (n == "conv_rows_plain") { if (!need_int(0)) goto bad; opt.conv_rows_plain = iv != 0; return 0; }
    if (n == "pbl_cost_buckets") { if (!is_int || iv < -1 || iv > 3) goto bad; opt.pbl_cost_buckets = (int)iv; return 0; }   // -1 automatic, 0 none, 1: four buckets, 2: two, 3: eight
    if (n == "prep_init_always") { if (!need_int(0)) goto bad; opt.prep_init_always = iv != 0; return 0; }
    if (n == "pbl_drain_lanes") { if (!is_int || iv < -1 || iv > 64) goto bad; opt.pbl_drain_lanes = (int)iv; return 0; }
    if (n == "bdate") {   // com_mod bdate (julian date of the run's start): fpx_partoutput_average names its file by it
      char *e2 = nullptr;
      const double b = strtod(value, &e2);
      if (e2 == value || *e2 != 0 || !(b > 0.)) goto bad;
      pa_bdate = b; pa_bdate_set = true;
      return 0;
    }
    if (n == "permute") {
      if (v == "auto") opt.permute = 0; else if (v == "direct") opt.permute = 1; else if (v == "staged") opt.permute = 2; else goto bad;
      return 0;
    }
    if (n == "pbl_slices") {   // "48,96,0": pass budgets of the successive launches; "" = back to the configuration's
      std::vector<int> caps;
      const char *q = value;
      while (*q) {
        char *e2 = nullptr;
        const long c = strtol(q, &e2, 10);
        if (e2 == q || c < 0 || c > 1000000) goto bad;
        caps.push_back((int)c);
        q = e2;
        if (*q == ',') q++; else if (*q) goto bad;
      }
      if ((int)caps.size() > kMaxSlices - 1) goto bad;
      opt.pbl_slices = caps;
      slice_caps.clear();
      pbl_grid = 0;      // another instance of the kernel may run the next step
      return 0;
    }
  bad:
    return fail(FPX_ERR_ARG, "fpx_set_option: unknown option or malformed value: " + n + " = " + v);
  }
  int get_info(const char *name, int64_t *value) override {
    const std::string n(name);
    if (n == "time_blended_packs") *value = blend_on() ? 1 : 0;
    else if (n == "blended_steps") *value = (int64_t)blended_steps;
    else if (n == "pbl_launches_per_step") {
      if (!slice_caps.empty()) *value = (int64_t)slice_caps.size();
      else if (!opt.pbl_slices.empty()) *value = (int64_t)opt.pbl_slices.size() + (opt.pbl_slices.back() != 0 ? 1 : 0);
      else if (cfg.pbl_slice_passes < 0) *value = 1;
      else if (cfg.pbl_slice_passes > 0) *value = kMaxSlices;
      else { const int d[] = {FPX_SLICE_SCHEDULE}; *value = (int64_t)(sizeof(d) / sizeof(d[0])); }
    } else if (n == "pbl_grid") *value = pbl_grid;
    else if (n == "pbl_blocks_per_cu") *value = pbl_per_cu;
    else if (n == "plumetraj_sweep_us") *value = (int64_t)(pt_sweep_ms * 1000.);   // of the last fpx_plumetraj: its passes of clustering.f90:78-162
    else if (n == "domainfill_flux_us") *value = (int64_t)(dfl_stage_ms[0] * 1000.);
    else if (n == "domainfill_stage1_us") *value = (int64_t)(dfl_stage_ms[1] * 1000.);
    else if (n == "domainfill_cand_us") *value = (int64_t)(dfl_stage_ms[2] * 1000.);
    else if (n == "domainfill_place_us") *value = (int64_t)(dfl_stage_ms[3] * 1000.);
    else if (n == "domainfill_candidates") *value = dfl_last_ncand;
    else if (n == "conv_batches") *value = conv_last.valid ? conv_last.batches : -1;   // matrix batches of the last fpx_convmix
    else if (n == "plumetraj_sweeps") { int m = 0; for (int v : pt_rec_it) m = std::max(m, v); *value = m; }
    else if (n == "pbl_list_length") {   // the four class counts k_list_counts left for the first launch of the last step
      unsigned int hc[4] = {0u, 0u, 0u, 0u};
      if (step_counter > 0) {
        HIPCHK(hipMemcpyAsync(hc, d_pbl_ctr + kCtrBase, sizeof(hc), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
      }
      *value = (int64_t)hc[0] + hc[1] + hc[2] + hc[3];
    }
    else if (n == "oh_branch") *value = oh_branch;
    else if (n == "oh_skipped") {
      unsigned int c = 0;
      if (oh_on) {
        HIPCHK(hipMemcpyAsync(&c, oh_d_skipped, sizeof(c), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
      }
      *value = c;
    }
    else return fail(FPX_ERR_ARG, "fpx_get_info: unknown name: " + n);
    return 0;
  }
  int counters(fpx_step_stats *out, int reset) override {
    Stats hs;
    HIPCHK(hipMemcpyAsync(&hs, d_stats, sizeof(Stats), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (out) { memset(out, 0, sizeof(*out)); fill_stats(out, hs, base); }
    snap = hs;
    if (reset) base = hs;
    return 0;
  }

  // the Langevin kernel specialised for the run's switches (gases: LEAN) or the general one
  typedef void (*loop_fn)(View<R>, Parts<R>, PblRec<R>, int, unsigned int, Stats *, const unsigned int *, unsigned int *, int, int, unsigned int *);
  // The kernel instance of this engine: by the run's switches, and by whether a step is one launch or several (time slices);
  // the gas kernels -- LEAN instances, see loop_table -- leave the aerosol slots of the stash out of the block's LDS.
  bool loop_sliced() const {
    if (!slice_caps.empty()) return slice_caps.size() > 1;
    if (!opt.pbl_slices.empty()) return opt.pbl_slices.size() > 1 || opt.pbl_slices.back() != 0;
    if (cfg.pbl_slice_passes != 0) return cfg.pbl_slice_passes > 0;
    const int d[] = {FPX_SLICE_SCHEDULE};
    return sizeof(d) / sizeof(d[0]) > 1 || d[0] != 0;
  }
  loop_fn loop_kernel(bool *is_lean = nullptr) const {
    bool lean = false;
    const loop_fn f = (loop_fn)step_kernel_loop((int)sizeof(R), !cfg.drydep && !cfg.lsettling, cfg.turboff ? -1 : cfg.turbswitch, cfg.cblflag, cfg.rng_mode, loop_sliced(), &lean);
    if (is_lean) *is_lean = lean;
    return f;
  }
  size_t loop_smem_bytes() const {
    bool lean = false;
    (void)loop_kernel(&lean);
    return sizeof(R) * ((size_t)stash_slots<R>(lean, loop_sliced()) * kStashStride + (size_t)cfg.nz);
  }

  int sync() override {
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }

  int kernel_time(double *ms, long long *launches, int reset, double *parts) override {
    double t[5];
    HIPCHK(step_timer.read(stream, t, launches, reset != 0));
    if (ms) *ms = t[0];
    if (parts) for (int k = 0; k < 4; k++) parts[k] = t[1 + k];
    return 0;
  }

  Scratch d_sort_rec;
  unsigned long long *d_disorder = nullptr;
  bool last_permute_staged = false;
  int alloc_parts(Parts<R> &Q) {
    const size_t cap = (size_t)P.cap;
    int rc;
    memset(&Q, 0, sizeof(Q));
    Q.cap = P.cap;
    if ((rc = dalloc(&Q.xt, cap))) return rc;
    if ((rc = dalloc(&Q.yt, cap))) return rc;
    R **rs[] = {&Q.zt, &Q.up, &Q.vp, &Q.wp, &Q.us, &Q.vs, &Q.ws};
    for (auto q : rs) if ((rc = dalloc(q, cap))) return rc;
    int **is[] = {&Q.idt, &Q.itra1, &Q.itramem, &Q.npoint, &Q.nclass, &Q.itrasplit};
    for (auto q : is) if ((rc = dalloc(q, cap))) return rc;
    if ((rc = dalloc(&Q.cbt, cap))) return rc;
    if ((rc = dalloc(&Q.xmass1, cap * cfg.nspec))) return rc;
    if (P.xscav) {
      if ((rc = dalloc(&Q.xscav, cap * cfg.nspec))) return rc;
      k_fill<R><<<(int)((cap * cfg.nspec + kBlock - 1) / kBlock), kBlock, 0, stream>>>(Q.xscav, (R)-1, 0, (long long)(cap * cfg.nspec), nullptr);
    }
    if ((rc = dalloc(&Q.pid, cap))) return rc;
    {   // zeroed like the first set (storage spaces behind numpart keep their contents across the ping-pong)
      R *rz[] = {Q.zt, Q.up, Q.vp, Q.wp, Q.us, Q.vs, Q.ws};
      for (R *q : rz) HIPCHK(hipMemsetAsync(q, 0, cap * sizeof(R), stream));
      HIPCHK(hipMemsetAsync(Q.xt, 0, cap * sizeof(double), stream));
      HIPCHK(hipMemsetAsync(Q.yt, 0, cap * sizeof(double), stream));
      HIPCHK(hipMemsetAsync(Q.xmass1, 0, cap * cfg.nspec * sizeof(R), stream));
      int *iz[] = {Q.idt, Q.itramem, Q.npoint, Q.nclass, Q.itrasplit};
      for (int *q : iz) HIPCHK(hipMemsetAsync(q, 0, cap * sizeof(int), stream));
      HIPCHK(hipMemsetAsync(Q.cbt, 0, cap * sizeof(short), stream));
    }
    return 0;
  }

  // The locality sort permutes the storage spaces 1..numpart among themselves; an operation that SHRINKS numpart (the
  // sender of a redistribution, fpx_set_numpart) must first put every particle back into the space of its number, or the
  // spaces beyond the new numpart would still hold live particles.
  int restore_particle_order() {
    if (!slot_of_pid) return 0;
    return sort_impl(true);
  }
  int sort_particles() override {
    if (!height_set) return fail(FPX_ERR_STATE, "sort_particles: set_height first");
    return sort_impl(false);
  }
  int sort_impl(bool by_pid) {
    const long long n = numpart;
    if (n < 2) { if (by_pid) slot_of_pid = nullptr; return 0; }
    int rc;
    if (!have_p2) {
      if ((rc = alloc_parts(P2))) return rc;
      const size_t cap = (size_t)P.cap;
      if ((rc = dalloc(&d_keys, cap))) return rc;
      if ((rc = dalloc(&d_keys2, cap))) return rc;
      if ((rc = dalloc(&d_vals, cap))) return rc;
      if ((rc = dalloc(&d_vals2, cap))) return rc;
      if ((rc = dalloc(&d_slot_of_pid, cap))) return rc;
      if ((rc = dalloc(&d_disorder, (size_t)1))) return rc;
      have_p2 = true;
    }
    const unsigned long long nkeys = (unsigned long long)cfg.nx * cfg.ny * cfg.nz + 1ull;
    if (nkeys > 0xFFFFFFFFull) return fail(FPX_ERR_UNSUPPORTED, "sort_particles: grid too large for 32-bit keys");
    unsigned int bits = 1;
    while ((1ull << bits) < (by_pid ? (unsigned long long)n : nkeys) + 1ull) bits++;
    const int nb = (int)((n + kBlock - 1) / kBlock);
    if (by_pid) k_sort_keys_pid<<<nb, kBlock, 0, stream>>>(P.pid, n, d_keys, d_vals);
    else k_sort_keys<R><<<nb, kBlock, 0, stream>>>(V, P, n, d_keys, d_vals, (unsigned int)(nkeys - 1ull));
    HIPCHK(hipGetLastError());
    size_t need = 0;
    HIPCHK(rocprim::radix_sort_pairs(nullptr, need, d_keys, d_keys2, d_vals, d_vals2, (size_t)n, 0u, bits, stream));
    HIPCHK(d_sort_tmp.reserve(need, stream));
    HIPCHK(rocprim::radix_sort_pairs(d_sort_tmp.as(), need, d_keys, d_keys2, d_vals, d_vals2, (size_t)n, 0u, bits, stream));
    // which gather: by the locality of the permutation (fpx_set_option "permute" = direct|staged overrides, for tests)
    bool staged = false;
    {
      if (opt.permute == 2) staged = true;
      else if (opt.permute != 1 && n >= (1 << 16)) {
        HIPCHK(hipMemsetAsync(d_disorder, 0, sizeof(unsigned long long), stream));
        k_perm_disorder<<<std::min(nb, 4096), kBlock, 0, stream>>>(d_vals2, n, 1u << 14, d_disorder);
        unsigned long long far = 0;
        HIPCHK(hipMemcpyAsync(&far, d_disorder, sizeof(far), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        staged = far * 2ull > (unsigned long long)n;
      }
    }
    last_permute_staged = staged;
    if (staged) {
      HIPCHK(d_sort_rec.reserve((size_t)n * sizeof(SortRecord<R>), stream));
      k_permute_pack<R><<<nb, kBlock, 0, stream>>>(P, d_sort_rec.as<SortRecord<R>>(), n);
      k_permute_unpack<R><<<nb, kBlock, 0, stream>>>(d_sort_rec.as<SortRecord<R>>(), P, P2, d_vals2, n, cfg.nspec);
      // 12.8 GB at 1e8 particles, needed once in a run: give it back
      HIPCHK(d_sort_rec.release(stream));
    } else {
      const int tiles_per_xcd = (nb + 7) / 8;
      k_permute<R, 0><<<8 * tiles_per_xcd, kBlock, 0, stream>>>(P, P2, d_vals2, n, cfg.nspec, tiles_per_xcd);
      k_permute<R, 1><<<8 * tiles_per_xcd, kBlock, 0, stream>>>(P, P2, d_vals2, n, cfg.nspec, tiles_per_xcd);
      k_permute<R, 2><<<8 * tiles_per_xcd, kBlock, 0, stream>>>(P, P2, d_vals2, n, cfg.nspec, tiles_per_xcd);
      k_permute<R, 3><<<8 * tiles_per_xcd, kBlock, 0, stream>>>(P, P2, d_vals2, n, cfg.nspec, tiles_per_xcd);
    }
    HIPCHK(hipGetLastError());
    if (cfg.device_partavg) {   // the sums move with their particle (perm = d_vals2, the same for both gathers)
      if (!pa_n[1] && (rc = partavg_alloc(1))) return rc;
      if (cfg.host_real_bytes == 4) pa::k_partavg_permute<float><<<(int)((P.cap + 255) / 256), 256, 0, stream>>>(partavg_state<float>(pa_cur), partavg_state<float>(pa_cur ^ 1), d_vals2, n);
      else pa::k_partavg_permute<double><<<(int)((P.cap + 255) / 256), 256, 0, stream>>>(partavg_state<double>(pa_cur), partavg_state<double>(pa_cur ^ 1), d_vals2, n);
      HIPCHK(hipGetLastError());
      pa_cur ^= 1;
    }
    // slots >= n keep their (dead) contents in both sets; swap roles
    std::swap(P, P2);
    if (n < P.cap) {
      // the untouched tail of the new front set must also be dead and identity-numbered
      const long long rest = P.cap - n;
      const int nbr = (int)((rest + kBlock - 1) / kBlock);
      k_fill<int><<<nbr, kBlock, 0, stream>>>(P.itra1, kDead, n, rest, nullptr);
      k_iota_pid<<<nbr, kBlock, 0, stream>>>(P.pid, n, rest);
      HIPCHK(hipGetLastError());
    }
    slot_of_pid = by_pid ? nullptr : d_slot_of_pid;      // back in particle-number order: the identity again
    slot_map_dirty = !by_pid;
    return 0;
  }

  // ---- output grids -----------------------------------------------------------
  int outgrid_init(const fpx_outgrid *g, const void *outheight) override {
    if (!g || !outheight) return fail(FPX_ERR_ARG, "outgrid_init: null argument");
    if (g->struct_bytes != (int32_t)sizeof(fpx_outgrid)) return fail(FPX_ERR_ARG, "outgrid_init: fpx_outgrid size mismatch (ABI)");
    if (g->numxgrid < 1 || g->numygrid < 1 || g->numzgrid < 1 || g->numzgrid > kMaxNz) return fail(FPX_ERR_ARG, "outgrid_init: bad grid extents");
    if (g->maxpointspec_act < 1 || g->nclassunc < 1 || g->nageclass < 1 || g->nageclass > kMaxAge) return fail(FPX_ERR_ARG, "outgrid_init: bad maxpointspec_act/nclassunc/nageclass");
    if (Gp.on) return fail(FPX_ERR_STATE, "outgrid_init: already initialised");
    Gp.numxgrid = g->numxgrid; Gp.numygrid = g->numygrid; Gp.numzgrid = g->numzgrid;
    Gp.maxspec = cfg.maxspec; Gp.maxpointspec_act = g->maxpointspec_act; Gp.nclassunc = g->nclassunc; Gp.nageclass = g->nageclass;
    for (int i = 0; i < kMaxAge; i++) Gp.lage[i] = i < g->nageclass ? g->lage[i] : 0x7fffffff;
    Gp.dxout = (R)g->dxout; Gp.dyout = (R)g->dyout; Gp.xoutshift = (R)g->xoutshift; Gp.youtshift = (R)g->youtshift;
    Gp.ind_samp = g->ind_samp; Gp.ioutputforeachrelease = g->ioutputforeachrelease; Gp.lusekerneloutput = g->lusekerneloutput;
    Gp.loutnext = 0; Gp.loutstep = 0;
    const size_t n_grid2 = (size_t)g->numxgrid * g->numygrid * cfg.maxspec * g->maxpointspec_act * g->nclassunc * g->nageclass;
    const size_t n_grid3 = n_grid2 * g->numzgrid;
    sum_grid.shape(n_grid3, sizeof(R)); sum_dry.shape(n_grid2, sizeof(float)); sum_wet.shape(n_grid2, sizeof(float));
    int rc;
    R *oh;
    if ((rc = dalloc(&oh, g->numzgrid))) return rc;
    std::vector<R> tmp(g->numzgrid);
    for (int k = 0; k < g->numzgrid; k++) tmp[k] = cfg.host_real_bytes == 4 ? (R)((const float *)outheight)[k] : (R)((const double *)outheight)[k];
    HIPCHK(hipMemcpyAsync(oh, tmp.data(), g->numzgrid * sizeof(R), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    Gp.outheight = oh;
    if ((rc = dalloc(&Gp.gridunc, n_grid3))) return rc;
    if ((rc = dalloc(&Gp.drygridunc, n_grid2))) return rc;
    if ((rc = dalloc(&Gp.wetgridunc, n_grid2))) return rc;
    HIPCHK(hipMemsetAsync(Gp.wetgridunc, 0, n_grid2 * sizeof(float), stream));
    HIPCHK(hipMemsetAsync(Gp.gridunc, 0, n_grid3 * sizeof(R), stream));
    HIPCHK(hipMemsetAsync(Gp.drygridunc, 0, n_grid2 * sizeof(float), stream));
    HIPCHK(hipStreamSynchronize(stream));
    Gp.nested = 0; Gp.numreceptor = 0;
    if (cfg.device_flux) {
      rc = cfg.host_real_bytes == 4 ? flux_init_t<float>(g, outheight) : flux_init_t<double>(g, outheight);
      if (rc) return rc;
    }
    if (cfg.device_initcond) {
      rc = cfg.host_real_bytes == 4 ? initcond_init_t<float>(g, outheight) : initcond_init_t<double>(g, outheight);
      if (rc) return rc;
    }
    Gp.on = 1;
    return 0;
  }
  // nested output grid: readoutgrid_nest.f90, outgrid_init_nest.f90 (same levels, classes, species as the mother grid)
  int outgrid_nest_init(const fpx_outgrid_nest *g) override {
    if (!g || g->struct_bytes != (int32_t)sizeof(fpx_outgrid_nest)) return fail(FPX_ERR_ARG, "outgrid_nest_init: null or fpx_outgrid_nest size mismatch (ABI)");
    if (!Gp.on) return fail(FPX_ERR_STATE, "outgrid_nest_init: fpx_outgrid_init first");
    if (Gp.nested) return fail(FPX_ERR_STATE, "outgrid_nest_init: already initialised");
    if (g->numxgridn < 1 || g->numygridn < 1 || !(g->dxoutn > 0) || !(g->dyoutn > 0)) return fail(FPX_ERR_ARG, "outgrid_nest_init: bad grid");
    Gp.numxgridn = g->numxgridn; Gp.numygridn = g->numygridn;
    Gp.dxoutn = (R)g->dxoutn; Gp.dyoutn = (R)g->dyoutn; Gp.xoutshiftn = (R)g->xoutshiftn; Gp.youtshiftn = (R)g->youtshiftn;
    const size_t n_grid2n = (size_t)g->numxgridn * g->numygridn * Gp.maxspec * Gp.maxpointspec_act * Gp.nclassunc * Gp.nageclass;
    const size_t n_grid3n = n_grid2n * Gp.numzgrid;
    sum_gridn.shape(n_grid3n, sizeof(R)); sum_dryn.shape(n_grid2n, sizeof(float)); sum_wetn.shape(n_grid2n, sizeof(float));
    int rc;
    if ((rc = dalloc(&Gp.griduncn, n_grid3n))) return rc;
    if ((rc = dalloc(&Gp.drygriduncn, n_grid2n))) return rc;
    if ((rc = dalloc(&Gp.wetgriduncn, n_grid2n))) return rc;
    HIPCHK(hipMemsetAsync(Gp.griduncn, 0, n_grid3n * sizeof(R), stream));
    HIPCHK(hipMemsetAsync(Gp.drygriduncn, 0, n_grid2n * sizeof(float), stream));
    HIPCHK(hipMemsetAsync(Gp.wetgriduncn, 0, n_grid2n * sizeof(float), stream));
    HIPCHK(hipStreamSynchronize(stream));
    Gp.nested = 1;
    return 0;
  }
  int download_real(void *host, const R *dev, size_t n) {   // device R -> host real kind
    if (!host) return 0;
    if ((size_t)cfg.host_real_bytes == sizeof(R)) {
      HIPCHK(hipMemcpyAsync(host, dev, n * sizeof(R), hipMemcpyDeviceToHost, stream));
      return 0;
    }
    HIPCHK(staging.reserve(n * cfg.host_real_bytes, stream));
    const int nb = (int)((n + kBlock - 1) / kBlock);
    k_convert<R><<<nb, kBlock, 0, stream>>>(dev, cfg.host_real_bytes == 8 ? staging.as<double>() : nullptr,
                                            cfg.host_real_bytes == 4 ? staging.as<float>() : nullptr, (long long)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(host, staging.as(), n * cfg.host_real_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));   // staging is reused
    return 0;
  }
  int get_grids_nest(void *griduncn, void *drygriduncn, void *wetgriduncn, int allreduce, int clear) override {
    if (!Gp.nested) return fail(FPX_ERR_STATE, "get_grids_nest: fpx_outgrid_nest_init first");
    // mpi_mod.f90:2543-2569 (mpif_tm_reduce_grid_nest): into the receive buffers, the partial sums stay.
    // concoutput_nest.f90 zeroes griduncn only; drygriduncn / wetgriduncn accumulate over the run
    return fetch({{&sum_gridn, Gp.griduncn, griduncn, true, clear != 0}, {&sum_dryn, Gp.drygriduncn, drygriduncn, false, false},
                  {&sum_wetn, Gp.wetgriduncn, wetgriduncn, false, false}}, allreduce, "get_grids_nest");
  }
  // receptor points: xreceptor, yreceptor (grid coordinates), receptorarea, readreceptors.f90:88-92
  int receptors_init(int n, const void *x, const void *y, const void *area) override {
    if (!Gp.on) return fail(FPX_ERR_STATE, "receptors_init: fpx_outgrid_init first");
    if (n < 1 || n > 1000 || !x || !y || !area) return fail(FPX_ERR_ARG, "receptors_init: bad argument");
    if (Gp.numreceptor) return fail(FPX_ERR_STATE, "receptors_init: already initialised");
    std::vector<R> tmp(3 * (size_t)n);
    const void *src[3] = {x, y, area};
    for (int k = 0; k < 3; k++)
      for (int i = 0; i < n; i++) tmp[(size_t)k * n + i] = cfg.host_real_bytes == 4 ? (R)((const float *)src[k])[i] : (R)((const double *)src[k])[i];
    int rc;
    R *d;
    if ((rc = dalloc(&d, 3 * (size_t)n))) return rc;
    HIPCHK(hipMemcpyAsync(d, tmp.data(), tmp.size() * sizeof(R), hipMemcpyHostToDevice, stream));
    if ((rc = dalloc(&Gp.creceptor, (size_t)n * cfg.maxspec))) return rc;
    HIPCHK(hipMemsetAsync(Gp.creceptor, 0, (size_t)n * cfg.maxspec * sizeof(R), stream));
    HIPCHK(hipStreamSynchronize(stream));
    Gp.receptor = d;
    Gp.numreceptor = n;
    sum_rec.shape((size_t)n * cfg.nspec, sizeof(R));      // the columns of the species in use
    return 0;
  }
  // creceptor(ld, maxspec) of the host (com_mod.f90:660): rows 1..numreceptor, columns 1..nspec are written
  int get_receptors(void *creceptor, int ld, int allreduce, int clear) override {
    if (!Gp.numreceptor) return fail(FPX_ERR_STATE, "get_receptors: fpx_receptors_init first");
    if (creceptor && ld < Gp.numreceptor) return fail(FPX_ERR_ARG, "get_receptors: leading dimension smaller than numreceptor");
    // mpi_mod.f90:2480-2484, into creceptor0; fetched densely in the host's kind, then column by column into the host's array
    const size_t col = (size_t)Gp.numreceptor * cfg.host_real_bytes;
    std::vector<unsigned char> tmp(creceptor ? col * cfg.nspec : 0);
    const int rc = fetch({{&sum_rec, Gp.creceptor, creceptor ? tmp.data() : nullptr, true, clear != 0}}, allreduce, "get_receptors");
    if (rc) return rc;
    for (int ks = 0; creceptor && ks < cfg.nspec; ks++)
      memcpy((unsigned char *)creceptor + (size_t)ks * ld * cfg.host_real_bytes, tmp.data() + ks * col, col);
    return 0;
  }
  int set_output_times(int loutnext, int loutstep) override {
    Gp.loutnext = loutnext; Gp.loutstep = loutstep;
    return 0;
  }
  int conccalc(int itime, double weight) override {
    if (!Gp.on) return fail(FPX_ERR_STATE, "conccalc: fpx_outgrid_init first");
    if (!height_set || (Gp.ind_samp == -1 && (!slot_loaded[0] || !slot_loaded[1]))) return fail(FPX_ERR_STATE, "conccalc: height / fields not set");
    if (numpart == 0) return 0;
    const int nb = (int)((numpart + kBlock - 1) / kBlock);
    sum_grid.invalidate(); sum_gridn.invalidate(); sum_rec.invalidate();   // k_conccalc adds to gridunc, griduncn and creceptor: earlier reductions are stale
    // (wave_kernel_add needs every lane of the wave: whole blocks of kBlock, no early return in the kernel)
    k_conccalc<R><<<nb, kBlock, 0, stream>>>(V, Gp, P, numpart, itime, (R)weight);
    HIPCHK(hipGetLastError());
    return 0;
  }
  // sum over the ranks of `send` into `recv` (device pointers, distinct buffers), on the handle's stream
  // n floats (elem = 4) or doubles (elem = 8)
  int reduce_into(const void *send, void *recv, size_t n, size_t elem, const char *who) {
    if (comm) {
      ncclResult_t r = ncclAllReduce(send, recv, n, elem == 8 ? ncclDouble : ncclFloat, ncclSum, comm, stream);
      if (r != ncclSuccess) return fail(FPX_ERR_DEVICE, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
      return 0;
    }
    const size_t bytes = n * elem;
    HIPCHK(red_pin.reserve(2 * bytes, stream));
    HIPCHK(hipMemcpyAsync(red_pin.as(), send, bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (host_allreduce(host_allreduce_user, red_pin.as(), red_pin.as<char>() + bytes, (int64_t)n, elem == 8 ? 1 : 0) != 0)
      return fail(FPX_ERR_DEVICE, std::string(who) + ": the host's all-reduce callback failed");
    HIPCHK(hipMemcpyAsync(recv, red_pin.as<char>() + bytes, bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));    // the bounce buffer is reused by the next grid
    return 0;
  }
  // The three things the getters and the writers do with an accumulator's sums over the ranks (RankSum, fpx_host_res.hpp).
  // reduce: the sums of the partial sums as they are now, into the receive buffer.  What makes them stale again is said
  // where it happens: the invalidate() calls next to the launches that add to an accumulator, to its zeroing by
  // fluxoutput, and to a restored checkpoint.
  int reduce(RankSum &s, const void *partial, const char *who) {
    if (!comm && !host_allreduce) return fail(FPX_ERR_STATE, std::string(who) + ": allreduce requested without fpx_comm_init / fpx_comm_init_host");
    const hipError_t e = s.reserve();
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    const int rc = reduce_into(partial, s.recv(), s.count(), s.elem(), who);
    if (!rc) s.filled();
    return rc;
  }
  // source: what the writer `who` writes -- the rank's own partial sums, or with reduced = 1 on several ranks the sums that
  // `getter` (allreduce = 1) left in the receive buffer, provided nothing has been added to the partial sums since
  int source(const RankSum &s, const void *partial, int reduced, const char *who, const char *getter, const void **src) {
    *src = partial;
    if (!reduced || comm_ranks == 1) return 0;
    if (!s.valid()) return fail(FPX_ERR_STATE, std::string(who) + ": reduced = 1 needs " + getter + " with allreduce = 1 first");
    *src = s.recv();
    return 0;
  }
  // fetch: the path of the getters.  All accumulators of the call are reduced first if that is asked (on one rank there
  // is nothing to reduce), then each is downloaded -- in the host's real kind (as_real: an array of R) or as it is; a null
  // host pointer still reduces -- and zeroed if the getter clears it; one synchronisation.
  struct Fetch { RankSum *sum; void *partial; void *host; bool as_real, clear; };
  int fetch(std::initializer_list<Fetch> accs, int allreduce, const char *who) {
    const bool reduced = allreduce && comm_ranks > 1;
    int rc;
    for (const Fetch &a : accs)
      if (reduced && (rc = reduce(*a.sum, a.partial, who))) return rc;
    for (const Fetch &a : accs) {
      const void *src = reduced ? a.sum->recv() : a.partial;
      if (a.as_real) { if ((rc = download_real(a.host, (const R *)src, a.sum->count()))) return rc; }
      else if (a.host) HIPCHK(hipMemcpyAsync(a.host, src, a.sum->bytes(), hipMemcpyDeviceToHost, stream));
    }
    for (const Fetch &a : accs)
      if (a.clear) HIPCHK(hipMemsetAsync(a.partial, 0, a.sum->bytes(), stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  // [live particles, numpart] of this rank and summed over the ranks: the reduction of numpart the reference's root does at
  // every output time (timemanager_mpi.f90:552-562) -- here with the count of the particles that are still alive next to it
  long long *d_count = nullptr;          // [0..1] local, [2..3] sums
  int count_particles(int64_t *local, int64_t *total, int allreduce) override {
    int rc;
    if (!d_count && (rc = dalloc(&d_count, 4))) return rc;
    HIPCHK(hipMemsetAsync(d_count, 0, 4 * sizeof(long long), stream));
    if (numpart > 0) {
      const int nb = (int)std::min<long long>((numpart + 255) / 256, 256 * 16);
      k_count_live<<<nb, 256, 0, stream>>>(P.itra1, numpart, (unsigned long long *)d_count);
      HIPCHK(hipGetLastError());
    }
    long long h[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(h, d_count, sizeof(long long), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    h[1] = numpart;
    h[2] = h[0]; h[3] = h[1];
    if (allreduce && comm_ranks > 1) {
      if (comm) {
        HIPCHK(hipMemcpyAsync(d_count, h, 2 * sizeof(long long), hipMemcpyHostToDevice, stream));
        ncclResult_t r = ncclAllReduce(d_count, d_count + 2, 2, ncclInt64, ncclSum, comm, stream);
        if (r != ncclSuccess) return fail(FPX_ERR_DEVICE, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
        HIPCHK(hipMemcpyAsync(h + 2, d_count + 2, 2 * sizeof(long long), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
      } else if (host_allreduce) {
        double snd[2] = {(double)h[0], (double)h[1]}, rcv[2] = {0, 0};   // exact below 2^53
        if (host_allreduce(host_allreduce_user, snd, rcv, 2, 1) != 0) return fail(FPX_ERR_DEVICE, "count_particles: the host's all-reduce callback failed");
        h[2] = (long long)rcv[0]; h[3] = (long long)rcv[1];
      } else {
        return fail(FPX_ERR_STATE, "count_particles: allreduce requested without fpx_comm_init / fpx_comm_init_host");
      }
    }
    if (local) { local[0] = h[0]; local[1] = h[1]; }
    if (total) { total[0] = h[2]; total[1] = h[3]; }
    return 0;
  }
  int comm_init_host(int nranks, int rank, fpx_allreduce_fn fn, void *user) override {
    if (nranks < 1 || rank < 0 || rank >= nranks || !fn) return fail(FPX_ERR_ARG, "comm_init_host: bad argument");
    if (comm || host_allreduce) return fail(FPX_ERR_STATE, "comm_init_host: communicator exists");
    host_allreduce = fn; host_allreduce_user = user;
    comm_ranks = nranks; comm_rank = rank;
    return 0;
  }
  int comm_init(const void *id, int nbytes, int nranks, int rank) override {
    if (!id || nbytes != (int)sizeof(ncclUniqueId) || nranks < 1 || rank < 0 || rank >= nranks) return fail(FPX_ERR_ARG, "comm_init: bad argument");
    if (comm || host_allreduce) return fail(FPX_ERR_STATE, "comm_init: communicator exists");
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    HIPCHK(hipSetDevice(cfg.device));
    ncclResult_t r = ncclCommInitRank(&comm, nranks, uid, rank);
    if (r != ncclSuccess) return fail(FPX_ERR_DEVICE, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    comm_ranks = nranks; comm_rank = rank;
    return 0;
  }
  int get_grids(void *gridunc, void *drygridunc, int allreduce, int clear) override {
    if (!Gp.on) return fail(FPX_ERR_STATE, "get_grids: fpx_outgrid_init first");
    // the one collective of the path (mpi_mod.f90:2471-2492): the sums land in gridunc0 / drygridunc0, the partial sums
    // stay where they are -- drygridunc keeps accumulating and is reduced again at the next output.
    // concoutput.f90:719-720 zeroes gridunc (and creceptor: fpx_get_receptors) only; the deposition grids are
    // cumulative over the run (zeroed once, outgrid_init.f90:317-318)
    return fetch({{&sum_grid, Gp.gridunc, gridunc, true, clear != 0}, {&sum_dry, Gp.drygridunc, drygridunc, false, false}}, allreduce, "get_grids");
  }

  // ---- gross mass fluxes (fpx_calcfluxes.hpp; fpx_config.device_flux) ------------------------------------------
  // flux and everything the kernels compare a position with are kept in the host's real kind H, whatever the engine
  // computes in: calcfluxes.f90 declares them default real.
  void *fx_flux = nullptr;                             // flux_mod's flux (its sums over the ranks: sum_flux)
  void *fx_outh = nullptr, *fx_outhh = nullptr;        // outheight, outheighthalf in H
  void *fx_xold = nullptr, *fx_yold = nullptr, *fx_zold = nullptr, *fx_mass = nullptr;
  unsigned char *fx_due = nullptr;
  size_t n_flux = 0;
  double fx_geo[4] = {};                               // dxout, dyout, xoutshift, youtshift as the host passed them
  IntervalTimer<4> fx_timer{{0, 1}, {2, 3}};           // around k_flux_save | around k_calcfluxes
  template <typename H>
  int flux_init_t(const fpx_outgrid *g, const void *outheight) {
    n_flux = (size_t)6 * g->numxgrid * g->numygrid * g->numzgrid * cfg.nspec * g->maxpointspec_act * g->nageclass;
    sum_flux.shape(n_flux, sizeof(H));
    fx_geo[0] = g->dxout; fx_geo[1] = g->dyout; fx_geo[2] = g->xoutshift; fx_geo[3] = g->youtshift;
    std::vector<H> oh((const H *)outheight, (const H *)outheight + g->numzgrid), ohh(g->numzgrid);
    {
#pragma clang fp contract(off)
      ohh[0] = oh[0] / (H)2.;                          // readoutgrid.f90:194-196
      for (int j = 1; j < g->numzgrid; j++) ohh[j] = (oh[j - 1] + oh[j]) / (H)2.;
    }
    int rc;
    H *a, *b, *f;
    if ((rc = dalloc(&a, (size_t)g->numzgrid)) || (rc = dalloc(&b, (size_t)g->numzgrid)) || (rc = dalloc(&f, n_flux))) return rc;
    HIPCHK(hipMemcpyAsync(a, oh.data(), g->numzgrid * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(b, ohh.data(), g->numzgrid * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(f, 0, n_flux * sizeof(H), stream));
    HIPCHK(hipStreamSynchronize(stream));
    fx_outh = a; fx_outhh = b; fx_flux = f;
    return 0;
  }
  // the scratch of k_flux_save (allocated at the first step that needs it) and an event set for this step
  int flux_prepare() {
    if (!fx_due) {
      const size_t cap = (size_t)P.cap, hb = (size_t)cfg.host_real_bytes;
      unsigned char *q;
      int rc;
      if ((rc = dalloc(&q, cap * hb))) return rc; fx_xold = q;
      if ((rc = dalloc(&q, cap * hb))) return rc; fx_yold = q;
      if ((rc = dalloc(&q, cap * hb))) return rc; fx_zold = q;
      if ((rc = dalloc(&q, cap * hb * cfg.nspec))) return rc; fx_mass = q;
      if ((rc = dalloc(&fx_due, cap))) return rc;
    }
    HIPCHK(fx_timer.begin(stream));
    return 0;      // the timer's current set is this step's; it counts once both kernels are in the stream (flux_launch)
  }
  template <typename H>
  cf::Args<H> flux_args() const {
    cf::Args<H> A;
    A.numxgrid = Gp.numxgrid; A.numygrid = Gp.numygrid; A.numzgrid = Gp.numzgrid; A.nspec = cfg.nspec;
    A.maxpointspec_act = Gp.maxpointspec_act; A.nageclass = Gp.nageclass;
    A.use_npoint = Gp.ioutputforeachrelease == 1 && cfg.mdomainfill == 0;
    A.nx = cfg.nx; A.nxmin1 = cfg.nx - 1;
    for (int i = 0; i < cf::kMaxAgeCf; i++) A.lage[i] = Gp.lage[i];
    A.dx = (H)cfg.dx; A.dy = (H)cfg.dy; A.dxout = (H)fx_geo[0]; A.dyout = (H)fx_geo[1]; A.xoutshift = (H)fx_geo[2]; A.youtshift = (H)fx_geo[3];
    A.outheight = (const H *)fx_outh; A.outheighthalf = (const H *)fx_outhh; A.flux = (H *)fx_flux;
    A.xold = (H *)fx_xold; A.yold = (H *)fx_yold; A.zold = (H *)fx_zold; A.mass = (H *)fx_mass; A.due = fx_due; A.cap = P.cap;
    return A;
  }
  template <typename H>
  int flux_launch(bool after, int itime) {
    static_assert(cf::kMaxAgeCf == kMaxAge, "age-class limit");
    const cf::Args<H> A = flux_args<H>();
    const Events<4> &fe = fx_timer.current();
    const int nb = (int)((numpart + 255) / 256);
    HIPCHK(hipEventRecord(fe[after ? 2 : 0], stream));
    if (!after) cf::k_flux_save<H, R><<<nb, 256, 0, stream>>>(A, P.xt, P.yt, P.zt, P.xmass1, P.itra1, P.cap, numpart, itime);
    else cf::k_calcfluxes<H, R><<<nb, 256, 0, stream>>>(A, P.xt, P.yt, P.zt, P.npoint, P.itramem, numpart, itime);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(fe[after ? 3 : 1], stream));
    if (after) { fx_timer.commit(); sum_flux.invalidate(); }   // k_calcfluxes adds to flux: the partial sums move on
    return 0;
  }
  int calcfluxes_time(double *ms, long long *launches, int reset) override {
    double t[2];
    HIPCHK(fx_timer.read(stream, t, launches, reset != 0));
    if (ms) *ms = t[0] + t[1];
    return 0;
  }
  int get_flux(void *flux, int allreduce, int clear) override {
    if (!cfg.device_flux) return fail(FPX_ERR_STATE, "get_flux: the engine was created without device_flux");
    if (!Gp.on || !fx_flux) return fail(FPX_ERR_STATE, "get_flux: fpx_outgrid_init first");
    return fetch({{&sum_flux, fx_flux, flux, false, clear != 0}}, allreduce, "get_flux");   // flux is in the host's kind already
  }
  // fluxoutput.f90:46-283 on the host from the downloaded grid (the grid is small next to the particles, and the file is
  // written record by record anyway), in the host's real kind
  template <typename H>
  int fluxoutput_t(int itime, const fpx_fluxout *f, const char *prefix, const void *src) {
#pragma clang fp contract(off)
    std::vector<H> fl(n_flux);
    HIPCHK(hipMemcpyAsync(fl.data(), src, n_flux * sizeof(H), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const int nxg = Gp.numxgrid, nyg = Gp.numygrid, nzg = Gp.numzgrid, ns = cfg.nspec, nkp = Gp.maxpointspec_act, na = Gp.nageclass;
    const H *area = (const H *)f->area, *areaeast = (const H *)f->areaeast, *areanorth = (const H *)f->areanorth;
    const H outstep = (H)f->outstep;
    auto at = [&](int i, int ix, int jy, int kz, int k, int kp, int nage) -> H {   // i, kz 1-based; the others 0-based
      return fl[(size_t)(i - 1) + 6 * ((size_t)ix + (size_t)nxg * ((size_t)jy + (size_t)nyg * ((size_t)(kz - 1) + (size_t)nzg * ((size_t)k + (size_t)ns * ((size_t)kp + (size_t)nkp * (size_t)nage)))))];
    };
    int hhmiss = 0;
    const int yyyymmdd = gv_caldate<H>(f->bdate + (double)itime / 86400., &hhmiss);
    char name[1200];
    snprintf(name, sizeof name, "%sgrid_flux_%08d%06d", prefix, yyyymmdd, hhmiss);
    RecFile file(name);
    if (!file.is_open()) return fail(FPX_ERR_ARG, std::string("fluxoutput: cannot open ") + name);
    // :61-134: cells per (species, age class) over all kp, and the sparse test
    std::vector<int> ncells((size_t)6 * ns * na, 0);
    for (int k = 0; k < ns; k++) for (int kp = 0; kp < nkp; kp++) for (int nage = 0; nage < na; nage++)
      for (int jy = 0; jy < nyg; jy++) for (int ix = 0; ix < nxg; ix++) for (int kz = 1; kz <= nzg; kz++)
        for (int i = 1; i <= 6; i++) if (at(i, ix, jy, kz, k, kp, nage) > (H)0) ncells[(size_t)(i - 1) + 6 * ((size_t)k + (size_t)ns * nage)]++;
    file.scalar((int32_t)itime);
    const int order[6] = {2, 1, 3, 4, 5, 6};           // eastward, westward, south, north, up, down (:146-276)
    for (int k = 0; k < ns && file.ok(); k++) for (int kp = 0; kp < nkp && file.ok(); kp++) for (int nage = 0; nage < na && file.ok(); nage++)
      for (int d = 0; d < 6; d++) {
        const int i = order[d];
        auto value = [&](int ix, int jy, int kz) -> H {
          const H a = i <= 2 ? areaeast[(size_t)ix + (size_t)nxg * ((size_t)jy + (size_t)nyg * (size_t)(kz - 1))]
                    : i <= 4 ? areanorth[(size_t)ix + (size_t)nxg * ((size_t)jy + (size_t)nyg * (size_t)(kz - 1))] : area[(size_t)ix + (size_t)nxg * (size_t)jy];
          return (H)1.e12 * at(i, ix, jy, kz, k, kp, nage) / a / outstep;
        };
        if (4 * ncells[(size_t)(i - 1) + 6 * ((size_t)k + (size_t)ns * nage)] < nxg * nyg * nzg) {
          file.scalar((int32_t)1);
          for (int kz = 1; kz <= nzg; kz++) for (int jy = 0; jy < nyg; jy++) for (int ix = 0; ix < nxg; ix++)
            if (at(i, ix, jy, kz, k, kp, nage) > (H)0) {
              const int32_t idx = ix + jy * nxg + kz * nxg * nyg;
              file.put(idx); file.put(value(ix, jy, kz)); file.end();
            }
          file.put((int32_t)-999); file.put((H)999.); file.end();
        } else {
          file.scalar((int32_t)2);
          for (int kz = 1; kz <= nzg; kz++) for (int ix = 0; ix < nxg; ix++) {
            for (int jy = 0; jy < nyg; jy++) file.put(value(ix, jy, kz));
            file.end();
          }
        }
      }
    if (!file.close()) return fail(FPX_ERR_ARG, std::string("fluxoutput: write error on ") + name);
    return 0;
  }
  int fluxoutput(int itime, const fpx_fluxout *f, const char *prefix, int reduced) override {
    if (!cfg.device_flux) return fail(FPX_ERR_STATE, "fluxoutput: the engine was created without device_flux");
    if (!Gp.on || !fx_flux) return fail(FPX_ERR_STATE, "fluxoutput: fpx_outgrid_init first");
    if (!f || f->struct_bytes != (int32_t)sizeof(fpx_fluxout)) return fail(FPX_ERR_ARG, "fluxoutput: null or fpx_fluxout size mismatch (ABI)");
    if (!f->area || !f->areaeast || !f->areanorth || !prefix) return fail(FPX_ERR_ARG, "fluxoutput: area, areaeast, areanorth and the path prefix are required");
    if (strlen(prefix) > 1000) return fail(FPX_ERR_ARG, "fluxoutput: prefix too long");
    const void *src;
    int rc = source(sum_flux, fx_flux, reduced, "fluxoutput", "fpx_get_flux", &src);
    if (rc) return rc;
    rc = cfg.host_real_bytes == 4 ? fluxoutput_t<float>(itime, f, prefix, src) : fluxoutput_t<double>(itime, f, prefix, src);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(fx_flux, 0, n_flux * cfg.host_real_bytes, stream));     // :289-303
    HIPCHK(hipStreamSynchronize(stream));
    sum_flux.invalidate();                   // flux starts from zero again: the sums just written are not its sums
    return 0;
  }

  // ---- per-particle averages over the output interval (fpx_partavg.hpp; fpx_config.device_partavg) -------------
  // npart_av and the fourteen sums of com_mod.f90:688-691 per storage space, in the host's real kind; a second set only once
  // a locality sort has to move them.  Zero at creation; nothing but fpx_partoutput_average resets them -- release and
  // splitting leave a space's sums as they find them, as the reference does.
  int *pa_n[2] = {nullptr, nullptr};
  void *pa_sum[2] = {nullptr, nullptr};
  int pa_cur = 0;
  IntervalTimer<2> pa_timer{{0, 1}};
  int partavg_alloc(int k) {
    const size_t cap = (size_t)P.cap, hb = (size_t)cfg.host_real_bytes;
    unsigned char *q;
    int rc;
    if ((rc = dalloc(&pa_n[k], cap))) return rc;
    if ((rc = dalloc(&q, cap * hb * pa::kSums))) return rc;
    pa_sum[k] = q;
    HIPCHK(hipMemsetAsync(pa_n[k], 0, cap * sizeof(int), stream));
    HIPCHK(hipMemsetAsync(q, 0, cap * hb * pa::kSums, stream));
    return 0;
  }
  template <typename H>
  pa::State<H> partavg_state(int k) const {
    pa::State<H> S;
    S.npart_av = pa_n[k]; S.sum = (H *)pa_sum[k]; S.cap = P.cap;
    return S;
  }
  template <typename H>
  DiagP<H> diag_args() const {
    DiagP<H> D;
    D.oro = (const H *)diag_oro;
    D.tropo[0] = (const H *)diag_tropo[0]; D.tropo[1] = (const H *)diag_tropo[1];
    D.d3 = (const H *)diag_d3;
    D.nxmax = cfg.nxmax; D.nymax = cfg.nymax;
    D.dx = (H)cfg.dx; D.dy = (H)cfg.dy; D.xlon0 = (H)cfg.xlon0; D.ylat0 = (H)cfg.ylat0;
    return D;
  }
  int partavg_prepare() {
    HIPCHK(pa_timer.begin(stream));
    return 0;
  }
  template <typename H>
  int partavg_launch(int itime) {
    const Events<2> &pe = pa_timer.current();
    HIPCHK(hipEventRecord(pe[0], stream));
    pa::k_partavg<R, H><<<(int)((numpart + 255) / 256), 256, 0, stream>>>(V, P, diag_args<H>(), partavg_state<H>(pa_cur), d_pbl_flag, kKeyNotDue, numpart, itime);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(pe[1], stream));
    pa_timer.commit();
    return 0;
  }
  int partavg_time(double *ms, long long *launches, int reset) override {
    double t;
    HIPCHK(pa_timer.read(stream, &t, launches, reset != 0));
    if (ms) *ms = t;
    return 0;
  }
  template <typename H>
  int get_partavg_t(long long first, long long count, int32_t *npart_av, void *const *sums) {
    const pa::State<H> S = partavg_state<H>(pa_cur);
    int rc;
    if (npart_av && (rc = get<int32_t, int>(npart_av, S.npart_av, first, count))) return rc;
    for (int k = 0; sums && k < pa::kSums; k++)
      if (sums[k] && (rc = get<H, H>((H *)sums[k], S.sum + (size_t)k * S.cap, first, count))) return rc;
    return 0;
  }
  int get_partavg(long long first, long long count, int32_t *npart_av, void *const *sums) override {
    if (!cfg.device_partavg) return fail(FPX_ERR_STATE, "get_partavg: the engine was created without device_partavg");
    if (first < 0 || count < 0 || first + count > P.cap) return fail(FPX_ERR_ARG, "get_partavg: range outside the storage spaces");
    if (count == 0) return 0;
    return cfg.host_real_bytes == 4 ? get_partavg_t<float>(first, count, npart_av, sums) : get_partavg_t<double>(first, count, npart_av, sums);
  }
  // partoutput_average.f90:54-201: the records are formed on the device, the host streams them.  Direct access, recl = 24,
  // no record markers; the file ends with the record of the last valid particle, the records of the others in between are
  // zero bytes (what the reference's runtime leaves in a hole).
  template <typename H>
  int partoutput_average_t(int itime, const char *name, int64_t *nrecords) {
    const long long n = numpart;
    RecFile file(name);
    if (!file.is_open()) return fail(FPX_ERR_ARG, std::string("partoutput_average: cannot open ") + name);
    Scratch b_out, b_stat, pin(true);
    unsigned int hs[2] = {0, 0};
    if (n > 0) {
      hipError_t e = b_out.reserve((size_t)n * 24, stream);
      if (e == hipSuccess) e = b_stat.reserve(2 * sizeof(unsigned int), stream);
      if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("partoutput_average: record buffer: ") + hipGetErrorString(e));
      unsigned int *out = b_out.as<unsigned int>(), *stat = b_stat.as<unsigned int>();
      e = hipMemsetAsync(out, 0, (size_t)n * 24, stream);
      if (e == hipSuccess) e = hipMemsetAsync(stat, 0, 2 * sizeof(unsigned int), stream);
      if (e == hipSuccess) {
        pa::k_partavg_out<R, H><<<(int)((n + 255) / 256), 256, 0, stream>>>(P, partavg_state<H>(pa_cur), n, itime, out, stat);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipMemcpyAsync(hs, stat, sizeof hs, hipMemcpyDeviceToHost, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      const size_t total = (size_t)hs[1] * 24, chunk = (size_t)64 << 20;
      if (e == hipSuccess && total) e = pin.reserve(std::min(chunk, total), stream);
      for (size_t off = 0; e == hipSuccess && file.ok() && off < total; off += chunk) {
        const size_t nbytes = std::min(chunk, total - off);
        e = hipMemcpyAsync(pin.as(), (const char *)out + off, nbytes, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e == hipSuccess) file.write(pin.as(), nbytes);      // direct access: no record markers
      }
      if (e != hipSuccess) return fail(FPX_ERR_DEVICE, std::string("partoutput_average: ") + hipGetErrorString(e));
    }
    if (!file.close()) return fail(FPX_ERR_ARG, std::string("partoutput_average: write error on ") + name);
    if (nrecords) *nrecords = hs[0];
    return 0;
  }
  double pa_bdate = 0;
  bool pa_bdate_set = false;
  int partoutput_average(int itime, const char *prefix, int64_t *nrecords) override {
    if (!cfg.device_partavg) return fail(FPX_ERR_STATE, "partoutput_average: the engine was created without device_partavg");
    if (!prefix) return fail(FPX_ERR_ARG, "partoutput_average: null path");
    if (strlen(prefix) > 1000) return fail(FPX_ERR_ARG, "partoutput_average: prefix too long");
    // with the run's start date known (fpx_set_option "bdate") the argument is path(2)(1:length(2)) and the name is formed as
    // partoutput_average.f90:45-62 does; without it the argument is the complete path of the file
    char name[1200];
    if (pa_bdate_set) {
      int hhmiss = 0;
      const int yyyymmdd = cfg.host_real_bytes == 4 ? gv_caldate<float>(pa_bdate + (double)itime / 86400., &hhmiss) : gv_caldate<double>(pa_bdate + (double)itime / 86400., &hhmiss);
      snprintf(name, sizeof name, "%spartposit_average_%08d%06d", prefix, yyyymmdd, hhmiss);
    } else snprintf(name, sizeof name, "%s", prefix);
    return cfg.host_real_bytes == 4 ? partoutput_average_t<float>(itime, name, nrecords) : partoutput_average_t<double>(itime, name, nrecords);
  }

  // ---- sensitivity to initial conditions (fpx_initcond.hpp; fpx_config.device_initcond) --------------------------
  // init_cond and everything the kernels compare a position with are kept in the host's real kind H, whatever the engine
  // computes in: initial_cond_calc.f90 declares them default real.  Allocated by fpx_outgrid_init, zero at creation;
  // nothing but the `clear` of fpx_get_initcond resets it -- it accumulates over the whole run.
  void *ic_grid = nullptr;                             // unc_mod's init_cond (its sums over the ranks: sum_ic)
  void *ic_outh = nullptr;                             // outheight in H
  size_t n_initcond = 0;
  double ic_geo[4] = {};                               // dxout, dyout, xoutshift, youtshift as the host passed them
  int ic_iofr = 0;
  IntervalTimer<2> ic_timer{{0, 1}}, ic_fin_timer{{0, 1}};   // k_initcond per step; k_initcond_finish
  template <typename H>
  int initcond_init_t(const fpx_outgrid *g, const void *outheight) {
    n_initcond = (size_t)g->numxgrid * g->numygrid * g->numzgrid * cfg.nspec * g->maxpointspec_act;   // outgrid_init.f90:296 (maxspec -> nspec)
    sum_ic.shape(n_initcond, sizeof(H));
    ic_geo[0] = g->dxout; ic_geo[1] = g->dyout; ic_geo[2] = g->xoutshift; ic_geo[3] = g->youtshift;
    ic_iofr = g->ioutputforeachrelease;
    int rc;
    H *a, *f;
    if ((rc = dalloc(&a, (size_t)g->numzgrid)) || (rc = dalloc(&f, n_initcond))) return rc;
    HIPCHK(hipMemcpyAsync(a, outheight, g->numzgrid * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(f, 0, n_initcond * sizeof(H), stream));
    HIPCHK(hipStreamSynchronize(stream));
    ic_outh = a; ic_grid = f;
    return 0;
  }
  template <typename H>
  ic::Args<H> initcond_args() const {
    ic::Args<H> A;
    A.linit_cond = cfg.linit_cond;
    A.nx = cfg.nx; A.ny = cfg.ny; A.nz = cfg.nz;
    A.numxgrid = Gp.numxgrid; A.numygrid = Gp.numygrid; A.numzgrid = Gp.numzgrid; A.nspec = cfg.nspec; A.maxpointspec_act = Gp.maxpointspec_act;
    A.use_npoint = ic_iofr == 1 && cfg.mdomainfill == 0;
    A.dx = (H)cfg.dx; A.dy = (H)cfg.dy; A.dxout = (H)ic_geo[0]; A.dyout = (H)ic_geo[1]; A.xoutshift = (H)ic_geo[2]; A.youtshift = (H)ic_geo[3];
    A.outheight = (const H *)ic_outh; A.init_cond = (H *)ic_grid;
    return A;
  }
  template <typename H>
  int initcond_launch() {
    const Events<2> &ie = ic_timer.current();
    HIPCHK(hipEventRecord(ie[0], stream));
    ic::k_initcond<R, H><<<(int)((numpart + 255) / 256), 256, 0, stream>>>(initcond_args<H>(), V, P, d_pbl_flag, kKeyNotDue, kDead, numpart);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ie[1], stream));
    ic_timer.commit();
    sum_ic.invalidate();                     // k_initcond adds the particles this step terminated to init_cond
    return 0;
  }
  // the device time of k_initcond and k_initcond_finish; the launches are the steps that ran k_initcond
  int initcond_time(double *ms, long long *launches, int reset) override {
    double t = 0, tf = 0;
    HIPCHK(ic_timer.read(stream, &t, launches, reset != 0));
    HIPCHK(ic_fin_timer.read(stream, &tf, nullptr, reset != 0));
    if (ms) *ms = t + tf;
    return 0;
  }
  // timemanager.f90:735-737
  int initcond_finish(int itime) override {
    if (!cfg.device_initcond) return fail(FPX_ERR_STATE, "initcond_finish: the engine was created without device_initcond");
    if (!Gp.on || !ic_grid) return fail(FPX_ERR_STATE, "initcond_finish: fpx_outgrid_init first");
    if (numpart == 0) return 0;
    if (!height_set || !slot_loaded[0] || !slot_loaded[1]) return fail(FPX_ERR_STATE, "initcond_finish: height and both field slots must be set first");
    HIPCHK(ic_fin_timer.begin(stream));
    const Events<2> &ie = ic_fin_timer.current();
    const int nb = (int)((numpart + 255) / 256);      // whole blocks: the kernel keeps its waves convergent
    HIPCHK(hipEventRecord(ie[0], stream));
    if (cfg.host_real_bytes == 4) ic::k_initcond_finish<R, float, kMaxNz><<<nb, 256, 0, stream>>>(initcond_args<float>(), V, P, numpart, itime);
    else ic::k_initcond_finish<R, double, kMaxNz><<<nb, 256, 0, stream>>>(initcond_args<double>(), V, P, numpart, itime);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ie[1], stream));
    ic_fin_timer.commit();
    sum_ic.invalidate();                     // k_initcond_finish adds every particle still alive to init_cond
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  int get_initcond(void *init_cond, int allreduce, int clear) override {
    if (!cfg.device_initcond) return fail(FPX_ERR_STATE, "get_initcond: the engine was created without device_initcond");
    if (!Gp.on || !ic_grid) return fail(FPX_ERR_STATE, "get_initcond: fpx_outgrid_init first");
    return fetch({{&sum_ic, ic_grid, init_cond, false, clear != 0}}, allreduce, "get_initcond");   // init_cond is in the host's kind already
  }
  // initial_cond_output.f90:58-130 on the host from the downloaded grid, in the host's real kind: per species one
  // unformatted sequential file
  template <typename H>
  int initial_cond_output_t(int itime, const fpx_initout *o, const char *prefix, const void *src) {
#pragma clang fp contract(off)
    std::vector<H> g(n_initcond);
    HIPCHK(hipMemcpyAsync(g.data(), src, n_initcond * sizeof(H), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    const int nxg = Gp.numxgrid, nyg = Gp.numygrid, nzg = Gp.numzgrid, ns = cfg.nspec, nkp = Gp.maxpointspec_act, np = V.numpoint;
    const H smallnum = std::numeric_limits<H>::min();      // tiny(0.0)
    std::vector<int32_t> di;
    std::vector<H> dr;
    for (int ks = 0; ks < ns; ks++) {
      char name[1200];
      snprintf(name, sizeof name, "%sgrid_initial_%03d", prefix, ks + 1);
      RecFile file(name);
      if (!file.is_open()) return fail(FPX_ERR_ARG, std::string("initial_cond_output: cannot open ") + name);
      const int32_t zero = 0;
      file.scalar((int32_t)itime);
      for (int kp = 0; kp < nkp && file.ok(); kp++) {
        const H fact_recept = o->ind_rel == 1 ? ((const H *)o->rho_rel)[kp] : (H)1.;
        const H xm = (H)rel_xmass_h[(size_t)ks * np + kp];
        for (int d = 0; d < 2; d++) { file.scalar(zero); file.record(nullptr, 0); file.scalar(zero); file.record(nullptr, 0); }   // :83-92
        di.clear(); dr.clear();
        H sp_fact = (H)-1.;
        bool sp_zer = true;
        const H *gk = g.data() + (size_t)nxg * nyg * nzg * ((size_t)ks + (size_t)ns * kp);
        for (int kz = 1; kz <= nzg; kz++) for (int jy = 0; jy < nyg; jy++) for (int ix = 0; ix < nxg; ix++) {
          const H v = gk[(size_t)ix + (size_t)nxg * ((size_t)jy + (size_t)nyg * (size_t)(kz - 1))];
          if (v > smallnum) {
            if (sp_zer) {
              di.push_back(ix + jy * nxg + kz * nxg * nyg);
              sp_zer = false;
              sp_fact = sp_fact * (H)-1.;
            }
            dr.push_back(sp_fact * v / xm * fact_recept);
          } else sp_zer = true;
        }
        const int32_t ci = (int32_t)di.size(), cr = (int32_t)dr.size();
        file.scalar(ci); file.record(di.data(), di.size() * 4);
        file.scalar(cr); file.record(dr.data(), dr.size() * sizeof(H));
      }
      if (!file.close()) return fail(FPX_ERR_ARG, std::string("initial_cond_output: write error on ") + name);
    }
    return 0;
  }
  int initial_cond_output(int itime, const fpx_initout *o, const char *prefix, int reduced) override {
    if (!cfg.device_initcond) return fail(FPX_ERR_STATE, "initial_cond_output: the engine was created without device_initcond");
    if (!Gp.on || !ic_grid) return fail(FPX_ERR_STATE, "initial_cond_output: fpx_outgrid_init first");
    if (!o || o->struct_bytes != (int32_t)sizeof(fpx_initout)) return fail(FPX_ERR_ARG, "initial_cond_output: null or fpx_initout size mismatch (ABI)");
    if (!prefix) return fail(FPX_ERR_ARG, "initial_cond_output: null path prefix");
    if (strlen(prefix) > 1000) return fail(FPX_ERR_ARG, "initial_cond_output: prefix too long");
    if (o->ind_rel == 1 && !o->rho_rel) return fail(FPX_ERR_ARG, "initial_cond_output: ind_rel = 1 needs rho_rel");
    if (V.numpoint < Gp.maxpointspec_act || rel_xmass_h.size() < (size_t)cfg.nspec * V.numpoint)
      return fail(FPX_ERR_STATE, "initial_cond_output: xmass of every release point is needed (fpx_set_release_points)");
    const void *src;
    const int rc = source(sum_ic, ic_grid, reduced, "initial_cond_output", "fpx_get_initcond", &src);
    if (rc) return rc;
    return cfg.host_real_bytes == 4 ? initial_cond_output_t<float>(itime, o, prefix, src) : initial_cond_output_t<double>(itime, o, prefix, src);
  }

  // ---- plume trajectories (fpx_plumetraj.hpp; iout = 4, 5) --------------------------------------------------------
  // Nothing here exists before fpx_plumetraj_init: the buffers are grow-only Scratch members a call reserves.
  bool pt_on = false;
  int pt_numpoint = 0, pt_K = 0;
  std::vector<int32_t> pt_start, pt_end;                 // ireleasestart, ireleaseend
  Scratch pt_keys[2], pt_vals[2], pt_tmp, pt_active, pt_bounds, pt_segs, pt_chunkseg, pt_part, pt_zl, pt_ncl, pt_pending;
  double pt_last_ms = 0, pt_sweep_ms = 0;
  // the records of the last call
  std::vector<int32_t> pt_rec_j, pt_rec_n, pt_rec_it, pt_rec_numb;
  std::vector<double> pt_rec_val;                        // [record][14 + 5 ncluster], exact copies of the values in H
  int plumetraj_init(const fpx_plumetraj_cfg *c) override {
    if (!c || c->struct_bytes != (int32_t)sizeof(fpx_plumetraj_cfg)) return fail(FPX_ERR_ARG, "plumetraj_init: null or fpx_plumetraj_cfg size mismatch (ABI)");
    if (c->numpoint < 1 || !c->ireleasestart || !c->ireleaseend) return fail(FPX_ERR_ARG, "plumetraj_init: numpoint >= 1 and both release-time arrays are needed");
    if (c->ncluster < 1 || c->ncluster > FPX_MAXCLUSTER) return fail(FPX_ERR_ARG, "plumetraj_init: ncluster must be 1 .. FPX_MAXCLUSTER");
    pt_numpoint = c->numpoint; pt_K = c->ncluster;
    pt_start.assign(c->ireleasestart, c->ireleasestart + c->numpoint);
    pt_end.assign(c->ireleaseend, c->ireleaseend + c->numpoint);
    pt_rec_j.clear(); pt_rec_n.clear(); pt_rec_it.clear(); pt_rec_numb.clear(); pt_rec_val.clear();
    pt_on = true;
    return 0;
  }
  template <typename H, int KM>
  int plumetraj_kernels(int itime, int nseg, int nchunk, bool any_clustered, const Events<4> &ev) {
    const int K = pt_K;
    const pt::Geo<H> G{(H)cfg.xlon0, (H)cfg.ylat0, (H)cfg.dx, (H)cfg.dy};
    pt::Seg<H> *segs = pt_segs.as<pt::Seg<H>>();
    const int *chunk_seg = pt_chunkseg.as<int>();
    const unsigned int *list = pt_vals[1].as<unsigned int>();
    unsigned char *ncl = pt_ncl.as<unsigned char>();
    double *part = pt_part.as<double>();
    int *pending = pt_pending.as<int>();
    HIPCHK(hipMemsetAsync(pending, 0, (pt::kMaxSweeps + 1) * sizeof(int), stream));
    HIPCHK(hipEventRecord(ev[1], stream));
    if (any_clustered) {
      pt::k_pt_seed<R, H><<<(nseg * K + 63) / 64, 64, 0, stream>>>(P, G, segs, nseg, K, list);
      HIPCHK(hipGetLastError());
      for (int l = 1; l <= pt::kMaxSweeps; l++) {        // clustering.f90:78
        pt::k_pt_sweep<R, H, KM><<<nchunk, pt::kThreads, 0, stream>>>(P, G, segs, chunk_seg, list, ncl, part, K);
        pt::k_pt_sweep_seg<H, KM><<<nseg, 64, 0, stream>>>(segs, part, K, l, pending);
        HIPCHK(hipGetLastError());
        if (l == 1) continue;                            // no release point leaves the loop in its first pass
        int more = 0;
        HIPCHK(hipMemcpyAsync(&more, pending + l, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (!more) break;
      }
    }
    HIPCHK(hipEventRecord(ev[2], stream));
    pt::k_pt_final1<R, H, KM><<<nchunk, pt::kThreads, 0, stream>>>(V, P, diag_args<H>(), segs, chunk_seg, list, ncl, pt_zl.as<H>(), part, itime);
    pt::k_pt_final1_seg<H, KM><<<nseg, 64, 0, stream>>>(segs, part, K);
    pt::k_pt_final2<R, H><<<nchunk, pt::kThreads, 0, stream>>>(P, G, segs, chunk_seg, list, ncl, pt_zl.as<H>(), part);
    pt::k_pt_final2_seg<H><<<nseg, 64, 0, stream>>>(segs, part, K);
    HIPCHK(hipGetLastError());
    return 0;
  }
  template <typename H>
  int plumetraj_t(int itime, const char *path, int32_t *nrecords) {
    const long long n = numpart;
    const int np = pt_numpoint, K = pt_K;
    pt_rec_j.clear(); pt_rec_n.clear(); pt_rec_it.clear(); pt_rec_numb.clear(); pt_rec_val.clear();
    pt_last_ms = 0; pt_sweep_ms = 0;
    std::vector<unsigned char> active((size_t)np);
    bool any = false;
    for (int j = 0; j < np; j++) {                        // plumetraj.f90:65
      const long long d = (long long)pt_start[j] - itime;
      active[j] = (d < 0 ? -d : d) <= (long long)cfg.lage_last;
      any = any || active[j];
    }
    std::vector<pt::Seg<H>> segs((size_t)np);
    if (n > 0 && any) {
      hipError_t e = hipSuccess;
      for (int k = 0; k < 2 && e == hipSuccess; k++) {
        e = pt_keys[k].reserve((size_t)n * 4, stream);
        if (e == hipSuccess) e = pt_vals[k].reserve((size_t)n * 4, stream);
      }
      if (e == hipSuccess) e = pt_active.reserve((size_t)np, stream);
      if (e == hipSuccess) e = pt_bounds.reserve(((size_t)np + 1) * 4, stream);
      if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("plumetraj: ") + hipGetErrorString(e));
      Events<4> ev;
      HIPCHK(ev.create());
      HIPCHK(hipEventRecord(ev[0], stream));
      HIPCHK(hipMemcpyAsync(pt_active.as(), active.data(), (size_t)np, hipMemcpyHostToDevice, stream));
      unsigned int *k0 = pt_keys[0].as<unsigned int>(), *k1 = pt_keys[1].as<unsigned int>();
      unsigned int *v0 = pt_vals[0].as<unsigned int>(), *v1 = pt_vals[1].as<unsigned int>();
      HIPCHK(hipMemsetAsync(k0, 0xFF, (size_t)n * 4, stream));   // a particle number no storage space holds: no member
      HIPCHK(hipMemsetAsync(v0, 0, (size_t)n * 4, stream));
      pt::k_pt_key<R><<<(int)((n + 255) / 256), 256, 0, stream>>>(V, P, n, itime, np, pt_active.as<unsigned char>(), k0, v0);
      HIPCHK(hipGetLastError());
      int bits = 1;
      while (bits < 32 && (1ll << bits) <= (long long)np) bits++;
      size_t tb = 0;
      HIPCHK(rocprim::radix_sort_pairs(nullptr, tb, k0, k1, v0, v1, (size_t)n, 0u, (unsigned int)bits, stream));
      if ((e = pt_tmp.reserve(tb, stream)) != hipSuccess) return fail(FPX_ERR_NOMEM, "plumetraj: sort storage");
      HIPCHK(rocprim::radix_sort_pairs(pt_tmp.as(), tb, k0, k1, v0, v1, (size_t)n, 0u, (unsigned int)bits, stream));
      pt::k_pt_bounds<<<(np + 1 + 255) / 256, 256, 0, stream>>>(k1, n, np, pt_bounds.as<int>());
      HIPCHK(hipGetLastError());
      std::vector<int> start((size_t)np + 1);
      HIPCHK(hipMemcpyAsync(start.data(), pt_bounds.as(), ((size_t)np + 1) * 4, hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      std::vector<int> chunk_seg;
      bool any_clustered = false;
      for (int j = 0; j < np; j++) {
        pt::Seg<H> &S = segs[j];
        memset(&S, 0, sizeof(S));
        S.begin = start[j]; S.n = start[j + 1] - start[j];
        S.chunk0 = (int)chunk_seg.size(); S.nchunk = (S.n + pt::kChunk - 1) / pt::kChunk;
        S.clustered = S.n >= K && S.n > 0;
        S.frozen = !S.clustered;
        any_clustered = any_clustered || S.clustered;
        chunk_seg.insert(chunk_seg.end(), (size_t)S.nchunk, j);
      }
      const int nchunk = (int)chunk_seg.size(), members = start[np];
      if (nchunk > 0) {
        if ((e = pt_segs.reserve(segs.size() * sizeof(pt::Seg<H>), stream)) != hipSuccess || (e = pt_chunkseg.reserve((size_t)nchunk * 4, stream)) != hipSuccess ||
            (e = pt_part.reserve((size_t)nchunk * pt::kMaxQ * 8, stream)) != hipSuccess || (e = pt_zl.reserve((size_t)members * sizeof(H), stream)) != hipSuccess ||
            (e = pt_ncl.reserve((size_t)members, stream)) != hipSuccess || (e = pt_pending.reserve((pt::kMaxSweeps + 1) * sizeof(int), stream)) != hipSuccess)
          return fail(FPX_ERR_NOMEM, std::string("plumetraj: ") + hipGetErrorString(e));
        HIPCHK(hipMemcpyAsync(pt_segs.as(), segs.data(), segs.size() * sizeof(pt::Seg<H>), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(pt_chunkseg.as(), chunk_seg.data(), (size_t)nchunk * 4, hipMemcpyHostToDevice, stream));
        const int rc = K <= 5 ? plumetraj_kernels<H, 5>(itime, np, nchunk, any_clustered, ev) : plumetraj_kernels<H, pt::kMaxCluster>(itime, np, nchunk, any_clustered, ev);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(segs.data(), pt_segs.as(), segs.size() * sizeof(pt::Seg<H>), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipEventRecord(ev[3], stream));
        HIPCHK(hipStreamSynchronize(stream));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[3]) == hipSuccess) pt_last_ms = ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) pt_sweep_ms = ms;
      }
    }
    std::string text;
    for (int j = 0; j < np; j++) {
      const pt::Seg<H> &S = segs[j];
      if (!active[j] || S.n <= 0) continue;               // plumetraj.f90:183
      pt_rec_j.push_back(j + 1); pt_rec_n.push_back(S.n); pt_rec_it.push_back(S.iterations);
      for (int k = 0; k < K; k++) pt_rec_numb.push_back(S.clustered ? S.numb[k] : 0);
      for (int k = 0; k < 14 + 5 * K; k++) pt_rec_val.push_back((double)S.val[k]);
      if (path) text += pt::pt_record<H>(j + 1, (int)(itime - (pt_start[j] + pt_end[j]) / 2), S.val);
    }
    if (path) {
      RecFile file(path, "ab");
      if (!file.is_open()) return fail(FPX_ERR_ARG, std::string("plumetraj: cannot open ") + path);
      file.write(text.data(), text.size());               // formatted text: no record markers
      if (!file.close()) return fail(FPX_ERR_ARG, std::string("plumetraj: write error on ") + path);
    }
    if (nrecords) *nrecords = (int32_t)pt_rec_j.size();
    return 0;
  }
  int plumetraj(int itime, const char *path, int32_t *nrecords) override {
    if (!pt_on) return fail(FPX_ERR_STATE, "plumetraj: fpx_plumetraj_init first");
    if (comm_ranks > 1) return fail(FPX_ERR_UNSUPPORTED, "plumetraj: a communicator of several ranks -- the seeds and the sums of a release point span the ranks");
    if (path && pt_K != 5) return fail(FPX_ERR_ARG, "plumetraj: the record's format has five clusters (plumetraj.f90:218-219); a path needs ncluster = 5");
    if (!height_set || !window_set || !slot_loaded[0] || !slot_loaded[1]) return fail(FPX_ERR_STATE, "plumetraj: height, both field slots and the wind-time window must be set first");
    if (!diag_have[DG_ORO] || !diag_have[DG_PV] || !diag_have[DG_PV + 1] || !diag_have[DG_TROPO] || !diag_have[DG_TROPO + 1])
      return fail(FPX_ERR_STATE, "plumetraj: oro, pv (fpx_upload_diag_fields or fpx_verttransform_ecmwf) and tropopause of both slots are needed");
    if (numpart > 0x7fffffffll) return fail(FPX_ERR_UNSUPPORTED, "plumetraj: more than 2^31 - 1 storage spaces in use");
    return cfg.host_real_bytes == 4 ? plumetraj_t<float>(itime, path, nrecords) : plumetraj_t<double>(itime, path, nrecords);
  }
  int get_plumetraj(int max_records, int32_t *jpoint, int32_t *npart, int32_t *iterations, int32_t *numb, void *values, int ld) override {
    if (!pt_on) return fail(FPX_ERR_STATE, "get_plumetraj: fpx_plumetraj_init first");
    const int nr = (int)pt_rec_j.size(), K = pt_K, nv = 14 + 5 * K;
    if (max_records < nr) return fail(FPX_ERR_ARG, "get_plumetraj: max_records is smaller than the number of records of the last call");
    if (values && ld < nv) return fail(FPX_ERR_ARG, "get_plumetraj: ld must be at least 14 + 5 ncluster");
    for (int r = 0; r < nr; r++) {
      if (jpoint) jpoint[r] = pt_rec_j[r];
      if (npart) npart[r] = pt_rec_n[r];
      if (iterations) iterations[r] = pt_rec_it[r];
      for (int k = 0; numb && k < K; k++) numb[(size_t)r * K + k] = pt_rec_numb[(size_t)r * K + k];
      for (int k = 0; values && k < nv; k++) {
        if (cfg.host_real_bytes == 4) ((float *)values)[(size_t)r * ld + k] = (float)pt_rec_val[(size_t)r * nv + k];
        else ((double *)values)[(size_t)r * ld + k] = pt_rec_val[(size_t)r * nv + k];
      }
    }
    return 0;
  }
  double plumetraj_ms() override { return pt_last_ms; }

  // ---- boundary conditions of a domain-filling run (fpx_domainfill.hpp; boundcond_domainfill.f90) -----------------
  // Nothing here exists before fpx_domainfill_init.
  bool dfl_on = false;
  fpx_domainfill_cfg dfl_cfg = {};
  std::vector<int32_t> dfl_nc_we, dfl_nc_sn;             // the host's numcolumn_we, numcolumn_sn
  std::vector<unsigned char> dfl_zc_we, dfl_zc_sn;       // the host's zcolumn_*, its bytes (boundcond.bin)
  std::vector<df::Loc> dfl_locs;                         // the release locations in the reference's loop order
  Scratch dfl_d_nc[2], dfl_d_zc[2], dfl_d_acc[2][2], dfl_d_locs, dfl_d_height;   // acc: [buffer][we | sn]
  int dfl_cur = 0;                                       // the buffer that holds acc_mass_*
  Scratch dfl_mmass, dfl_first, dfl_accv, dfl_accsum, dfl_cnt, dfl_term, dfl_uni, dfl_target, dfl_arank, dfl_tmp;
  Scratch dfl_cx, dfl_cy, dfl_cz, dfl_cm, dfl_cn, dfl_ca;
  Ran1 dfl_ran1 = [] { Ran1 r; r.idum = -11; return r; }();   // boundcond_domainfill.f90:48: integer :: idummy = -11 (SAVE'd)
  double dfl_last_ms = 0, dfl_stage_ms[4] = {0, 0, 0, 0};
  long long dfl_last_ncand = 0;
  size_t dfl_acc_bytes(int side) const { return (size_t)2 * (side == 0 ? cfg.nymax : cfg.nxmax) * dfl_cfg.maxcolumn * cfg.host_real_bytes; }

  int domainfill_init(const fpx_domainfill_cfg *c) override {
    if (!c || c->struct_bytes != (int32_t)sizeof(fpx_domainfill_cfg)) return fail(FPX_ERR_ARG, "domainfill_init: null or fpx_domainfill_cfg size mismatch (ABI)");
    if (cfg.mdomainfill != 1 && cfg.mdomainfill != 2) return fail(FPX_ERR_ARG, "domainfill_init: the run is not domain-filling (mdomainfill = 0)");
    if (comm_ranks > 1) return fail(FPX_ERR_UNSUPPORTED, "domainfill_init: a communicator of several ranks -- the vacancies and the serial stream span the ranks");
    if (!height_set) return fail(FPX_ERR_STATE, "domainfill_init: fpx_set_height first");
    if (!c->numcolumn_we || !c->numcolumn_sn || !c->zcolumn_we || !c->zcolumn_sn || !c->acc_mass_we || !c->acc_mass_sn)
      return fail(FPX_ERR_ARG, "domainfill_init: numcolumn_*, zcolumn_* and acc_mass_* are required");
    if (c->maxcolumn < 2) return fail(FPX_ERR_ARG, "domainfill_init: maxcolumn >= 2 (the first height of a column reads the second)");
    if (c->nclassunc < 1) return fail(FPX_ERR_ARG, "domainfill_init: nclassunc >= 1");
    if (!(c->xmassperparticle > 0.) || !std::isfinite(c->xmassperparticle)) return fail(FPX_ERR_ARG, "domainfill_init: xmassperparticle must be positive");
    if (c->nx_we[0] < 0 || c->nx_we[0] > c->nx_we[1] || c->nx_we[1] > cfg.nx - 2 || c->ny_sn[0] < 0 || c->ny_sn[0] > c->ny_sn[1] || c->ny_sn[1] > cfg.ny - 2)
      return fail(FPX_ERR_ARG, "domainfill_init: nx_we must lie in 0 .. nx-2 and ny_sn in 0 .. ny-2, ascending");
    const int nymax = cfg.nymax, nxmax = cfg.nxmax, mc = c->maxcolumn, hb = cfg.host_real_bytes;
    auto rd = [&](const void *p, size_t i) -> double { return hb == 4 ? (double)((const float *)p)[i] : ((const double *)p)[i]; };
    std::vector<df::Loc> locs;
    const double top = height_host[cfg.nz - 1];
    for (int side = 0; side < 2; side++) {
      const int lo = side == 0 ? c->ny_sn[0] : c->nx_we[0], hi = side == 0 ? c->ny_sn[1] : c->nx_we[1], nrow = side == 0 ? nymax : nxmax;
      const int32_t *nc = side == 0 ? c->numcolumn_we : c->numcolumn_sn;
      const void *zc = side == 0 ? c->zcolumn_we : c->zcolumn_sn;
      for (int row = lo; row <= hi; row++)
        for (int k = 0; k < 2; k++) {
          const int n = nc[k + 2 * row];
          if (n < 0 || n > mc) return fail(FPX_ERR_ARG, "domainfill_init: a column with a negative number of heights or more than maxcolumn");
          if (n == 2) return fail(FPX_ERR_ARG, "domainfill_init: a column of exactly two release heights (boundcond_domainfill.f90:117 reads zcolumn(.., 0), outside its array)");
          for (int j = 1; j <= n; j++) {
            if (!(rd(zc, (size_t)k + 2 * ((size_t)row + (size_t)nrow * (j - 1))) < top))
              return fail(FPX_ERR_ARG, "domainfill_init: a release height reaches height(nz) (the level search :134-141 finds nothing)");
            locs.push_back(df::Loc{side, row, k, j});
          }
        }
    }
    dfl_cfg = *c;
    dfl_nc_we.assign(c->numcolumn_we, c->numcolumn_we + (size_t)2 * nymax);
    dfl_nc_sn.assign(c->numcolumn_sn, c->numcolumn_sn + (size_t)2 * nxmax);
    dfl_cfg.numcolumn_we = dfl_cfg.numcolumn_sn = nullptr;
    dfl_cfg.zcolumn_we = dfl_cfg.zcolumn_sn = dfl_cfg.acc_mass_we = dfl_cfg.acc_mass_sn = nullptr;
    dfl_zc_we.assign((const unsigned char *)c->zcolumn_we, (const unsigned char *)c->zcolumn_we + dfl_acc_bytes(0));
    dfl_zc_sn.assign((const unsigned char *)c->zcolumn_sn, (const unsigned char *)c->zcolumn_sn + dfl_acc_bytes(1));
    dfl_locs = std::move(locs);
    hipError_t e = hipSuccess;
    for (int side = 0; side < 2 && e == hipSuccess; side++) {
      const std::vector<int32_t> &nc = side == 0 ? dfl_nc_we : dfl_nc_sn;
      const std::vector<unsigned char> &zc = side == 0 ? dfl_zc_we : dfl_zc_sn;
      const void *acc = side == 0 ? c->acc_mass_we : c->acc_mass_sn;
      if ((e = dfl_d_nc[side].reserve(nc.size() * 4, stream)) == hipSuccess) e = hipMemcpyAsync(dfl_d_nc[side].as(), nc.data(), nc.size() * 4, hipMemcpyHostToDevice, stream);
      if (e == hipSuccess && (e = dfl_d_zc[side].reserve(zc.size(), stream)) == hipSuccess) e = hipMemcpyAsync(dfl_d_zc[side].as(), zc.data(), zc.size(), hipMemcpyHostToDevice, stream);
      for (int b = 0; b < 2 && e == hipSuccess; b++)
        if ((e = dfl_d_acc[b][side].reserve(dfl_acc_bytes(side), stream)) == hipSuccess) e = hipMemcpyAsync(dfl_d_acc[b][side].as(), acc, dfl_acc_bytes(side), hipMemcpyHostToDevice, stream);
    }
    std::vector<unsigned char> hh((size_t)cfg.nz * hb);
    for (int k = 0; k < cfg.nz; k++) { if (hb == 4) ((float *)hh.data())[k] = (float)height_host[k]; else ((double *)hh.data())[k] = height_host[k]; }
    if (e == hipSuccess && (e = dfl_d_height.reserve(hh.size(), stream)) == hipSuccess) e = hipMemcpyAsync(dfl_d_height.as(), hh.data(), hh.size(), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && (e = dfl_d_locs.reserve(dfl_locs.size() * sizeof(df::Loc), stream)) == hipSuccess && !dfl_locs.empty())
      e = hipMemcpyAsync(dfl_d_locs.as(), dfl_locs.data(), dfl_locs.size() * sizeof(df::Loc), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("domainfill_init: ") + hipGetErrorString(e));
    dfl_cur = 0;
    dfl_ran1 = Ran1(); dfl_ran1.idum = -11;
    dfl_on = true;
    return 0;
  }

  template <typename H>
  int boundcond_t(int itime, int64_t *numpart_io, int32_t *npc_io, fpx_domainfill_stats *out) {
    const int nloc = (int)dfl_locs.size();
    const long long cap = P.cap;
    const bool seq = cfg.rng_mode == FPX_RNG_TABLE_SEQ;
    numpart = *numpart_io;
    df::Fields<R, H> F{V.w3, V.r2, (const H *)diag_d3, dfl_d_height.as<H>(), cfg.nx, cfg.ny, cfg.nz, V.m1, V.m2};
    df::Cfg<H> C;
    for (int k = 0; k < 2; k++) { C.nx_we[k] = dfl_cfg.nx_we[k]; C.ny_sn[k] = dfl_cfg.ny_sn[k]; }
    C.nxmax = cfg.nxmax; C.nymax = cfg.nymax; C.maxcolumn = dfl_cfg.maxcolumn;
    C.mdomainfill = cfg.mdomainfill; C.nclassunc = dfl_cfg.nclassunc;
    C.xmpp = (H)dfl_cfg.xmassperparticle;
    C.dx = (H)cfg.dx; C.dy = (H)cfg.dy; C.ylat0 = (H)cfg.ylat0;
    C.dt1 = (H)(itime - V.memtime0); C.dt2 = (H)(V.memtime1 - itime);      // :79-81
    C.dtt = (H)1. / (C.dt1 + C.dt2);
    C.lsync = (H)cfg.lsynctime;
    for (int k = 0; k < 2; k++) {                                          // :334-335, the one libm call, in the host's kind
      C.ylat_sn[k] = C.ylat0 + (H)C.ny_sn[k] * C.dy;
      C.cos_sn[k] = (H)std::cos(C.ylat_sn[k] * ((H)3.14159265 / (H)180.));
    }
    C.nc_we = dfl_d_nc[0].as<int>(); C.nc_sn = dfl_d_nc[1].as<int>();
    C.zc_we = dfl_d_zc[0].as<H>(); C.zc_sn = dfl_d_zc[1].as<H>();
    const int nxt = 1 - dfl_cur;
    hipError_t e = hipSuccess;
    auto need = [&](Scratch &s, size_t bytes) { if (e == hipSuccess) e = s.reserve(bytes, stream); };
    need(dfl_mmass, ((size_t)nloc + 1) * 4); need(dfl_first, ((size_t)nloc + 1) * 4); need(dfl_accv, ((size_t)nloc + 1) * 8);
    need(dfl_accsum, 8); need(dfl_cnt, sizeof(df::Counters)); need(dfl_term, (size_t)std::max<long long>(numpart, 1) * 4);
    size_t tb = 0, tb2 = 0;
    if (e == hipSuccess) {
      (void)rocprim::exclusive_scan(nullptr, tb, dfl_mmass.as<unsigned int>(), dfl_first.as<unsigned int>(), 0u, (size_t)nloc + 1, rocprim::plus<unsigned int>(), stream);
      (void)rocprim::reduce(nullptr, tb2, dfl_accv.as<double>(), dfl_accsum.as<double>(), 0., (size_t)std::max(nloc, 1), rocprim::plus<double>(), stream);
      tb = std::max(tb, tb2);
    }
    need(dfl_tmp, tb);
    Events<5> ev;
    if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("boundcond_domainfill: ") + hipGetErrorString(e));
    df::Counters *cnt = dfl_cnt.as<df::Counters>();
    unsigned int *mmass = dfl_mmass.as<unsigned int>(), *first = dfl_first.as<unsigned int>();
    HIPCHK(hipEventRecord(ev[0], stream));
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(df::Counters), stream));
    HIPCHK(hipMemsetAsync(dfl_accsum.as(), 0, 8, stream));
    // ---- flux, mmass and its scan in the reference's loop order ------------------------------------------------
    std::vector<unsigned int> h_first((size_t)nloc + 1, 0u);
    if (nloc > 0) {
      // the acc_mass of the entries that are no release location carry over
      for (int side = 0; side < 2; side++)
        HIPCHK(hipMemcpyAsync(dfl_d_acc[nxt][side].as(), dfl_d_acc[dfl_cur][side].as(), dfl_acc_bytes(side), hipMemcpyDeviceToDevice, stream));
      HIPCHK(hipMemsetAsync(mmass + nloc, 0, 4, stream));
      df::k_df_flux<R, H><<<(nloc + 255) / 256, 256, 0, stream>>>(F, C, dfl_d_locs.as<df::Loc>(), nloc, dfl_d_acc[dfl_cur][0].as<H>(), dfl_d_acc[dfl_cur][1].as<H>(),
                                                                  dfl_d_acc[nxt][0].as<H>(), dfl_d_acc[nxt][1].as<H>(), mmass, dfl_accv.as<double>());
      HIPCHK(hipGetLastError());
      HIPCHK(rocprim::exclusive_scan(dfl_tmp.as(), tb, mmass, first, 0u, (size_t)nloc + 1, rocprim::plus<unsigned int>(), stream));
      HIPCHK(rocprim::reduce(dfl_tmp.as(), tb2, dfl_accv.as<double>(), dfl_accsum.as<double>(), 0., (size_t)nloc, rocprim::plus<double>(), stream));
      // the one round trip before the end: the launches and the buffers below are sized by the number of candidates
      // (parity mode: the scan itself, which tells the host which candidate draws what)
      if (seq) HIPCHK(hipMemcpyAsync(h_first.data(), first, ((size_t)nloc + 1) * 4, hipMemcpyDeviceToHost, stream));
      else HIPCHK(hipMemcpyAsync(&h_first[nloc], first + nloc, 4, hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipEventRecord(ev[1], stream));
    HIPCHK(hipStreamSynchronize(stream));
    const unsigned int ncand = h_first[nloc];
    if ((long long)ncand > 0x3fffffffll) return fail(FPX_ERR_NOMEM, "boundcond_domainfill: more than 2^30 particles required in one call");
    // ---- stage 1: terminate and flag; the spaces behind numpart are vacant, so the first ncand vacancies lie in 1 .. numpart + ncand
    const long long scan_n = std::min<long long>(cap, std::max<long long>(numpart + (long long)ncand, 1));
    unsigned int *flags = nullptr, *rank = nullptr;
    if (rel_scratch((size_t)scan_n, &flags, &rank)) return fail(FPX_ERR_NOMEM, "boundcond_domainfill: scratch");
    size_t tb3 = 0, tb4 = 0;
    (void)rocprim::exclusive_scan(nullptr, tb3, flags, rank, 0u, (size_t)scan_n, rocprim::plus<unsigned int>(), stream);
    need(dfl_arank, ((size_t)ncand + 1) * 4); need(dfl_ca, ((size_t)ncand + 1) * 4);
    if (e == hipSuccess) (void)rocprim::exclusive_scan(nullptr, tb4, dfl_ca.as<unsigned int>(), dfl_arank.as<unsigned int>(), 0u, (size_t)ncand + 1, rocprim::plus<unsigned int>(), stream);
    void *tmp = nullptr;
    if (e == hipSuccess && rel_scan_tmp(std::max(tb3, tb4), &tmp)) e = hipErrorOutOfMemory;
    need(dfl_target, (size_t)std::max(ncand, 1u) * 4);
    need(dfl_cx, (size_t)ncand * 8); need(dfl_cy, (size_t)ncand * 8); need(dfl_cz, (size_t)ncand * sizeof(H)); need(dfl_cm, (size_t)ncand * sizeof(H));
    need(dfl_cn, (size_t)ncand * 4); need(dfl_uni, (size_t)3 * ncand * sizeof(H));
    if (e != hipSuccess) return fail(FPX_ERR_NOMEM, std::string("boundcond_domainfill: ") + hipGetErrorString(e));
    const int do_x = !cfg.xglobal || dfl_cfg.nx_we[1] != cfg.nx - 2;       // :67
    df::k_df_stage1<R><<<(int)std::min<long long>((scan_n + 255) / 256, 2048), 256, 0, stream>>>(P, slot_map(), numpart, scan_n, itime, (double)(H)dfl_cfg.nx_we[0], (double)(H)dfl_cfg.nx_we[1],
                                                                      (double)(H)dfl_cfg.ny_sn[0], (double)(H)dfl_cfg.ny_sn[1], do_x, flags, dfl_term.as<unsigned int>(), cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(rocprim::exclusive_scan(tmp, tb3, flags, rank, 0u, (size_t)scan_n, rocprim::plus<unsigned int>(), stream));
    HIPCHK(hipEventRecord(ev[2], stream));
    // ---- candidates ------------------------------------------------------------------------------------------------
    df::CandOut<H> O{dfl_cx.as<double>(), dfl_cy.as<double>(), dfl_cz.as<H>(), dfl_cm.as<H>(), dfl_cn.as<int>(), dfl_ca.as<unsigned int>()};
    unsigned int *arank = dfl_arank.as<unsigned int>();
    Ran1 stream_copy = dfl_ran1;                          // the real stream advances only when the call succeeds
    const bool seq2 = seq && cfg.mdomainfill == 2;
    std::vector<H> uni;
    if (ncand > 0) {
      if (seq) {
        uni.resize((size_t)3 * ncand);
        if (seq2) {                                       // the worst case of three per candidate, resolved on the device
          for (size_t i = 0; i < uni.size(); i++) uni[i] = stream_copy.template next<H>();
        } else {                                          // every candidate is accepted: x | y, z at an interior height, nclass
          for (int l = 0; l < nloc; l++) {
            const df::Loc &L = dfl_locs[l];
            const int nc = (L.side == 0 ? dfl_nc_we : dfl_nc_sn)[L.k + 2 * L.row];
            const bool interior = L.j != 1 && L.j != nc;
            for (unsigned int c = h_first[l]; c < h_first[l + 1]; c++) {
              uni[c] = stream_copy.template next<H>();
              uni[(size_t)ncand + c] = interior ? stream_copy.template next<H>() : (H)0;
              uni[(size_t)2 * ncand + c] = stream_copy.template next<H>();
            }
          }
        }
        HIPCHK(hipMemcpyAsync(dfl_uni.as(), uni.data(), uni.size() * sizeof(H), hipMemcpyHostToDevice, stream));
      }
      HIPCHK(hipMemsetAsync(O.accepted + ncand, 0, 4, stream));
      if (seq2) df::k_df_cand_seq<R, H><<<1, 64, 0, stream>>>(F, C, dfl_d_locs.as<df::Loc>(), first, nloc, ncand, dfl_uni.as<H>(), O, cnt);
      else df::k_df_cand<R, H><<<(int)((ncand + 255) / 256), 256, 0, stream>>>(F, C, dfl_d_locs.as<df::Loc>(), first, nloc, ncand, seq ? dfl_uni.as<H>() : (const H *)nullptr,
                                                                            itime, (unsigned long long)cfg.seed, O);
      HIPCHK(hipGetLastError());
      HIPCHK(rocprim::exclusive_scan(tmp, tb4, O.accepted, arank, 0u, (size_t)ncand + 1, rocprim::plus<unsigned int>(), stream));
      k_rel_targets<<<(int)((scan_n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(flags, rank, scan_n, (long long)ncand, dfl_target.as<unsigned int>());
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ev[3], stream));
    // ---- decide, then commit and place (both do nothing when the call fails) ---------------------------------------
    df::k_df_decide<<<1, 64, 0, stream>>>(flags, rank, scan_n, arank, ncand, cnt);
    df::k_df_commit<R><<<64, 256, 0, stream>>>(P, slot_map(), dfl_term.as<unsigned int>(), cnt);
    if (ncand > 0)
      df::k_df_place<R, H><<<(int)((ncand + 255) / 256), 256, 0, stream>>>(P, slot_map(), O, arank, dfl_target.as<unsigned int>(), ncand, itime, (int)*npc_io, cfg.mintime,
                                                                           cfg.ldirect, dfl_cfg.itsplit, cnt);
    HIPCHK(hipGetLastError());
    df::Counters hc;
    double accsum = 0;
    HIPCHK(hipMemcpyAsync(&hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&accsum, dfl_accsum.as(), 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(ev[4], stream));
    HIPCHK(hipStreamSynchronize(stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[0], ev[4]) == hipSuccess) dfl_last_ms = ms;
    for (int k = 0; k < 4; k++) if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) dfl_stage_ms[k] = ms;
    dfl_last_ncand = ncand;
    if (!hc.ok)
      return fail(FPX_ERR_NOMEM, "boundcond_domainfill: too many particles required (boundcond_domainfill.f90:307-310); nothing was changed");
    // ---- the call succeeded: acc_mass, numpart, numparticlecount and the stream follow ------------------------------
    if (nloc > 0) dfl_cur = nxt;
    if (seq) {
      if (seq2) for (unsigned int i = 0; i < hc.consumed; i++) (void)dfl_ran1.template next<H>();
      else dfl_ran1 = stream_copy;
    }
    if (hc.naccepted > 0) numpart = std::max<long long>(numpart, (long long)hc.maxpid + 1);   // :303
    *numpart_io = numpart;
    *npc_io = (int32_t)(*npc_io + (int32_t)hc.naccepted);
    if (hc.naccepted > 0 || hc.nterm > 0) maybe_new = true;
    if (out) {
      out->n_terminated = hc.nterm; out->n_released = hc.naccepted; out->n_rejected = (int64_t)ncand - hc.naccepted;
      out->numactiveparticles = (int64_t)hc.nactive + hc.naccepted; out->accmasst = accsum;
    }
    return 0;
  }
  int boundcond_domainfill(int itime, int64_t *numpart_io, int32_t *npc_io, fpx_domainfill_stats *out) override {
    if (!dfl_on) return fail(FPX_ERR_STATE, "boundcond_domainfill: fpx_domainfill_init first");
    if (comm_ranks > 1) return fail(FPX_ERR_UNSUPPORTED, "boundcond_domainfill: a communicator of several ranks -- the vacancies and the serial stream span the ranks");
    if (!numpart_io || !npc_io) return fail(FPX_ERR_ARG, "boundcond_domainfill: numpart and numparticlecount are required");
    if (*numpart_io < 0 || *numpart_io > P.cap) return fail(FPX_ERR_ARG, "boundcond_domainfill: numpart outside capacity");
    if (out) memset(out, 0, sizeof(*out));
    if (dfl_cfg.gdomainfill) return 0;                                     // :54
    if (!height_set || !window_set || !slot_loaded[0] || !slot_loaded[1]) return fail(FPX_ERR_STATE, "boundcond_domainfill: height, both field slots and the wind-time window must be set first");
    if (!diag_have[DG_PV] || !diag_have[DG_PV + 1]) return fail(FPX_ERR_STATE, "boundcond_domainfill: pv of both slots is needed (fpx_upload_diag_fields or fpx_verttransform_ecmwf)");
    if (P.cap > 0x7fffffffll) return fail(FPX_ERR_UNSUPPORTED, "boundcond_domainfill: more than 2^31 - 1 storage spaces");
    return cfg.host_real_bytes == 4 ? boundcond_t<float>(itime, numpart_io, npc_io, out) : boundcond_t<double>(itime, numpart_io, npc_io, out);
  }
  int domainfill_acc(void *we, void *sn, const void *we_in, const void *sn_in) override {
    if (!dfl_on) return fail(FPX_ERR_STATE, "domainfill_acc: fpx_domainfill_init first");
    void *out[2] = {we, sn};
    const void *in[2] = {we_in, sn_in};
    for (int side = 0; side < 2; side++) {
      if (out[side]) HIPCHK(hipMemcpyAsync(out[side], dfl_d_acc[dfl_cur][side].as(), dfl_acc_bytes(side), hipMemcpyDeviceToHost, stream));
      if (in[side]) HIPCHK(hipMemcpyAsync(dfl_d_acc[dfl_cur][side].as(), in[side], dfl_acc_bytes(side), hipMemcpyHostToDevice, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  int boundcond_output(const char *path) override {
    if (!dfl_on) return fail(FPX_ERR_STATE, "boundcond_output: fpx_domainfill_init first");
    if (!path) return fail(FPX_ERR_ARG, "boundcond_output: path is required");
    std::vector<unsigned char> acc[2];
    for (int side = 0; side < 2; side++) acc[side].resize(dfl_acc_bytes(side));
    int rc = domainfill_acc(acc[0].data(), acc[1].data(), nullptr, nullptr);
    if (rc) return rc;
    const size_t total = (dfl_nc_we.size() + dfl_nc_sn.size()) * 4 + 2 * (dfl_acc_bytes(0) + dfl_acc_bytes(1));
    if (total > RecFile::kMaxRecord) return fail(FPX_ERR_UNSUPPORTED, "boundcond_output: the record exceeds 2 GiB (the reference's compiler would split it into subrecords)");
    RecFile file(path);
    if (!file.is_open()) return fail(FPX_ERR_ARG, std::string("boundcond_output: cannot open ") + path);
    // :568-572, one sequential unformatted record
    file.put(dfl_nc_we.data(), dfl_nc_we.size() * 4); file.put(dfl_nc_sn.data(), dfl_nc_sn.size() * 4);
    file.put(dfl_zc_we.data(), dfl_zc_we.size()); file.put(dfl_zc_sn.data(), dfl_zc_sn.size());
    file.put(acc[0].data(), acc[0].size()); file.put(acc[1].data(), acc[1].size());
    file.end();
    if (!file.close()) return fail(FPX_ERR_ARG, std::string("boundcond_output: write error on ") + path);
    return 0;
  }
  double domainfill_ms() override { return dfl_last_ms; }

  // ---- nested grids --------------------------------------------------------------
  int nest_nxmaxn = 0, nest_nymaxn = 0;
  bool nest_loaded[kMaxNests][2] = {};
  NestDesc<R> h_nest[kMaxNests] = {};   // host copy of the device table V.nest
  double nest_geo[kMaxNests][6] = {};   // xln, yln, xrn, yrn, xresoln, yresoln as the host gave them (fpx_ohreaction compares in the host's kind)
  int nests_init(const fpx_nests *n) override {
    if (!n || n->struct_bytes != (int32_t)sizeof(fpx_nests)) return fail(FPX_ERR_ARG, "nests_init: null or fpx_nests size mismatch (ABI)");
    if (n->numbnests < 1 || n->numbnests > kMaxNests) return fail(FPX_ERR_ARG, "nests_init: numbnests out of range");
    if (V.numbnests) return fail(FPX_ERR_STATE, "nests_init: already initialised");
    if (conv_gfs) return fail(FPX_ERR_UNSUPPORTED, "nests_init: fpx_conv_init_gfs has run on this handle: the reference has no GFS nests");
    if (cfg.interpolhmix) return fail(FPX_ERR_UNSUPPORTED, "nests_init: interpolhmix with nested wind fields -- the reference reads the unset h1 for a particle inside a nest (advance.f90:254-266)");
    int rc;
    for (int l = 0; l < n->numbnests; l++) {
      if (n->nxn[l] < 2 || n->nyn[l] < 2 || n->nxn[l] > n->nxmaxn || n->nyn[l] > n->nymaxn) return fail(FPX_ERR_ARG, "nests_init: bad nest extents");
      if ((long long)n->nxn[l] * n->nyn[l] * cfg.nz > 0xFFFFFFF0ll) return fail(FPX_ERR_ARG, "nests_init: nest too large: nxn*nyn*nz must fit 32 bits");
      if (!(n->xln[l] >= 0 && n->yln[l] >= 0 && n->xrn[l] <= cfg.nx - 1 && n->yrn[l] <= cfg.ny - 1)) return fail(FPX_ERR_ARG, "nests_init: nest outside the mother grid (gridcheck_nests.f90:381)");
      NestDesc<R> &N = h_nest[l];
      N.nx = n->nxn[l]; N.ny = n->nyn[l];
      N.xl = (R)n->xln[l]; N.yl = (R)n->yln[l]; N.xr = (R)n->xrn[l]; N.yr = (R)n->yrn[l];
      N.xres = (R)n->xresoln[l]; N.yres = (R)n->yresoln[l];
      nest_geo[l][0] = n->xln[l]; nest_geo[l][1] = n->yln[l]; nest_geo[l][2] = n->xrn[l]; nest_geo[l][3] = n->yrn[l]; nest_geo[l][4] = n->xresoln[l]; nest_geo[l][5] = n->yresoln[l];
      const size_t ncol = (size_t)n->nxn[l] * n->nyn[l], nlev = ncol * cfg.nz;
      R *p;
      if ((rc = dalloc(&p, nlev * 6))) return rc; N.w3 = p;
      if ((rc = dalloc(&p, nlev * 4))) return rc; N.r2 = p;
      if ((rc = dalloc(&p, ncol * 8))) return rc; N.sfc = p;
      if ((rc = dalloc(&p, ncol))) return rc; N.hcell = p;
      if ((rc = dalloc(&p, ncol))) return rc; N.tropo = p;
      if (cfg.drydep) { if ((rc = dalloc(&p, ncol * 2 * cfg.nspec))) return rc; N.vdep = p; }
    }
    nest_nxmaxn = n->nxmaxn; nest_nymaxn = n->nymaxn;
    NestDesc<R> *dn;
    if ((rc = dalloc(&dn, (size_t)n->numbnests))) return rc;
    HIPCHK(hipMemcpyAsync(dn, h_nest, sizeof(NestDesc<R>) * n->numbnests, hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    V.nest = dn;
    V.numbnests = n->numbnests;
    return 0;
  }
  // ---- wet deposition -----------------------------------------------------------
  int wet_init(const fpx_wet_config *w) override {
    if (!w || w->struct_bytes != (int32_t)sizeof(fpx_wet_config)) return fail(FPX_ERR_ARG, "wet_init: null or fpx_wet_config size mismatch (ABI)");
    if (wet_on) return fail(FPX_ERR_STATE, "wet_init: already initialised");
    memset(&Wp, 0, sizeof(Wp));
    for (int i = 0; i < FPX_MAXSPEC; i++) {
      Wp.wetdepspec[i] = w->wetdepspec[i];
      Wp.weta_gas[i] = (R)w->weta_gas[i]; Wp.wetb_gas[i] = (R)w->wetb_gas[i];
      Wp.crain_aero[i] = (R)w->crain_aero[i]; Wp.csnow_aero[i] = (R)w->csnow_aero[i];
      Wp.ccn_aero[i] = (R)std::max(w->ccn_aero[i], 0.0);   // get_wetscav.f90:257-258
      Wp.in_aero[i] = (R)std::max(w->in_aero[i], 0.0);
      Wp.henry[i] = (R)w->henry[i];
    }
    Wp.readclouds = w->readclouds;
    const size_t ncol = (size_t)cfg.nx * cfg.ny, nlev = ncol * cfg.nz;
    int rc;
    R *p;
    signed char *c8;
    if ((rc = dalloc(&p, ncol * 6))) return rc; Wp.prec = p;
    if ((rc = dalloc(&p, ncol * 2))) return rc; Wp.ctwc = p;
    HIPCHK(hipMemsetAsync(p, 0, ncol * 2 * sizeof(R), stream));
    if ((rc = dalloc(&p, nlev * 2))) return rc; Wp.ttw = p;
    if ((rc = dalloc(&c8, nlev * 2))) return rc; Wp.clouds = c8;
    HIPCHK(hipStreamSynchronize(stream));
    wet_on = true;
    return 0;
  }
  // lsprec, convprec, tcc, ctwc, tt, clouds of one grid and time slot (a nest's: lsprecn ... with strides nxmaxn, nymaxn, nzmax)
  int upload_wet(int g, int slot, const fpx_wet_fields *f, int readclouds_nest) {
    const HostGrid G = host_grid(g);
    const int s = slot - 1;
    int rc;
    if (g > 0) {   // a nest's packs are allocated with its first upload
      WetNest<R> &W = h_wnest[g - 1];
      if (!W.prec) {
        const size_t ncol = (size_t)G.nx * G.ny;
        R *p; signed char *q;
        if ((rc = dalloc(&p, ncol * 6))) return rc; W.prec = p;
        if ((rc = dalloc(&p, ncol * 2))) return rc; W.ctwc = p;
        if ((rc = dalloc(&p, ncol * cfg.nz * 2))) return rc; W.ttw = p;
        if ((rc = dalloc(&q, ncol * cfg.nz * 2))) return rc; W.clouds = q;
        if (!d_wnest) { if ((rc = dalloc(&d_wnest, (size_t)kMaxNests))) return rc; }
      }
      W.readclouds = readclouds_nest ? 1 : 0;
    }
    const WetNest<R> W = g > 0 ? h_wnest[g - 1] : WetNest<R>{Wp.prec, Wp.ctwc, Wp.ttw, Wp.clouds, Wp.readclouds};
    if ((rc = p2(G, f->lsprec, W.prec, 6, s * 3 + 0)) || (rc = p2(G, f->convprec, W.prec, 6, s * 3 + 1)) || (rc = p2(G, f->tcc, W.prec, 6, s * 3 + 2))) return rc;
    if (f->ctwc && (rc = p2(G, f->ctwc, W.ctwc, 2, s))) return rc;
    if ((rc = p3(G, f->tt, W.ttw, 2, s))) return rc;
    if ((rc = pack3<signed char>(G, f->clouds, (signed char *)W.clouds, 2, s))) return rc;   // integer(1) cloud classes: same x<->z transpose
    if (g > 0) {   // the kernels find the nests' packs through the device table
      HIPCHK(hipMemcpyAsync(d_wnest, h_wnest, sizeof(h_wnest), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));
      Wp.nest = d_wnest;
      wet_nest_slot[g - 1][s] = true;
    } else wet_slot[s] = true;
    return 0;
  }
  int upload_wet_fields(int slot, const fpx_wet_fields *f) override {
    if (!wet_on) return fail(FPX_ERR_STATE, "upload_wet_fields: fpx_wet_init first");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "upload_wet_fields: slot must be 1 or 2");
    if (!f || !f->lsprec || !f->convprec || !f->tcc || !f->tt || !f->clouds) return fail(FPX_ERR_ARG, "upload_wet_fields: lsprec, convprec, tcc, tt, clouds are required");
    if (Wp.readclouds && !f->ctwc) return fail(FPX_ERR_ARG, "upload_wet_fields: ctwc required with readclouds");
    return upload_wet(0, slot, f, 0);
  }
  int upload_wet_nest_fields(int nest, int slot, const fpx_wet_fields *f, int readclouds_nest) override {
    if (!wet_on) return fail(FPX_ERR_STATE, "upload_wet_nest_fields: fpx_wet_init first");
    if (nest < 1 || nest > V.numbnests) return fail(FPX_ERR_ARG, "upload_wet_nest_fields: nest out of range (fpx_nests_init first)");
    if (slot != 1 && slot != 2) return fail(FPX_ERR_ARG, "upload_wet_nest_fields: slot must be 1 or 2");
    if (!f || !f->lsprec || !f->convprec || !f->tcc || !f->tt || !f->clouds) return fail(FPX_ERR_ARG, "upload_wet_nest_fields: lsprecn, convprecn, tccn, ttn, cloudsn are required");
    if (readclouds_nest && !f->ctwc) return fail(FPX_ERR_ARG, "upload_wet_nest_fields: ctwcn required with readclouds_nest");
    return upload_wet(nest, slot, f, readclouds_nest);
  }
  int wetdepo(int itime, int ltsample, int loutnext) override {
    if (!wet_on || !wet_slot[0] || !wet_slot[1]) return fail(FPX_ERR_STATE, "wetdepo: fpx_wet_init and both slots of fpx_upload_wet_fields first");
    for (int l = 0; l < V.numbnests; l++)   // get_wetscav.f90:126-128 reads the nest's own fields for a particle inside a nest
      if (!wet_nest_slot[l][0] || !wet_nest_slot[l][1]) return fail(FPX_ERR_STATE, "wetdepo: nested grids are configured: fpx_upload_wet_nest_fields (both slots) for every nest first");
    if (!height_set || !window_set) return fail(FPX_ERR_STATE, "wetdepo: height / wind-time window not set");
    if (numpart == 0) return 0;
    const int nb = (int)((numpart + kBlock - 1) / kBlock);
    sum_wet.invalidate(); sum_wetn.invalidate();           // k_wetdepo adds to wetgridunc / wetgriduncn
    // (wave_kernel_add needs every lane of the wave: whole blocks of kBlock, no early return in the kernel)
    k_wetdepo<R><<<nb, kBlock, 0, stream>>>(V, Gp, Wp, P, numpart, itime, ltsample, loutnext);
    HIPCHK(hipGetLastError());
    return 0;
  }
  int get_wetgrid(void *wetgridunc, int allreduce) override {
    if (!Gp.on) return fail(FPX_ERR_STATE, "get_wetgrid: fpx_outgrid_init first");
    return fetch({{&sum_wet, Gp.wetgridunc, wetgridunc, false, false}}, allreduce, "get_wetgrid");   // mpi_mod.f90:2486-2488, into wetgridunc0
  }

  // ---- OH chemistry (fpx_ohreaction.hpp; gethourlyOH.f90, ohreaction.f90) --------------------------------------
  // Nothing here exists before fpx_oh_init.  oh_mod lives on the host side in the host's real kind (oh4 or oh8), where
  // gethourlyOH runs; the device holds the two hourly fields, their blend, the three axes and the counter of skipped particles.
  oh::Hourly<float> oh4;
  oh::Hourly<double> oh8;
  bool oh_on = false, oh_have_hourly = false;
  int oh_branch = -1;
  void *oh_d_hourly = nullptr, *oh_d_blend = nullptr, *oh_d_axes = nullptr;
  unsigned int *oh_d_skipped = nullptr;
  double oh_cc[FPX_MAXSPEC] = {}, oh_dc[FPX_MAXSPEC] = {}, oh_nc[FPX_MAXSPEC] = {};
  Events<2> oh_ev;
  bool oh_timed = false, oh_ev_made = false;
  oh::Hourly<float> &oh_state(float *) { return oh4; }
  oh::Hourly<double> &oh_state(double *) { return oh8; }
  template <typename H> oh::Hourly<H> &oh_state() { return oh_state((H *)nullptr); }
  template <typename H>
  int oh_init_t(const fpx_oh_config *c) {
    oh::Hourly<H> &S = oh_state<H>();
    S.nx = c->nxOH; S.ny = c->nyOH; S.nz = c->nzOH; S.ldirect = cfg.ldirect; S.bdate = c->bdate;
    const size_t cells = S.cells();
    auto take = [](std::vector<H> &v, const void *p, size_t n) { v.assign((const H *)p, (const H *)p + n); };
    take(S.lon, c->lonOH, S.nx); take(S.lat, c->latOH, S.ny); take(S.alt, c->altOH, S.nz);
    std::vector<H> axes((size_t)S.nx + S.ny + S.nz);
    std::copy(S.lon.begin(), S.lon.end(), axes.begin());
    std::copy(S.lat.begin(), S.lat.end(), axes.begin() + S.nx);
    oh::alt_tops(S.alt.data(), S.nz, axes.data() + S.nx + S.ny);
    const char *names[3] = {"lonOH", "latOH", "altOHtop (ohreaction.f90:114-117; its first nzOH-1 entries, the last repeats the one before)"};
    const int lens[3] = {S.nx, S.ny, S.nz - 1}, offs[3] = {0, S.nx, S.nx + S.ny};
    for (int a = 0; a < 3; a++)
      if (const char *why = oh::check_axis(axes.data() + offs[a], lens[a]))
        return fail(FPX_ERR_UNSUPPORTED, std::string("oh_init: ") + names[a] + " " + why + ": the nearest-index search of fpx_ohreaction bisects a strictly increasing axis");
    take(S.field, c->OH_field, cells * 12); take(S.jr, c->jrate_average, (size_t)360 * 180 * 12);
    take(S.lonjr, c->lonjr, 360); take(S.latjr, c->latjr, 180);
    S.prepare();
    int rc;
    H *p;
    if ((rc = dalloc(&p, cells * 2))) return rc; oh_d_hourly = p;
    if ((rc = dalloc(&p, cells))) return rc; oh_d_blend = p;
    if ((rc = dalloc(&p, axes.size()))) return rc; oh_d_axes = p;
    if ((rc = dalloc(&oh_d_skipped, 1))) return rc;
    HIPCHK(hipMemcpyAsync(oh_d_axes, axes.data(), axes.size() * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(oh_d_hourly, 0, cells * 2 * sizeof(H), stream));
    HIPCHK(hipMemsetAsync(oh_d_skipped, 0, sizeof(unsigned int), stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  int oh_init(const fpx_oh_config *c) override {
    if (!c || c->struct_bytes != (int32_t)sizeof(fpx_oh_config)) return fail(FPX_ERR_ARG, "oh_init: null or fpx_oh_config size mismatch (ABI)");
    if (oh_on) return fail(FPX_ERR_STATE, "oh_init: already initialised");
    if (!c->lonOH || !c->latOH || !c->altOH || !c->OH_field || !c->jrate_average || !c->lonjr || !c->latjr) return fail(FPX_ERR_ARG, "oh_init: lonOH, latOH, altOH, OH_field, jrate_average, lonjr, latjr are required");
    if (c->nxOH < 1 || c->nyOH < 1 || c->nzOH < 2) return fail(FPX_ERR_ARG, "oh_init: nxOH, nyOH >= 1 and nzOH >= 2 are required (altOHtop, ohreaction.f90:114-117)");
    if ((long long)c->nxOH * c->nyOH * c->nzOH > 0x7FFFFFF0ll) return fail(FPX_ERR_ARG, "oh_init: OH grid too large");
    if (oh_lds_bytes(c->nxOH, c->nyOH, c->nzOH) > 48 * 1024) return fail(FPX_ERR_UNSUPPORTED, "oh_init: lonOH, latOH, altOHtop and height do not fit the 48 KB of LDS k_ohreaction stages them in");
    for (int l = 0; l < V.numbnests; l++)
      if (h_nest[l].nx > cfg.nx || h_nest[l].ny > cfg.ny)
        return fail(FPX_ERR_UNSUPPORTED, "oh_init: a nest with nxn > nx or nyn > ny: ohreaction.f90:133 reads tt of the mother grid with the nest's indices, there beyond the field");
    bool any = false;
    for (int k = 0; k < cfg.nspec; k++) {
      oh_cc[k] = c->ohcconst[k]; oh_dc[k] = c->ohdconst[k]; oh_nc[k] = c->ohnconst[k];
      any = any || oh_cc[k] > 0.;
    }
    if (!any) return fail(FPX_ERR_ARG, "oh_init: no species has ohcconst > 0: there is no reaction to compute (readreleases.f90:377-380)");
    const int rc = cfg.host_real_bytes == 4 ? oh_init_t<float>(c) : oh_init_t<double>(c);
    if (rc) return rc;
    oh_on = true;
    return 0;
  }
  size_t oh_lds_bytes(int nxo, int nyo, int nzo) const { return ((size_t)nxo + nyo + nzo + 1) * cfg.host_real_bytes + (size_t)cfg.nz * sizeof(R); }
  template <typename H>
  int oh_upload(int first, int count) {      // fields first .. first + count - 1 of OH_hourly to the device
    const oh::Hourly<H> &S = oh_state<H>();
    HIPCHK(hipMemcpyAsync((H *)oh_d_hourly + (size_t)first * S.cells(), S.hourly.data() + (size_t)first * S.cells(), (size_t)count * S.cells() * sizeof(H), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
  }
  template <typename H>
  int gethourlyOH_t(int itime) {
    oh::Hourly<H> &S = oh_state<H>();
    oh_branch = S.step(itime);
    if (oh_branch == oh::BR_ADVANCE) {     // OH_hourly(:,:,:,1) = OH_hourly(:,:,:,2) on the device too; the new field 2 is uploaded
      HIPCHK(hipMemcpyAsync(oh_d_hourly, (const H *)oh_d_hourly + S.cells(), S.cells() * sizeof(H), hipMemcpyDeviceToDevice, stream));
      return oh_upload<H>(1, 1);
    }
    if (oh_branch == oh::BR_INIT) return oh_upload<H>(0, 2);
    return 0;
  }
  int gethourlyOH(int itime) override {
    if (!oh_on) return fail(FPX_ERR_STATE, "gethourlyOH: fpx_oh_init first");
    const int rc = cfg.host_real_bytes == 4 ? gethourlyOH_t<float>(itime) : gethourlyOH_t<double>(itime);
    if (!rc) oh_have_hourly = true;
    return rc;
  }
  template <typename H>
  int oh_hourly_io(void *field, void *mt, bool set) {
    oh::Hourly<H> &S = oh_state<H>();
    if (set) {
      if (field) std::copy((const H *)field, (const H *)field + 2 * S.cells(), S.hourly.begin());
      if (mt) { S.memtime[0] = ((const H *)mt)[0]; S.memtime[1] = ((const H *)mt)[1]; }
      return field ? oh_upload<H>(0, 2) : 0;
    }
    if (field) std::copy(S.hourly.begin(), S.hourly.end(), (H *)field);
    if (mt) { ((H *)mt)[0] = S.memtime[0]; ((H *)mt)[1] = S.memtime[1]; }
    return 0;
  }
  int get_oh_hourly(void *oh_hourly, void *memohtime) override {
    if (!oh_on) return fail(FPX_ERR_STATE, "get_oh_hourly: fpx_oh_init first");
    return cfg.host_real_bytes == 4 ? oh_hourly_io<float>(oh_hourly, memohtime, false) : oh_hourly_io<double>(oh_hourly, memohtime, false);
  }
  int set_oh_hourly(const void *oh_hourly, const void *memohtime) override {
    if (!oh_on) return fail(FPX_ERR_STATE, "set_oh_hourly: fpx_oh_init first");
    if (!oh_hourly || !memohtime) return fail(FPX_ERR_ARG, "set_oh_hourly: OH_hourly and memOHtime are required");
    const int rc = cfg.host_real_bytes == 4 ? oh_hourly_io<float>((void *)oh_hourly, (void *)memohtime, true) : oh_hourly_io<double>((void *)oh_hourly, (void *)memohtime, true);
    if (!rc) oh_have_hourly = true;
    return rc;
  }
  template <typename H>
  int ohreaction_t(int itime, int ltsample) {
#pragma clang fp contract(off)
    const oh::Hourly<H> &S = oh_state<H>();
    if (S.memtime[1] == S.memtime[0]) return fail(FPX_ERR_STATE, "ohreaction: memOHtime(1) == memOHtime(2)");
    // n of ohreaction.f90:85-87: nint(itime - 0.5*ltsample) in the default kind, the slot itself (not memind(n))
    const long long interp_time = (long long)std::llround((H)itime - (H)0.5 * (H)ltsample);
    const int slot = std::llabs((long long)V.memtime0 - interp_time) < std::llabs((long long)V.memtime1 - interp_time) ? 0 : 1;
    if (!diag_have[DG_TT + slot]) return fail(FPX_ERR_STATE, std::string("ohreaction: tt of time slot ") + (slot ? "2" : "1") + " is not on the device (fpx_upload_diag_fields or a transform); ohreaction.f90:85-87,133 reads that slot, not memind's");
    oh::Args<H> A;
    memset(&A, 0, sizeof(A));
    A.nxOH = S.nx; A.nyOH = S.ny; A.nzOH = S.nz; A.nztop = S.nz - 1;
    A.lon = (const H *)oh_d_axes; A.lat = A.lon + S.nx; A.alttop = A.lat + S.ny;
    A.oh = (const H *)oh_d_blend;
    A.d3 = (const H *)diag_d3;
    A.nx = cfg.nx; A.ny = cfg.ny; A.nz = cfg.nz;
    A.slot = slot;
    A.dx = (H)cfg.dx; A.dy = (H)cfg.dy; A.xlon0 = (H)cfg.xlon0; A.ylat0 = (H)cfg.ylat0;
    A.numbnests = V.numbnests;
    for (int l = 0; l < V.numbnests; l++) {
      A.xl[l] = (H)nest_geo[l][0]; A.yl[l] = (H)nest_geo[l][1]; A.xr[l] = (H)nest_geo[l][2]; A.yr[l] = (H)nest_geo[l][3];
      A.xres[l] = (H)nest_geo[l][4]; A.yres[l] = (H)nest_geo[l][5];
    }
    for (int k = 0; k < cfg.nspec; k++)
      if (oh_cc[k] > 0.) { A.spec[A.nreact] = k; A.cc[A.nreact] = (H)oh_cc[k]; A.dc[A.nreact] = (H)oh_dc[k]; A.nc[A.nreact] = (H)oh_nc[k]; A.nreact++; }
    A.tl = (H)std::abs(ltsample);
    A.small = (H)std::numeric_limits<R>::min();
    A.skipped = oh_d_skipped;
    const H tnum = (H)itime - S.memtime[0], tden = S.memtime[1] - S.memtime[0];
    if (!oh_ev_made) { HIPCHK(oh_ev.create()); oh_ev_made = true; }
    oh_timed = false;
    HIPCHK(hipMemsetAsync(oh_d_skipped, 0, sizeof(unsigned int), stream));
    HIPCHK(hipEventRecord(oh_ev[0], stream));
    const long long cells = (long long)S.cells();
    oh::k_oh_blend<H><<<(int)((cells + 255) / 256), 256, 0, stream>>>((const H *)oh_d_hourly, (const H *)oh_d_hourly + cells, tnum, tden, (H *)oh_d_blend, cells);
    HIPCHK(hipGetLastError());
    if (numpart > 0) {
      oh::k_ohreaction<R, H><<<(int)((numpart + 255) / 256), 256, oh_lds_bytes(S.nx, S.ny, S.nz), stream>>>(A, P, V.height, numpart);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(oh_ev[1], stream));
    oh_timed = true;
    return 0;
  }
  int ohreaction(int itime, int ltsample, int loutnext) override {
    (void)loutnext;                        // ldeltat of ohreaction.f90:47-51 is never read
    if (!oh_on) return fail(FPX_ERR_STATE, "ohreaction: fpx_oh_init first");
    if (!oh_have_hourly) return fail(FPX_ERR_STATE, "ohreaction: no hourly OH fields yet (fpx_gethourlyOH or fpx_set_oh_hourly first)");
    if (!height_set || !window_set) return fail(FPX_ERR_STATE, "ohreaction: height / wind-time window not set");
    return cfg.host_real_bytes == 4 ? ohreaction_t<float>(itime, ltsample) : ohreaction_t<double>(itime, ltsample);
  }
  int ohreaction_ms(double *ms) override {
    *ms = 0.;
    if (!oh_timed) return 0;
    float t = 0;
    HIPCHK(hipEventSynchronize(oh_ev[1]));
    HIPCHK(hipEventElapsedTime(&t, oh_ev[0], oh_ev[1]));
    *ms = t;
    return 0;
  }
  // checkpoint, bit 3 of header.reserved: last, what gethourlyOH carries from hour to hour -- it cannot be recomputed from itime
  // (the first call's memOHtime(1) = 0 and its date): uint64 cells of the OH grid, int32 whether hourly fields exist, int32 0,
  // memOHtime(2) and OH_hourly(nxOH,nyOH,nzOH,2) in the host's real kind
  static constexpr int32_t kCkptOh = 8;
  uint64_t oh_cells() const { return cfg.host_real_bytes == 4 ? oh4.cells() : oh8.cells(); }
  uint64_t ckpt_oh_bytes(const CkptHeader &h) const { return (h.reserved & kCkptOh) ? 16 + (2 + 2 * oh_cells()) * (uint64_t)cfg.host_real_bytes : 0; }
  template <typename H>
  int ckpt_put_oh(FILE *fh) {
    const oh::Hourly<H> &S = oh_state<H>();
    const uint64_t cnt = S.cells();
    const int32_t have[2] = {oh_have_hourly ? 1 : 0, 0};
    if (fwrite(&cnt, 8, 1, fh) != 1 || fwrite(have, 4, 2, fh) != 2 || fwrite(S.memtime, sizeof(H), 2, fh) != 2 ||
        fwrite(S.hourly.data(), sizeof(H), S.hourly.size(), fh) != S.hourly.size()) return fail(FPX_ERR_ARG, "checkpoint_write: write error");
    return 0;
  }
  template <typename H>
  int ckpt_get_oh(FILE *fh) {
    oh::Hourly<H> &S = oh_state<H>();
    uint64_t cnt = 0;
    int32_t have[2] = {0, 0};
    if (fread(&cnt, 8, 1, fh) != 1 || cnt != S.cells() || fread(have, 4, 2, fh) != 2 || fread(S.memtime, sizeof(H), 2, fh) != 2 ||
        fread(S.hourly.data(), sizeof(H), S.hourly.size(), fh) != S.hourly.size()) return fail(FPX_ERR_ARG, "checkpoint_read: the OH section is short or of another OH grid");
    oh_have_hourly = have[0] != 0;
    return oh_upload<H>(0, 2);
  }

  void *stream_ptr() override { return (void *)stream; }
};


FPX_TU_CLOSE
#if FPX_TU_REAL != 8
EngineBase *make_engine_f32(const fpx_config *cfg, int *rc) {
  auto *p = new (std::nothrow) Engine<float>();
  if (!p) { *rc = fail(FPX_ERR_NOMEM, "fpx_create: out of host memory"); return nullptr; }
  *rc = p->init(cfg);
  return p;
}
#endif
#if FPX_TU_REAL != 4
const void *step_kernel_prep_f64(bool, bool, bool, bool);
const void *step_kernel_prep_f32(bool, bool, bool, bool);
const void *step_kernel_loop_f64(bool, int, int, int, bool, bool *);
const void *step_kernel_loop_f32(bool, int, int, int, bool, bool *);
const void *step_kernel_finish_f64(bool, bool, bool);
const void *step_kernel_finish_f32(bool, bool, bool);
const void *step_kernel_prep(int rb, bool drydep, bool init, bool polar, bool nest) {
  return rb == 8 ? step_kernel_prep_f64(drydep, init, polar, nest) : step_kernel_prep_f32(drydep, init, polar, nest);
}
const void *step_kernel_loop(int rb, bool lean, int turbswitch, int cblflag, int rng_mode, bool susp, bool *is_lean) {
  return rb == 8 ? step_kernel_loop_f64(lean, turbswitch, cblflag, rng_mode, susp, is_lean) : step_kernel_loop_f32(lean, turbswitch, cblflag, rng_mode, susp, is_lean);
}
const void *step_kernel_finish(int rb, bool drydep, bool polar, bool nest) {
  return rb == 8 ? step_kernel_finish_f64(drydep, polar, nest) : step_kernel_finish_f32(drydep, polar, nest);
}
#endif
}  // namespace fpx

#if FPX_TU_REAL != 4
// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
struct fpx_engine {
  fpx::EngineBase *impl;
};

#define FPX_GUARD(h)                                                   \
  if (!(h) || !(h)->impl) return fpx::fail(FPX_ERR_ARG, "null handle")

extern "C" {

int fpx_abi_version(void) { return 4; }

int fpx_polar_maps(int32_t host_real_bytes, double dy, double north[9], double south[9]) {
  if (!north || !south || !(dy > 0)) return fpx::fail(FPX_ERR_ARG, "fpx_polar_maps: bad argument");
  if (host_real_bytes == 4) {
    float n[9], s[9];
    fpx::polar_maps<float>((float)dy, n, s);
    for (int i = 0; i < 9; i++) { north[i] = n[i]; south[i] = s[i]; }
  } else if (host_real_bytes == 8) {
    fpx::polar_maps<double>(dy, north, south);
  } else {
    return fpx::fail(FPX_ERR_ARG, "fpx_polar_maps: host_real_bytes must be 4 or 8");
  }
  return FPX_OK;
}
const char *fpx_last_error(void) { return fpx::g_err.c_str(); }

int fpx_create(fpx_handle *out, const fpx_config *cfg) {
  if (!out || !cfg) return fpx::fail(FPX_ERR_ARG, "fpx_create: null argument");
  *out = nullptr;
  if (cfg->struct_bytes != (int32_t)sizeof(fpx_config)) return fpx::fail(FPX_ERR_ARG, "fpx_create: fpx_config size mismatch (ABI)");
  if (cfg->host_real_bytes != 4 && cfg->host_real_bytes != 8) return fpx::fail(FPX_ERR_ARG, "fpx_create: host_real_bytes must be 4 or 8");
  if (cfg->rng_mode < 0 || cfg->rng_mode > 2) return fpx::fail(FPX_ERR_ARG, "fpx_create: bad rng_mode");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fpx::fail(FPX_ERR_DEVICE, "fpx_create: no HIP device visible");
  if (cfg->device < 0 || cfg->device >= ndev) return fpx::fail(FPX_ERR_ARG, "fpx_create: device ordinal out of range");
  fpx::EngineBase *e = nullptr;
  int rc;
  if (cfg->compute_real_bytes == 8) {
    auto *p = new (std::nothrow) fpx::Engine<double>();
    if (!p) return fpx::fail(FPX_ERR_NOMEM, "fpx_create: out of host memory");
    rc = p->init(cfg);
    e = p;
  } else if (cfg->compute_real_bytes == 4) {
    e = fpx::make_engine_f32(cfg, &rc);
    if (!e) return rc;
  } else {
    return fpx::fail(FPX_ERR_ARG, "fpx_create: compute_real_bytes must be 4 or 8");
  }
  if (rc) { delete e; return rc; }
  fpx_engine *h = new (std::nothrow) fpx_engine{e};
  if (!h) { delete e; return fpx::fail(FPX_ERR_NOMEM, "fpx_create: out of host memory"); }
  *out = h;
  return FPX_OK;
}

int fpx_destroy(fpx_handle h) {
  if (!h) return FPX_OK;
  delete h->impl;
  delete h;
  return FPX_OK;
}

int fpx_set_height(fpx_handle h, const void *height, int32_t n) { FPX_GUARD(h); return h->impl->set_height(height, n); }
int fpx_upload_fields(fpx_handle h, int32_t slot, const fpx_fields *f) { FPX_GUARD(h); return h->impl->upload_fields(slot, f); }
int fpx_verttransform_ecmwf(fpx_handle h, int32_t slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out) { FPX_GUARD(h); return h->impl->verttransform(slot, m, sfc, out); }
int fpx_verttransform_nest(fpx_handle h, int32_t nest, int32_t slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out) { FPX_GUARD(h); return h->impl->verttransform_nest(nest, slot, m, sfc, out); }
int fpx_verttransform_gfs(fpx_handle h, int32_t slot, const fpx_model_levels *m, const fpx_fields *sfc, const fpx_fields_out *out, void *pplev_out) { FPX_GUARD(h); return h->impl->verttransform_gfs(slot, m, sfc, out, pplev_out); }
int fpx_upload_diag_fields(fpx_handle h, int32_t slot, const fpx_diag_fields *f) { FPX_GUARD(h); return h->impl->upload_diag_fields(slot, f); }
int fpx_partoutput(fpx_handle h, int32_t itime, const char *path, int64_t *nparticles) { FPX_GUARD(h); return h->impl->partoutput(itime, path, nparticles); }
int fpx_readpartpositions(fpx_handle h, const char *path, const fpx_restart *r, int64_t *numpart, int32_t *numparticlecount, int32_t *itimein) {
  FPX_GUARD(h);
  return h->impl->readpartpositions(path, r, numpart, numparticlecount, itimein);
}
int fpx_concoutput(fpx_handle h, int32_t itime, const fpx_concout *c, const char *prefix, int32_t clear) { FPX_GUARD(h); return h->impl->concoutput(itime, c, prefix, clear); }
int fpx_partoutput_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_partoutput_time: null"); *ms = h->impl->po_ms(); return FPX_OK; }
int fpx_calcpar(fpx_handle h, int32_t slot, const fpx_calcpar_in *c, const fpx_calcpar_out *out) { FPX_GUARD(h); return h->impl->calcpar(slot, c, out); }
int fpx_getvdep_init(fpx_handle h, const fpx_getvdep_tables *t) { FPX_GUARD(h); return h->impl->getvdep_init(t); }
int fpx_getvdep(fpx_handle h, int32_t slot, const fpx_getvdep_in *g, void *vdep_out) { FPX_GUARD(h); return h->impl->getvdep(slot, g, vdep_out); }
int fpx_calcpar_nest(fpx_handle h, int32_t nest, int32_t slot, const fpx_calcpar_in *c, const fpx_calcpar_out *out) { FPX_GUARD(h); return h->impl->calcpar_nest(nest, slot, c, out); }
int fpx_calcpar_gfs(fpx_handle h, int32_t slot, const fpx_calcpar_gfs_in *c, const fpx_calcpar_out *out) { FPX_GUARD(h); return h->impl->calcpar_gfs(slot, c, out); }
int fpx_getvdep_nest_init(fpx_handle h, int32_t nest, const void *xlandusen) { FPX_GUARD(h); return h->impl->getvdep_nest_init(nest, xlandusen); }
int fpx_getvdep_nest(fpx_handle h, int32_t nest, int32_t slot, const fpx_getvdep_in *g, void *vdep_out) { FPX_GUARD(h); return h->impl->getvdep_nest(nest, slot, g, vdep_out); }
int fpx_calcpv_init(fpx_handle h, const fpx_calcpv_cfg *c) { FPX_GUARD(h); return h->impl->calcpv_init(c); }
int fpx_get_pvh(fpx_handle h, int32_t nest, void *pvh_out) { FPX_GUARD(h); return h->impl->get_pvh(nest, pvh_out); }
int fpx_calcpv_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_calcpv_time: null"); *ms = h->impl->pv_ms(); return FPX_OK; }
int fpx_getvdep_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_getvdep_time: null"); *ms = h->impl->gv_ms(); return FPX_OK; }
int fpx_calcpar_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_calcpar_time: null"); *ms = h->impl->cp_ms(); return FPX_OK; }
int fpx_verttransform_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_verttransform_time: null"); *ms = h->impl->vt_ms(); return FPX_OK; }
int fpx_set_windtime(fpx_handle h, const int32_t memtime[2], const int32_t memind[2]) { FPX_GUARD(h); return h->impl->set_windtime(memtime, memind); }
int fpx_rng_fill_table(fpx_handle h) { FPX_GUARD(h); return h->impl->rng_fill_table(); }
int fpx_rng_set_table(fpx_handle h, const void *t, int32_t n) { FPX_GUARD(h); return h->impl->rng_set_table(t, n); }
int fpx_rng_get_table(fpx_handle h, void *t, int32_t n) { FPX_GUARD(h); return h->impl->rng_get_table(t, n); }
int fpx_upload_particles(fpx_handle h, int64_t first, int64_t count, const fpx_particles *p) { FPX_GUARD(h); return h->impl->upload_particles(first, count, p); }
int fpx_download_particles(fpx_handle h, int64_t first, int64_t count, const fpx_particles *p) { FPX_GUARD(h); return h->impl->download_particles(first, count, p); }
int fpx_set_numpart(fpx_handle h, int64_t n) { FPX_GUARD(h); return h->impl->set_numpart(n); }
int fpx_set_release_points(fpx_handle h, int32_t numpoint, const void *xmass, const int32_t *npart) { FPX_GUARD(h); return h->impl->set_release_points(numpoint, xmass, npart); }
int fpx_release_init(fpx_handle h, const fpx_release *r) { FPX_GUARD(h); return h->impl->release_init(r); }
int fpx_releaseparticles(fpx_handle h, int32_t itime, int64_t *numpart, int32_t *numparticlecount, void *xmasssave, void *rho_rel, int64_t *nreleased) {
  FPX_GUARD(h);
  return h->impl->releaseparticles(itime, numpart, numparticlecount, xmasssave, rho_rel, nreleased);
}
int fpx_split_particles(fpx_handle h, int32_t itime, int64_t *numpart) { FPX_GUARD(h); return h->impl->split_particles(itime, numpart); }
// mpi_mod.f90:566-658 (mpif_calculate_part_redist): which pairs of ranks exchange how many particles.  Pure host logic.
int fpx_redist_plan(const int64_t *npart_per_process, int32_t nranks, int32_t rank, int32_t ipout, int32_t *role, int32_t *peer, int64_t *num_trans) {
  if (!role || !peer || !num_trans) return FPX_ERR_ARG;
  *role = 0; *peer = -1; *num_trans = 0;
  if (!npart_per_process || nranks < 1 || rank < 0 || rank >= nranks) return FPX_ERR_ARG;
  if (nranks == 1 || ipout == 3) return 0;                           // :597, :613
  const double mp_redist_fract = 0.2;                                // mpi_mod.f90:156-157
  const int64_t mp_min_redist = 100000;
  std::vector<float> sorted((size_t)nranks);                         // the reference sorts the counts as default reals
  std::vector<int> idx((size_t)nranks);
  for (int i = 0; i < nranks; i++) { sorted[i] = (float)npart_per_process[i]; idx[i] = i; }
  for (int i = 0; i <= nranks - 2; i++) {                            // :616-631, the reference's selection sort, ties included
    float pmin = sorted[i];
    int imin = idx[i];
    for (int jj = i + 1; jj <= nranks - 1; jj++) {
      if (pmin <= sorted[jj]) continue;
      const float z = pmin; pmin = sorted[jj]; sorted[jj] = z;
      const int nn = imin; imin = idx[jj]; idx[jj] = nn;
    }
    sorted[i] = pmin; idx[i] = imin;
  }
  int m = nranks - 1;
  for (int i = 0; i <= nranks / 2 - 1; i++, m--) {                   // :639-655
    const int64_t hi = npart_per_process[idx[m]], lo = npart_per_process[idx[i]], nt = hi - lo;
    if (rank != idx[m] && rank != idx[i]) continue;
    if (hi > mp_min_redist && (float)nt / (float)hi > (float)mp_redist_fract) {
      *role = rank == idx[m] ? 1 : 2;
      *peer = rank == idx[m] ? idx[i] : idx[m];
      *num_trans = nt / 2;
    }
  }
  return 0;
}
uint64_t fpx_redist_bytes(fpx_handle h, int64_t num_trans) { if (!h || !h->impl) return 0; return (uint64_t)h->impl->redist_bytes(num_trans); }
int fpx_redist_pack(fpx_handle h, int32_t itime, int64_t num_trans, void *buf, uint64_t buf_bytes, int64_t *numpart) { FPX_GUARD(h); return h->impl->redist_pack(itime, num_trans, buf, (size_t)buf_bytes, numpart); }
int fpx_redist_unpack(fpx_handle h, int32_t itime, int64_t num_trans, const void *buf, uint64_t buf_bytes, int64_t *numpart) { FPX_GUARD(h); return h->impl->redist_unpack(itime, num_trans, buf, (size_t)buf_bytes, numpart); }
int fpx_step(fpx_handle h, int32_t itime, fpx_step_stats *st) { FPX_GUARD(h); return h->impl->step(itime, st, false); }
int fpx_step_async(fpx_handle h, int32_t itime) { FPX_GUARD(h); return h->impl->step(itime, nullptr, true); }
int fpx_sync(fpx_handle h) { FPX_GUARD(h); return h->impl->sync(); }
int fpx_counters(fpx_handle h, fpx_step_stats *st, int32_t reset) { FPX_GUARD(h); return h->impl->counters(st, reset); }
int fpx_kernel_time(fpx_handle h, double *ms, int64_t *launches, int32_t reset) {
  FPX_GUARD(h);
  long long l = 0;
  int rc = h->impl->kernel_time(ms, &l, reset, nullptr);
  if (launches) *launches = l;
  return rc;
}
int fpx_kernel_times(fpx_handle h, double ms[4], int64_t *launches, int32_t reset) {
  FPX_GUARD(h);
  long long l = 0;
  double tot = 0;
  int rc = h->impl->kernel_time(&tot, &l, reset, ms);
  if (launches) *launches = l;
  return rc;
}
int fpx_sort_particles(fpx_handle h) { FPX_GUARD(h); return h->impl->sort_particles(); }
int fpx_conv_init(fpx_handle h, const fpx_conv_config *c) { FPX_GUARD(h); return h->impl->conv_init(c); }
int fpx_upload_conv_fields(fpx_handle h, int32_t slot, const fpx_conv_fields *f) { FPX_GUARD(h); return h->impl->upload_conv_fields(slot, f); }
int fpx_convmix(fpx_handle h, int32_t itime, int64_t *nmoved) { FPX_GUARD(h); return h->impl->convmix(itime, nmoved); }
int fpx_convmix_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return FPX_ERR_ARG; *ms = h->impl->conv_ms(); return 0; }
int fpx_conv_columns(fpx_handle h, const int32_t *col, int32_t ncol, int32_t *lconv, int32_t *nconvtop, void *fmassfrac, void *uvzlev) {
  FPX_GUARD(h);
  return h->impl->conv_columns(col, ncol, lconv, nconvtop, fmassfrac, uvzlev);
}
int fpx_conv_init_gfs(fpx_handle h, const fpx_conv_gfs_config *c) { FPX_GUARD(h); return h->impl->conv_init_gfs(c); }
int fpx_upload_conv_gfs_fields(fpx_handle h, int32_t slot, const fpx_conv_gfs_fields *f) { FPX_GUARD(h); return h->impl->upload_conv_gfs_fields(slot, f); }
int fpx_conv_soundings(fpx_handle h, const int32_t *col, int32_t ncol, void *psconv, void *pconv, void *phconv, void *dpr, void *tconv, void *qconv) {
  FPX_GUARD(h);
  return h->impl->conv_soundings(col, ncol, psconv, pconv, phconv, dpr, tconv, qconv);
}
int fpx_upload_diag_nest_fields(fpx_handle h, int32_t nest, int32_t slot, const fpx_diag_fields *f) { FPX_GUARD(h); return h->impl->upload_diag_nest_fields(nest, slot, f); }
int fpx_upload_conv_nest_fields(fpx_handle h, int32_t nest, int32_t slot, const fpx_conv_fields *f) { FPX_GUARD(h); return h->impl->upload_conv_nest_fields(nest, slot, f); }
int fpx_get_cbaseflux_nest(fpx_handle h, int32_t nest, void *cb) { FPX_GUARD(h); return h->impl->cbaseflux_nest_io(nest, cb, false); }
int fpx_set_cbaseflux_nest(fpx_handle h, int32_t nest, const void *cb) { FPX_GUARD(h); return h->impl->cbaseflux_nest_io(nest, (void *)cb, true); }
int fpx_get_cbaseflux(fpx_handle h, void *cb) { FPX_GUARD(h); return h->impl->cbaseflux_io(cb, false); }
int fpx_set_cbaseflux(fpx_handle h, const void *cb) { FPX_GUARD(h); return h->impl->cbaseflux_io((void *)cb, true); }
int fpx_checkpoint_write(fpx_handle h, const char *path, int32_t itime, int32_t numparticlecount) {
  FPX_GUARD(h);
  return h->impl->checkpoint_write(path, itime, numparticlecount);
}
int fpx_checkpoint_read(fpx_handle h, const char *path, int32_t *itime, int64_t *numpart, int32_t *numparticlecount) {
  FPX_GUARD(h);
  return h->impl->checkpoint_read(path, itime, numpart, numparticlecount);
}
int fpx_seed_particles(fpx_handle h, int64_t n, uint64_t seed, double frac_pbl, double zmax, double lat_margin_cells, int32_t itime0) {
  FPX_GUARD(h);
  return h->impl->seed_particles(n, seed, frac_pbl, zmax, lat_margin_cells, itime0);
}
int fpx_outgrid_init(fpx_handle h, const fpx_outgrid *g, const void *outheight) { FPX_GUARD(h); return h->impl->outgrid_init(g, outheight); }
int fpx_set_output_times(fpx_handle h, int32_t loutnext, int32_t loutstep) { FPX_GUARD(h); return h->impl->set_output_times(loutnext, loutstep); }
int fpx_conccalc(fpx_handle h, int32_t itime, double weight) { FPX_GUARD(h); return h->impl->conccalc(itime, weight); }
int fpx_get_grids(fpx_handle h, void *gridunc, void *drygridunc, int32_t allreduce, int32_t clear) { FPX_GUARD(h); return h->impl->get_grids(gridunc, drygridunc, allreduce, clear); }
int fpx_get_flux(fpx_handle h, void *flux, int32_t allreduce, int32_t clear) { FPX_GUARD(h); return h->impl->get_flux(flux, allreduce, clear); }
int fpx_fluxoutput(fpx_handle h, int32_t itime, const fpx_fluxout *f, const char *prefix, int32_t reduced) { FPX_GUARD(h); return h->impl->fluxoutput(itime, f, prefix, reduced); }
int fpx_calcfluxes_time(fpx_handle h, double *ms, int64_t *launches, int32_t reset) {
  FPX_GUARD(h);
  long long l = 0;
  const int rc = h->impl->calcfluxes_time(ms, &l, reset);
  if (launches) *launches = l;
  return rc;
}
int fpx_get_partavg(fpx_handle h, int64_t first, int64_t count, int32_t *npart_av, void *const *sums) { FPX_GUARD(h); return h->impl->get_partavg(first, count, npart_av, sums); }
int fpx_partoutput_average(fpx_handle h, int32_t itime, const char *path_or_prefix, int64_t *nrecords) { FPX_GUARD(h); return h->impl->partoutput_average(itime, path_or_prefix, nrecords); }
int fpx_partavg_time(fpx_handle h, double *ms, int64_t *launches, int32_t reset) {
  FPX_GUARD(h);
  long long l = 0;
  const int rc = h->impl->partavg_time(ms, &l, reset);
  if (launches) *launches = l;
  return rc;
}
int fpx_initcond_finish(fpx_handle h, int32_t itime) { FPX_GUARD(h); return h->impl->initcond_finish(itime); }
int fpx_get_initcond(fpx_handle h, void *init_cond, int32_t allreduce, int32_t clear) { FPX_GUARD(h); return h->impl->get_initcond(init_cond, allreduce, clear); }
int fpx_initial_cond_output(fpx_handle h, int32_t itime, const fpx_initout *o, const char *prefix, int32_t reduced) { FPX_GUARD(h); return h->impl->initial_cond_output(itime, o, prefix, reduced); }
int fpx_plumetraj_init(fpx_handle h, const fpx_plumetraj_cfg *c) { FPX_GUARD(h); return h->impl->plumetraj_init(c); }
int fpx_plumetraj(fpx_handle h, int32_t itime, const char *path, int32_t *nrecords) { FPX_GUARD(h); return h->impl->plumetraj(itime, path, nrecords); }
int fpx_get_plumetraj(fpx_handle h, int32_t max_records, int32_t *jpoint, int32_t *npart, int32_t *iterations, int32_t *numb, void *values, int32_t ld) {
  FPX_GUARD(h);
  return h->impl->get_plumetraj(max_records, jpoint, npart, iterations, numb, values, ld);
}
int fpx_domainfill_init(fpx_handle h, const fpx_domainfill_cfg *c) { FPX_GUARD(h); return h->impl->domainfill_init(c); }
int fpx_boundcond_domainfill(fpx_handle h, int32_t itime, int64_t *numpart, int32_t *numparticlecount, fpx_domainfill_stats *out) {
  FPX_GUARD(h);
  return h->impl->boundcond_domainfill(itime, numpart, numparticlecount, out);
}
int fpx_get_domainfill_acc(fpx_handle h, void *acc_mass_we, void *acc_mass_sn) { FPX_GUARD(h); return h->impl->domainfill_acc(acc_mass_we, acc_mass_sn, nullptr, nullptr); }
int fpx_set_domainfill_acc(fpx_handle h, const void *acc_mass_we, const void *acc_mass_sn) { FPX_GUARD(h); return h->impl->domainfill_acc(nullptr, nullptr, acc_mass_we, acc_mass_sn); }
int fpx_boundcond_output(fpx_handle h, const char *path) { FPX_GUARD(h); return h->impl->boundcond_output(path); }
int fpx_domainfill_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_domainfill_time: null"); *ms = h->impl->domainfill_ms(); return FPX_OK; }
int fpx_plumetraj_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_plumetraj_time: null"); *ms = h->impl->plumetraj_ms(); return FPX_OK; }
int fpx_initcond_time(fpx_handle h, double *ms, int64_t *launches, int32_t reset) {
  FPX_GUARD(h);
  long long l = 0;
  const int rc = h->impl->initcond_time(ms, &l, reset);
  if (launches) *launches = l;
  return rc;
}
int fpx_comm_unique_id(void *id, int32_t nbytes) {
  if (!id || nbytes != (int32_t)sizeof(ncclUniqueId)) return fpx::fail(FPX_ERR_ARG, "fpx_comm_unique_id: the id is 128 bytes");
  ncclUniqueId uid;
  ncclResult_t r = ncclGetUniqueId(&uid);
  if (r != ncclSuccess) return fpx::fail(FPX_ERR_DEVICE, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  memcpy(id, &uid, sizeof(uid));
  return FPX_OK;
}
int fpx_count_particles(fpx_handle h, int64_t local[2], int64_t total[2], int32_t allreduce) { FPX_GUARD(h); return h->impl->count_particles(local, total, allreduce); }
int fpx_set_release_heights(fpx_handle h, int32_t numpoint, const void *zpoint1, const void *zpoint2) { FPX_GUARD(h); return h->impl->set_release_heights(numpoint, zpoint1, zpoint2); }
int fpx_set_option(fpx_handle h, const char *name, const char *value) { FPX_GUARD(h); if (!name || !value) return fpx::fail(FPX_ERR_ARG, "fpx_set_option: null argument"); return h->impl->set_option(name, value); }
int fpx_get_info(fpx_handle h, const char *name, int64_t *value) { FPX_GUARD(h); if (!name || !value) return fpx::fail(FPX_ERR_ARG, "fpx_get_info: null argument"); return h->impl->get_info(name, value); }
int fpx_lane_stats(fpx_handle h, uint64_t *out, int32_t n, int32_t reset) { FPX_GUARD(h); if (!out || n < 0) return fpx::fail(FPX_ERR_ARG, "fpx_lane_stats: bad argument"); return h->impl->lane_stats(out, n, reset); }
int fpx_comm_init(fpx_handle h, const void *id, int32_t nbytes, int32_t nranks, int32_t rank) { FPX_GUARD(h); return h->impl->comm_init(id, nbytes, nranks, rank); }
int fpx_comm_init_host(fpx_handle h, int32_t nranks, int32_t rank, fpx_allreduce_fn fn, void *user) { FPX_GUARD(h); return h->impl->comm_init_host(nranks, rank, fn, user); }
int fpx_nests_init(fpx_handle h, const fpx_nests *n) { FPX_GUARD(h); return h->impl->nests_init(n); }
int fpx_upload_nest_fields(fpx_handle h, int32_t nest, int32_t slot, const fpx_fields *f) { FPX_GUARD(h); return h->impl->upload_nest_fields(nest, slot, f); }
int fpx_wet_init(fpx_handle h, const fpx_wet_config *w) { FPX_GUARD(h); return h->impl->wet_init(w); }
int fpx_upload_wet_fields(fpx_handle h, int32_t slot, const fpx_wet_fields *f) { FPX_GUARD(h); return h->impl->upload_wet_fields(slot, f); }
int fpx_wetdepo(fpx_handle h, int32_t itime, int32_t ltsample, int32_t loutnext) { FPX_GUARD(h); return h->impl->wetdepo(itime, ltsample, loutnext); }
int fpx_get_wetgrid(fpx_handle h, void *wetgridunc, int32_t allreduce) { FPX_GUARD(h); return h->impl->get_wetgrid(wetgridunc, allreduce); }
int fpx_oh_init(fpx_handle h, const fpx_oh_config *c) { FPX_GUARD(h); return h->impl->oh_init(c); }
int fpx_gethourlyOH(fpx_handle h, int32_t itime) { FPX_GUARD(h); return h->impl->gethourlyOH(itime); }
int fpx_ohreaction(fpx_handle h, int32_t itime, int32_t ltsample, int32_t loutnext) { FPX_GUARD(h); return h->impl->ohreaction(itime, ltsample, loutnext); }
int fpx_get_oh_hourly(fpx_handle h, void *OH_hourly_out, void *memOHtime_out) { FPX_GUARD(h); return h->impl->get_oh_hourly(OH_hourly_out, memOHtime_out); }
int fpx_set_oh_hourly(fpx_handle h, const void *OH_hourly, const void *memOHtime) { FPX_GUARD(h); return h->impl->set_oh_hourly(OH_hourly, memOHtime); }
int fpx_ohreaction_time(fpx_handle h, double *ms) { FPX_GUARD(h); if (!ms) return fpx::fail(FPX_ERR_ARG, "fpx_ohreaction_time: null"); return h->impl->ohreaction_ms(ms); }
void *fpx_stream(fpx_handle h) { return (h && h->impl) ? h->impl->stream_ptr() : nullptr; }
int fpx_upload_wet_nest_fields(fpx_handle h, int32_t nest, int32_t slot, const fpx_wet_fields *f, int32_t readclouds_nest) { FPX_GUARD(h); return h->impl->upload_wet_nest_fields(nest, slot, f, readclouds_nest); }
int fpx_outgrid_nest_init(fpx_handle h, const fpx_outgrid_nest *g) { FPX_GUARD(h); return h->impl->outgrid_nest_init(g); }
int fpx_get_grids_nest(fpx_handle h, void *griduncn, void *drygriduncn, void *wetgriduncn, int32_t allreduce, int32_t clear) { FPX_GUARD(h); return h->impl->get_grids_nest(griduncn, drygriduncn, wetgriduncn, allreduce, clear); }
int fpx_receptors_init(fpx_handle h, int32_t numreceptor, const void *xreceptor, const void *yreceptor, const void *receptorarea) { FPX_GUARD(h); return h->impl->receptors_init(numreceptor, xreceptor, yreceptor, receptorarea); }
int fpx_get_receptors(fpx_handle h, void *creceptor, int32_t ld, int32_t allreduce, int32_t clear) { FPX_GUARD(h); return h->impl->get_receptors(creceptor, ld, allreduce, clear); }

int fpx_math_probe(int32_t fn, const double *x, double *y, int64_t n) {
  if (fn < 0 || (fn > 33 && fn < 40) || fn > 43 || !x || !y || n < 0) return FPX_ERR_ARG;
  if (n == 0) return FPX_OK;
  const int64_t nin = (fn == 12 || fn == 13 || fn == 42 || fn == 43) ? 2 * n : n;   // fn 12, 13: x[0 .. n) the points, x[n .. 2n) their exp(-x*x); 42, 43: the exponents
  fpx::Scratch bx, by;
  if (bx.reserve(nin * sizeof(double), nullptr) != hipSuccess || by.reserve(n * sizeof(double), nullptr) != hipSuccess) return FPX_ERR_NOMEM;
  double *dx = bx.as<double>(), *dy = by.as<double>();
  hipError_t e = hipMemcpy(dx, x, nin * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (fn >= 12 && fn <= 14) fpx::k_erf_probe<<<(unsigned)((n + fpx::kBlock - 1) / fpx::kBlock), fpx::kBlock>>>(fn, dx, dy, n);
    else fpx::k_math_probe<<<(unsigned)((n + fpx::kBlock - 1) / fpx::kBlock), fpx::kBlock>>>(fn, dx, dy, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(y, dy, n * sizeof(double), hipMemcpyDeviceToHost);
  return e == hipSuccess ? FPX_OK : FPX_ERR_DEVICE;
}

int fpx_hanna_probe(const double *in, double *out, int64_t n) {
  if (!in || !out || n < 0) return FPX_ERR_ARG;
  if (n == 0) return FPX_OK;
  fpx::Scratch bx, by;
  if (bx.reserve(5 * n * sizeof(double), nullptr) != hipSuccess || by.reserve(10 * n * sizeof(double), nullptr) != hipSuccess) return FPX_ERR_NOMEM;
  double *dx = bx.as<double>(), *dy = by.as<double>();
  hipError_t e = hipMemcpy(dx, in, 5 * n * sizeof(double), hipMemcpyHostToDevice);
  for (int which = 0; which < 2 && e == hipSuccess; which++) {   // out: all points of the engine's form, then all of the plain one
    fpx::k_hanna_probe<<<(unsigned)((n + fpx::kBlock - 1) / fpx::kBlock), fpx::kBlock>>>(which, dx, dy, n);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out + 10 * n * which, dy, 10 * n * sizeof(double), hipMemcpyDeviceToHost);
  }
  return e == hipSuccess ? FPX_OK : FPX_ERR_DEVICE;
}

int fpx_cbl_probe(int32_t form, const double *in, double *out, int64_t n) {
  if ((form != 0 && form != 1) || !in || !out || n < 0) return FPX_ERR_ARG;
  if (n == 0) return FPX_OK;
  fpx::Scratch bx, by;
  if (bx.reserve(10 * n * sizeof(double), nullptr) != hipSuccess || by.reserve(3 * n * sizeof(double), nullptr) != hipSuccess) return FPX_ERR_NOMEM;
  double *dx = bx.as<double>(), *dy = by.as<double>();
  hipError_t e = hipMemcpy(dx, in, 10 * n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)((n + fpx::kBlock - 1) / fpx::kBlock);
    if (form == 0) fpx::k_cbl_probe<0><<<blocks, fpx::kBlock>>>(dx, dy, n);
    else fpx::k_cbl_probe<1><<<blocks, fpx::kBlock>>>(dx, dy, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dy, 3 * n * sizeof(double), hipMemcpyDeviceToHost);
  return e == hipSuccess ? FPX_OK : FPX_ERR_DEVICE;
}

}  // extern "C"
template <typename R>
static int find_level_probe(const R *height, int32_t nz, const R *z, const int32_t *guess, int64_t n, int32_t *idx, R *zz) {
  fpx::Scratch bh, bz, bg, bi, bzz;
  hipError_t e = bh.reserve(nz * sizeof(R), nullptr);
  if (e == hipSuccess) e = bz.reserve(n * sizeof(R), nullptr);
  if (e == hipSuccess) e = bg.reserve(n * sizeof(int), nullptr);
  if (e == hipSuccess) e = bi.reserve(n * sizeof(int), nullptr);
  if (e == hipSuccess) e = bzz.reserve(2 * n * sizeof(R), nullptr);
  R *dh = bh.as<R>(), *dz = bz.as<R>(), *dzz = bzz.as<R>();
  int *dg = bg.as<int>(), *di = bi.as<int>();
  const bool nomem = e != hipSuccess;
  if (e == hipSuccess) e = hipMemcpy(dh, height, nz * sizeof(R), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dz, z, n * sizeof(R), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dg, guess, n * sizeof(int), hipMemcpyHostToDevice);
  for (int which = 0; which < 2 && e == hipSuccess; which++) {   // all points of the search from the guess, then all of the plain one
    fpx::k_find_level_probe<R><<<(unsigned)((n + fpx::kBlock - 1) / fpx::kBlock), fpx::kBlock>>>(which, dh, nz, dz, dg, n, di, dzz);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(idx + n * which, di, n * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(zz + 2 * n * which, dzz, 2 * n * sizeof(R), hipMemcpyDeviceToHost);
  }
  return e == hipSuccess ? FPX_OK : nomem ? FPX_ERR_NOMEM : FPX_ERR_DEVICE;
}

extern "C" {
int fpx_find_level_probe(int32_t real_bytes, const void *height, int32_t nz, const void *z, const int32_t *guess, int64_t n, int32_t *idx, void *zz) {
  if ((real_bytes != 4 && real_bytes != 8) || !height || nz < 2 || nz > fpx::kMaxNz || !z || !guess || !idx || !zz || n < 0) return FPX_ERR_ARG;
  if (n == 0) return FPX_OK;
  if (real_bytes == 8) return find_level_probe<double>((const double *)height, nz, (const double *)z, guess, n, idx, (double *)zz);
  return find_level_probe<float>((const float *)height, nz, (const float *)z, guess, n, idx, (float *)zz);
}

}  // extern "C"
#endif   // FPX_TU_REAL != 4
