// C ABI of libgmpnp.so (include/gmpnp.h): handle, host drivers of assembly, preconditioner setup,
// BiCGStab and the damped Newton loop ([3P] dolfin::NewtonSolver semantics).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include <hip/hip_ext.h>

#include "gmpnp_kernels.h"
#include "gmpnp_step_limit.h"
#include "gmpnp_band_lu.h"
#include "gmpnp_dist_kernels.h"
#include "gmpnp_multilevel.h"
#include "gmpnp_host_rules.h"

using namespace gmpnp;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return fail(GMPNP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));              \
  } while (0)

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count, bool zero = true, size_t pad = 0) {  // pad: zeroed elements behind the n counted ones
    if (p) { (void)hipFree(p); p = nullptr; }
    n = count;
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count + pad, 1) * sizeof(T));
    if (e == hipSuccess && (zero || pad)) e = hipMemset(p, 0, std::max<size_t>(count + pad, 1) * sizeof(T));
    return e;
  }
  hipError_t upload(const std::vector<T>& v) {
    hipError_t e = alloc(v.size(), v.empty());
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};

// The nouns of a record stream's messages: "<prefix>: no <what> is open (<open_call>)", "... the buffer is full (read the records and
// <reopen>)", "... the <rows> asked for have not been written".
struct RecordNouns {
  const char *prefix, *what, *open_call, *rows, *reopen;
  std::string say(const std::string& tail) const { return std::string(prefix) + ": " + tail; }
  std::string not_open() const { return say(std::string("no ") + what + " is open (" + open_call + ")"); }
};

// A device buffer of per-step records (rule: gmpnp_host_rules.h "record streams"): [capacity + 1][width] records, appended to without
// host synchronisation and read in chunks.  The row behind the buffer is the timing hook's (gmpnp_time_kernel 29 / 31 / 32).
template <class Rec>
struct RecordStream {
  const RecordNouns& nouns;
  DevBuf<Rec> rec;
  int width = 0, capacity = 0, count = 0;   // width: records per step
  bool open = false;
  explicit RecordStream(const RecordNouns& n) : nouns(n) {}
  // an empty buffer of `cap` rows of `w` records: allocated again only where either changed
  int reserve(int cap, int w, hipStream_t stream) {
    if (capacity != cap || width != w) {
      HIP_TRY(hipStreamSynchronize(stream));
      capacity = 0;   // (alloc frees the old buffer first: an allocation that fails leaves no capacity a later open could take for a buffer)
      HIP_TRY(rec.alloc(record_rows(cap) * (size_t)w));
      capacity = cap; width = w;
    }
    count = 0;
    return GMPNP_OK;
  }
  Rec* row(int slot) const { return rec.p + (size_t)slot * width; }
  Rec* hook_row() const { return row(capacity); }
  bool full() const { return !record_can_append(count, capacity); }
  int refuse_full() const { return fail(GMPNP_ERR_INVALID, nouns.say(std::string("the buffer is full (read the records and ") + nouns.reopen + ")")); }
  int read(int32_t first, int32_t n, Rec* out, hipStream_t stream) const {
    if (!record_range_valid(first, n, count))
      return fail(GMPNP_ERR_INVALID, nouns.say(std::string("the ") + nouns.rows + " asked for have not been written"));
    HIP_TRY(hipMemcpyAsync(out, row(first), (size_t)n * width * sizeof(Rec), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return GMPNP_OK;
  }
  void close() { open = false; }
};

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

// device side of gmpnp_project_gradient / gmpnp_project_cellwise (gmpnp_project.h), allocated on first use
struct gmpnp_projector {
  DevBuf<double> cellvol, cellval, mass, diag, f, b, x, r, p, Ap, dpart;
  double* h_part = nullptr;   // pinned: dot-product partials
  int nblocks = 0;
  bool mass_ready = false;
  ~gmpnp_projector() { if (h_part) (void)hipHostFree(h_part); }
};

// device side of gmpnp_column_select / gmpnp_group_column_select (gmpnp_stats.h), allocated on first use
struct gmpnp_selector {
  DevBuf<double> cnt;                   // [n][256] bucket counts + [n] NaN counts: what the group all-reduces
  DevBuf<uint32_t> part, part_nan;      // per-workgroup histogram rows of the local handles (first handle of the call only)
  DevBuf<uint8_t> io;                   // SelIo: selections, prefixes, results
  void* h_io = nullptr;                 // pinned SelIo
  ~gmpnp_selector() { if (h_io) (void)hipHostFree(h_io); }
};

// device side of gmpnp_species_budget / gmpnp_group_species_budget (gmpnp_budget.h), allocated on first use
struct gmpnp_budgeter {
  DevBuf<double> EF;                                    // element rows at the current u: the budget's own (the solver's EF stays)
  DevBuf<double> wall_w, exit_w, exit_val, point_w;     // geometry-only facet tables (internal node order)
  DevBuf<int32_t> exit_ptr, exit_col, status;           // status: where the budget's element pass reports (not the solver's word)
  DevBuf<double> part_c, part_r, table;                 // workgroup partials of the cell / row pass; [nf][GMPNP_BUDGET_COLUMNS]: what a group all-reduces
  int nblk_c = 0, nblk_r = 0;
  double* h_table = nullptr;                            // pinned read-back
  ~gmpnp_budgeter() { if (h_table) (void)hipHostFree(h_table); }
};

// device side of the step limiter (gmpnp_step_limit.h), allocated by the first limited Newton solve / gmpnp_step_limit call: a
// handle that never asks for it keeps the buffers and launches it had
struct gmpnp_step_limiter {
  DevBuf<double> part, dx;          // workgroup partials; the correction of gmpnp_step_limit / gmpnp_time_kernel(21) (internal order)
  DevBuf<int32_t> part_node;
  int nblk = 0;
  StepReport* h_report = nullptr;   // pinned: what workgroup 0 of the update writes
  StepReport* d_report = nullptr;   // ... its device address
  ~gmpnp_step_limiter() { if (h_report) (void)hipHostFree(h_report); }
};

// device side of the adaptive time stepping (gmpnp_time_step.h), allocated by the first call of its family (gmpnp_time_error /
// _accept / _reject): a handle that never asks for it keeps the buffers and launches it had
namespace gmpnp { struct TimeReport; }
struct gmpnp_time_stepper {
  DevBuf<double> unm1;                          // the accepted state before u_n (internal order)
  DevBuf<double> part, part_max;                // workgroup partials of the estimator
  DevBuf<int32_t> part_dof, part_bad;
  int nblk = 0;
  bool has_history = false;                     // u_nm1 holds an accepted state (gmpnp_time_accept since create / set_state / assign_previous)
  // second order (gmpnp_time_order.h): the two vectors are allocated by the first call that asks for order 2
  DevBuf<double> unm2, ustar;                   // the accepted state before u_nm1; u* = a u_n - b u_nm1 of the last BDF2 set-up
  int order = 1;                                // gmpnp_set_time_order
  int levels = 0;                               // accepted states behind u_n: 0, 1 (u_nm1) or 2 (u_nm2 too); has_history = levels >= 1
  bool star_formed = false;                     // u* holds what gmpnp_set_time_step_bdf2 wrote
  void dropped() { has_history = false; levels = 0; }
  void accepted() { has_history = true; levels = std::min(levels + 1, order == 2 ? 2 : 1); }
  TimeReport* h_report = nullptr;               // pinned: what k_time_reduce writes
  TimeReport* d_report = nullptr;               // ... its device address
  ~gmpnp_time_stepper() { if (h_report) (void)hipHostFree(h_report); }
};

// device side of the Stern-layer boundary condition (gmpnp_stern.h), allocated by the first gmpnp_set_stern with model != 0: a handle
// that never asks for it keeps the buffers, launches and pointers it had
struct gmpnp_sterner {
  gmpnp_stern_t opt{};
  int n_nodes = 0, n_pairs = 0;
  DevBuf<int32_t> node, nf_ptr, nf_ent, fnodes, pair_row, pf_ptr, pf_ent;
  DevBuf<int64_t> addr;
  DevBuf<double> area, sum;
};

// device side of the surface kinetics (gmpnp_kinetics.h), allocated by the first gmpnp_set_kinetics with n_reactions != 0: a handle
// that never asks for it keeps the buffers, launches and pointers it had
struct gmpnp_kineticist {
  gmpnp_kinetics_t opt{};
  int n_nodes = 0;
  DevBuf<gmpnp_kinetics_t> d_opt;
  DevBuf<int32_t> node, status;   // status: the word of gmpnp_kinetics_currents' own launches
  DevBuf<int64_t> addr;
  DevBuf<double> w, sum;
};

// device side of the galvanostatic mode (gmpnp_galvanostat.h), allocated by the first gmpnp_set_galvanostat with on != 0: a handle
// that never asks for it keeps the buffers, launches and pointers it had
namespace gmpnp { struct GalvReport; }
struct gmpnp_galvanostat {
  gmpnp_galvanostat_t opt{};
  DevBuf<double> scal;                  // [kGalvScalars]: p_M, its twin at u_n, dp and the verdict of the last reduce, the hook's own slots
  DevBuf<double> b, y, z, x, zero;      // b = dF/dp_M, y = J^-1 F, z = J^-1 b (internal order); x: the hook's vector; zero: all zeros
  DevBuf<int32_t> status;               // the word of the hooks' own launches
  gmpnp::GalvReport* h_report = nullptr;   // pinned [2]: what k_galv_reduce / k_galv_potential write ([1]: the hooks')
  gmpnp::GalvReport* d_report = nullptr;   // ... its device address
  ~gmpnp_galvanostat() { if (h_report) (void)hipHostFree(h_report); }
};

// device side of gmpnp_frequency_response (gmpnp_response.h), allocated by the first call: a handle that never asks for it keeps the
// buffers and launches it had
namespace gmpnp { struct RespOut; }
struct gmpnp_responder {
  DevBuf<double> blocks;               // L, D, U [NF*NF][nv] and b [NF][nv]: level 0 of the response's own (K at inv_dt = 0, b = dF/dp_M)
  DevBuf<double> b, mass, sigma;       // b in internal order; [3][nv] mass entries of a species row; the chunk's sigma
  DevBuf<double2> ws, x;               // [chunk][nv][8][8] eliminated blocks and right-hand sides; [chunk][nv][8] the solution
  DevBuf<int32_t> fstat, status;       // per-frequency word of the solve; the word of the set-up's own launches
  DevBuf<gmpnp::RespOut> out;
  size_t cap_freq = 0;                 // frequencies ws / x / sigma / fstat / out hold
  int last_chunk = 0;                  // frequencies of the last chunk solved (gmpnp_time_kernel 27)
  gmpnp::RespOut* h_out = nullptr;     // pinned [cap_freq]
  double* h_x = nullptr;               // pinned [h_x_freq][nv][8][2], allocated when x is asked for
  size_t h_x_freq = 0;
  ~gmpnp_responder() { if (h_out) (void)hipHostFree(h_out); if (h_x) (void)hipHostFree(h_x); }
};

// device side of gmpnp_frequency_response_3d (gmpnp_response_band.h), allocated by the first call: a handle that never asks for it keeps
// the buffers and launches it had.  The complex band is storage of the response's own (a BandView<BandComplex> of gmpnp_band_lu.h's
// kernels, one member per frequency); the handle's real band (gmpnp_solver::lu) is not touched.
namespace gmpnp { struct CBandState; }
struct gmpnp_band_responder {
  DevBuf<double> mass, rhs, kvals;     // [nb] mass per node block; b = dF/dp_M (internal order); the SELL values of K = J at inv_dt = 0
  DevBuf<double> sigma, rmax;          // the chunk's sigma; [chunk][nslices] residual maxima
  DevBuf<double2> band, dinv;          // [chunk][n][2b+1][81], [chunk][n][81]
  DevBuf<double2> x, r, dx, y, part;   // [chunk][ndof] each; [chunk][16][4][9] partial sums of the substitution
  DevBuf<int32_t> pos, node, fstat, status;   // elimination order; per-frequency word of the pivots; the word of the set-up's own launches
  DevBuf<gmpnp::CBandState> st;
  DevBuf<gmpnp::RespOut> out;
  int n = 0, b = 0;
  size_t cap_freq = 0;                 // frequencies the chunk storage holds
  int last_chunk = 0;                  // frequencies of the last chunk solved (gmpnp_time_kernel 30)
  gmpnp::RespOut* h_out = nullptr;     // pinned [cap_freq]
  ~gmpnp_band_responder() { if (h_out) (void)hipHostFree(h_out); }
};

// device side of gmpnp_electrode_tangent / gmpnp_electrode_advance (gmpnp_tangent.h), allocated by the first call: a handle that never
// asks for it keeps the buffers and launches it had
namespace gmpnp { struct TanOut; }
struct gmpnp_tangenter {
  DevBuf<double> c, z, Jz;             // [10][ndof] internal order: the columns dF/dtheta_k, the tangents, J z_k
  DevBuf<double> cols_store;           // per level of the cyclic-reduction pyramid: b, bi, x with 8 columns each
  DevBuf<double> alpha;                // the advance's step factor
  DevBuf<int32_t> status;              // the word of the column and functional launches
  DevBuf<gmpnp::TanOut> out;
  gmpnp::TanOut* h_out = nullptr;      // pinned [10]
  int last_n = 0;                      // columns of the last call (gmpnp_time_kernel 28, gmpnp_tangent_columns)
  int col_pM = -1;                     // where the p_M column of the last call sits
  bool fresh = false;                  // z[col_pM] belongs to the present u, p_M and options: gmpnp_electrode_advance may use it
  bool cols_fresh = false;             // every z of the last call does: gmpnp_parameter_advance may use the columns whose status is 0
  int32_t param[GMPNP_TANGENT_MAX_COLUMNS] = {}, col_status[GMPNP_TANGENT_MAX_COLUMNS] = {};   // the last call's parameters and the status words of their columns
  ~gmpnp_tangenter() { if (h_out) (void)hipHostFree(h_out); }
};

// device side of the electrode trace (gmpnp_trace.h), allocated by the first gmpnp_electrode_trace_open: a handle that never asks for it
// keeps the buffers and launches it had
constexpr RecordNouns kTraceNouns{"electrode trace", "trace", "gmpnp_electrode_trace_open", "records", "open the trace again"};
struct gmpnp_tracer {
  RecordStream<gmpnp_electrode_record_t> rec{kTraceNouns};   // one record per step
  DevBuf<ElectrodeAccum> acc;             // [2]: D_prev, Q, Q_D of the trace; the hook's own
  DevBuf<double> w;                       // [n_nodes] w_I of the Stern nodes (read while the kinetics, which hold the same, are off)
  DevBuf<int32_t> status;                 // the word of the Stern and kinetic launches of an open / append (not the solver's)
};

// device side of the wall profile (gmpnp_wall_profile.h), allocated by the first gmpnp_wall_profile_open: a handle that never asks for it
// keeps the buffers and launches it had
constexpr RecordNouns kWallProfileNouns{"wall profile", "profile", "gmpnp_wall_profile_open", "records", "open the profile again"};
struct gmpnp_wall_profiler {
  RecordStream<gmpnp_wall_profile_record_t> rec{kWallProfileNouns};   // n_bins records per step
  DevBuf<double> Q;                          // [2][n_bins][4]: the charges of the bins; the hook's own
  DevBuf<double> w, edges;                   // [n_nodes] w_I of the Stern nodes; [n_bins + 1]
  DevBuf<int32_t> bin_ptr, bin_pos;          // CSR over the bins of positions in the Stern node list, ascending inside a bin
  DevBuf<int32_t> status;                    // the word of the Stern and kinetic launches of an append (not the solver's)
  std::vector<double> h_edges;               // the edges of the lists the device holds
  int n_bins = 0;                            // of the lists the device holds (0: none a later open could take for valid)
};

// device side of the transient sensitivities (gmpnp_sensitivity.h), allocated by the first gmpnp_sensitivity_open: a handle that never
// asks for it keeps the buffers and launches it had
constexpr RecordNouns kSensNouns{"sensitivities", "buffer", "gmpnp_sensitivity_open", "steps", "open again with start = 2"};
struct gmpnp_sensitizer {
  DevBuf<double> S, S_hook;               // [n][ndof] internal order: the state sensitivities; gmpnp_time_kernel(31)'s own
  DevBuf<double> c, Jz;                   // [10][ndof] the columns dF/dtheta_k of the step; J s_k
  DevBuf<double> mass;                    // [3][nv] the species rows' mass entries (species_mass_1d)
  DevBuf<double> store;                   // per level of the cyclic-reduction pyramid: b, bi, x with 8 columns, then with 2 columns
  RecordStream<gmpnp_sensitivity_record_t> rec{kSensNouns};   // n records per step
  DevBuf<ElectrodeAccum> acc;             // [2][10]: dD_prev, dQ, dQ_D per column; the hook's own
  DevBuf<int32_t> status;                 // the word of the column launches
  int n = 0;
  bool stepped = false;                   // a right-hand side has been formed since the open
  int32_t param[GMPNP_TANGENT_MAX_COLUMNS] = {};
};

// device side of the accelerated cycle map (gmpnp_cycle.h), allocated by the first gmpnp_cycle_open: a handle that never asks for it
// keeps the buffers and launches it had
namespace gmpnp { struct CycleReport; }
struct gmpnp_cycler {
  DevBuf<double> X, G, w;                 // [depth + 1][ndof] ring of the pairs (x_j, g_j), internal order; the frozen weights
  DevBuf<double> part, part_max, alpha;   // workgroup partials of the residual; the mix's step factor
  DevBuf<int32_t> part_dof, part_bad;
  int depth = 0, cap = 0, nblk = 0;
  int start = 0, window = 0;              // pair j of the window (oldest first) sits in slot (start + j) % cap
  bool open = false, begun = false, ended = false;   // begun: x_k is written; ended: a report is out and no mix has used it
  bool report_bad = false;                // the last report met a NaN / Inf: gmpnp_cycle_mix is refused
  gmpnp::CycleReport* h_report = nullptr;   // pinned: what k_cycle_reduce writes
  gmpnp::CycleReport* d_report = nullptr;   // ... its device address
  ~gmpnp_cycler() { if (h_report) (void)hipHostFree(h_report); }
};

struct gmpnp_solver {
  Topology t;
  gmpnp_model_t model{};
  gmpnp_quadrature_t quad{};
  gmpnp_options_t opts{};
  int dim = 0, nf = 0, nn = 0, ndof = 0, nb = 0, ncoarse = 0;
  int n_resblocks = 0;
  hipStream_t stream = nullptr;
  Ctx c{};
  // boundary facets kept on the host (internal vertex ids) to rebuild flux tables when the model changes
  std::vector<int32_t> wall_f, exit_f, point_v;
  // device storage
  DevBuf<gmpnp_model_t> d_model; DevBuf<gmpnp_quadrature_t> d_quad;
  DevBuf<double> coords, u, un, F, bcval, bndF, rob_val, EF, EJ, vals, vals_s, Dinv, AP, AcPart, Ac, Aci;
  DevBuf<double> kr, krhat, kp0, kp1, kv0, kv1, ks, kt, ky, kx, kxp, kb, yc, cpart_r0, cpart_r1, cpart_p0, cpart_p1, cpart_v0, cpart_v1, cpart_t,
      part_a, part_b, part_f;
  DevBuf<int32_t> cells, robF_ptr, rob_col, rob_row, n2e_ptr, n2e, rowptr, cols, cptr, contrib, slice_colbase,
      slice_node0, slice_nn, node_slice, sell_cols, sell_blk, wl_slice, wl_kpos, tile_slice0, tile_agg, tile_slot,
      tile_aggs, tile_nagg, tile_cols, tile_colslot, sell_lcol, agg, agg_start, row_aggs, status;
  DevBuf<int64_t> rob_addr, slice_off;
  DevBuf<int32_t> rob_blk; DevBuf<double> rob_blk_val; DevBuf<uint32_t> rob_blk_mask;   // the Robin entries by node block
  DevBuf<uint8_t> bcflag, sell_aggslot;
  DevBuf<KrylovScalars> scal; DevBuf<TileRec> tile_rec;
  std::vector<uint8_t> h_bcflag, h_bcflag_dev;   // flags being built / flags the device holds
  double* h_bcval = nullptr;    // pinned [ndof]
  double* h_stage = nullptr;    // pinned [ndof]: staging of the file-order <-> internal-order vector transfers
  // pinned read-back areas
  KrylovScalars* h_scal = nullptr; double* h_part = nullptr; int32_t* h_status = nullptr;
  HostPoll* h_poll = nullptr;   // progress mirror the B kernels write (fine-grained pinned memory)
  // gmpnp_host_rules.h: the resolved options and the policies of the linear solves inside Newton (each owns its state)
  Settings cfg; BurstHint burst; CoarseReuse coarse; DirectFallback direct; PredictedX0 x0;
  bool jacobian_valid = false, precond_valid = false;
  int precond_mode = -1;
  const double* shadow_src = nullptr; double shadow_rho0 = 0.0;  // shadow vector of the next krylov() pass (after a breakdown: krand)
  int last_done = 0;            // exit code of the last device Krylov loop (1 converged, 2 iteration cap, 3 breakdown / divergence)
  DevBuf<double> krand;         // pseudo-random shadow vector for a pass that follows a breakdown
  bool state_jumped = true;     // u was set from outside since the last Newton solve: the Jacobian moves a lot, no coarse reuse
  DevBuf<uint32_t> ticket;
  DevBuf<double> supg_rho;  // [nv][ns] internal order
  bool fused_half = false;  // two launches per BiCGStab iteration (coarse workgroups inside the tile launch); opts.launch_form
  int resident_slots = 0;   // workgroups of k_half_a/b the device holds at once (occupancy query at create)
  unsigned fused_seq = 0;   // fused launches so far in the current solve
  // SpMV event sampling (eager mode)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool; size_t ev_used = 0;
  std::vector<int> ev_halves;   // half-iterations inside bracket i (0: the bracket is not counted)
  int64_t solve_index = 0;
  int64_t spmv_launched = 0, spmv_sampled = 0; double spmv_us_sum = 0.0;
  // block-tridiagonal direct solver (1D): cyclic-reduction pyramid
  std::vector<TriLevel> tri; DevBuf<double> tri_store; DevBuf<int32_t> tri_kpos; bool tri_ok = false;
  // block-banded LU (3D): direct solver / fallback of the Krylov solve; storage is allocated on first use
  DevBuf<double> lu_band, lu_dinv, lu_y, lu_part; DevBuf<int32_t> lu_pos, lu_node; BandView<BandReal> lu{}; bool lu_ready = false;
  // asynchronous coarse refresh: the Galerkin product + inverse of THIS iteration's matrix run on a side stream while
  // BiCGStab uses the inverse built from the previous iteration's matrix; adopted at the next set-up (double buffer)
  hipStream_t stream2 = nullptr; hipEvent_t ev_mat = nullptr, ev_chain = nullptr, ev_jac = nullptr, ev_dots = nullptr;
  DevBuf<double> Aci2; double* aci_buf[2] = {nullptr, nullptr}; int aci_cur = 0;
  bool chain_in_flight = false;
  // Jacobian gather beside Newton's convergence test (newton(), launch_jac_gather_ahead): the gather of the NEXT iteration's
  // matrix runs on the side stream behind k_element, into the value buffer the context does not point at, while the main
  // stream forms the residual norm and the host judges it.  `go_on` adopts both: c.vals and vals_spare change places, and
  // so do `stream` and `stream2` — the iteration carries on in the stream that holds the gather, behind it, and the stream
  // the host has just synchronised becomes the side stream (a way back through an event costs about what the overlap
  // gains).  Any other verdict leaves c.vals, and with it every reader of the Jacobian, as it was.
  DevBuf<double> vals2; double* vals_spare = nullptr;
  hipEvent_t ev_elem = nullptr, ev_gather = nullptr;
  int chain_level = 0;           // GMPNP_NEWTON_CHAIN: 0 the serial chain, 1 the gather beside the test, 2 (default) with the folded launches
  bool gather_pending = false;   // a gather into vals_spare is in flight on the side stream (ev_gather)
  int direct_solves = 0;        // band LU solves since create (factorisations)
  hipEvent_t ev_phase[6] = {};
  hipEvent_t ev_poll[2] = {};
  // mesh partition (gmpnp_create_partition): halo plan in INTERNAL node ids, buffers of the fused exchanges
  bool partitioned = false; int part_rank = 0, part_size = 1;
  bool staged_element = false;   // k_element writes its records through LDS, record by record (large 3D meshes)
  bool matp = false;        // materialised vector form of the BiCGStab half-iterations (opts.vector_form; automatic above 768 MB of matrix)
  bool prereduce = false;   // unpartitioned, many tile slots per aggregate: k_dist_reduce feeds the coarse kernels (Ctx::dist)
  std::vector<int32_t> nb_rank, send_ptr, recv_ptr;   // neighbours; [n_neighbours + 1] offsets into the node lists
  DevBuf<int32_t> send_nodes, recv_nodes, tile_cols_x;
  DevBuf<double> sendbuf, recvbuf, red_i, red_a, red_b, red_norm;
  double* h_red = nullptr;   // pinned [8]: all-reduced ||b||^2 and status bits
  std::unique_ptr<gmpnp_projector> projector;
  std::unique_ptr<gmpnp_selector> selector;
  std::unique_ptr<gmpnp_budgeter> budgeter;
  std::unique_ptr<gmpnp_step_limiter> limiter;
  std::unique_ptr<gmpnp_time_stepper> stepper;
  std::unique_ptr<gmpnp_sterner> sterner;
  std::unique_ptr<gmpnp_kineticist> kineticist;
  std::unique_ptr<gmpnp_galvanostat> galvanostat;
  std::unique_ptr<gmpnp_responder> responder;
  std::unique_ptr<gmpnp_band_responder> band_responder;
  std::unique_ptr<gmpnp_tangenter> tangenter;
  std::unique_ptr<gmpnp_tracer> tracer;
  std::unique_ptr<gmpnp_sensitizer> sensitizer;
  std::unique_ptr<gmpnp_wall_profiler> wall_profiler;
  std::unique_ptr<gmpnp_cycler> cycler;
  // bndF + the Stern term (potential rows) + the kinetic term (species rows): what Ctx::bndF points at while either option is on
  // (boundary_rebind); allocated by the first of them
  DevBuf<double> bnd_dyn;
  // geometric multilevel term (gmpnp_attach_coarse_level, gmpnp_multilevel.h): the link to the next-coarser level (tables in the
  // internal orders of both handles) and this handle's buffers when it serves as a coarse level itself
  gmpnp_solver* ml_coarse = nullptr; double ml_theta = 1.0; bool ml_is_coarse = false;
  int ml_sweeps = 2;   // as the COARSEST level: smoothing steps per application (an intermediate level runs a V(1,1) cycle)
  double ml_omega = 0.7;   // damping of the smoothing steps
  int ml_mid_jacobi = 1;   // intermediate levels smooth with node-block Jacobi alone (the slab coarse space stays with the coarsest level)
  DevBuf<int32_t> ml_par, ml_child_ptr, ml_child, ml_copy;
  DevBuf<double> ml_r, ml_w, ml_z;
  DevBuf<uint8_t> ml_tbc;   // partitioned levels: TRUE Dirichlet flags of the local dofs, ghost rows included (k_pml_flags)
  DevBuf<double> ml_tbd;    // ... their staging as doubles for the halo exchange

  ~gmpnp_solver() {
    for (auto& e : ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : ev_phase) if (e) (void)hipEventDestroy(e);
    for (auto& e : ev_poll) if (e) (void)hipEventDestroy(e);
    if (h_scal) (void)hipHostFree(h_scal);
    if (h_poll) (void)hipHostFree(h_poll);
    if (h_bcval) (void)hipHostFree(h_bcval);
    if (h_stage) (void)hipHostFree(h_stage);
    if (h_part) (void)hipHostFree(h_part);
    if (h_status) (void)hipHostFree(h_status);
    if (h_red) (void)hipHostFree(h_red);
    if (stream2) { if (stream) (void)hipStreamSynchronize(stream); (void)hipStreamSynchronize(stream2); (void)hipStreamDestroy(stream2); }   // (the two change roles: newton())
    if (ev_mat) (void)hipEventDestroy(ev_mat);
    if (ev_chain) (void)hipEventDestroy(ev_chain);
    if (ev_jac) (void)hipEventDestroy(ev_jac);
    if (ev_dots) (void)hipEventDestroy(ev_dots);
    if (ev_elem) (void)hipEventDestroy(ev_elem);
    if (ev_gather) (void)hipEventDestroy(ev_gather);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {

// ---- dispatch on (dim, n_fields) ---------------------------------------------------------------
#define GMPNP_DISPATCH(s, CALL)                                   \
  do {                                                            \
    if ((s)->dim == 3 && (s)->nf == 9) { constexpr int DIM = 3, NF = 9; CALL; } \
    else if ((s)->dim == 1 && (s)->nf == 7) { constexpr int DIM = 1, NF = 7; CALL; } \
    else return fail(GMPNP_ERR_INVALID, "unsupported (dim, n_fields)"); \
  } while (0)

int grid_for(int n, int block) { return (n + block - 1) / block; }

// gmpnp_stern.h: the Stern term of the potential rows in front of a residual gather, its Jacobian entries behind the Jacobian gather
inline bool stern_on(const gmpnp_solver* s) { return s->sterner && s->sterner->opt.model != 0; }
int stern_launch_residual(gmpnp_solver* s, int32_t* status);
int stern_launch_jacobian(gmpnp_solver* s);
int stern_launch_sum(gmpnp_solver* s, double* table_entry);
// gmpnp_kinetics.h: the kinetic term of the species rows beside the Stern term, its Jacobian entries behind the Stern entries
inline bool kinetics_on(const gmpnp_solver* s) { return s->kineticist && s->kineticist->opt.n_reactions != 0; }
int kinetics_launch_residual(gmpnp_solver* s, int32_t* status);
int kinetics_launch_jacobian(gmpnp_solver* s);
int kinetics_launch_sum(gmpnp_solver* s, int32_t* status, double* table);
// gmpnp_galvanostat.h: p_M as one more unknown; the Stern kernels read it through this pointer (nullptr: the option's own value)
inline bool galvanostat_on(const gmpnp_solver* s) { return s->galvanostat && s->galvanostat->opt.on != 0; }
inline const double* galvanostat_p_M(const gmpnp_solver* s) { return galvanostat_on(s) ? s->galvanostat->scal.p : nullptr; }
int galvanostat_shift(gmpnp_solver* s, bool to_previous);
int galvanostat_launch_iteration(gmpnp_solver* s);
template <int DIM, int NF>
int newton_galvanostat(gmpnp_solver* s, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st);
// gmpnp_response.h: the two launches of the last chunk of the last gmpnp_frequency_response (gmpnp_time_kernel 27)
bool response_has_chunk(const gmpnp_solver* s);
int response_time_chunk(gmpnp_solver* s);
// gmpnp_response_band.h: every launch of the last chunk of the last gmpnp_frequency_response_3d (gmpnp_time_kernel 30)
bool response_band_has_chunk(const gmpnp_solver* s);
int response_band_time_chunk(gmpnp_solver* s);
// gmpnp_tangent.h: the multi-column chain(s) of the last gmpnp_electrode_tangent (gmpnp_time_kernel 28); whatever changes u, p_M or an
// option drops the tangent the advance would use
bool tangent_has_chain(const gmpnp_solver* s);
int tangent_time_chain(gmpnp_solver* s);
inline void tangent_drop(gmpnp_solver* s) { if (s->tangenter) { s->tangenter->fresh = false; s->tangenter->cols_fresh = false; } }
// gmpnp_trace.h: the launches of one gmpnp_electrode_trace_append into a slot and accumulators of the hook's own (gmpnp_time_kernel 29)
bool trace_is_open(const gmpnp_solver* s);
int trace_time_append(gmpnp_solver* s);
// gmpnp_sensitivity.h: the launches of one gmpnp_sensitivity_step on a second S, a slot and accumulators of the hook's own (gmpnp_time_kernel 31)
bool sensitivity_is_open(const gmpnp_solver* s);
int sensitivity_time_step(gmpnp_solver* s);
// gmpnp_wall_profile.h: the launches of one gmpnp_wall_profile_append into the row of slots and the charges of the hook's own (gmpnp_time_kernel 32)
bool wall_profile_is_open(const gmpnp_solver* s);
int wall_profile_time_append(gmpnp_solver* s);
// gmpnp_cycle.h: residual + reduce + mix on the window of an open cycle, between a bracket that keeps u and u_n (gmpnp_time_kernel 33)
bool cycle_has_window(const gmpnp_solver* s);
int cycle_time_launch(gmpnp_solver* s);
int cycle_kernel_begin(gmpnp_solver* s, DevBuf<double>& keep);
int cycle_kernel_end(gmpnp_solver* s, DevBuf<double>& keep);

// Either option on: bnd_dyn <- bndF (which restores the rows of an option just switched off; the kernels of the options that are on
// rewrite theirs in front of every residual gather) and the context reads bnd_dyn.  Both off: the context reads the constant bndF.
int boundary_rebind(gmpnp_solver* s) {
  if (!stern_on(s) && !kinetics_on(s)) { s->c.bndF = s->bndF.p; return GMPNP_OK; }
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (s->bnd_dyn.n != (size_t)s->ndof) HIP_TRY(s->bnd_dyn.alloc((size_t)s->ndof, false));
  HIP_TRY(hipMemcpy(s->bnd_dyn.p, s->bndF.p, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToDevice));
  s->c.bndF = s->bnd_dyn.p;
  return GMPNP_OK;
}

size_t coarse_lds_bytes(int n, int nf) { return (size_t)(n * n + n * nf + 2 * nf * nf) * sizeof(double); }

// Facet / point integrals that do not depend on u, and the Robin mass entries (SURVEY App. D "facets").
int rebuild_boundary(gmpnp_solver* s) {
  const Topology& t = s->t;
  const int nf = s->nf, ns = nf - 1;
  std::vector<double> bnd((size_t)s->ndof, 0.0);
  struct Ent { int row, col; double v; };
  std::vector<Ent> ents;
  auto area = [&](const int32_t* f) {
    const double* a = &t.coords[(size_t)f[0] * 3]; const double* b = &t.coords[(size_t)f[1] * 3];
    const double* c = &t.coords[(size_t)f[2] * 3];
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    return 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
  };
  if (s->dim == 3) {
    for (size_t k = 0; k + 2 < s->wall_f.size(); k += 3) {
      const int32_t* f = &s->wall_f[k]; const double ar = area(f);
      for (int i = 0; i < ns; ++i)
        if (s->model.wall_flux[i] != 0.0)
          for (int a = 0; a < 3; ++a) bnd[(size_t)f[a] * nf + i] += s->model.wall_flux[i] * ar / 3.0;
    }
    for (size_t k = 0; k + 2 < s->exit_f.size(); k += 3) {
      const int32_t* f = &s->exit_f[k]; const double ar = area(f);
      for (int i = 0; i < ns; ++i) {
        const double kap = s->model.exit_kappa[i];
        if (kap == 0.0) continue;
        for (int a = 0; a < 3; ++a) {
          bnd[(size_t)f[a] * nf + i] += -kap * ar / 3.0;
          for (int b = 0; b < 3; ++b) ents.push_back({f[a] * nf + i, f[b] * nf + i, kap * ar * (a == b ? 2.0 : 1.0) / 12.0});
        }
      }
    }
  }
  for (int v : s->point_v)
    for (int i = 0; i < ns; ++i) bnd[(size_t)v * nf + i] += s->model.point_flux[i];
  // merge duplicates (stable order of first appearance => deterministic)
  std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.row != b.row ? a.row < b.row : a.col < b.col; });
  std::vector<int32_t> rrow, rcol, rptr((size_t)s->ndof + 1, 0); std::vector<double> rval; std::vector<int64_t> raddr;
  // ... and by node block (an entry couples species i of two nodes: it sits on the diagonal of its block)
  std::vector<int32_t> rblk(t.cols.size(), -1); std::vector<double> rbval; std::vector<uint32_t> rbmask;
  bool blk_ok = true;
  for (size_t k = 0; k < ents.size();) {
    size_t j = k; double v = 0.0;
    while (j < ents.size() && ents[j].row == ents[k].row && ents[j].col == ents[k].col) v += ents[j++].v;
    const int row = ents[k].row, col = ents[k].col;
    const int I = row / nf, i = row % nf, J = col / nf, jf = col % nf;
    const int32_t* b = t.cols.data() + t.rowptr[I]; const int32_t* e = t.cols.data() + t.rowptr[I + 1];
    const int blk = (int)(std::lower_bound(b, e, J) - t.cols.data());
    const int kpos = t.sellk[blk];
    const int sl = t.node_slice[I], il = I - t.slice_node0[sl];
    if (i != jf || i >= ns) blk_ok = false;
    else {
      if (rblk[blk] < 0) { rblk[blk] = (int32_t)rbmask.size(); rbmask.push_back(0u); rbval.resize(rbval.size() + ns, 0.0); }
      rbmask[rblk[blk]] |= 1u << i; rbval[(size_t)rblk[blk] * ns + i] = v;
    }
    rrow.push_back(row); rcol.push_back(col); rval.push_back(v);
    raddr.push_back(t.slice_off[sl] + (int64_t)(kpos * nf + jf) * kWave + il * nf + i);
    rptr[row + 1]++;
    k = j;
  }
  for (int r = 0; r < s->ndof; ++r) rptr[r + 1] += rptr[r];
  HIP_TRY(s->bndF.upload(bnd)); HIP_TRY(s->robF_ptr.upload(rptr)); HIP_TRY(s->rob_col.upload(rcol));
  HIP_TRY(s->rob_row.upload(rrow)); HIP_TRY(s->rob_val.upload(rval)); HIP_TRY(s->rob_addr.upload(raddr));
  s->c.bndF = s->bndF.p; s->c.robF_ptr = s->robF_ptr.p; s->c.rob_col = s->rob_col.p; s->c.rob_row = s->rob_row.p;
  s->c.rob_val = s->rob_val.p; s->c.rob_addr = s->rob_addr.p; s->c.n_robin = (int)rval.size();
  s->c.rob_blk = nullptr;   // (entries off a block's diagonal: none today; the gather would leave them to k_robin_add)
  if (blk_ok && !rval.empty()) {
    HIP_TRY(s->rob_blk.upload(rblk)); HIP_TRY(s->rob_blk_val.upload(rbval)); HIP_TRY(s->rob_blk_mask.upload(rbmask));
    s->c.rob_blk = s->rob_blk.p; s->c.rob_blk_val = s->rob_blk_val.p; s->c.rob_blk_mask = s->rob_blk_mask.p;
  }
  return boundary_rebind(s);   // the new constant vector under the Stern and kinetic terms (nothing to do with both off)
}

int check_model(const gmpnp_model_t* m, int dim) {
  if (!m) return fail(GMPNP_ERR_INVALID, "model is NULL");
  if (m->dim != dim) return fail(GMPNP_ERR_INVALID, "model.dim != mesh.dim");
  if (m->n_species < 1 || m->n_species > GMPNP_MAX_SPECIES) return fail(GMPNP_ERR_INVALID, "model.n_species out of range");
  if (m->n_bilinear < 0 || m->n_bilinear > GMPNP_MAX_BILINEAR) return fail(GMPNP_ERR_INVALID, "model.n_bilinear out of range");
  for (int t = 0; t < m->n_bilinear; ++t)
    if (m->bil_j[t] < 0 || m->bil_j[t] >= m->n_species || m->bil_k[t] < 0 || m->bil_k[t] >= m->n_species)
      return fail(GMPNP_ERR_INVALID, "model.bil_j/bil_k out of range");
  if (!(m->inv_dt == m->inv_dt)) return fail(GMPNP_ERR_INVALID, "model.inv_dt is NaN");
  return GMPNP_OK;
}

// ---- device passes --------------------------------------------------------------------------
template <int DIM, int NF>
int launch_element(gmpnp_solver* s, bool want_j) {
  const int g = grid_for(s->t.nc, 64);
  if constexpr (DIM == 3) {
    // large meshes: record stores staged through LDS (k_element<.., STAGED>); the reference meshes keep the direct form
    if (want_j && s->staged_element) {
      hipLaunchKernelGGL((k_element<DIM, NF, true, true>), dim3(g), dim3(64), 0, s->stream, s->c);
      HIP_TRY(hipGetLastError());
      return GMPNP_OK;
    }
  }
  if (want_j) hipLaunchKernelGGL((k_element<DIM, NF, true>), dim3(g), dim3(64), 0, s->stream, s->c);
  else hipLaunchKernelGGL((k_element<DIM, NF, false>), dim3(g), dim3(64), 0, s->stream, s->c);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

template <int DIM, int NF>
int launch_res_gather(gmpnp_solver* s) {
  hipLaunchKernelGGL((k_res_gather<DIM, NF>), dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream, s->c);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

template <int DIM, int NF>
int launch_jac_gather(gmpnp_solver* s, bool fold_robin = false) {
  const int g = grid_for(s->c.n_work * kWave, kVecBlock);   // n_work = 8 equal runs, each a whole number of workgroups
  if (fold_robin && s->c.n_robin > 0 && s->c.rob_blk) {   // Newton's chain: one launch
    hipLaunchKernelGGL((k_jac_gather<DIM, NF, true>), dim3(g), dim3(kVecBlock), 0, s->stream, s->c);
  } else {
    hipLaunchKernelGGL((k_jac_gather<DIM, NF>), dim3(g), dim3(kVecBlock), 0, s->stream, s->c);
    if (s->c.n_robin > 0) hipLaunchKernelGGL(k_robin_add, dim3(grid_for(s->c.n_robin, 256)), dim3(256), 0, s->stream, s->c);
  }
  HIP_TRY(hipGetLastError());
  if (stern_on(s)) { int rc = stern_launch_jacobian(s); if (rc) return rc; }
  if (kinetics_on(s)) return kinetics_launch_jacobian(s);
  return GMPNP_OK;
}

// The same launches on the side stream, into vals_spare, behind `ev_elem` (recorded in the main stream where the element
// records and the dynamic boundary vector of this state are complete).  Nothing in the main stream waits for them here.
template <int DIM, int NF>
int launch_jac_gather_ahead(gmpnp_solver* s) {
  HIP_TRY(hipStreamWaitEvent(s->stream2, s->ev_elem, 0));
  hipStream_t keep = s->stream; double* cur = s->c.vals;
  s->stream = s->stream2; s->c.vals = s->vals_spare;   // (as ml_setup lends a stream: every launch below takes both from the handle)
  const int rc = launch_jac_gather<DIM, NF>(s, s->chain_level >= 2);
  s->stream = keep; s->c.vals = cur;
  if (rc) return rc;
  HIP_TRY(hipEventRecord(s->ev_gather, s->stream2));
  s->gather_pending = true;
  return GMPNP_OK;
}
// where newton() may do so: the handle got the second value buffer at create and no multilevel level holds a copy of its context
inline bool gather_ahead_ok(const gmpnp_solver* s) { return s->vals_spare && s->stream2 && !s->ml_coarse && !s->ml_is_coarse; }

int drain_spmv_events(gmpnp_solver* s);
int budget_launch_any(gmpnp_solver* s);   // gmpnp_budget.h: the launch chain of one species-budget call
int time_launch_any(gmpnp_solver* s);     // gmpnp_time_step.h: estimator + reduce + shift, between the bracket that keeps u_n and u_nm1
int time_kernel_begin(gmpnp_solver* s, DevBuf<double>& keep);
int time_kernel_end(gmpnp_solver* s, DevBuf<double>& keep);
int time_launch_any2(gmpnp_solver* s);    // gmpnp_time_order.h: history + estimator + reduce + three-deep shift, bracket as above with u_nm2
int time_kernel_begin2(gmpnp_solver* s, DevBuf<double>& keep);
int time_kernel_end2(gmpnp_solver* s, DevBuf<double>& keep);
// The residual, Jacobian and budget contexts read their previous state from c.un: u_n, or u* after a BDF2 set-up.  Whatever
// makes u* stale (a plain gmpnp_set_time_step, a u_n written from outside, order 1) points it back at u_n.
inline void time_read_un(gmpnp_solver* s) { s->c.un = s->un.p; }

// sum of row `row` (0 .. 2) of the pinned partials the reduction kernels store (k_res_gather, k_true_residual: row 0; k_dots3: three)
double sum_partials(const gmpnp_solver* s, int row) {
  double acc = 0.0;
  for (int i = 0; i < s->n_resblocks; ++i) acc += s->h_part[(size_t)row * s->n_resblocks + i];
  return acc;
}

// residual at the current u: returns ||b||_2 and the device status flags
template <int DIM, int NF>
int residual(gmpnp_solver* s, bool want_j, double* norm, int* flags, bool gather_ahead = false) {
  int rc = launch_element<DIM, NF>(s, want_j); if (rc) return rc;
  if (stern_on(s)) { rc = stern_launch_residual(s, s->status.p); if (rc) return rc; }
  if (kinetics_on(s)) { rc = kinetics_launch_residual(s, s->status.p); if (rc) return rc; }
  if (gather_ahead) HIP_TRY(hipEventRecord(s->ev_elem, s->stream));
  rc = launch_res_gather<DIM, NF>(s); if (rc) return rc;
  if (gather_ahead) { rc = launch_jac_gather_ahead<DIM, NF>(s); if (rc) return rc; }   // (enqueued behind the main stream's own work)
  // the partials and the status word land in pinned host memory by the kernel's own stores: no copy in the stream
  HIP_TRY(hipStreamSynchronize(s->stream));
  rc = drain_spmv_events(s); if (rc) return rc;
  *norm = std::sqrt(sum_partials(s, 0));
  *flags = *s->h_status;
  return GMPNP_OK;
}

// `refresh` = false keeps the previous Dinv and coarse inverse (any nonsingular block scaling and any coarse operator
// give a valid right preconditioner) and only re-scales the new matrix: the cheap path of a lagged preconditioner.
// The coarse chain: the Galerkin product P^T A P (the partitioned set-up all-reduces it before the inverse), then its inverse.
template <int NF>
void launch_coarse_galerkin(gmpnp_solver* s, const Ctx& c, hipStream_t st) {
  hipLaunchKernelGGL((k_coarse_rows<NF>), dim3(s->t.nslices), dim3(64), 0, st, c);
  hipLaunchKernelGGL((k_coarse_sum<NF>), dim3(s->t.nagg * s->c.coarse_chunks), dim3(kVecBlock), 0, st, c);
  hipLaunchKernelGGL(k_coarse_reduce, dim3(grid_for(s->ncoarse * s->ncoarse, kVecBlock)), dim3(kVecBlock), 0, st, c);
}
template <int NF>
void launch_coarse_chain(gmpnp_solver* s, const Ctx& c, hipStream_t st) {
  launch_coarse_galerkin<NF>(s, c, st);
  hipLaunchKernelGGL((k_coarse_invert<NF>), dim3(1), dim3(512), coarse_lds_bytes(s->ncoarse, NF), st, c);
}

// `allow_async` (Newton): unless `refresh_coarse` demands an inverse of THIS matrix now, the coarse chain of this matrix
// is started on the side stream and the solve runs with the inverse the previous chain left (any coarse operator gives a
// valid preconditioner; one iteration of staleness costs < 1 % BiCGStab iterations, the chain is 155 us of a single
// stream otherwise).  The chain reads vals_s and owns AP / AcPart / Ac: it is awaited (in stream order, the host does
// not block) before the next k_scale_columns and before any chain in the main stream.
template <int DIM, int NF>
int ml_setup(gmpnp_solver* s);
template <int DIM, int NF>
int setup_preconditioner(gmpnp_solver* s, int mode, bool refresh = true, bool refresh_coarse = true, bool allow_async = false) {
  s->c.use_coarse = (mode == GMPNP_LINEAR_BICGSTAB_TWOLEVEL) ? 1 : 0;
  if (!s->precond_valid || s->precond_mode != mode) refresh = refresh_coarse = true;
  if constexpr (DIM == 3 && NF == 9) {
    if (s->ml_coarse && refresh) { int rc = ml_setup<DIM, NF>(s); if (rc) return rc; }   // level Jacobians at the injected state
  }
  if (refresh) hipLaunchKernelGGL((k_block_inverse<NF>), dim3(grid_for(s->t.nv, 4)), dim3(64), 0, s->stream, s->c);
  const bool had_chain = s->chain_in_flight;
  if (had_chain) { HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_chain, 0)); s->chain_in_flight = false; }
  hipLaunchKernelGGL((k_scale_columns<NF>), dim3(grid_for(s->c.n_work * kWave, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->c);
  if (s->c.use_coarse && refresh) {
    const bool async = allow_async && s->cfg.coarse_async && s->stream2 != nullptr;
    if (async && !refresh_coarse) {
      if (had_chain) { s->aci_cur ^= 1; s->c.Aci = s->aci_buf[s->aci_cur]; }   // adopt what the previous chain left
      HIP_TRY(hipEventRecord(s->ev_mat, s->stream));
      HIP_TRY(hipStreamWaitEvent(s->stream2, s->ev_mat, 0));
      Ctx c2 = s->c; c2.Aci = s->aci_buf[s->aci_cur ^ 1];
      launch_coarse_chain<NF>(s, c2, s->stream2);
      HIP_TRY(hipEventRecord(s->ev_chain, s->stream2));
      s->chain_in_flight = true;
    } else if (refresh_coarse) {
      launch_coarse_chain<NF>(s, s->c, s->stream);   // inverse of this matrix, now (a pending side-stream result is dropped; the next set-up starts a new chain)
    }
  }
  HIP_TRY(hipGetLastError());
  s->precond_valid = true; s->precond_mode = mode;
  return GMPNP_OK;
}

// ---- geometric multilevel term (gmpnp_multilevel.h); every launch goes to the FINEST handle's stream ------------------------------
template <int NF>
int apply_minv(gmpnp_solver* s, int mode, const double* src, double* dst, double scale_dst, double scale_x, const NewtonUpdate* upd = nullptr);
template <int NF>
int ml_level_apply(gmpnp_solver* top, gmpnp_solver* L);
// L->ml_r holds the restricted residual r of level L; L->ml_w = S_L r, one V(1,1) cycle from x = 0 (a FIXED linear operator, as
// BiCGStab requires) with the level's own two-level preconditioner M_L^-1 = Dinv_L (I + Ps Aci Ps^T) as the smoother:
//     x  = w M_L^-1 r                                       pre-smoothing (w = ml_omega, damped)
//     x += mask P S_{L+1} mask P^T (r - J_L x)              coarse-grid correction, if a coarser level is attached
//     x += w M_L^-1 (r - J_L x)                             post-smoothing; the COARSEST level repeats it ml_sweeps - 1 times
// Two SpMVs with the level's Jacobian per cycle (1/8 of the next finer level's each).  Scratch: the level handle's Krylov vectors
// (it never runs a solve of its own).
template <int NF>
int ml_level_apply(gmpnp_solver* top, gmpnp_solver* L) {
  hipStream_t st = top->stream, keep = L->stream;
  const int n = (int)L->ndof;
  const dim3 vg(grid_for(n, 256));
  auto smooth = [&](const double* src, double scale_dst) -> int {   // ml_w = scale_dst * ml_w + omega * M_L^-1 src
    if (L->ml_coarse && L->ml_mid_jacobi) {   // intermediate level: damped node-block Jacobi alone, one launch
      hipLaunchKernelGGL((k_ml_jacobi<NF>), vg, dim3(256), 0, st, (const double*)L->c.Dinv, src, L->ml_w.p, scale_dst, L->ml_omega, n);
      return GMPNP_OK;
    }
    L->stream = st;
    const int rc = apply_minv<NF>(L, GMPNP_LINEAR_BICGSTAB_TWOLEVEL, src, L->ml_w.p, scale_dst, L->ml_omega, nullptr);
    L->stream = keep;
    return rc;
  };
  auto residual = [&]() {   // ks = r - J_L ml_w, one launch
    hipLaunchKernelGGL((k_spmv_residual<NF>), dim3(L->t.own_ntiles), dim3(kKrylovThreads), 0, st, L->c, (const double*)L->ml_w.p, (const double*)L->ml_r.p, L->ks.p);
  };
  int rc = smooth(L->ml_r.p, 0.0); if (rc) return rc;
  if (gmpnp_solver* C = L->ml_coarse) {
    residual();
    hipLaunchKernelGGL((k_ml_restrict<NF>), dim3(grid_for(C->ndof, 256)), dim3(256), 0, st, (const double*)L->ks.p, L->c.bcflag, (const int32_t*)L->ml_child_ptr.p,
                       (const int32_t*)L->ml_child.p, C->c.bcflag, C->ml_r.p, (int)C->ndof);
    rc = ml_level_apply<NF>(top, C); if (rc) return rc;
    hipLaunchKernelGGL((k_ml_prolong_add<NF>), vg, dim3(256), 0, st, (const double*)C->ml_w.p, (const int32_t*)L->ml_par.p, L->c.bcflag, L->ml_w.p, n);
    residual();
    rc = smooth(L->ks.p, 1.0); if (rc) return rc;
  } else {
    for (int k = 1; k < L->ml_sweeps; ++k) { residual(); rc = smooth(L->ks.p, 1.0); if (rc) return rc; }
  }
  return GMPNP_OK;
}
// coarse part of T src on the finest level: leaves it in s->ml_coarse->ml_w (to be prolonged by the caller's kernel)
template <int NF>
int ml_correction(gmpnp_solver* s, const double* src) {
  gmpnp_solver* C = s->ml_coarse;
  hipLaunchKernelGGL((k_ml_restrict<NF>), dim3(grid_for(C->ndof, 256)), dim3(256), 0, s->stream, src, s->c.bcflag, (const int32_t*)s->ml_child_ptr.p,
                     (const int32_t*)s->ml_child.p, C->c.bcflag, C->ml_r.p, (int)C->ndof);
  return ml_level_apply<NF>(s, C);
}
// z = vec + theta D T vec: the operand a materialised half-iteration stages
template <int NF>
int ml_stage(gmpnp_solver* s, const double* vec) {
  int rc = ml_correction<NF>(s, vec); if (rc) return rc;
  hipLaunchKernelGGL((k_ml_stage<NF>), dim3(grid_for(s->ndof, kMlStageNodes * NF)), dim3(kMlStageNodes * NF), 0, s->stream, s->c, (const double*)s->ml_coarse->ml_w.p,
                     (const int32_t*)s->ml_par.p, vec, s->ml_z.p, s->ml_theta);
  return GMPNP_OK;
}
// Once per preconditioner set-up: the state goes one level down by injection, the coarser level assembles ITS Jacobian there
// (element kernel + gather of this library on the level's own mesh) and sets up its own two-level preconditioner — which, if a
// still coarser level is attached to it, does the same one level further down (setup_preconditioner calls this function).
template <int DIM, int NF>
int ml_setup(gmpnp_solver* s) {
  gmpnp_solver* C = s->ml_coarse;
  hipStream_t keep = C->stream;
  C->stream = s->stream;   // (the level handle's own stream stays unused: everything of the hierarchy is ordered in the finest handle's)
  hipLaunchKernelGGL((k_ml_inject<NF>), dim3(grid_for(C->ndof, 256)), dim3(256), 0, s->stream, (const double*)s->u.p, (const int32_t*)s->ml_copy.p, C->u.p, (int)C->ndof);
  int rc = launch_element<DIM, NF>(C, true);
  if (!rc) rc = launch_jac_gather<DIM, NF>(C);
  if (!rc) { C->jacobian_valid = true; rc = setup_preconditioner<DIM, NF>(C, GMPNP_LINEAR_BICGSTAB_TWOLEVEL, true, true, false); }
  C->stream = keep;
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// What half-iteration A (h = 0) or B (h = 1) of an iteration of parity `par` leaves for the next one: its phase, the per-rank
// sums it all-reduces (into `red`), and the vectors whose ghost rows it sends (the next half unpacks them).
struct Half {
  int phase, nout; double* red;
  int nvec; VecListW vecs;
};
inline Half half_of(gmpnp_solver* s, int h, int par) {
  const int n = s->ncoarse;
  if (h == 0) return Half{1, 2 + 3 * n, s->red_a.p, 3, VecListW{{s->kr.p, s->c.kv[par], s->c.kp[par], nullptr}}};
  return Half{2, 4 + n, s->red_b.p, 2, VecListW{{s->ks.p, s->kt.p, nullptr, nullptr}}};
}
inline VecList read_only(const VecListW& w) { return VecList{{w.p[0], w.p[1], w.p[2], w.p[3]}}; }

// One half-iteration of the fused BiCGStab: one launch (coarse workgroups inside the tile launch), two, or three.
template <int NF, int WHICH>
int launch_half(gmpnp_solver* s, int k) {
  const dim3 cg(std::max(1, s->t.nagg));
  if (s->fused_half) {
    const dim3 fg(s->t.nagg + s->t.own_ntiles);
    const unsigned target = (unsigned)(++s->fused_seq);
    if (WHICH == 0) hipLaunchKernelGGL((k_half_a<NF>), fg, dim3(kKrylovThreads), 0, s->stream, s->c, k, target);
    else hipLaunchKernelGGL((k_half_b<NF>), fg, dim3(kKrylovThreads), 0, s->stream, s->c, k, target);
  } else if (s->matp) {   // materialised vectors: coarse kernel, streaming vector update, tile kernel staging one vector
    const dim3 vg(grid_for(s->ndof, 256));
    // with a multilevel term the tile kernel stages vec + theta D T vec (ml_stage) instead of the vector k_vec_a / k_vec_b wrote
    if (WHICH == 0) {
      hipLaunchKernelGGL((k_coarse_a<NF>), cg, dim3(kCoarseThreads), 0, s->stream, s->c, k);
      hipLaunchKernelGGL(k_vec_a, vg, dim3(256), 0, s->stream, s->c, k);
      if (s->ml_coarse) {
        if constexpr (NF == 9) { int rc = ml_stage<NF>(s, s->c.kp[k & 1]); if (rc) return rc; }
        Ctx cc = s->c; cc.stage_a = s->ml_z.p;
        hipLaunchKernelGGL((k_bicg_a_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, cc, k);
      } else hipLaunchKernelGGL((k_bicg_a_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, k);
    } else {
      hipLaunchKernelGGL((k_coarse_b<NF>), cg, dim3(kCoarseThreads), 0, s->stream, s->c, k);
      hipLaunchKernelGGL(k_vec_b, vg, dim3(256), 0, s->stream, s->c, k);
      if (s->ml_coarse) {
        if constexpr (NF == 9) { int rc = ml_stage<NF>(s, s->c.ks); if (rc) return rc; }
        Ctx cc = s->c; cc.stage_b = s->ml_z.p;
        hipLaunchKernelGGL((k_bicg_b_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, cc, k);
      } else hipLaunchKernelGGL((k_bicg_b_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, k);
    }
  } else if (WHICH == 0) {
    hipLaunchKernelGGL((k_coarse_a<NF>), cg, dim3(kCoarseThreads), 0, s->stream, s->c, k);
    hipLaunchKernelGGL((k_bicg_a<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, k);
  } else {
    hipLaunchKernelGGL((k_coarse_b<NF>), cg, dim3(kCoarseThreads), 0, s->stream, s->c, k);
    hipLaunchKernelGGL((k_bicg_b<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, k);
  }
  if (s->prereduce) {   // the sums the next coarse kernel reads
    const Half h = half_of(s, WHICH, k & 1);
    hipLaunchKernelGGL(k_dist_reduce, dim3(h.nout), dim3(256), 0, s->stream, s->c, h.phase, k & 1, h.red);
  }
  s->spmv_launched++;
  return GMPNP_OK;
}

int drain_spmv_events(gmpnp_solver* s) {
  for (size_t i = 0; i < s->ev_used; ++i) {
    if (s->ev_halves[i] <= 0) continue;   // a bracket that reached into the launches behind the end of its solve
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev_pool[i].first, s->ev_pool[i].second));
    s->spmv_us_sum += 1000.0 * ms; s->spmv_sampled += s->ev_halves[i];
  }
  s->ev_used = 0;
  return GMPNP_OK;
}

// Iteration k of the solve (k = 0, 1, ...): the index is a kernel ARGUMENT, so no kernel has to read it back from
// memory before it can address its parity buffers.
template <int NF>
int enqueue_iteration(gmpnp_solver* s, int k) {
  int rc = launch_half<NF, 0>(s, k);
  if (rc) return rc;
  return launch_half<NF, 1>(s, k);
}

// Start values of a BiCGStab pass; rho0 = (rhat, r_0), ||r_0|| = bnorm
KrylovScalars krylov_start(double rho0, double bnorm, double rtol, double atol, int maxit) {
  KrylovScalars init{};
  init.rho[0] = init.rho[1] = rho0; init.alpha = 1.0;
  init.tol = std::max(rtol * bnorm, atol); init.rr = init.rr0 = bnorm * bnorm; init.max_iters = maxit;
  if (!(bnorm > 0.0)) init.done = 1;  // zero right-hand side: dx = 0
  return init;
}
// The stats of a finished pass, and GMPNP_ERR_LINEAR ("<what> stopped without convergence ...") unless it converged
int krylov_verdict(const KrylovScalars& res, double bnorm, gmpnp_linear_stats_t* st, const char* what) {
  if (st) { st->iterations = res.iters; st->converged = (res.done == 1); st->residual_norm = std::sqrt(res.rr); st->rhs_norm = bnorm; }
  if (res.done == 1) return GMPNP_OK;
  char buf[200];
  snprintf(buf, sizeof buf, "%s stopped without convergence (code %d) after %d iterations, ||r|| = %.3e, ||b|| = %.3e",
           what, res.done, res.iters, std::sqrt(res.rr), bnorm);
  return fail(GMPNP_ERR_LINEAR, buf);
}

// Solve J dx = rhs (rhs already in c.kr on the device, ||rhs|| = bnorm) with the fused right-preconditioned BiCGStab;
// leaves y in c.ky; the caller applies M^{-1} (apply_minv).
template <int NF>
int krylov(gmpnp_solver* s, int mode, double bnorm, double rtol, double atol, int maxit, gmpnp_linear_stats_t* st, bool restart = false,
           const double* warm_w = nullptr) {
  const int use_coarse = (mode == GMPNP_LINEAR_BICGSTAB_TWOLEVEL) ? 1 : 0;
  s->c.use_coarse = use_coarse;
  s->fused_seq = 0;
  const KrylovScalars init = krylov_start(s->shadow_src ? s->shadow_rho0 : bnorm * bnorm, bnorm, rtol, atol, maxit);
  // one launch: shadow vector (r_0, or a pseudo-random vector after a breakdown), y = 0, P^T r_0 partials
  // where A(0) expects them, hand-over flags cleared, scalars from the kernel argument
  hipLaunchKernelGGL((k_krylov_init<NF>), dim3(s->t.own_ntiles), dim3(kVecBlock), 0, s->stream, s->c, s->shadow_src, init, s->cpart_v1.p, warm_w);
  if (s->prereduce && use_coarse) hipLaunchKernelGGL(k_dist_reduce, dim3(s->ncoarse), dim3(256), 0, s->stream, s->c, 0, 0, s->red_i.p);
  // the previous solve wrote its verdict before the host left its loop and nothing of it writes the mirror afterwards
  volatile HostPoll* hp = s->h_poll;
  hp->done = 0; hp->iters = 0; hp->rr = 0.0;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  const int B = s->cfg.burst_iters;
  // Bursts of B iterations; kernels of a converged solve exit at their first instruction.
  const int first = s->burst.first(use_coarse, s->opts.krylov_batch, B, restart);
  int next_k = 0;  // iteration index of the next launch (the device stops advancing once `done` is set)
  auto burst = [&](int iters) -> int {
    for (int it = 0; it < iters; ++it) { int rc = enqueue_iteration<NF>(s, next_k++); if (rc) return rc; }
    return GMPNP_OK;
  };
  KrylovScalars res = init;
  int launched = 0, slot = 0;
  // Timing for the roofline (opts.profile_every = N > 0): ONE event pair around the first burst of every Nth solve — a run of
  // back-to-back half-iterations, all of them live (checked against the solve's iteration count afterwards).  Elapsed time /
  // half-iterations = what a half-iteration costs in the solve, launch gaps included.  (Events attached to single dispatches
  // read 1.5 us more than rocprofv3's kernel durations: a dispatch with a completion signal of its own is a slower dispatch.)
  const int every = s->opts.profile_every;
  long bracket = -1;
  if (every > 0 && !restart && !res.done && first >= 2 && (s->solve_index++ % every) == 0) {
    if (s->ev_used == s->ev_pool.size()) {
      hipEvent_t a, b; HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b)); s->ev_pool.push_back({a, b}); s->ev_halves.push_back(0);
    }
    bracket = (long)s->ev_used++;
    s->ev_halves[bracket] = 0;
    HIP_TRY(hipEventRecord(s->ev_pool[bracket].first, s->stream));
  }
  if (!res.done) {
    int rc = burst(first); if (rc) return rc;
    if (bracket >= 0) HIP_TRY(hipEventRecord(s->ev_pool[bracket].second, s->stream));
    launched = first;
    bool mirror_ok = s->cfg.host_poll != 0;
    while (mirror_ok) {
      // The B kernels report progress straight into pinned host memory: launch the next burst, then spin until the
      // iterations launched BEFORE it are done (or the solve is).  No copy kernel and no event in the stream.
      const int target = launched;
      rc = burst(B); if (rc) return rc;
      launched += B;
      const double t_spin = now_ms();
      int spins = 0;
      while (!hp->done && hp->iters < target) {
        __builtin_ia32_pause();
        if ((++spins & 0xfff) == 0 && now_ms() - t_spin > 5000.0) { mirror_ok = false; break; }  // GPU stuck or mirror not visible
      }
      if (!mirror_ok) break;
      if (hp->done) {
        std::atomic_thread_fence(std::memory_order_acquire);
        res.done = hp->done; res.iters = hp->iters; res.rr = hp->rr;
        break;
      }
      if (launched > maxit + 4 * B) { mirror_ok = false; break; }  // defensive: the device test ends the loop at max_iters
    }
    while (!mirror_ok) {
      HIP_TRY(hipMemcpyAsync(&s->h_scal[slot], s->scal.p, sizeof(KrylovScalars), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipEventRecord(s->ev_poll[slot], s->stream));
      rc = burst(B); if (rc) return rc;  // speculative: overlaps the read-back
      launched += B;
      HIP_TRY(hipEventSynchronize(s->ev_poll[slot]));
      res = s->h_scal[slot];
      slot ^= 1;
      if (res.done) break;
      if (launched > maxit + 4 * B) break;  // defensive: the device test ends the loop at max_iters
    }
    // the sampled launches' events are read at the next point where the stream is synchronised anyway (residual(),
    // the end of gmpnp_linear_solve, gmpnp_spmv_profile): no wait of its own
  }
  if (bracket >= 0 && res.done == 1 && res.iters > first) s->ev_halves[bracket] = 2 * first;   // every launch of the burst did its work
  s->burst.solve_done(use_coarse, res.iters, restart);
  s->last_done = res.done;
  return krylov_verdict(res, bnorm, st, "BiCGStab");
}

// dst = scale_dst*dst + scale_x * M^{-1} src,  M^{-1} = Dinv (I + P Aci P^T)
template <int NF>
int apply_minv(gmpnp_solver* s, int mode, const double* src, double* dst, double scale_dst, double scale_x,
               const NewtonUpdate* upd) {
  s->c.use_coarse = (mode == GMPNP_LINEAR_BICGSTAB_TWOLEVEL) ? 1 : 0;
  const bool pre = s->prereduce && s->c.use_coarse;
  if (s->c.use_coarse)
    hipLaunchKernelGGL((k_restrict<NF>), dim3(s->t.own_ntiles), dim3(kVecBlock), 0, s->stream, s->c, src, s->cpart_v0.p);
  if (pre) hipLaunchKernelGGL(k_dist_reduce, dim3(s->ncoarse), dim3(256), 0, s->stream, s->c, 3, 0, s->red_i.p);
  hipLaunchKernelGGL((k_minv_apply<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, src,
                     (const double*)s->cpart_v0.p, dst, scale_dst, scale_x, upd ? *upd : NewtonUpdate{nullptr, nullptr, 0.0, 0.0, 0.0},
                     pre ? (const double*)s->red_i.p : (const double*)nullptr);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// kr = kb - J kx with the unscaled matrix; returns ||kr|| (synchronises the stream)
template <int NF>
int true_residual(gmpnp_solver* s, double* rn) {
  hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, (const double*)s->kx.p, s->kt.p);
  hipLaunchKernelGGL(k_true_residual, dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream, (const double*)s->kb.p, (const double*)s->kt.p,
                     s->kr.p, s->c.part_f, (int)s->ndof);
  HIP_TRY(hipStreamSynchronize(s->stream));
  *rn = std::sqrt(sum_partials(s, 0));
  return GMPNP_OK;
}

// Krylov solve with the answer checked: BiCGStab stops on its RECURSIVE residual, which can drift away from
// b - J dx over thousands of iterations (plain Jacobi mode on stiff systems).  After each pass the true residual is
// formed with the unscaled matrix; if it misses the target grossly (> 1000x), the solve restarts on it (dx accumulates
// in kx).  stats->residual_norm reports the TRUE residual.
// rhs in c.kr on entry; dx = kx on return.
// A predicted start (gmpnp_host_rules.h) leaves BiCGStab only b - J x0 to remove: the same absolute target is reached in far
// fewer iterations.  Falls back to x0 = 0 when x0 does not reduce the residual.
// What the caller asks for; the defaults: a cold solve, checked after every pass.
struct KrylovRequest {
  int mode = GMPNP_LINEAR_BICGSTAB_TWOLEVEL, maxit = 1;
  double bnorm = 0.0, rtol = 0.0, atol = 0.0;   // ||rhs||; targets on ||b - J x||
  int verify_above = 0;          // a first pass that converged within this many iterations goes unchecked (short solves do not drift)
  double warm_scale = 0.0, warm_prev = 0.0;   // predicted_start(): x0 = warm_scale * kx + warm_prev * kxp; (0, 0) = cold start
  bool rhs_ready = false;        // k_res_gather already left b in kr AND kb (Newton)
  bool x0_ready = false;         // kx already holds x0 (left by the previous Newton update)
  bool dots_in_flight = false;   // w = J x0 and its dot products were started on the side stream (ev_dots)
  bool refine = false;           // go on while passes still halve the true residual (gmpnp_linear_solve)
  const NewtonUpdate* upd = nullptr;   // Newton update + next predicted start, applied by the final M^-1 launch of a normal solve
  bool upd_done = false;         // out: that launch applied `upd`
};

template <int NF>
int krylov_verified(gmpnp_solver* s, gmpnp_linear_stats_t* st, KrylovRequest& q) {
  const int n = s->ndof;
  if (!std::isfinite(q.bnorm)) return fail(GMPNP_ERR_LINEAR, "right-hand side of the linear system is not finite");
  const double tol = std::max(q.rtol * q.bnorm, q.atol);
  // kb keeps the right-hand side
  if (!q.rhs_ready) HIP_TRY(hipMemcpyAsync(s->kb.p, s->kr.p, n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  q.upd_done = false;
  gmpnp_linear_stats_t total{}; total.rhs_norm = q.bnorm;
  double rhs_norm = q.bnorm;
  bool warm = false, fold_start = false;
  if (q.warm_scale != 0.0 && q.bnorm > 0.0) {
    // x0 = warm_scale * kx + warm_prev * kxp (left in kx by the previous Newton update when `x0_ready`); accepted when
    // it removes at least half of the residual: one plain SpMV, three dots, one host round trip
    if (!q.x0_ready) hipLaunchKernelGGL(k_warm_start, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, s->kx.p, s->kxp.p, q.warm_scale, q.warm_prev, n);
    if (q.dots_in_flight) {   // w = J x0 and the dot products were started on the side stream right after the Jacobian gather
      HIP_TRY(hipEventSynchronize(s->ev_dots));
      HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_dots, 0));   // kt is read by k_start_residual below
    } else {
      hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, (const double*)s->kx.p, s->kt.p);
      hipLaunchKernelGGL(k_dots3, dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream, (const double*)s->kt.p, (const double*)s->kb.p,
                         s->c.part_f, n, s->n_resblocks);
      HIP_TRY(hipStreamSynchronize(s->stream));
    }
    // The predicted correction is taken as it is.  (Scaling it by the minimal-residual multiple (w,b)/(w,w) makes |r0|
    // smaller every time and BiCGStab slower all the same: 18.8k instead of 17.3k iterations over the bench, round 1.)
    // r0 = b - w: formed by the first pass's k_krylov_init where one follows (fold_start), by a launch of its own otherwise
    if (accept_predicted_start(sum_partials(s, 0), sum_partials(s, 1), sum_partials(s, 2), &rhs_norm)) {
      fold_start = s->chain_level >= 2 && !s->partitioned && rhs_norm > tol;
      if (!fold_start) hipLaunchKernelGGL(k_start_residual, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, s->kr.p, (const double*)s->kb.p,
                                          (const double*)s->kt.p, n);
      warm = true;
    }  // else: kr still holds b, cold start
  }
  // Restarted BiCGStab.  A pass runs at most `restart_every` iterations; then (and after a breakdown) the true residual
  // b - J x is formed with the unscaled matrix and the next pass starts from it with a fresh shadow vector.  This bounds
  // the drift of the recursive residual, and it is what keeps BiCGStab from blowing up on the stiff systems of the
  // thinnest pores (L_50_R_1: ||r|| reached 1e53 inside 10,000 unrestarted iterations, the reference's direct solver
  // sails through).  A pass that ends in a breakdown or in a residual 1e5 times its start (device test) is thrown away
  // and repeated with a pseudo-random shadow vector.  Short solves (the normal case) take exactly one pass and no check.
  constexpr int restart_every = 1000;
  bool have_x = warm;      // kx holds a partial solution
  bool random_shadow = false;
  double pass_start = rhs_norm;   // true residual the current pass started from
  int bad_passes = 0;
  for (int pass = 0;; ++pass) {
    gmpnp_linear_stats_t ls{};
    int rc = GMPNP_OK;
    const int cap = std::min(restart_every, q.maxit - total.iterations);
    if (rhs_norm <= tol) { ls.converged = 1; ls.residual_norm = rhs_norm; s->last_done = 1; }  // nothing left to do
    else {
      if (random_shadow) {  // (rhat, r0) of the new shadow vector
        hipLaunchKernelGGL(k_fill_hash, dim3(grid_for(n, 256)), dim3(256), 0, s->stream, s->krand.p, (unsigned)(pass * 2654435761u), n);
        hipLaunchKernelGGL(k_dots3, dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream, (const double*)s->krand.p, (const double*)s->kr.p,
                           s->c.part_f, n, s->n_resblocks);
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->shadow_src = s->krand.p; s->shadow_rho0 = sum_partials(s, 0);
      }
      const bool first_cold = (pass == 0 && !warm);
      rc = krylov<NF>(s, q.mode, rhs_norm, first_cold ? q.rtol : 0.0, first_cold ? q.atol : tol, cap, &ls, pass > 0,
                      pass == 0 && fold_start ? (const double*)s->kt.p : nullptr);
      s->shadow_src = nullptr;
    }
    total.iterations += ls.iterations; total.converged = ls.converged; total.residual_norm = ls.residual_norm;
    if (rc && rc != GMPNP_ERR_LINEAR) { if (st) *st = total; return rc; }
    const bool usable = (s->last_done == 1 || s->last_done == 2);  // converged or cap reached: y is a valid partial solution
    if (usable && ls.iterations > 0) {
      // the normal end of a solve inside Newton (first pass, converged, short enough to go unchecked): the final
      // M^-1 application also applies the Newton update and leaves the predicted start of the next solve
      const bool final_now = q.upd && pass == 0 && s->last_done == 1 && ls.iterations <= q.verify_above && q.bnorm > 0.0 && !s->ml_coarse;
      int rc2 = apply_minv<NF>(s, q.mode, s->ky.p, s->kx.p, have_x ? 1.0 : 0.0, 1.0, final_now ? q.upd : nullptr); if (rc2) return rc2;
      if constexpr (NF == 9) {
        if (s->ml_coarse) {   // x += theta T y (the multilevel term of M^-1 applied to the Krylov solution)
          rc2 = ml_correction<NF>(s, s->ky.p); if (rc2) return rc2;
          hipLaunchKernelGGL((k_ml_add_solution<NF>), dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->c, (const double*)s->ml_coarse->ml_w.p,
                             (const int32_t*)s->ml_par.p, s->kx.p, s->ml_theta);
        }
      }
      if (final_now) q.upd_done = true;
      have_x = true; random_shadow = false;
    } else if (!usable) {
      random_shadow = true; ++bad_passes;
      HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
      if (!have_x) HIP_TRY(hipMemcpyAsync(s->kr.p, s->kb.p, n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));  // kr was the work vector
    }
    if (!have_x && s->last_done == 1) {  // zero right-hand side
      HIP_TRY(hipMemsetAsync(s->kx.p, 0, n * sizeof(double), s->stream)); have_x = true;
    }
    if (!(q.bnorm > 0.0)) break;
    if (pass == 0 && s->last_done == 1 && ls.iterations <= q.verify_above) break;  // short solves do not drift
    double rn = rhs_norm;
    if (have_x) { int rc2 = true_residual<NF>(s, &rn); if (rc2) return rc2; }  // kr = b - J x
    total.residual_norm = rn;
    // Converged by the recurrence and within 1000x of the target by the true residual: accepted.  (A 1e-10 solve of a
    // small right-hand side ends at the attainable accuracy of b - J dx in fp64, 3-30x the target late in a run.)
    // A non-finite true residual is a failed solve whatever the recurrence reported: the caller's direct fallback takes
    // over (3D) and nothing of this x reaches u.
    const bool finite = std::isfinite(rn);
    // `refine` (gmpnp_linear_solve): a pass that converged by its recurrence but left a true residual above the target is
    // followed by another pass on b - J x while passes still halve it; the 1000x acceptance then only covers stagnation at the
    // attainable accuracy.  (Without it, the generated 14 ... 370-vertex cylinders ended at 1.6e-9 ... 1.7e-8 of a 1e-10
    // target with 1e-13 attainable, and the solve said converged.)  Inside Newton the rule is unchanged.
    if (s->last_done == 1 && finite && rn <= tol) break;
    if (s->last_done == 1 && finite && rn <= 1e3 * tol && !(q.refine && rn < 0.5 * pass_start)) break;
    if (total.iterations >= q.maxit || bad_passes > 8 || !finite) {
      if (st) { total.converged = 0; *st = total; }
      char buf[200];
      snprintf(buf, sizeof buf, "BiCGStab stopped without convergence after %d iterations in %d passes (%d breakdowns), ||b - J x|| = %.3e, ||b|| = %.3e",
               total.iterations, pass + 1, bad_passes, rn, q.bnorm);
      return fail(GMPNP_ERR_LINEAR, buf);
    }
    rhs_norm = rn;  // next pass solves J ddx = r (already in kr)
    pass_start = rn;
  }
  if (st) *st = total;
  return GMPNP_OK;
}

// ---- 1D direct solver ---------------------------------------------------------------------------
int build_tridiagonal(gmpnp_solver* s) {
  const Topology& t = s->t; const int nv = t.nv, nf = s->nf;
  s->tri_ok = false;
  if (s->dim != 1) return GMPNP_OK;
  std::vector<int32_t> kp((size_t)nv * 3, -1);
  for (int I = 0; I < nv; ++I)
    for (int k = t.rowptr[I]; k < t.rowptr[I + 1]; ++k) {
      const int J = t.cols[k];
      if (J == I - 1) kp[(size_t)I * 3] = t.sellk[k];
      else if (J == I) kp[(size_t)I * 3 + 1] = t.sellk[k];
      else if (J == I + 1) kp[(size_t)I * 3 + 2] = t.sellk[k];
      else return GMPNP_OK;  // internal order is not the path order: direct solver unavailable
    }
  std::vector<int> ns; for (int n = nv;; n = (n + 1) / 2) { ns.push_back(n); if (n == 1) break; }
  size_t total = 0;
  for (int n : ns) total += (size_t)n * (5 * nf * nf + 3 * nf);
  HIP_TRY(s->tri_store.alloc(total));
  HIP_TRY(s->tri_kpos.upload(kp));
  double* p = s->tri_store.p;
  s->tri.clear();
  for (int n : ns) {
    TriLevel l{}; l.n = n;
    auto take = [&](size_t cnt) { double* q = p; p += cnt; return q; };
    l.L = take((size_t)nf * nf * n); l.D = take((size_t)nf * nf * n); l.U = take((size_t)nf * nf * n); l.b = take((size_t)nf * n);
    l.Li = take((size_t)nf * nf * n); l.Ui = take((size_t)nf * nf * n); l.bi = take((size_t)nf * n); l.x = take((size_t)nf * n);
    s->tri.push_back(l);
  }
  s->tri_ok = true;
  return GMPNP_OK;
}

// The top of the cyclic-reduction pyramid (every level whose upper neighbour has at most kBcrTailRows rows) is ONE launch,
// k_bcr_tail: levels l0 .. nl - 1 (tri[l0 + 1].n <= kBcrTailRows); the levels below l0 are one launch each, down and up.
int bcr_tail_first_level(const gmpnp_solver* s) {
  const int nl = (int)s->tri.size();
  int l0 = nl - 1;
  while (l0 > 0 && s->tri[l0].n <= kBcrTailRows && nl - l0 < kBcrTailLevels) --l0;
  return l0;
}

// Solve J x = rhs (device pointer, internal order) by block cyclic reduction; x stays in tri[0].x (SoA).
template <int NF>
int tri_solve(gmpnp_solver* s, const double* rhs) {
  if (!s->tri_ok) return fail(GMPNP_ERR_INVALID, "block-tridiagonal solver needs a 1D mesh in path order");
  hipLaunchKernelGGL((k_tri_extract<NF>), dim3(grid_for(s->t.nv * NF * NF, kVecBlock)), dim3(kVecBlock), 0, s->stream,
                     s->c, s->tri[0], s->tri_kpos.p, rhs);
  const int nl = (int)s->tri.size(), l0 = bcr_tail_first_level(s);
  for (int l = 0; l < l0; ++l)
    hipLaunchKernelGGL((k_bcr_forward<NF>), dim3(grid_for(s->tri[l + 1].n, 4)), dim3(64), 0, s->stream, s->tri[l],
                       s->tri[l + 1], s->status.p);
  {
    TriTail tt{};
    tt.nlev = nl - l0;
    for (int l = l0; l < nl; ++l) tt.lv[l - l0] = s->tri[l];
    hipLaunchKernelGGL((k_bcr_tail<NF>), dim3(1), dim3(kBcrTailThreads), 0, s->stream, tt, s->status.p);
  }
  for (int l = l0 - 1; l >= 0; --l)
    hipLaunchKernelGGL((k_bcr_backward<NF>), dim3(grid_for(s->tri[l].n * NF, kVecBlock)), dim3(kVecBlock), 0, s->stream,
                       s->tri[l], s->tri[l + 1]);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

template <int NF>
int tri_apply(gmpnp_solver* s, double* dst, double scale_dst, double scale_x) {
  hipLaunchKernelGGL((k_tri_apply<NF>), dim3(grid_for(s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, s->tri[0], dst,
                     scale_dst, scale_x, s->ndof);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// ---- 3D direct solver: block-banded LU ------------------------------------------------------------
template <int NF>
int band_prepare(gmpnp_solver* s) {
  if (s->lu_ready) return GMPNP_OK;
  const Topology& t = s->t;
  const int n = t.nv, b = std::max(t.lu_band, kBandPanel - 1);   // the substitution's panel triangle lies inside the stored band
  const double gb = (double)n * (2.0 * b + 1.0) * NF * NF * sizeof(double) / 1e9;
  char buf[200];
  if (gb > s->cfg.lu_max_gb) {
    snprintf(buf, sizeof buf, "block-banded LU needs %.1f GB (%d node blocks, band %d), above gmpnp_options_t.band_lu_max_gb = %.1f", gb, n, b, s->cfg.lu_max_gb);
    return fail(GMPNP_ERR_INVALID, buf);
  }
  HIP_TRY(s->lu_band.alloc((size_t)n * (2 * b + 1) * NF * NF, false));
  HIP_TRY(s->lu_dinv.alloc((size_t)n * NF * NF)); HIP_TRY(s->lu_y.alloc((size_t)n * NF));
  HIP_TRY(s->lu_pos.upload(t.lu_pos)); HIP_TRY(s->lu_node.upload(t.lu_node));
  HIP_TRY(s->lu_part.alloc((size_t)kBandPanel * kBandChunks * NF));
  BandView<BandReal>& lu = s->lu;   // a batch of one (BandReal::kBatched is false): no strides, every launch is live
  lu = BandView<BandReal>{};
  lu.band = s->lu_band.p; lu.dinv = s->lu_dinv.p; lu.lu_pos = s->lu_pos.p; lu.lu_node = s->lu_node.p; lu.n = n; lu.b = b;
  lu.status = s->status.p; lu.status_bit = 2;
  s->lu_ready = true;
  return GMPNP_OK;
}

// The launch chains of gmpnp_band_lu.h's kernels for a batch of m bands (the Newton path: 1; the 3D frequency response: a chunk of
// frequencies): S is BandReal or BandComplex.
// the factorisation of bands already scattered: D_0^-1, then one launch per pivot block
template <int NF, class S>
int band_launch_factor(hipStream_t stream, const BandView<S>& lu, int m) {
  constexpr int G = kBandThreads / (NF * NF);
  hipLaunchKernelGGL((k_band_step<NF, S>), dim3(1, 1, m), dim3(kBandThreads), 0, stream, lu, -1);
  for (int k = 0; k + 1 < lu.n; ++k) {
    const int w = std::min(lu.b, lu.n - 1 - k);
    hipLaunchKernelGGL((k_band_step<NF, S>), dim3(grid_for(w, S::kColChunk), grid_for(w, G) + 1, m), dim3(kBandThreads), 0, stream, lu, k);
  }
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}
// one substitution of every live member: rhs -> x (both internal order); y [m][n NF] and part [m][kBandPanel][kBandChunks][NF] are its workspace
template <int NF, class S>
int band_launch_substitute(hipStream_t stream, const BandView<S>& lu, int m, const typename S::Store* rhs, typename S::Store* y,
                           typename S::Store* part, typename S::Store* x) {
  using T = typename S::Store;
  const int n = lu.n, P = kBandPanel;
  hipLaunchKernelGGL((k_band_gather<NF, S>), dim3(grid_for(n * NF, 256), m), dim3(256), 0, stream, lu, rhs, y);
  for (int K0 = 0; K0 < n; K0 += P) {   // forward: panels in elimination order
    const int K1 = std::min(K0 + P, n);
    hipLaunchKernelGGL((k_band_panel<NF, S, true>), dim3(K1 - K0, kBandChunks, m), dim3(NF * kWave), 0, stream, lu, (const T*)y, part, K0, K1);
    hipLaunchKernelGGL((k_band_tri<NF, S, true>), dim3(m), dim3(NF * kWave), 0, stream, lu, y, (const T*)part, x, K0, K1);
  }
  for (int K0 = ((n - 1) / P) * P; K0 >= 0; K0 -= P) {   // backward: the same panels in reverse
    const int K1 = std::min(K0 + P, n);
    hipLaunchKernelGGL((k_band_panel<NF, S, false>), dim3(K1 - K0, kBandChunks, m), dim3(NF * kWave), 0, stream, lu, (const T*)y, part, K0, K1);
    hipLaunchKernelGGL((k_band_tri<NF, S, false>), dim3(m), dim3(NF * kWave), 0, stream, lu, y, (const T*)part, x, K0, K1);
  }
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// factorise the assembled Jacobian (c.vals)
template <int NF>
int band_factor(gmpnp_solver* s) {
  int rc = band_prepare<NF>(s); if (rc) return rc;
  HIP_TRY(hipMemsetAsync(s->lu.band, 0, s->lu_band.n * sizeof(double), s->stream));
  hipLaunchKernelGGL((k_band_scatter<NF>), dim3(s->t.nslices), dim3(64), 0, s->stream, s->c, s->lu);
  rc = band_launch_factor<NF>(s->stream, s->lu, 1); if (rc) return rc;
  s->direct_solves++;
  return GMPNP_OK;
}

template <int NF>
int band_substitute(gmpnp_solver* s, const double* rhs, double* x) {
  return band_launch_substitute<NF>(s->stream, s->lu, 1, rhs, s->lu_y.p, s->lu_part.p, x);
}

// One solve with the factorisation the stream holds: rhs in kb, x in kx, checked with the true residual kr = b - J kx and refined by
// band_refine_again (gmpnp_host_rules.h) against `tol` (the pivoting is restricted to the node blocks).  *rn = the last ||b - J x||;
// the verdict on it is the caller's.
template <int NF>
int band_refined_substitute(gmpnp_solver* s, double tol, double* rn) {
  int rc = band_substitute<NF>(s, s->kb.p, s->kx.p); if (rc) return rc;
  rc = true_residual<NF>(s, rn); if (rc) return rc;
  double best = 0.0;
  for (int round = 0; band_refine_again(round, rule_finite(*rn), *rn, best, tol); ++round) {
    best = *rn;
    rc = band_substitute<NF>(s, s->kr.p, s->ks.p); if (rc) return rc;
    hipLaunchKernelGGL(k_axpy, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->kx.p, (const double*)s->ks.p, 1.0, (int)s->ndof);
    rc = true_residual<NF>(s, rn); if (rc) return rc;
  }
  return GMPNP_OK;
}

// Direct solve of J dx = b with b in kb: dx in kx, checked and refined with the true residual.  stats->residual_norm = ||b - J dx||.
// `as_direct` (the Newton loop): an answer that is finite but misses the tolerance is RETURNED, not refused — the reference's
// MUMPS / UMFPACK hand back whatever the factorisation gives (3D:792), and it is Newton's own residual test that judges the step;
// st->converged = 0 says so.  The parity hook gmpnp_linear_solve keeps the strict verdict.
template <int NF>
int band_solve(gmpnp_solver* s, double bnorm, double rtol, double atol, gmpnp_linear_stats_t* st, bool as_direct = false) {
  const double tol = std::max(rtol * bnorm, atol);
  int rc = band_factor<NF>(s); if (rc) return rc;
  double rn = 0.0;
  rc = band_refined_substitute<NF>(s, tol, &rn); if (rc) return rc;
  HIP_TRY(hipMemcpy(s->h_status, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (*s->h_status & 2) return fail(GMPNP_ERR_LINEAR, "block-banded LU: singular pivot block");
  if (st) { st->converged = (rn == rn && rn <= 1e3 * tol) ? 1 : 0; st->residual_norm = rn; st->rhs_norm = bnorm; }
  if (as_direct && rn == rn && !std::isinf(rn)) return GMPNP_OK;
  if (!(rn == rn) || rn > 1e3 * tol) {
    char buf[200];
    snprintf(buf, sizeof buf, "block-banded LU: ||b - J x|| = %.3e after refinement, ||b|| = %.3e", rn, bnorm);
    return fail(GMPNP_ERR_LINEAR, buf);
  }
  return GMPNP_OK;
}

// gmpnp_options_t.phase_timing: device time per phase of a Newton iteration (five event records and one more wait per iteration)
int mark_phase(gmpnp_solver* s, int i) {
  if (s->cfg.phase_timing) HIP_TRY(hipEventRecord(s->ev_phase[i], s->stream));
  return GMPNP_OK;
}
int collect_phases(gmpnp_solver* s, gmpnp_newton_stats_t& st) {   // after the residual that follows the update (phases 0-3 marked)
  if (!s->cfg.phase_timing) return GMPNP_OK;
  float ms01 = 0.f, ms12 = 0.f, ms23 = 0.f, ms3 = 0.f;
  (void)hipEventElapsedTime(&ms01, s->ev_phase[0], s->ev_phase[1]);
  (void)hipEventElapsedTime(&ms12, s->ev_phase[1], s->ev_phase[2]);
  (void)hipEventElapsedTime(&ms23, s->ev_phase[2], s->ev_phase[3]);
  HIP_TRY(hipEventRecord(s->ev_phase[4], s->stream));
  HIP_TRY(hipEventSynchronize(s->ev_phase[4]));
  (void)hipEventElapsedTime(&ms3, s->ev_phase[3], s->ev_phase[4]);
  st.ms_assemble += ms01 + ms3;   // Jacobian assembly + next residual (device time)
  st.ms_setup += ms12;
  st.ms_krylov += ms23;
  return GMPNP_OK;
}

// ---- step limiter (gmpnp_step_limit.h) ------------------------------------------------------------
int step_prepare(gmpnp_solver* s) {
  if (s->limiter) return GMPNP_OK;
  std::unique_ptr<gmpnp_step_limiter> L(new gmpnp_step_limiter);
  L->nblk = std::max(1, grid_for(s->t.nv, kVecBlock));
  HIP_TRY(L->part.alloc((size_t)L->nblk)); HIP_TRY(L->part_node.alloc((size_t)L->nblk)); HIP_TRY(L->dx.alloc((size_t)s->ndof));
  HIP_TRY(hipHostMalloc((void**)&L->h_report, 64, hipHostMallocCoherent | hipHostMallocMapped));
  std::memset(L->h_report, 0, 64);
  { void* dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, L->h_report, 0)); L->d_report = (StepReport*)dp; }
  s->limiter = std::move(L);
  return GMPNP_OK;
}
StepLimitIo step_limit_io(const gmpnp_solver* s, const double* dx) {
  const gmpnp_step_limiter* L = s->limiter.get();
  return StepLimitIo{s->u.p, dx, s->d_model.p, L->part.p, L->part_node.p, s->t.nv};
}
StepUpdateIo step_update_io(const gmpnp_solver* s, const double* dx, double* xp, double omega, double tau, int32_t* status) {
  const gmpnp_step_limiter* L = s->limiter.get();
  return StepUpdateIo{s->u.p, dx, xp, L->part.p, L->part_node.p, L->nblk, s->ndof, omega, tau, L->d_report, status};
}
// the two launches of a limited update: u -= omega alpha dx, xp = dx, the report in pinned memory (read behind the next synchronisation)
template <int NF>
int step_launch(gmpnp_solver* s, const double* dx, double* xp, double omega, double tau, int32_t* status) {
  const gmpnp_step_limiter* L = s->limiter.get();
  hipLaunchKernelGGL((k_step_limit<NF>), dim3(L->nblk), dim3(kVecBlock), 0, s->stream, step_limit_io(s, dx));
  hipLaunchKernelGGL(k_limited_update, dim3(grid_for(s->ndof, kVecBlock)), dim3(kVecBlock), 0, s->stream, step_update_io(s, dx, xp, omega, tau, status));
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// The linear step of one Newton iteration, by solver kind: solves J dx = F (||F|| = r, the Jacobian gathered) and applies
// u <- u - omega dx.  With the step limiter (o.step_fraction != 0) the step ends with dx in kx and newton() applies the update.
template <int DIM, int NF>
int tridiagonal_step(gmpnp_solver* s, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t&, double) {
  int rc = mark_phase(s, 2); if (rc) return rc;
  if constexpr (DIM == 1) {
    rc = tri_solve<NF>(s, s->F.p); if (rc) return rc;
    if (o.step_fraction != 0.0) return tri_apply<NF>(s, s->kx.p, 0.0, 1.0);
    return tri_apply<NF>(s, s->u.p, 1.0, -o.relaxation_parameter);
  } else {
    return fail(GMPNP_ERR_INVALID, "block-tridiagonal solver needs a 1D mesh");
  }
}

template <int DIM, int NF>
int direct_step(gmpnp_solver* s, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st, double r) {
  if constexpr (DIM == 3) {
    HIP_TRY(hipMemcpyAsync(s->kb.p, s->F.p, s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    int rc = mark_phase(s, 2); if (rc) return rc;
    gmpnp_linear_stats_t ls{};
    rc = band_solve<NF>(s, r, o.krylov_relative_tolerance, o.krylov_absolute_tolerance, &ls, true); if (rc) return rc;
    st.direct_solves++; s->x0.left(false);
    if (o.step_fraction != 0.0) return GMPNP_OK;
    hipLaunchKernelGGL(k_axpy, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->u.p, (const double*)s->kx.p,
                       -o.relaxation_parameter, (int)s->ndof);
    return GMPNP_OK;
  } else {
    return fail(GMPNP_ERR_INVALID, "block-banded LU is the 3D direct solver (1D meshes: GMPNP_LINEAR_BLOCK_TRIDIAGONAL)");
  }
}

template <int DIM, int NF>
int krylov_step(gmpnp_solver* s, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st, double r) {
  const int it = st.iterations;
  // x0 = wa dx_k + wb dx_{k-1}, the predicted start of this solve (gmpnp_host_rules.h; gmpnp_options_t.warm_start)
  // (a limited solve starts every linear solve from zero: the prediction assumes a constant step length)
  const bool limited = o.step_fraction != 0.0;
  const int warm_start = limited ? 0 : s->cfg.warm_start;
  const double q = 1.0 - o.relaxation_parameter;
  const auto [wa, wb] = predicted_start(warm_start, q, it);
  const bool x0_ready = s->x0.ready(it, wa);
  // The test of the predicted start (w = J x0 and three dot products, then a host decision) needs the new Jacobian only: it runs
  // on the side stream while the main stream builds the preconditioner, and the host waits for ITS event, so neither the two
  // kernels nor the round trip sit on the critical path.
  const bool dots_in_flight = x0_ready && s->stream2 && s->cfg.warm_async;
  if (dots_in_flight) {
    HIP_TRY(hipEventRecord(s->ev_jac, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->stream2, s->ev_jac, 0));
    hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream2, s->c, (const double*)s->kx.p, s->kt.p);
    hipLaunchKernelGGL(k_dots3, dim3(s->n_resblocks), dim3(kVecBlock), 0, s->stream2, (const double*)s->kt.p, (const double*)s->kb.p,
                       s->c.part_f, (int)s->ndof, s->n_resblocks);
    HIP_TRY(hipEventRecord(s->ev_dots, s->stream2));
  }
  const bool async_ok = s->cfg.coarse_async != 0 && DIM == 3;
  const bool coarse_fresh = s->coarse.fresh(async_ok, s->cfg.coarse_lag, it, s->state_jumped);
  int rc = setup_preconditioner<DIM, NF>(s, o.linear_solver, true, coarse_fresh, async_ok); if (rc) return rc;
  rc = mark_phase(s, 2); if (rc) return rc;
  gmpnp_linear_stats_t ls{};
  s->burst.expect(it);
  // coefficients of the NEXT iteration's predicted start, which this solve's update leaves in kx
  const auto [na, nb] = predicted_start(warm_start, q, it + 1);
  const NewtonUpdate upd{s->u.p, s->kxp.p, o.relaxation_parameter, na, nb};
  KrylovRequest req;
  req.mode = o.linear_solver; req.bnorm = r; req.rtol = o.krylov_relative_tolerance; req.atol = o.krylov_absolute_tolerance;
  // inside Newton only long solves are checked: a short one does not drift, and Newton's own residual test sees whatever is left
  req.maxit = o.krylov_maximum_iterations; req.verify_above = 500; req.warm_scale = wa; req.warm_prev = wb;
  req.rhs_ready = true; req.x0_ready = x0_ready; req.dots_in_flight = dots_in_flight; req.upd = na != 0.0 ? &upd : nullptr;
  rc = krylov_verified<NF>(s, &ls, req);
  if (dots_in_flight) HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_dots, 0));  // whatever path the solve took: kt and vals are free again
  s->burst.record(it, ls.iterations);
  if (rc == GMPNP_OK) s->direct.krylov_converged(it);
  s->coarse.solved(coarse_fresh, ls.iterations);
  if (it < GMPNP_MAX_NEWTON_HISTORY) st.krylov_per_iteration[it] = ls.iterations;
  st.krylov_iterations += ls.iterations;
  if constexpr (DIM == 3) {
    // the band LU takes over for this system (kb still holds b) and, by DirectFallback, for the solves that follow
    if (rc == GMPNP_ERR_LINEAR && s->cfg.direct_fallback) {
      const std::string why = g_err;
      HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
      gmpnp_linear_stats_t ds{};
      rc = band_solve<NF>(s, r, o.krylov_relative_tolerance, o.krylov_absolute_tolerance, &ds, true);
      if (rc) g_err = why + "; direct fallback: " + g_err;
      else { st.direct_solves++; s->coarse.fell_back(); s->direct.fell_back(); }
    }
  }
  if (rc) {
    HIP_TRY(hipMemcpy(s->h_status, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*s->h_status) g_err += " [" + status_message(*s->h_status) + "]";
    return rc;
  }
  // x <- x - omega dx (done by the solve's last kernel in the normal case)
  if (limited) s->x0.left(false);   // dx stays in kx: newton() applies the limited update
  else if (req.upd_done) s->x0.left(true);
  else if (na != 0.0) {
    hipLaunchKernelGGL(k_update_predict, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->u.p, s->kx.p, s->kxp.p,
                       o.relaxation_parameter, na, nb, (int)s->ndof);
    s->x0.left(true);
  } else {
    hipLaunchKernelGGL(k_axpy, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->u.p, (const double*)s->kx.p,
                       -o.relaxation_parameter, (int)s->ndof);
    s->x0.left(false);
  }
  return GMPNP_OK;
}

template <int DIM, int NF>
int newton(gmpnp_solver* s, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t& st) {
  const double t0 = now_ms();
  HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  double r = 0.0; int flags = 0;
  const double ta = now_ms();
  // Every residual evaluation also leaves the element Jacobian records (k_element<.., true>, 43 us instead of 27): the
  // state only changes in the update, so the records of the convergence test ARE those of the next iteration's
  // Jacobian, and the separate element pass per iteration (another 43 us) is gone.  Wasted only on the last test of a solve.
  // ... and where the handle allows it, the gather of those records runs beside the test (gmpnp_solver::vals2).  A gather
  // that no iteration adopts (converged, limit, failed, an error) is awaited by the main stream in stream order when this
  // function returns: whatever follows may write u, the element records or the spare buffer.
  const bool ahead = gather_ahead_ok(s);
  struct Orphan {
    gmpnp_solver* s;
    ~Orphan() { if (s->gather_pending) { (void)hipStreamWaitEvent(s->stream, s->ev_gather, 0); s->gather_pending = false; } }
  } orphan{s};
  int rc = residual<DIM, NF>(s, true, &r, &flags, ahead); if (rc) return rc;
  st.ms_assemble += now_ms() - ta;
  NewtonJudge judge(o, st, s->cfg.strict_steric != 0);
  NewtonJudge::Verdict v = judge.first(r, flags);
  const bool band_lu_asked = o.linear_solver == GMPNP_LINEAR_BAND_LU;
  const bool limited = o.step_fraction != 0.0;
  if (limited) { rc = step_prepare(s); if (rc) return rc; }
  while (v == NewtonJudge::go_on) {
    if (s->gather_pending && s->cfg.phase_timing) HIP_TRY(hipEventRecord(s->ev_phase[0], s->stream));
    else { rc = mark_phase(s, 0); if (rc) return rc; }
    if (s->gather_pending) {
      // started behind k_element: adopt its buffer and its stream.  The stream left behind is idle (residual() synchronised it),
      // and what the other one holds in front of the gather, the coarse chain of the previous iteration, is awaited through
      // ev_chain as before.  (Phase 0 was stamped there: assembly time counts from the verdict to the end of the gather.)
      std::swap(s->c.vals, s->vals_spare);
      std::swap(s->stream, s->stream2);
      s->gather_pending = false;
    } else {
      rc = launch_jac_gather<DIM, NF>(s); if (rc) return rc;   // element records: left by the last residual evaluation
    }
    s->jacobian_valid = true;
    rc = mark_phase(s, 1); if (rc) return rc;
    if (o.linear_solver == GMPNP_LINEAR_BLOCK_TRIDIAGONAL) rc = tridiagonal_step<DIM, NF>(s, o, st, r);
    else if (band_lu_asked || s->direct.use_direct()) rc = direct_step<DIM, NF>(s, o, st, r);
    else rc = krylov_step<DIM, NF>(s, o, st, r);
    if (rc) return rc;
    if (limited) { rc = step_launch<NF>(s, s->kx.p, s->kxp.p, o.relaxation_parameter, o.step_fraction, s->status.p); if (rc) return rc; }
    rc = mark_phase(s, 3); if (rc) return rc;
    st.iterations++;
    // (no gather beside a test that is expected to end the solve: last_test_expected, gmpnp_host_rules.h)
    const int nr = st.n_residuals;
    const bool last = nr >= 2 && nr < GMPNP_MAX_NEWTON_HISTORY &&
                      last_test_expected(st.residuals[nr - 2], st.residuals[nr - 1], judge.r0, o.relative_tolerance, o.absolute_tolerance,
                                         st.iterations, o.maximum_iterations);
    rc = residual<DIM, NF>(s, true, &r, &flags, ahead && !last); if (rc) return rc;  // synchronises the stream
    if (limited) record_step(st, st.iterations - 1, s->limiter->h_report->alpha);   // written by the update, in front of that synchronisation
    rc = collect_phases(s, st); if (rc) return rc;
    v = judge.next(r, flags);
  }
  if (v == NewtonJudge::failed) return fail(judge.code, judge.message);
  s->state_jumped = false;
  s->direct.newton_done(band_lu_asked);
  st.ms_total = now_ms() - t0;
  return v == NewtonJudge::converged ? GMPNP_OK : fail(judge.code, judge.message);
}

int upload_vec(gmpnp_solver* s, const double* file_order, double* dev) {
  const int nf = s->nf, nv = s->t.nv;
  HIP_TRY(hipStreamSynchronize(s->stream));   // the staging buffer is free again
  for (int i = 0; i < nv; ++i) std::memcpy(&s->h_stage[(size_t)i * nf], &file_order[(size_t)s->t.perm[i] * nf], nf * sizeof(double));
  HIP_TRY(hipMemcpyAsync(dev, s->h_stage, (size_t)s->ndof * sizeof(double), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

int download_vec(gmpnp_solver* s, const double* dev, double* file_order) {
  const int nf = s->nf, nv = s->t.nv;
  HIP_TRY(hipMemcpyAsync(s->h_stage, dev, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (int i = 0; i < nv; ++i) std::memcpy(&file_order[(size_t)s->t.perm[i] * nf], &s->h_stage[(size_t)i * nf], nf * sizeof(double));
  return GMPNP_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

#ifndef GMPNP_BUILD_ID
#define GMPNP_BUILD_ID "unstamped"
#endif
const char* gmpnp_version(void) { return "gmpnp-mi355x 0.2 (gfx950)"; }
const char* gmpnp_build_id(void) { return GMPNP_BUILD_ID; }
const char* gmpnp_last_error(void) { return g_err.c_str(); }

static int create_impl(const gmpnp_mesh_t* mesh, const gmpnp_model_t* model, const gmpnp_quadrature_t* quad,
                       const gmpnp_options_t* opts, const gmpnp_partition_t* part, gmpnp_solver** out);

int gmpnp_create(const gmpnp_mesh_t* mesh, const gmpnp_model_t* model, const gmpnp_quadrature_t* quad,
                 const gmpnp_options_t* opts, gmpnp_solver** out) {
  return create_impl(mesh, model, quad, opts, nullptr, out);
}

int gmpnp_create_partition(const gmpnp_mesh_t* mesh, const gmpnp_model_t* model, const gmpnp_quadrature_t* quad,
                           const gmpnp_options_t* opts, const gmpnp_partition_t* part, gmpnp_solver** out) {
  if (!part) return fail(GMPNP_ERR_INVALID, "partition is NULL");
  if (part->size < 1 || part->rank < 0 || part->rank >= part->size || part->n_neighbours < 0) return fail(GMPNP_ERR_INVALID, "bad partition rank / size");
  if (part->n_neighbours > 0 && (!part->neighbour_rank || !part->send_ptr || !part->recv_ptr || !part->send_vertices || !part->recv_vertices))
    return fail(GMPNP_ERR_INVALID, "partition: halo plan missing");
  return create_impl(mesh, model, quad, opts, part, out);
}

static int create_impl(const gmpnp_mesh_t* mesh, const gmpnp_model_t* model, const gmpnp_quadrature_t* quad,
                       const gmpnp_options_t* opts, const gmpnp_partition_t* part, gmpnp_solver** out) {
  if (!mesh || !quad || !out) return fail(GMPNP_ERR_INVALID, "NULL argument");
  *out = nullptr;
  int rc = check_model(model, mesh->dim); if (rc) return rc;
  const int nf = model->n_species + 1;
  if (!((mesh->dim == 3 && nf == 9) || (mesh->dim == 1 && nf == 7)))
    return fail(GMPNP_ERR_INVALID, "supported spaces: 3D with 8 species + potential, 1D with 6 species + potential");
  if (quad->nq_f < 1 || quad->nq_f > GMPNP_MAX_QUAD || quad->nq_j < 1 || quad->nq_j > GMPNP_MAX_QUAD)
    return fail(GMPNP_ERR_INVALID, "quadrature size out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(GMPNP_ERR_HIP, "no HIP device visible: libgmpnp.so has no CPU fallback");
  std::unique_ptr<gmpnp_solver> s(new gmpnp_solver);
  if (opts) s->opts = *opts;
  if (s->opts.device_id < 0 || s->opts.device_id >= ndev) return fail(GMPNP_ERR_INVALID, "device_id out of range");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  // a partitioned handle keeps to one stream (no side stream) and the group drives its launches; whether the coarse workgroups
  // may ride inside the tile launches (peer transport, gmpnp_group.h) is still the caller's choice + the residency proof below
  const bool part_fused_ok = part && !s->opts.shared_device && s->opts.launch_form != 4;
  if (part) {
    if (mesh->dim != 3) return fail(GMPNP_ERR_INVALID, "mesh partitions exist for 3D meshes");
    s->opts.shared_device = 1; s->opts.launch_form = 4;
  }
  std::string err = resolve_options(s->opts, mesh->dim, &s->cfg);
  if (!err.empty()) return fail(GMPNP_ERR_INVALID, err);
  err = build_topology(*mesh, nf, s->opts.n_aggregates, s->t, part);
  if (!err.empty()) return fail(GMPNP_ERR_INVALID, err);
  Topology& t = s->t;
  s->dim = mesh->dim; s->nf = nf; s->nn = mesh->dim + 1; s->ndof = t.nv * nf; s->nb = (int)t.cols.size();
  s->ncoarse = t.nagg * nf;
  s->model = *model; s->quad = *quad;
  auto conv_facets = [&](int n, const int32_t* f, std::vector<int32_t>& dst, const char* what) -> int {
    if (n < 0 || (n > 0 && !f)) return fail(GMPNP_ERR_INVALID, std::string("bad ") + what);
    dst.resize((size_t)n * 3);
    for (size_t k = 0; k < dst.size(); ++k) {
      if (f[k] < 0 || f[k] >= t.nv) return fail(GMPNP_ERR_INVALID, std::string(what) + " references a vertex outside the mesh");
      dst[k] = t.iperm[f[k]];
    }
    return GMPNP_OK;
  };
  if (mesh->dim == 3) {
    rc = conv_facets(mesh->n_wall_facets, mesh->wall_facets, s->wall_f, "wall_facets"); if (rc) return rc;
    rc = conv_facets(mesh->n_exit_facets, mesh->exit_facets, s->exit_f, "exit_facets"); if (rc) return rc;
  }
  for (int k = 0; k < mesh->n_point_vertices; ++k) {
    const int v = mesh->point_vertices[k];
    if (v < 0 || v >= t.nv) return fail(GMPNP_ERR_INVALID, "point_vertices references a vertex outside the mesh");
    s->point_v.push_back(t.iperm[v]);
  }
  HIP_TRY(hipStreamCreate(&s->stream));
  for (auto& e : s->ev_phase) HIP_TRY(hipEventCreate(&e));

  const int nv = t.nv, nc = t.nc, nn = s->nn, ndof = s->ndof;
  const int ej_stride = (mesh->dim == 3) ? Lay<3, 9>::EJ_STRIDE : Lay<1, 7>::EJ_STRIDE;
  s->n_resblocks = grid_for(ndof, kVecBlock);
  std::vector<gmpnp_model_t> mv(1, s->model); std::vector<gmpnp_quadrature_t> qv(1, s->quad);
  HIP_TRY(s->d_model.upload(mv)); HIP_TRY(s->d_quad.upload(qv));
  HIP_TRY(s->coords.upload(t.coords)); HIP_TRY(s->cells.upload(t.cells));
  HIP_TRY(s->u.alloc(ndof)); HIP_TRY(s->un.alloc(ndof)); HIP_TRY(s->F.alloc(ndof));
  s->h_bcflag.assign(ndof, 0); s->h_bcflag_dev.assign(ndof, 0);
  HIP_TRY(hipHostMalloc((void**)&s->h_bcval, (size_t)ndof * sizeof(double)));
  HIP_TRY(hipHostMalloc((void**)&s->h_stage, (size_t)ndof * sizeof(double)));
  std::memset(s->h_bcval, 0, (size_t)ndof * sizeof(double));
  HIP_TRY(s->bcflag.upload(s->h_bcflag)); HIP_TRY(s->bcval.alloc(ndof));
  HIP_TRY(s->EF.alloc((size_t)nc * nn * nf)); HIP_TRY(s->EJ.alloc((size_t)nc * ej_stride));
  HIP_TRY(s->n2e_ptr.upload(t.n2e_ptr)); HIP_TRY(s->n2e.upload(t.n2e));
  HIP_TRY(s->rowptr.upload(t.rowptr)); HIP_TRY(s->cols.upload(t.cols));
  HIP_TRY(s->cptr.upload(t.cptr)); HIP_TRY(s->contrib.upload(t.contrib));
  // vals_s keeps its columns in pairs (value_pair_offset): a pair is 16-byte aligned because every slice starts at an even value
  for (int q = 0; q <= t.nslices; ++q) if (t.slice_off[q] & 1) return fail(GMPNP_ERR_INVALID, "internal: a slice of the value arrays starts at an odd offset");
  { const size_t pad = (size_t)kRowPad * nf * kWave;  // the Krylov kernels preload unconditionally past short slices
    HIP_TRY(s->vals.alloc((size_t)t.slice_off[t.nslices], true, pad)); HIP_TRY(s->vals_s.alloc((size_t)t.slice_off[t.nslices], true, pad)); }
  HIP_TRY(s->slice_off.upload(t.slice_off)); HIP_TRY(s->slice_colbase.upload(t.slice_colbase));
  HIP_TRY(s->slice_node0.upload(t.slice_node0)); HIP_TRY(s->slice_nn.upload(t.slice_nn)); HIP_TRY(s->node_slice.upload(t.node_slice));
  HIP_TRY(s->sell_cols.upload(t.sell_cols)); HIP_TRY(s->sell_aggslot.upload(t.sell_aggslot));
  HIP_TRY(s->wl_slice.upload(t.wl_slice)); HIP_TRY(s->wl_kpos.upload(t.wl_kpos));
  HIP_TRY(s->sell_blk.upload(t.sell_blk));
  HIP_TRY(s->tile_slice0.upload(t.tile_slice0)); HIP_TRY(s->tile_agg.upload(t.tile_agg)); HIP_TRY(s->tile_slot.upload(t.tile_slot));
  HIP_TRY(s->tile_aggs.upload(t.tile_aggs)); HIP_TRY(s->tile_nagg.upload(t.tile_nagg));
  HIP_TRY(s->tile_rec.upload(t.tile_rec)); HIP_TRY(s->tile_cols.upload(t.tile_cols));
  HIP_TRY(s->tile_colslot.upload(t.tile_colslot)); HIP_TRY(s->sell_lcol.upload(t.sell_lcol));
  HIP_TRY(s->Dinv.alloc((size_t)nv * nf * nf));
  HIP_TRY(s->agg.upload(t.agg)); HIP_TRY(s->agg_start.upload(t.agg_start)); HIP_TRY(s->row_aggs.upload(t.row_aggs));
  HIP_TRY(s->AP.alloc((size_t)ndof * kMaxRowAggs * nf));
  // a few dozen nodes per chunk: 32 chunks per aggregate on the reference meshes, up to 1024 on refined ones (one workgroup each;
  // with the fixed 32 a twice-refined mesh spent 1.9 ms here, 770 nodes in a serial loop per thread)
  s->c.coarse_chunks = std::min(1024, std::max(kCoarseChunks, nv / std::max(1, s->t.nagg) / 24));
  HIP_TRY(s->AcPart.alloc((size_t)s->c.coarse_chunks * s->ncoarse * s->ncoarse));
  HIP_TRY(s->Ac.alloc((size_t)s->ncoarse * s->ncoarse)); HIP_TRY(s->Aci.alloc((size_t)s->ncoarse * s->ncoarse));
  HIP_TRY(s->Aci2.alloc((size_t)s->ncoarse * s->ncoarse));
  const gmpnp_options_t& po = s->opts;
  s->chain_level = GMPNP_NEWTON_CHAIN_DEFAULT;
  if (const char* env = std::getenv("GMPNP_NEWTON_CHAIN")) s->chain_level = std::atoi(env);
  if (s->cfg.coarse_async || s->cfg.warm_async) {   // the side stream exists only when something uses it
    // The second value buffer of the gather beside Newton's test: unpartitioned 3D handles with the side stream, where it is cheap
    // (matrix up to kGatherAheadCapBytes).  GMPNP_NEWTON_CHAIN=0 in the environment keeps the serial chain (A/B runs, tests).
    // The two streams of such a handle change roles (newton()), so the side stream is created like the main one.
    const size_t vbytes = ((size_t)t.slice_off[t.nslices] + (size_t)kRowPad * nf * kWave) * sizeof(double);
    const bool chain = s->chain_level >= 1 && !part && mesh->dim == 3 && vbytes <= kGatherAheadCapBytes;
    if (chain) HIP_TRY(hipStreamCreate(&s->stream2));
    else HIP_TRY(hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&s->ev_mat, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&s->ev_chain, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&s->ev_jac, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&s->ev_dots, hipEventDisableTiming));
    if (chain) {
      HIP_TRY(s->vals2.alloc((size_t)t.slice_off[t.nslices], true, (size_t)kRowPad * nf * kWave));   // zero padding as in vals
      s->vals_spare = s->vals2.p;
      HIP_TRY(hipEventCreateWithFlags(&s->ev_elem, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&s->ev_gather, hipEventDisableTiming));
    }
  }
  for (DevBuf<double>* b : {&s->kr, &s->krhat, &s->kp0, &s->kp1, &s->kv0, &s->kv1, &s->ks, &s->kt, &s->ky, &s->kx, &s->kxp, &s->kb}) HIP_TRY(b->alloc(ndof));
  HIP_TRY(s->yc.alloc((size_t)kMaxCoarse * 32));  // [nagg <= 16][ncoarse] column-block products (+ development stamps)
  for (DevBuf<double>* b : {&s->cpart_v0, &s->cpart_v1, &s->cpart_t, &s->cpart_r0, &s->cpart_r1, &s->cpart_p0, &s->cpart_p1})
    HIP_TRY(b->alloc((size_t)s->ncoarse * t.tile_slots));
  HIP_TRY(s->krand.alloc(ndof));
  HIP_TRY(s->ticket.alloc(16 * 66));  // counter + 64 replicated flags, one cache line each
  HIP_TRY(s->part_a.alloc((size_t)2 * t.ntiles));  // (rhat,v) partials, then ||r||^2 partials
  HIP_TRY(s->part_b.alloc((size_t)4 * t.ntiles));
  HIP_TRY(s->part_f.alloc((size_t)3 * s->n_resblocks));
  HIP_TRY(s->scal.alloc(1)); HIP_TRY(s->status.alloc(1));
  HIP_TRY(hipHostMalloc((void**)&s->h_scal, 3 * sizeof(KrylovScalars)));
  HIP_TRY(hipHostMalloc((void**)&s->h_poll, 64, hipHostMallocCoherent | hipHostMallocMapped));
  std::memset(s->h_poll, 0, 64);
  { void* dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, s->h_poll, 0)); s->c.poll = (HostPoll*)dp; }
  for (auto& e : s->ev_poll) HIP_TRY(hipEventCreate(&e));
  {  // Two launches per iteration (coarse workgroups inside the tile launch, tile workgroups wait for their flags) only
     // where the runtime's occupancy figure proves the whole launch resident at once: a waiting workgroup must never
     // keep the workgroup it waits for off the machine.  Not on a device the caller shares with other work.
    hipDeviceProp_t prop{};
    HIP_TRY(hipGetDeviceProperties(&prop, s->opts.device_id));
    int occ_a = 0, occ_b = 0;
    if (mesh->dim == 3) {
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_a, k_half_a<9>, kKrylovThreads, 0));
      HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_b, k_half_b<9>, kKrylovThreads, 0));
    }
    s->resident_slots = std::min(occ_a, occ_b) * prop.multiProcessorCount;
    const bool resident = mesh->dim == 3 && (s->t.ntiles + s->t.nagg) <= s->resident_slots;
    if (po.launch_form == 2 && (!resident || po.shared_device)) {
      char buf[200];
      snprintf(buf, sizeof buf, "launch_form 2 refused: %d workgroups per launch, %d resident at once (%d per CU x %d CUs)%s",
               s->t.ntiles + s->t.nagg, s->resident_slots, std::min(occ_a, occ_b), prop.multiProcessorCount,
               po.shared_device ? ", device declared shared" : "");
      return fail(GMPNP_ERR_INVALID, buf);
    }
    s->fused_half = po.launch_form == 4 ? false : (resident && !po.shared_device && !s->prereduce);
    if (part) s->fused_half = resident && part_fused_ok;
    // Vector form.  On-the-fly (the tile kernels recompute p / s at their column nodes from four / two vectors: one launch
    // per half-iteration) wins while the operands are cache resident; materialised (k_vec_a / k_vec_b write p / s for all
    // rows first, the tile kernels stage one vector) wins once the gathers cost memory bandwidth: matrix above 768 MB.
    const double matrix_mb = (double)s->nb * nf * nf * sizeof(double) / 1e6;
    s->matp = !part && mesh->dim == 3 && (po.vector_form == 1 || (po.vector_form == 0 && matrix_mb > 768.0));
    if (s->matp) {
      if (po.launch_form == 2) return fail(GMPNP_ERR_INVALID, "vector_form 1 (materialised) has its own launches: not with launch_form 2");
      s->fused_half = false;
    }
  }
  HIP_TRY(hipHostMalloc((void**)&s->h_part, 3 * std::max(s->n_resblocks, 1) * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped));
  HIP_TRY(hipHostMalloc((void**)&s->h_status, 64, hipHostMallocCoherent | hipHostMallocMapped));
  *s->h_status = 0;

  Ctx& c = s->c;
  c.nv = nv; c.nc = nc; c.ndof = ndof; c.nb = s->nb; c.nslices = t.nslices; c.ntiles = t.ntiles; c.n_work = (int)t.wl_slice.size();
  c.nagg = t.nagg; c.ncoarse = s->ncoarse; c.tile_slots = t.tile_slots; c.n_robin = 0; c.use_coarse = 1;
  c.model = s->d_model.p; c.quad = s->d_quad.p; c.coords = s->coords.p; c.cells = s->cells.p;
  c.u = s->u.p; c.un = s->un.p; c.F = s->F.p; c.bcflag = s->bcflag.p; c.bcval = s->bcval.p;
  c.EF = s->EF.p; c.EJ = s->EJ.p; c.n2e_ptr = s->n2e_ptr.p; c.n2e = s->n2e.p;
  c.rowptr = s->rowptr.p; c.cols = s->cols.p; c.cptr = s->cptr.p; c.contrib = s->contrib.p;
  c.vals = s->vals.p; c.vals_s = s->vals_s.p; c.slice_off = s->slice_off.p; c.slice_colbase = s->slice_colbase.p;
  c.slice_node0 = s->slice_node0.p; c.slice_nn = s->slice_nn.p; c.node_slice = s->node_slice.p;
  c.sell_cols = s->sell_cols.p; c.sell_aggslot = s->sell_aggslot.p; c.wl_slice = s->wl_slice.p; c.wl_kpos = s->wl_kpos.p;
  c.sell_blk = s->sell_blk.p; c.tile_slice0 = s->tile_slice0.p; c.tile_agg = s->tile_agg.p; c.tile_slot = s->tile_slot.p;
  c.tile_aggs = s->tile_aggs.p; c.tile_nagg = s->tile_nagg.p;
  c.tile_rec = s->tile_rec.p; c.col_stride = t.col_stride; c.tile_cols = s->tile_cols.p; c.tile_colslot = s->tile_colslot.p; c.sell_lcol = s->sell_lcol.p;
  c.Dinv = s->Dinv.p; c.agg = s->agg.p; c.agg_start = s->agg_start.p; c.row_aggs = s->row_aggs.p;
  c.AP = s->AP.p; c.AcPart = s->AcPart.p; c.Ac = s->Ac.p; c.Aci = s->Aci.p;
  s->aci_buf[0] = s->Aci.p; s->aci_buf[1] = s->Aci2.p; s->aci_cur = 0;
  c.kr = s->kr.p; c.krhat = s->krhat.p; c.kp[0] = s->kp0.p; c.kp[1] = s->kp1.p; c.kv[0] = s->kv0.p; c.kv[1] = s->kv1.p;
  c.ks = s->ks.p; c.kt = s->kt.p; c.ky = s->ky.p; c.kx = s->kx.p; c.kb = s->kb.p; c.yc = s->yc.p;
  c.cpart_r[0] = s->cpart_r0.p; c.cpart_r[1] = s->cpart_r1.p; c.cpart_p[0] = s->cpart_p0.p; c.cpart_p[1] = s->cpart_p1.p;
  c.cpart_v[0] = s->cpart_v0.p; c.cpart_v[1] = s->cpart_v1.p; c.cpart_t = s->cpart_t.p;
  c.ticket = s->ticket.p; c.part_a = s->part_a.p; c.part_rr = s->part_a.p + t.ntiles; c.part_b = s->part_b.p;
  { void* dp = nullptr; HIP_TRY(hipHostGetDevicePointer(&dp, s->h_part, 0)); c.part_f = (double*)dp;
    HIP_TRY(hipHostGetDevicePointer(&dp, s->h_status, 0)); c.status_host = (int32_t*)dp; }
  c.scal = s->scal.p; c.status = s->status.p;
  c.own_node0 = t.own_node0; c.own_node1 = t.own_node1; c.own_agg0 = t.own_agg0; c.own_agg1 = t.own_agg1; c.tile0 = t.own_tile0; c.dist = 0;
  c.wl_run_blocks = t.wl_run_blocks;
  // Pre-reduced sums for the coarse kernels (red_i / red_a / red_b).  Large meshes: an aggregate has thousands of tile slots,
  // and summing them inside every coarse workgroup (and inside every workgroup of k_minv_apply) costs more than one
  // k_dist_reduce launch per half-iteration (refine 2, before: k_coarse_a 92 us, k_minv_apply 5.5 ms per call).  Partitioned handles
  // use the same buffers for their all-reduced sums.
  HIP_TRY(s->red_i.alloc(s->ncoarse)); HIP_TRY(s->red_a.alloc(2 + 3 * (size_t)s->ncoarse)); HIP_TRY(s->red_b.alloc(4 + (size_t)s->ncoarse));
  c.red_i = s->red_i.p; c.red_a = s->red_a.p; c.red_b = s->red_b.p;
  s->staged_element = mesh->dim == 3 && s->opts.element_stores != 1;   // measured faster at every size: 36.6 vs 40.5 us on L_50_R_5, 1.18 vs 2.00 ms at two refinements
  s->prereduce = !part && mesh->dim == 3 && t.tile_slots > 128;
  if (s->prereduce) c.dist = 1;
  if (part) {
    s->partitioned = true; s->part_rank = part->rank; s->part_size = part->size;
    std::vector<int32_t> sn, rn;
    s->send_ptr.assign(1, 0); s->recv_ptr.assign(1, 0);
    for (int q = 0; q < part->n_neighbours; ++q) {
      if (part->neighbour_rank[q] < 0 || part->neighbour_rank[q] >= part->size || part->neighbour_rank[q] == part->rank)
        return fail(GMPNP_ERR_INVALID, "partition: bad neighbour rank");
      s->nb_rank.push_back(part->neighbour_rank[q]);
      for (int k = part->send_ptr[q]; k < part->send_ptr[q + 1]; ++k) {
        const int v = part->send_vertices[k];
        if (v < 0 || v >= nv || !part->vertex_owned[v]) return fail(GMPNP_ERR_INVALID, "partition: send list must name owned local vertices");
        sn.push_back(t.iperm[v]);
      }
      for (int k = part->recv_ptr[q]; k < part->recv_ptr[q + 1]; ++k) {
        const int v = part->recv_vertices[k];
        if (v < 0 || v >= nv || part->vertex_owned[v]) return fail(GMPNP_ERR_INVALID, "partition: receive list must name ghost vertices");
        rn.push_back(t.iperm[v]);
      }
      s->send_ptr.push_back((int32_t)sn.size()); s->recv_ptr.push_back((int32_t)rn.size());
    }
    HIP_TRY(s->send_nodes.upload(sn)); HIP_TRY(s->recv_nodes.upload(rn));
    {  // the tiles' column lists with every ghost node replaced by -(its index in the receive list + 1): exchange-prologue launches
      std::vector<int32_t> slot_of(nv, -1), tcx = t.tile_cols;
      for (size_t k = 0; k < rn.size(); ++k) slot_of[rn[k]] = (int32_t)k;
      for (auto& node : tcx) if (node >= 0 && node < nv && slot_of[node] >= 0) node = -(slot_of[node] + 1);
      HIP_TRY(s->tile_cols_x.upload(tcx));
    }
    const size_t wmax = (size_t)nf * nf;   // widest exchange: the inverse diagonal blocks of the ghost nodes
    HIP_TRY(s->sendbuf.alloc(std::max<size_t>(1, sn.size() * wmax))); HIP_TRY(s->recvbuf.alloc(std::max<size_t>(1, rn.size() * wmax)));
    HIP_TRY(s->red_norm.alloc(8));
    HIP_TRY(hipHostMalloc((void**)&s->h_red, 8 * sizeof(double)));
    c.dist = 1;
  }
  rc = rebuild_boundary(s.get()); if (rc) return rc;
  rc = build_tridiagonal(s.get()); if (rc) return rc;
  // the coarse inverse keeps its whole matrix in LDS: opt in to > 64 KiB of dynamic LDS
  if (nf == 9) HIP_TRY(hipFuncSetAttribute((const void*)k_coarse_invert<9>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)coarse_lds_bytes(s->ncoarse, 9)));
  else HIP_TRY(hipFuncSetAttribute((const void*)k_coarse_invert<7>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)coarse_lds_bytes(s->ncoarse, 7)));
  HIP_TRY(hipDeviceSynchronize());
  *out = s.release();
  return GMPNP_OK;
}

void gmpnp_destroy(gmpnp_solver* s) {
  if (!s) return;
  (void)hipSetDevice(s->opts.device_id);
  (void)hipDeviceSynchronize();
  delete s;
}

int gmpnp_set_model(gmpnp_solver* s, const gmpnp_model_t* model) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  int rc = check_model(model, s->dim); if (rc) return rc;
  if (model->n_species + 1 != s->nf) return fail(GMPNP_ERR_INVALID, "n_species cannot change after create");
  tangent_drop(s);
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->model = *model;
  HIP_TRY(hipMemcpy(s->d_model.p, &s->model, sizeof(gmpnp_model_t), hipMemcpyHostToDevice));
  s->jacobian_valid = false; s->precond_valid = false;
  return rebuild_boundary(s);
}

int gmpnp_set_supg(gmpnp_solver* s, const double* rho, const int32_t* w_index) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  tangent_drop(s);
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->jacobian_valid = false;
  if (!rho) { s->c.supg_rho = nullptr; return GMPNP_OK; }
  if (kinetics_on(s)) return fail(GMPNP_ERR_INVALID, "SUPG terms: not with the surface kinetics on (gmpnp_set_kinetics)");
  if (s->dim != 1) return fail(GMPNP_ERR_INVALID, "SUPG stabilisation exists for 1D meshes only (reference 1D:597-722)");
  const int ns = s->nf - 1, nv = s->t.nv;
  std::vector<double> tmp((size_t)nv * ns);
  for (int I = 0; I < nv; ++I)
    for (int j = 0; j < ns; ++j) {
      const double v = rho[(size_t)s->t.perm[I] * ns + j];
      if (!(v == v) || v < 0.0) return fail(GMPNP_ERR_INVALID, "SUPG parameters must be finite and non-negative");
      tmp[(size_t)I * ns + j] = v;
    }
  HIP_TRY(s->supg_rho.upload(tmp));
  s->c.supg_rho = s->supg_rho.p;
  for (int j = 0; j < GMPNP_MAX_SPECIES; ++j) {
    const int w = (w_index && j < ns) ? w_index[j] : j;
    if (j < ns && (w < 0 || w >= ns)) return fail(GMPNP_ERR_INVALID, "SUPG gradient index out of range");
    s->c.supg_w[j] = w;
  }
  return GMPNP_OK;
}

int gmpnp_set_dirichlet(gmpnp_solver* s, int64_t n, const int64_t* dofs, const double* values) {
  if (!s || n < 0 || (n > 0 && (!dofs || !values))) return fail(GMPNP_ERR_INVALID, "bad arguments");
  tangent_drop(s);
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));   // the pinned value buffer may still be in flight
  std::fill(s->h_bcflag.begin(), s->h_bcflag.end(), 0);
  std::memset(s->h_bcval, 0, (size_t)s->ndof * sizeof(double));
  for (int64_t k = 0; k < n; ++k) {
    const int64_t d = dofs[k];
    if (d < 0 || d >= s->ndof) return fail(GMPNP_ERR_INVALID, "Dirichlet dof out of range");
    const int r = s->t.iperm[d / s->nf] * s->nf + (int)(d % s->nf);
    s->h_bcflag[r] = 1; s->h_bcval[r] = values[k];
  }
  if (s->h_bcflag != s->h_bcflag_dev) {  // the dof SET rarely changes (3D: only the CO2 value moves between time steps)
    HIP_TRY(hipMemcpy(s->bcflag.p, s->h_bcflag.data(), s->ndof, hipMemcpyHostToDevice));
    s->h_bcflag_dev = s->h_bcflag;
  }
  HIP_TRY(hipMemcpyAsync(s->bcval.p, s->h_bcval, s->ndof * sizeof(double), hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->jacobian_valid = false;
  return GMPNP_OK;
}

int gmpnp_set_state(gmpnp_solver* s, const double* u, const double* u_n) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  tangent_drop(s);
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (u) { int rc = upload_vec(s, u, s->u.p); if (rc) return rc; s->state_jumped = true; }
  if (u_n) { int rc = upload_vec(s, u_n, s->un.p); if (rc) return rc; }
  s->jacobian_valid = false;
  if (u_n && s->stepper) { s->stepper->dropped(); time_read_un(s); }   // adaptive time stepping: u_nm1 no longer precedes u_n
  return GMPNP_OK;
}

int gmpnp_get_state(gmpnp_solver* s, double* u_out, double* u_n_out) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  if (u_out) { int rc = download_vec(s, s->u.p, u_out); if (rc) return rc; }
  if (u_n_out) { int rc = download_vec(s, s->un.p, u_n_out); if (rc) return rc; }
  return GMPNP_OK;
}

int gmpnp_assign_previous(gmpnp_solver* s) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  // stream-ordered: whatever reads u_n next is launched behind this copy, and every read-back synchronises the stream
  HIP_TRY(hipMemcpyAsync(s->un.p, s->u.p, s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
  if (s->stepper) { s->stepper->dropped(); time_read_un(s); }   // adaptive time stepping: u_nm1 was not shifted (gmpnp_time_accept does both)
  if (galvanostat_on(s)) return galvanostat_shift(s, true);
  return GMPNP_OK;
}

int gmpnp_newton_solve(gmpnp_solver* s, const gmpnp_newton_options_t* o, gmpnp_newton_stats_t* stats) {
  if (!s || !o) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (o->maximum_iterations < 0 || o->krylov_maximum_iterations < 1) return fail(GMPNP_ERR_INVALID, "bad iteration limits");
  if (o->linear_solver < 0 || o->linear_solver > GMPNP_LINEAR_BAND_LU) return fail(GMPNP_ERR_INVALID, "unknown linear_solver");
  if (o->linear_solver == GMPNP_LINEAR_BLOCK_TRIDIAGONAL && !s->tri_ok)
    return fail(GMPNP_ERR_INVALID, "block-tridiagonal solver needs a 1D mesh in path order");
  if (!step_fraction_valid(o->step_fraction)) return fail(GMPNP_ERR_INVALID, "step_fraction must be 0 (off) or lie in (0, 1)");
  tangent_drop(s);
  gmpnp_newton_stats_t local{};
  gmpnp_newton_stats_t& st = stats ? *stats : local;
  st = fresh_newton_stats();
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc;
  if (galvanostat_on(s)) {
    if (o->linear_solver == GMPNP_LINEAR_BICGSTAB_TWOLEVEL || o->linear_solver == GMPNP_LINEAR_BICGSTAB_JACOBI)
      return fail(GMPNP_ERR_INVALID, "galvanostat: the BiCGStab solvers are not available with the option on (1D: GMPNP_LINEAR_BLOCK_TRIDIAGONAL, 3D: GMPNP_LINEAR_BAND_LU)");
    if ((s->dim == 1) != (o->linear_solver == GMPNP_LINEAR_BLOCK_TRIDIAGONAL))
      return fail(GMPNP_ERR_INVALID, "galvanostat: 1D handles take GMPNP_LINEAR_BLOCK_TRIDIAGONAL, 3D handles GMPNP_LINEAR_BAND_LU");
    GMPNP_DISPATCH(s, rc = (newton_galvanostat<DIM, NF>(s, *o, st)));
    return rc;
  }
  GMPNP_DISPATCH(s, rc = (newton<DIM, NF>(s, *o, st)));
  return rc;
}

int gmpnp_step_limit(gmpnp_solver* s, const double* dx, double tau, double* alpha, double* lambda, int64_t* node) {
  if (!s || !dx) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (!(tau > 0.0 && tau < 1.0)) return fail(GMPNP_ERR_INVALID, "step_fraction must lie in (0, 1)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = step_prepare(s); if (rc) return rc;
  gmpnp_step_limiter* L = s->limiter.get();
  rc = upload_vec(s, dx, L->dx.p); if (rc) return rc;
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_step_limit<NF>), dim3(L->nblk), dim3(kVecBlock), 0, s->stream, step_limit_io(s, L->dx.p)));
  hipLaunchKernelGGL(k_step_report, dim3(1), dim3(kVecBlock), 0, s->stream, step_update_io(s, L->dx.p, nullptr, 1.0, tau, nullptr));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  const StepReport r = *L->h_report;
  if (r.bad) return fail(GMPNP_ERR_NUMERIC, status_message(16));
  if (alpha) *alpha = r.alpha;
  if (lambda) *lambda = r.lambda;
  if (node) *node = r.node >= 0 ? (int64_t)s->t.perm[r.node] : -1;
  return GMPNP_OK;
}

int32_t gmpnp_n_fields(const gmpnp_solver* s) { return s ? s->nf : 0; }
int64_t gmpnp_n_dofs(const gmpnp_solver* s) { return s ? s->ndof : 0; }
int64_t gmpnp_n_blocks(const gmpnp_solver* s) { return s ? s->nb : 0; }
int64_t gmpnp_jacobian_nnz(const gmpnp_solver* s) { return s ? (int64_t)s->nb * s->nf * s->nf : 0; }
int32_t gmpnp_n_aggregates(const gmpnp_solver* s) { return s ? s->t.nagg : 0; }
int32_t gmpnp_krylov_launches_per_iteration(const gmpnp_solver* s) { return s ? (s->fused_half ? 2 : 4) : 0; }

int gmpnp_assemble(gmpnp_solver* s, int32_t want_jacobian, double* F_out, double* norm_out) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  double r = 0.0; int flags = 0; int rc;
  GMPNP_DISPATCH(s, rc = (residual<DIM, NF>(s, want_jacobian != 0, &r, &flags)));
  if (rc) return rc;
  if (want_jacobian) {
    GMPNP_DISPATCH(s, rc = (launch_jac_gather<DIM, NF>(s)));
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->jacobian_valid = true; s->precond_valid = false;
  }
  if (norm_out) *norm_out = r;
  if (F_out) { rc = download_vec(s, s->F.p, F_out); if (rc) return rc; }
  if ((flags & 1) && s->cfg.strict_steric) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
  if (flags & (32 | 64)) return fail(GMPNP_ERR_NUMERIC, status_message(flags));
  return GMPNP_OK;
}

int gmpnp_get_jacobian_csr(gmpnp_solver* s, int32_t* indptr, int32_t* indices, double* data) {
  if (!s || !indptr || !indices || !data) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (!s->jacobian_valid) return fail(GMPNP_ERR_INVALID, "no Jacobian assembled for the current state");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const Topology& t = s->t; const int nf = s->nf;
  std::vector<double> v((size_t)t.slice_off[t.nslices]);
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(v.data(), s->c.vals, v.size() * sizeof(double), hipMemcpyDeviceToHost));   // (c.vals: either of vals / vals2)
  int64_t pos = 0; indptr[0] = 0;
  std::vector<std::pair<int, int>> order;  // (file column node, kpos)
  for (int vf = 0; vf < t.nv; ++vf) {
    const int I = t.iperm[vf], sl = t.node_slice[I], il = I - t.slice_node0[sl];
    order.clear();
    for (int k = t.rowptr[I]; k < t.rowptr[I + 1]; ++k) order.push_back({t.perm[t.cols[k]], t.sellk[k]});
    std::sort(order.begin(), order.end());
    for (int i = 0; i < nf; ++i) {
      for (auto& pr : order)
        for (int j = 0; j < nf; ++j) {
          indices[pos] = pr.first * nf + j;
          data[pos] = v[(size_t)t.slice_off[sl] + (size_t)(pr.second * nf + j) * kWave + il * nf + i];
          ++pos;
        }
      indptr[(size_t)vf * nf + i + 1] = (int32_t)pos;
    }
  }
  return GMPNP_OK;
}

int gmpnp_spmv(gmpnp_solver* s, const double* x, double* y) {
  if (!s || !x || !y) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (!s->jacobian_valid) return fail(GMPNP_ERR_INVALID, "no Jacobian assembled for the current state");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = upload_vec(s, x, s->kx.p); if (rc) return rc;
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c,
                                       (const double*)s->kx.p, s->kt.p));
  HIP_TRY(hipGetLastError());
  return download_vec(s, s->kt.p, y);
}

int gmpnp_spmv_scaled(gmpnp_solver* s, const double* x, double* y) {
  if (!s || !x || !y) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (!s->jacobian_valid || !s->precond_valid) return fail(GMPNP_ERR_INVALID, "no preconditioner set up for the current Jacobian (a linear or Newton solve sets it up)");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  int rc = upload_vec(s, x, s->kx.p); if (rc) return rc;
  GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_spmv_scaled<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c,
                                       (const double*)s->kx.p, s->kt.p));
  HIP_TRY(hipGetLastError());
  return download_vec(s, s->kt.p, y);
}

int gmpnp_linear_solve(gmpnp_solver* s, const double* b, double* x, int32_t mode, double rtol, double atol,
                       int32_t maxit, gmpnp_linear_stats_t* stats) {
  if (!s || !b || !x) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (!s->jacobian_valid) return fail(GMPNP_ERR_INVALID, "no Jacobian assembled for the current state");
  if (mode < 0 || mode > GMPNP_LINEAR_BAND_LU) return fail(GMPNP_ERR_INVALID, "unknown linear_solver");
  if (maxit < 1) return fail(GMPNP_ERR_INVALID, "max_iterations < 1");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipMemsetAsync(s->status.p, 0, sizeof(int32_t), s->stream));
  int rc = upload_vec(s, b, s->kr.p); if (rc) return rc;
  double bn = 0.0;
  for (int64_t i = 0; i < s->ndof; ++i) bn += b[i] * b[i];
  bn = std::sqrt(bn);
  if (mode == GMPNP_LINEAR_BLOCK_TRIDIAGONAL) {
    if (s->dim != 1) return fail(GMPNP_ERR_INVALID, "block-tridiagonal solver needs a 1D mesh");
    rc = tri_solve<7>(s, s->kr.p); if (rc) return rc;
    rc = tri_apply<7>(s, s->kx.p, 0.0, 1.0); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(s->h_status, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (*s->h_status & 14) return fail(GMPNP_ERR_LINEAR, status_message(*s->h_status));
    if (stats) { stats->iterations = 1; stats->converged = 1; stats->residual_norm = 0.0; stats->rhs_norm = bn; }
    return download_vec(s, s->kx.p, x);
  }
  if (mode == GMPNP_LINEAR_BAND_LU) {
    if (s->dim != 3) return fail(GMPNP_ERR_INVALID, "block-banded LU is the 3D direct solver (1D meshes: GMPNP_LINEAR_BLOCK_TRIDIAGONAL)");
    HIP_TRY(hipMemcpyAsync(s->kb.p, s->kr.p, s->ndof * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
    gmpnp_linear_stats_t ls{};
    rc = band_solve<9>(s, bn, rtol, atol, &ls);
    ls.iterations = 1;
    if (stats) *stats = ls;
    if (rc) return rc;
    return download_vec(s, s->kx.p, x);
  }
  GMPNP_DISPATCH(s, rc = (setup_preconditioner<DIM, NF>(s, mode)));
  if (rc) return rc;
  gmpnp_linear_stats_t ls{};
  KrylovRequest req;
  req.mode = mode; req.bnorm = bn; req.rtol = rtol; req.atol = atol; req.maxit = maxit; req.refine = true;
  GMPNP_DISPATCH(s, rc = (krylov_verified<NF>(s, &ls, req)));
  if (stats) *stats = ls;
  HIP_TRY(hipMemcpy(s->h_status, s->status.p, sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_TRY(hipStreamSynchronize(s->stream));
  { int rc2 = drain_spmv_events(s); if (rc2) return rc2; }
  if (*s->h_status & 14) return fail(GMPNP_ERR_LINEAR, status_message(*s->h_status));
  if (rc) return rc;
  return download_vec(s, s->kx.p, x);
}

int gmpnp_attach_coarse_level(gmpnp_solver* fine, gmpnp_solver* coarse, const int32_t* parents, double theta, int32_t sweeps) {
  if (!fine || !coarse || !parents) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (fine == coarse || coarse->ml_is_coarse) return fail(GMPNP_ERR_INVALID, "a level handle serves one finer level");
  if (stern_on(fine) || stern_on(coarse)) return fail(GMPNP_ERR_INVALID, "multilevel term: not with the Stern boundary condition on a level (gmpnp_set_stern)");
  if (kinetics_on(fine) || kinetics_on(coarse)) return fail(GMPNP_ERR_INVALID, "multilevel term: not with the surface kinetics on a level (gmpnp_set_kinetics)");
  if (galvanostat_on(fine) || galvanostat_on(coarse)) return fail(GMPNP_ERR_INVALID, "multilevel term: not with the galvanostat on a level (gmpnp_set_galvanostat)");
  if (fine->dim != 3 || coarse->dim != 3 || fine->nf != 9 || coarse->nf != 9) return fail(GMPNP_ERR_INVALID, "multilevel term: 3D pore problems (9 fields)");
  if (fine->partitioned != coarse->partitioned) return fail(GMPNP_ERR_INVALID, "multilevel term: both levels partitioned, or neither");
  if (fine->opts.device_id != coarse->opts.device_id) return fail(GMPNP_ERR_INVALID, "the levels live on one device");
  if (!(theta > 0.0)) return fail(GMPNP_ERR_INVALID, "theta must be positive");
  if (sweeps < 1 || sweeps > 16) return fail(GMPNP_ERR_INVALID, "sweeps: 1 ... 16");
  // partition handles of one rank (gmpnp_group.h, "multilevel term"): `parents` in the coarse handle's LOCAL file order
  const bool part = fine->partitioned;
  if (part && (fine->part_rank != coarse->part_rank || fine->part_size != coarse->part_size))
    return fail(GMPNP_ERR_INVALID, "multilevel term: the levels must be partition handles of the same rank of partitions of the same size");
  if (!part && coarse->t.nv >= fine->t.nv) return fail(GMPNP_ERR_INVALID, "the coarse level has fewer vertices");
  LevelTables tb;
  const std::string err = build_level_tables(fine->t.perm, coarse->t.iperm, fine->t.own_node0, fine->t.own_node1, coarse->t.own_node0,
                                             coarse->t.own_node1, parents, part, &tb);
  if (!err.empty()) return fail(GMPNP_ERR_INVALID, err);
  HIP_TRY(hipSetDevice(fine->opts.device_id));
  HIP_TRY(fine->ml_par.upload(tb.par)); HIP_TRY(fine->ml_child_ptr.upload(tb.child_ptr)); HIP_TRY(fine->ml_child.upload(tb.child)); HIP_TRY(fine->ml_copy.upload(tb.copy));
  HIP_TRY(fine->ml_z.alloc(fine->ndof));
  if (part) { HIP_TRY(fine->ml_tbc.alloc(fine->ndof)); HIP_TRY(fine->ml_tbd.alloc(fine->ndof)); }
  HIP_TRY(coarse->ml_r.alloc(coarse->ndof)); HIP_TRY(coarse->ml_w.alloc(coarse->ndof));
  fine->ml_coarse = coarse; fine->ml_theta = theta; coarse->ml_is_coarse = true; coarse->ml_sweeps = sweeps;
  // the staged operand exists in the materialised vector form only (k_vec_a / k_vec_b write the vector, the tile kernels stage one)
  fine->matp = true; fine->fused_half = false;
  fine->precond_valid = false;
  return GMPNP_OK;
}

int gmpnp_time_kernel(gmpnp_solver* s, int32_t kernel, int32_t launches, double* avg_us) {
  if (!s || !avg_us || launches < 1) return fail(GMPNP_ERR_INVALID, "bad arguments");
  if (kernel == 24 && !stern_on(s)) return fail(GMPNP_ERR_INVALID, "kernel 24 is the Stern boundary condition: the option is off (gmpnp_set_stern)");
  if (kernel == 25 && !kinetics_on(s)) return fail(GMPNP_ERR_INVALID, "kernel 25 is the surface kinetics: the option is off (gmpnp_set_kinetics)");
  if (kernel == 26 && !galvanostat_on(s)) return fail(GMPNP_ERR_INVALID, "kernel 26 is the galvanostat: the option is off (gmpnp_set_galvanostat)");
  if (kernel == 27 && !response_has_chunk(s)) return fail(GMPNP_ERR_INVALID, "kernel 27 is one chunk of the frequency response: no call has been made (gmpnp_frequency_response)");
  if (kernel == 28 && !tangent_has_chain(s)) return fail(GMPNP_ERR_INVALID, "kernel 28 is the multi-column chain of the electrode tangent: no call has been made on this Jacobian (gmpnp_electrode_tangent, 1D)");
  if (kernel == 29 && !trace_is_open(s)) return fail(GMPNP_ERR_INVALID, "kernel 29 is one append of the electrode trace: no trace is open (gmpnp_electrode_trace_open)");
  if (kernel == 30 && !response_band_has_chunk(s)) return fail(GMPNP_ERR_INVALID, "kernel 30 is one chunk of the 3D frequency response: no call has been made (gmpnp_frequency_response_3d), or the Stern option is off");
  if (kernel == 31 && !sensitivity_is_open(s)) return fail(GMPNP_ERR_INVALID, "kernel 31 is one step of the transient sensitivities: no buffer is open (gmpnp_sensitivity_open)");
  if (kernel == 32 && !wall_profile_is_open(s)) return fail(GMPNP_ERR_INVALID, "kernel 32 is one append of the wall profile: no profile is open (gmpnp_wall_profile_open)");
  if (kernel == 33 && !cycle_has_window(s)) return fail(GMPNP_ERR_INVALID, "kernel 33 is the cycle residual and mix: no cycle is open with a pair in its window (gmpnp_cycle_open, gmpnp_cycle_end)");
  if ((kernel == 0 || kernel == 18 || kernel == 24 || kernel == 25 || kernel == 26) && !s->jacobian_valid)
    return fail(GMPNP_ERR_INVALID, "no Jacobian assembled for the current state");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  hipEvent_t a, b; HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
  int rc = GMPNP_OK;
  auto one = [&]() -> int {
    int r = GMPNP_OK;
    switch (kernel) {
      case 0: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_spmv_plain<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, (const double*)s->kx.p, s->kt.p)); break;
      case 1: GMPNP_DISPATCH(s, r = (launch_element<DIM, NF>(s, true))); break;
      case 2: GMPNP_DISPATCH(s, r = (launch_jac_gather<DIM, NF>(s))); break;
      case 3: GMPNP_DISPATCH(s, r = (launch_res_gather<DIM, NF>(s))); break;
      case 4: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_bicg_a<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, 1)); break;
      case 5: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_bicg_b<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, 1)); break;
      case 6: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_coarse_a<NF>), dim3(std::max(1, s->t.nagg)), dim3(kCoarseThreads), 0, s->stream, s->c, 1)); break;
      case 7: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_coarse_b<NF>), dim3(std::max(1, s->t.nagg)), dim3(kCoarseThreads), 0, s->stream, s->c, 1)); break;
      case 8: hipLaunchKernelGGL(k_copy2, dim3(1), dim3(64), 0, s->stream, s->yc.p, (double*)nullptr, s->cpart_t.p, 64); break;
      case 9: hipLaunchKernelGGL(k_stream_read, dim3(2048), dim3(256), 0, s->stream, (const double2*)s->vals_s.p, s->vals_s.n / 2, s->part_f.p); break;
      case 10: hipLaunchKernelGGL(k_stream_read, dim3(512), dim3(256), 0, s->stream, (const double2*)s->vals_s.p, s->vals_s.n / 2, s->part_f.p); break;
      case 11: hipLaunchKernelGGL(k_stream_read, dim3(8192), dim3(256), 0, s->stream, (const double2*)s->vals_s.p, s->vals_s.n / 2, s->part_f.p); break;
      case 12: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_half_a<NF>), dim3(s->t.nagg + s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, 1,
                                                    (unsigned)(++s->fused_seq))); break;
      case 13: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_half_b<NF>), dim3(s->t.nagg + s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, 1,
                                                    (unsigned)(++s->fused_seq))); break;
      case 14: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_bicg_a_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, 1)); break;
      case 15: GMPNP_DISPATCH(s, hipLaunchKernelGGL((k_bicg_b_mat<NF>), dim3(s->t.own_ntiles), dim3(kKrylovThreads), 0, s->stream, s->c, 1)); break;
      case 16: hipLaunchKernelGGL(k_vec_a, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->c, 1); break;
      case 17: hipLaunchKernelGGL(k_vec_b, dim3(grid_for(s->ndof, 256)), dim3(256), 0, s->stream, s->c, 1); break;
      case 18:   // the whole 1D direct solve: extraction + ~13 levels of block cyclic reduction down and up (k_bcr_forward / k_bcr_tail / k_bcr_backward)
        if (s->dim != 1 || !s->tri_ok) return fail(GMPNP_ERR_INVALID, "kernel 18 is the 1D block-cyclic-reduction solve");
        r = tri_solve<7>(s, s->F.p); break;
      case 19: GMPNP_DISPATCH(s, r = (launch_element<DIM, NF>(s, false))); break;
      case 20: r = budget_launch_any(s); break;   // element pass without J, cell pass, row pass, final sums
      case 21:   // the step limiter's two launches on a zero correction (alpha = 1, u -= 0: the state stays)
        GMPNP_DISPATCH(s, r = (step_launch<NF>(s, s->limiter->dx.p, s->limiter->dx.p, 1.0, 0.9, nullptr))); break;
      case 22: r = time_launch_any(s); break;   // k_time_error + k_time_reduce + k_time_shift
      case 23: r = time_launch_any2(s); break;  // k_time_history + k_time_error2 + k_time_reduce + k_time_shift3
      case 24: r = stern_launch_residual(s, s->status.p); if (!r) r = stern_launch_jacobian(s); break;   // k_stern_residual + k_stern_jacobian
      case 25: r = kinetics_launch_residual(s, s->status.p); if (!r) r = kinetics_launch_jacobian(s); break;   // k_kinetics_residual + k_kinetics_jacobian
      case 26: r = galvanostat_launch_iteration(s); break;   // k_galv_rhs + k_galv_reduce + k_galv_direction + k_galv_potential + k_galv_reduce (G alone)
      case 27: r = response_time_chunk(s); break;   // k_response_solve + k_response_functional on the last chunk's frequencies
      case 28: r = tangent_time_chain(s); break;    // extraction, k_bcr_forward_cols / k_bcr_tail_cols / k_bcr_backward_cols, application
      case 29: r = trace_time_append(s); break;     // k_stern_residual + k_kinetics_residual (kinetics on) + k_electrode_record
      case 30: r = response_band_time_chunk(s); break;   // k_cband_scatter, k_band_step<9, BandComplex> per pivot, the solve and three refinement rounds, k_cband_functional
      case 31: r = sensitivity_time_step(s); break;      // assembly, columns, k_sens_rhs, chain(s), application, k_spmv_plain per column, k_sens_record
      case 32: r = wall_profile_time_append(s); break;   // k_stern_residual + k_kinetics_residual (kinetics on) + k_wall_profile
      case 33: r = cycle_time_launch(s); break;          // k_cycle_residual + k_cycle_reduce + k_cycle_mix (direction) + k_step_limit + k_cycle_mix (apply)
      default: return fail(GMPNP_ERR_INVALID, "unknown kernel id");
    }
    return r;
  };
  if (kernel == 12 || kernel == 13) { HIP_TRY(hipMemset(s->ticket.p, 0, 16 * 66 * sizeof(uint32_t))); s->fused_seq = 0; }
  if ((kernel >= 4 && kernel <= 7) || (kernel >= 12 && kernel <= 17)) {  // Krylov kernels: a live (not finished) solve state
    KrylovScalars z{}; z.rho[0] = z.rho[1] = 1.0; z.alpha = 1.0; z.omega = 1.0; z.beta = 0.5; z.tol = 0.0; z.max_iters = 1 << 30;
    HIP_TRY(hipMemcpy(s->scal.p, &z, sizeof z, hipMemcpyHostToDevice));
  }
  if (kernel == 21) {
    rc = step_prepare(s); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(s->limiter->dx.p, 0, (size_t)s->ndof * sizeof(double), s->stream));
  }
  DevBuf<double> keep;   // kernel 22 shifts u into u_n: u_n and u_nm1 are put back behind the launches
  if (kernel == 22) { rc = time_kernel_begin(s, keep); if (rc) return rc; }
  if (kernel == 23) { rc = time_kernel_begin2(s, keep); if (rc) return rc; }
  if (kernel == 33) { rc = cycle_kernel_begin(s, keep); if (rc) return rc; }   // the mix writes u and u_n
  // kernel 22: whatever happens between the bracket's two halves, u_n and u_nm1 are put back (g_err keeps the first message)
  auto restore = [&](int code) { if (kernel != 22 && kernel != 23 && kernel != 33) return code; const std::string msg = g_err;
                                 const int rc2 = kernel == 22 ? time_kernel_end(s, keep) : kernel == 23 ? time_kernel_end2(s, keep) : cycle_kernel_end(s, keep);
                                 if (code) { g_err = msg; return code; } return rc2; };
  rc = one(); if (rc) return restore(rc);  // warm
  float ms = 0.f;
  auto timed = [&]() -> int {
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipEventRecord(a, s->stream));
    for (int i = 0; i < launches && rc == GMPNP_OK; ++i) rc = one();
    HIP_TRY(hipEventRecord(b, s->stream));
    HIP_TRY(hipEventSynchronize(b));
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    return rc;
  };
  rc = restore(timed());
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  if (rc) return rc;
  *avg_us = 1000.0 * ms / launches;
  if (kernel == 24 || kernel == 25) { s->jacobian_valid = false; s->precond_valid = false; }   // every launch added the Stern / kinetic entries once more
  return GMPNP_OK;
}

int gmpnp_event_overhead(gmpnp_solver* s, int32_t pairs, double* mean_us) {
  if (!s || !mean_us || pairs < 1) return fail(GMPNP_ERR_INVALID, "bad arguments");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  hipEvent_t a, b; HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
  double sum = 0.0;
  for (int i = 0; i < pairs; ++i) {
    // keep the stream busy in front of the pair, as inside a solve
    hipLaunchKernelGGL(k_copy2, dim3(1), dim3(64), 0, s->stream, s->yc.p, (double*)nullptr, s->cpart_t.p, 64);
    HIP_TRY(hipEventRecord(a, s->stream)); HIP_TRY(hipEventRecord(b, s->stream));
    hipLaunchKernelGGL(k_copy2, dim3(1), dim3(64), 0, s->stream, s->yc.p, (double*)nullptr, s->cpart_t.p, 64);
    HIP_TRY(hipEventSynchronize(b));
    float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, a, b)); sum += 1000.0 * ms;
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  *mean_us = sum / pairs;
  return GMPNP_OK;
}

#ifdef GMPNP_DEV_HOOKS  // development builds only (tools/): not part of the ABI, not in the shipped library
// resident workgroups per CU of the fused 3D Krylov kernels
int gmpnp_debug_occupancy(int* out4) {
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out4[0], k_bicg_a<9>, kKrylovThreads, 0));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out4[1], k_bicg_b<9>, kKrylovThreads, 0));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out4[2], k_spmv_plain<9>, kKrylovThreads, 0));
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out4[3], k_coarse_a<9>, kCoarseThreads, 0));
  return GMPNP_OK;
}

// debug only (not declared in gmpnp.h): raw device buffers, internal order
int gmpnp_debug_read(gmpnp_solver* s, int which, double* out, int64_t n) {
  if (!s || !out) return fail(GMPNP_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  const double* src = nullptr; int64_t cap = 0;
  switch (which) {
    case 0: src = s->krhat.p; cap = s->ndof; break;
    case 1: src = s->vals_s.p; cap = (int64_t)s->vals_s.n; break;   // raw: inside a block position the pair layout of value_pair_offset, not [j][lane]
    case 2: src = s->Dinv.p; cap = (int64_t)s->Dinv.n; break;
    case 3: src = s->c.Aci; cap = (int64_t)s->Aci.n; break;
    case 4: src = s->c.vals; cap = (int64_t)s->vals.n; break;
    case 5: src = s->Ac.p; cap = (int64_t)s->Ac.n; break;
    case 6: src = s->kr.p; cap = s->ndof; break;
    case 7: src = s->ky.p; cap = s->ndof; break;
    case 8: src = s->ks.p; cap = s->ndof; break;
    case 9: src = s->kt.p; cap = s->ndof; break;
    case 10: src = s->kp0.p; cap = s->ndof; break;
    case 11: src = s->kp1.p; cap = s->ndof; break;
    case 12: src = s->kv0.p; cap = s->ndof; break;
    case 13: src = s->kv1.p; cap = s->ndof; break;
    case 14: src = s->yc.p; cap = (int64_t)s->yc.n; break;
    default: return GMPNP_ERR_INVALID;
  }
  if (n > cap) n = cap;
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(out, src, n * sizeof(double), hipMemcpyDeviceToHost));
  return (int)0;
}
#endif  // GMPNP_DEV_HOOKS

int gmpnp_spmv_profile(gmpnp_solver* s, int64_t* n_sampled, double* mean_us, int64_t* n_launched) {
  if (!s) return fail(GMPNP_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(s->opts.device_id));
  HIP_TRY(hipStreamSynchronize(s->stream));
  { int rc = drain_spmv_events(s); if (rc) return rc; }
  if (n_sampled) *n_sampled = s->spmv_sampled;
  if (mean_us) *mean_us = s->spmv_sampled ? s->spmv_us_sum / s->spmv_sampled : 0.0;
  if (n_launched) *n_launched = s->spmv_launched;
  s->spmv_sampled = 0; s->spmv_us_sum = 0.0; s->spmv_launched = 0;
  return GMPNP_OK;
}

}  // extern "C"

#include "gmpnp_group.h"
#include "gmpnp_project.h"
#include "gmpnp_ensemble.h"
#include "gmpnp_stats.h"
#include "gmpnp_budget.h"
#include "gmpnp_time_step.h"
#include "gmpnp_time_step_ens.h"
#include "gmpnp_time_order.h"
#include "gmpnp_stern.h"
#include "gmpnp_kinetics.h"
#include "gmpnp_galvanostat.h"
#include "gmpnp_response.h"
#include "gmpnp_tangent.h"
#include "gmpnp_trace.h"
#include "gmpnp_sensitivity.h"
#include "gmpnp_response_band.h"
#include "gmpnp_wall_profile.h"
#include "gmpnp_cycle.h"
