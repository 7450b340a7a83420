// Ensemble of independent problems on one mesh (include/gmpnp.h, "ensemble of problems"): 1D members, and 3D members below.
// Included at the end of gmpnp_api.hip: uses the handle type and the helpers defined there.
//
// One Newton iteration of B members is ONE launch chain: Jacobian gather, block-tridiagonal extraction, the cyclic reduction
// down (one launch per level), the tail (one wave per member), the reduction up, the update, and the residual (element kernel +
// gather) at the new iterate.  Every launch carries all ACTIVE members: blockIdx.y (the tail: blockIdx.x) indexes the active list,
// the member's Ctx / TriLevel pyramid / status word come from a per-member table in device memory.  The batched kernels call the
// single handle's code (the bodies of k_element and k_jac_gather, res_gather_body, tri_extract_entry, bcr_forward_row,
// bcr_top_row, bcr_backward_entry, tri_apply_entry), so a member computes exactly what its handle computes alone.  Members are
// independent: nothing waits inside a launch, the launch boundaries are the only ordering.  One host synchronisation per
// iteration: the residual partials of every member land in that member's pinned buffer, the host forms the norms and decides
// per member with the one Newton rule (NewtonJudge, gmpnp_host_rules.h), then uploads the next active list.
#pragma once

namespace gmpnp {

constexpr int kEnsMaxMembers = 64;   // gmpnp_ensemble_create refuses more
constexpr int kEnsMaxLevels = 32;    // cyclic-reduction levels: ceil(log2(n_vertices)) + 1

struct EnsMember {
  Ctx c;
  TriLevel tri[kEnsMaxLevels];
  int32_t* status;
  const int32_t* tri_kpos;
  // step limiter (gmpnp_step_limit.h; set for the members of a limited solve): the member's kxp, partials and pinned report
  double* kxp; double* sl_part; int32_t* sl_node; StepReport* sl_report;
};

template <int DIM, int NF, bool STAGED_ = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GMPNP_ELEMENT_WAVES, GMPNP_ELEMENT_WAVES))) void k_element_ens(
    const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  constexpr bool WANT_J = true, STAGED = STAGED_;
  const Ctx& c = tab[act[blockIdx.y]].c;   // (a copy of the context here costs 864 bytes of scratch per lane; the gather's copy costs none)
#include "gmpnp_element_body.inc"
}
template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_res_gather_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  res_gather_body<DIM, NF>(tab[act[blockIdx.y]].c);
}
template <int DIM, int NF>
__global__ __launch_bounds__(kVecBlock) void k_jac_gather_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  const Ctx c = tab[act[blockIdx.y]].c;
  constexpr bool ROBIN = false;   // members keep k_robin_add_ens
#include "gmpnp_jac_gather_body.inc"
}
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_tri_extract_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel l0 = M.tri[0];
  tri_extract_entry<NF>(M.c, l0, M.tri_kpos, M.c.F, blockIdx.x * kVecBlock + threadIdx.x);
}
template <int NF>
__global__ __launch_bounds__(64) void k_bcr_forward_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int l) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel lo = M.tri[l], hi = M.tri[l + 1];
  bcr_forward_row<NF>(lo, hi, M.status, blockIdx.x * 4 + ((int)threadIdx.x >> 4));
}
// k_bcr_tail of one member per workgroup (one wave each): levels l0 .. l0 + nlev - 1
template <int NF>
__global__ __launch_bounds__(kBcrTailThreads) void k_bcr_tail_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act,
                                                                  const int l0, const int nlev) {
  const EnsMember& M = tab[act[blockIdx.x]];
  const TriLevel* lv = M.tri + l0;
  int32_t* status = M.status;
  const int t = threadIdx.x;
  for (int l = 0; l + 1 < nlev; ++l) {
    const TriLevel lo = lv[l], hi = lv[l + 1];
    for (int ih0 = 0; ih0 < hi.n; ih0 += kBcrTailThreads / 16) bcr_forward_row<NF>(lo, hi, status, ih0 + (t >> 4));
    __syncthreads();
  }
  {
    const TriLevel top = lv[nlev - 1];
    if (t < 64) bcr_top_row<NF>(top, status);
  }
  __syncthreads();
  for (int l = nlev - 2; l >= 0; --l) {
    const TriLevel lo = lv[l], hi = lv[l + 1];
    for (int q = t; q < lo.n * NF; q += kBcrTailThreads) bcr_backward_entry<NF>(lo, hi, q);
    __syncthreads();
  }
}
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_bcr_backward_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int l) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel lo = M.tri[l], hi = M.tri[l + 1];
  bcr_backward_entry<NF>(lo, hi, blockIdx.x * kVecBlock + threadIdx.x);
}
// u <- u - omega x (tri_apply of the single handle with scale_dst = 1, scale_x = -omega)
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_tri_apply_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const double scale_x) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel l0 = M.tri[0];
  tri_apply_entry<NF>(l0, M.c.u, 1.0, scale_x, M.c.ndof, blockIdx.x * kVecBlock + threadIdx.x);
}
// limited update (gmpnp_newton_options_t.step_fraction): kx <- x, the member's ratio partials, then its own alpha and update
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_tri_dx_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  const EnsMember& M = tab[act[blockIdx.y]];
  const TriLevel l0 = M.tri[0];
  tri_apply_entry<NF>(l0, M.c.kx, 0.0, 1.0, M.c.ndof, blockIdx.x * kVecBlock + threadIdx.x);
}
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_step_limit_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  const EnsMember& M = tab[act[blockIdx.y]];
  step_limit_body<NF>(StepLimitIo{M.c.u, M.c.kx, M.c.model, M.sl_part, M.sl_node, M.c.nv});
}
__global__ __launch_bounds__(kVecBlock) void k_limited_update_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int nblk,
                                                                  const double omega, const double tau) {
  const EnsMember& M = tab[act[blockIdx.y]];
  step_update_body<true>(StepUpdateIo{M.c.u, M.c.kx, M.kxp, M.sl_part, M.sl_node, nblk, M.c.ndof, omega, tau, M.sl_report, M.status});
}
// u_n <- u of member blockIdx.y (all members)
__global__ __launch_bounds__(256) void k_ens_assign(const EnsMember* __restrict__ tab, const int ndof) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ndof) return;
  const Ctx& c = tab[blockIdx.y].c;
  c.un[i] = c.u[i];
}
// dst[m][i] = u of member m (internal order)
__global__ __launch_bounds__(256) void k_ens_gather_u(const EnsMember* __restrict__ tab, double* __restrict__ dst, const int ndof) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ndof) return;
  dst[(size_t)blockIdx.y * ndof + i] = tab[blockIdx.y].c.u[i];
}


// ---- 3D members: set-up, BiCGStab and the end of a solve of the two-level path, batched -------------------
// What a member's launches of ONE Newton iteration take as kernel arguments on its own handle: the start values of its BiCGStab
// pass, the Newton update its last M^-1 application carries, and whether kx holds an accepted predicted start.
struct EnsIter3 {
  KrylovScalars init;
  NewtonUpdate upd;    // upd.u == nullptr: the update is a launch of its own (k_axpy_u_ens)
  double scale_dst;    // 1: dx accumulates on the predicted start in kx
};
#define GMPNP_ENS_CTX const Ctx& c = tab[act[blockIdx.y]].c
__global__ void k_robin_add_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) { GMPNP_ENS_CTX; robin_add_body(c); }
template <int NF>
__global__ __launch_bounds__(64) void k_block_inverse_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) { GMPNP_ENS_CTX; block_inverse_body<NF>(c); }
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_scale_columns_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) { GMPNP_ENS_CTX; scale_columns_body<NF>(c); }
template <int NF>
__global__ __launch_bounds__(64) void k_coarse_rows_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) { GMPNP_ENS_CTX; coarse_rows_body<NF>(c); }
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_coarse_sum_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) { GMPNP_ENS_CTX; coarse_sum_body<NF>(c); }
__global__ __launch_bounds__(kVecBlock) void k_coarse_reduce_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) { GMPNP_ENS_CTX; coarse_reduce_body(c); }
// one workgroup per member
template <int NF>
__global__ __launch_bounds__(512) void k_coarse_invert_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  coarse_invert_body<NF>(tab[act[blockIdx.x]].c);
}
// warm-start test: kt = J kx, then the partials of (kt, kb), (kt, kt), (kb, kb) in the member's pinned buffer; kr = kb - kt
template <int NF>
__global__ __launch_bounds__(kKrylovThreads) void k_spmv_plain_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  GMPNP_ENS_CTX;
  spmv_plain_body<NF, false>(c, c.kx, nullptr, c.kt);
}
__global__ __launch_bounds__(kVecBlock) void k_dots3_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  GMPNP_ENS_CTX;
  dots3_body(c.kt, c.kb, c.part_f, c.ndof, (int)gridDim.x, 0, 0x7fffffff);
}
__global__ __launch_bounds__(256) void k_start_residual_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  GMPNP_ENS_CTX;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c.ndof) c.kr[i] = c.kb[i] - c.kt[i];
}
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_krylov_init_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act,
                                                               const EnsIter3* __restrict__ it) {
  const int m = act[blockIdx.y];
  const Ctx& c = tab[m].c;
  krylov_init_body<NF>(c, nullptr, it[m].init, c.cpart_v[1]);
}
template <int NF>
__global__ __launch_bounds__(kCoarseThreads) void k_coarse_a_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int k) {
  GMPNP_ENS_CTX;
  coarse_a_body<NF, false>(c, k, blockIdx.x, 0u);
}
template <int NF>
__global__ __launch_bounds__(kCoarseThreads) void k_coarse_b_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int k) {
  GMPNP_ENS_CTX;
  coarse_b_body<NF, false>(c, k, blockIdx.x, 0u);
}
template <int NF>
__global__ __launch_bounds__(kKrylovThreads) void k_bicg_a_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int k) {
  GMPNP_ENS_CTX;
  bicg_a_body<NF, false>(c, k, c.tile0 + xcd_tile(blockIdx.x, gridDim.x), 0u);
}
template <int NF>
__global__ __launch_bounds__(kKrylovThreads) void k_bicg_b_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const int k) {
  GMPNP_ENS_CTX;
  bicg_b_body<NF, false>(c, k, c.tile0 + xcd_tile(blockIdx.x, gridDim.x), 0u);
}
// end of a solve: P^T ky, then kx = scale_dst kx + M^-1 ky with the member's Newton update
template <int NF>
__global__ __launch_bounds__(kVecBlock) void k_restrict_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act) {
  GMPNP_ENS_CTX;
  restrict_body<NF>(c, c.ky, c.cpart_v[0]);
}
template <int NF>
__global__ __launch_bounds__(kKrylovThreads) void k_minv_apply_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act,
                                                                    const EnsIter3* __restrict__ it) {
  const int m = act[blockIdx.y];
  const Ctx& c = tab[m].c;
  minv_apply_body<NF>(c, c.ky, c.cpart_v[0], c.kx, it[m].scale_dst, 1.0, it[m].upd, nullptr);
}
// u += a kx (k_axpy of the single handle): the update of a member whose solve carries no predicted start
__global__ __launch_bounds__(256) void k_axpy_u_ens(const EnsMember* __restrict__ tab, const int32_t* __restrict__ act, const double a) {
  GMPNP_ENS_CTX;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c.ndof) c.u[i] += a * c.kx[i];
}
#undef GMPNP_ENS_CTX

}  // namespace gmpnp

// the active lists of a 3D solve: one device region each (a queued launch keeps reading its own), pinned staging per parity
constexpr int kEnsLists = 10;
enum EnsList { L_ACT = 0, L_BATCH, L_COARSE, L_WARM, L_START, L_KRY, L_END, L_AXPY, L_RES, L_TIME };

// adaptive time stepping of the members (gmpnp_time_step_ens.h), allocated by the first call of that family: an ensemble that
// never asks keeps the buffers it had
namespace gmpnp { struct EnsTimeRec; }
struct gmpnp_ens_time {
  gmpnp::EnsTimeRec* d_rec = nullptr;     // [kEnsMaxMembers]: per-member arguments of the listed members' launches
  gmpnp::EnsTimeRec* h_rec = nullptr;     // pinned [2][kEnsMaxMembers]: their staging, alternating
  gmpnp::TimeReport* h_report = nullptr;  // pinned [kEnsMaxMembers]: what k_time_reduce_ens writes
  gmpnp::TimeReport* d_report = nullptr;  // ... its device address
  gmpnp_model_t* h_model = nullptr;       // pinned [n]: staging of gmpnp_ensemble_set_time_step
  int slot = 0;
  ~gmpnp_ens_time() {
    if (d_rec) (void)hipFree(d_rec);
    if (h_rec) (void)hipHostFree(h_rec);
    if (h_report) (void)hipHostFree(h_report);
    if (h_model) (void)hipHostFree(h_model);
  }
};

struct gmpnp_ensemble {
  std::vector<gmpnp_solver*> m;   // owned by the caller
  int device = 0, ndof = 0, nv = 0;
  hipStream_t stream = nullptr;
  DevBuf<EnsMember> tab; DevBuf<int32_t> act; DevBuf<double> ustage; DevBuf<EnsIter3> it3;
  EnsMember* h_tab = nullptr;   // pinned [n]: staging of the member table
  EnsIter3* h_it3 = nullptr;    // pinned [2][n]: per-iteration arguments of 3D members, alternating
  int32_t* h_act = nullptr;     // pinned [2][kEnsLists][kEnsMaxMembers]: active lists, alternating (1D: the first two rows)
  double* h_u = nullptr;        // pinned [n][ndof]
  int act_slot = 0;
  std::vector<std::string> err;   // last failure of each member ("" = none)
  std::unique_ptr<gmpnp_ens_time> tstep;
  ~gmpnp_ensemble() {
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    tstep.reset();
    if (h_tab) (void)hipHostFree(h_tab);
    if (h_act) (void)hipHostFree(h_act);
    if (h_it3) (void)hipHostFree(h_it3);
    if (h_u) (void)hipHostFree(h_u);
  }
};

namespace {

// every member's own stream drained: what a member call queued (gmpnp_assign_previous) is done before the ensemble reads its state
int ens_drain_members(gmpnp_ensemble* e) {
  for (gmpnp_solver* s : e->m) HIP_TRY(hipStreamSynchronize(s->stream));
  return GMPNP_OK;
}

// the configuration an ensemble solve supports, per member: checked at create and again before every solve (SUPG can be set later)
int ens_check_member(const gmpnp_solver* s, const gmpnp_solver* s0, int k) {
  char buf[200];
  auto bad = [&](const char* why) { snprintf(buf, sizeof buf, "ensemble member %d: %s", k, why); return fail(GMPNP_ERR_INVALID, buf); };
  if (!s) return bad("NULL handle");
  const bool is3d = s->dim == 3 && s->nf == 9;
  if (!is3d && (s->dim != 1 || s->nf != 7)) return bad("ensembles hold 1D problems (6 species + potential) or 3D problems (8 species + potential)");
  if (s0 && s->dim != s0->dim) return bad("1D and 3D members cannot share an ensemble");
  if (s->partitioned) return bad("partitioned handles cannot join an ensemble");
  if (galvanostat_on(s)) return bad("the galvanostat is on (gmpnp_set_galvanostat): ensembles do not solve for the electrode potential");
  if (stern_on(s)) return bad("the Stern boundary condition is on (gmpnp_set_stern): ensembles do not apply it");
  if (kinetics_on(s)) return bad("the surface kinetics are on (gmpnp_set_kinetics): ensembles do not apply them");
  if (s->stepper && s->stepper->order == 2) return bad("the handle steps at order 2 (gmpnp_set_time_order): ensembles have no second-order time stepping");
  if (is3d) {
    if (s->ml_coarse || s->ml_is_coarse) return bad("a multilevel coarse level is attached: not supported in an ensemble");
    if (!s->opts.shared_device) return bad("3D members are created with shared_device = 1 (one stream, four launches per BiCGStab iteration)");
    if (s->fused_half || s->stream2) return bad("3D members use the four-launch BiCGStab form on one stream");
    if (s->matp) return bad("the materialised vector form (vector_form 1) is not supported in an ensemble");
    if (s->prereduce) return bad("mesh too large for an ensemble (more than 128 tile slots per aggregate)");
    if (!s->cfg.host_poll) return bad("progress_by_copy is not supported in an ensemble");
  } else {
    if (!s->tri_ok) return bad("the block-tridiagonal solver needs a 1D mesh in path order");
    if (s->c.supg_rho) return bad("SUPG terms are set (gmpnp_set_supg): not supported in an ensemble");
    if ((int)s->tri.size() > kEnsMaxLevels) return bad("mesh too large for the ensemble's level table");
    if (s->c.n_robin != 0) return bad("Robin terms are not part of the 1D model");
  }
  if (s == s0) return GMPNP_OK;
  if (s->opts.device_id != s0->opts.device_id) return bad("members live on different devices");
  const Topology& a = s->t; const Topology& b = s0->t;
  if (a.nv != b.nv || a.nc != b.nc || a.perm != b.perm || a.cells != b.cells || s->ndof != s0->ndof || a.nslices != b.nslices ||
      s->c.n_work != s0->c.n_work || s->c.wl_run_blocks != s0->c.wl_run_blocks || s->n_resblocks != s0->n_resblocks ||
      s->tri.size() != s0->tri.size())
    return bad("topology differs from member 0 (mesh, vertex order, cells or storage layout)");
  if (is3d && (a.nagg != b.nagg || s->ncoarse != s0->ncoarse || s->c.coarse_chunks != s0->c.coarse_chunks || s->c.n_robin != s0->c.n_robin ||
               a.ntiles != b.ntiles || a.own_ntiles != b.own_ntiles || a.tile_slots != b.tile_slots || a.col_stride != b.col_stride ||
               s->staged_element != s0->staged_element))
    return bad("topology differs from member 0 (aggregates, coarse chunks, tiles, Robin entries or element store form)");
  return GMPNP_OK;
}

int ens_upload_table(gmpnp_ensemble* e) {
  const int n = (int)e->m.size();
  for (int k = 0; k < n; ++k) {
    gmpnp_solver* s = e->m[k];
    EnsMember rec{};
    rec.c = s->c;
    for (size_t l = 0; l < s->tri.size(); ++l) rec.tri[l] = s->tri[l];
    rec.status = s->status.p; rec.tri_kpos = s->tri_kpos.p;
    rec.kxp = s->kxp.p;
    if (s->limiter) { rec.sl_part = s->limiter->part.p; rec.sl_node = s->limiter->part_node.p; rec.sl_report = s->limiter->d_report; }
    std::memcpy(&e->h_tab[k], &rec, sizeof rec);
  }
  HIP_TRY(hipMemcpyAsync(e->tab.p, e->h_tab, (size_t)n * sizeof(EnsMember), hipMemcpyHostToDevice, e->stream));
  return GMPNP_OK;
}

// the active list of the next launches: stream-ordered copy from a pinned slot the host does not touch again before the copy ran
// (the slots alternate, and every iteration ends with a synchronisation of the stream)
int ens_upload_active(gmpnp_ensemble* e, const std::vector<int32_t>& act) {
  int32_t* src = e->h_act + (size_t)e->act_slot * kEnsMaxMembers;
  e->act_slot ^= 1;
  std::memcpy(src, act.data(), act.size() * sizeof(int32_t));
  HIP_TRY(hipMemcpyAsync(e->act.p, src, act.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  return GMPNP_OK;
}

// element kernel + residual gather of the active members at their current u (leaves F and the element Jacobian records)
int ens_residual(gmpnp_ensemble* e, int nact) {
  gmpnp_solver* s0 = e->m[0];
  hipLaunchKernelGGL((k_element_ens<1, 7>), dim3(grid_for(s0->t.nc, 64), nact), dim3(64), 0, e->stream, (const EnsMember*)e->tab.p,
                     (const int32_t*)e->act.p);
  hipLaunchKernelGGL((k_res_gather_ens<1, 7>), dim3(s0->n_resblocks, nact), dim3(kVecBlock), 0, e->stream, (const EnsMember*)e->tab.p,
                     (const int32_t*)e->act.p);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// J dx = F by block cyclic reduction and u <- u - omega dx for the active members (gather, tri_solve and tri_apply of newton());
// tau != 0: the limited update of newton(), every member with its own alpha
int ens_update(gmpnp_ensemble* e, int nact, double omega, double tau) {
  gmpnp_solver* s0 = e->m[0];
  const EnsMember* tab = e->tab.p; const int32_t* act = e->act.p;
  constexpr int NF = 7;
  hipLaunchKernelGGL((k_jac_gather_ens<1, NF>), dim3(grid_for(s0->c.n_work * kWave, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act);
  hipLaunchKernelGGL((k_tri_extract_ens<NF>), dim3(grid_for(s0->t.nv * NF * NF, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act);
  const int nl = (int)s0->tri.size(), l0 = bcr_tail_first_level(s0);
  for (int l = 0; l < l0; ++l)
    hipLaunchKernelGGL((k_bcr_forward_ens<NF>), dim3(grid_for(s0->tri[l + 1].n, 4), nact), dim3(64), 0, e->stream, tab, act, l);
  hipLaunchKernelGGL((k_bcr_tail_ens<NF>), dim3(nact), dim3(kBcrTailThreads), 0, e->stream, tab, act, l0, nl - l0);
  for (int l = l0 - 1; l >= 0; --l)
    hipLaunchKernelGGL((k_bcr_backward_ens<NF>), dim3(grid_for(s0->tri[l].n * NF, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act, l);
  if (tau != 0.0) {
    const int nblk = s0->limiter->nblk;
    hipLaunchKernelGGL((k_tri_dx_ens<NF>), dim3(grid_for(s0->ndof, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act);
    hipLaunchKernelGGL((k_step_limit_ens<NF>), dim3(nblk, nact), dim3(kVecBlock), 0, e->stream, tab, act);
    hipLaunchKernelGGL(k_limited_update_ens, dim3(grid_for(s0->ndof, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act, nblk, omega, tau);
  } else
    hipLaunchKernelGGL((k_tri_apply_ens<NF>), dim3(grid_for(s0->ndof, kVecBlock), nact), dim3(kVecBlock), 0, e->stream, tab, act, -omega);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// ---- 3D members ------------------------------------------------------------------------------------------------------------------
// one of the lists of a 3D solve: its own device region, staged in the pinned row of the current parity (the parity flips once per
// Newton iteration, and every iteration ends with a synchronisation of the stream: a row is rewritten two iterations later)
int ens_upload_list(gmpnp_ensemble* e, int list, const std::vector<int32_t>& v) {
  if (v.empty()) return GMPNP_OK;
  int32_t* src = e->h_act + ((size_t)e->act_slot * kEnsLists + list) * kEnsMaxMembers;
  std::memcpy(src, v.data(), v.size() * sizeof(int32_t));
  HIP_TRY(hipMemcpyAsync(e->act.p + (size_t)list * kEnsMaxMembers, src, v.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  return GMPNP_OK;
}
const int32_t* ens_list(const gmpnp_ensemble* e, int list) { return e->act.p + (size_t)list * kEnsMaxMembers; }

// element kernel (record stores as the members have them) + residual gather of the listed members at their current u
template <int NF>
int ens3_residual(gmpnp_ensemble* e, int list, int nact) {
  gmpnp_solver* s0 = e->m[0];
  const EnsMember* tab = e->tab.p; const int32_t* act = ens_list(e, list);
  const dim3 g(grid_for(s0->t.nc, 64), nact);
  if (s0->staged_element) hipLaunchKernelGGL((k_element_ens<3, NF, true>), g, dim3(64), 0, e->stream, tab, act);
  else hipLaunchKernelGGL((k_element_ens<3, NF, false>), g, dim3(64), 0, e->stream, tab, act);
  hipLaunchKernelGGL((k_res_gather_ens<3, NF>), dim3(s0->n_resblocks, nact), dim3(kVecBlock), 0, e->stream, tab, act);
  HIP_TRY(hipGetLastError());
  return GMPNP_OK;
}

// Newton on every member with the two-level (or node-block Jacobi) BiCGStab: newton() / krylov_step() / krylov_verified() / krylov()
// of the single handle with every launch carrying a list of members, the host decisions taken per member by the member's own rule
// objects.  A member whose linear solve leaves the normal path (band LU due, predicted start to be formed by k_warm_start, first
// pass not converged within verify_above iterations) is finished by the serial step on its own handle, in the ensemble's stream.
template <int NF>
int ens3_newton(gmpnp_ensemble* e, const gmpnp_newton_options_t& o, gmpnp_newton_stats_t* stats, int32_t* status) {
  constexpr int DIM = 3, verify_above = 500, restart_every = 1000;   // as krylov_step / krylov_verified
  const int n = (int)e->m.size();
  gmpnp_solver* s0 = e->m[0];
  const int mode = o.linear_solver, use_coarse = (mode == GMPNP_LINEAR_BICGSTAB_TWOLEVEL) ? 1 : 0;
  const EnsMember* tab = e->tab.p;
  const double t0 = now_ms();
  { int rc = ens_drain_members(e); if (rc) return rc; }
  for (gmpnp_solver* s : e->m) s->c.use_coarse = use_coarse;
  { int rc = ens_upload_table(e); if (rc) return rc; }
  std::vector<char> live(n, 1);
  std::vector<double> rn(n, 0.0);   // residual norm of the member's current iterate
  std::vector<NewtonJudge> judge; judge.reserve(n);
  for (int k = 0; k < n; ++k) {
    stats[k] = fresh_newton_stats(); status[k] = GMPNP_OK; e->err[k].clear();
    judge.emplace_back(o, stats[k], e->m[k]->cfg.strict_steric != 0);
    HIP_TRY(hipMemsetAsync(e->m[k]->status.p, 0, sizeof(int32_t), e->stream));
  }
  auto settle = [&](int k, bool first) {
    gmpnp_solver* s = e->m[k];
    const double r = std::sqrt(sum_partials(s, 0));
    rn[k] = r;
    const NewtonJudge::Verdict v = first ? judge[k].first(r, *s->h_status) : judge[k].next(r, *s->h_status);
    if (v == NewtonJudge::go_on) return;
    live[k] = 0;
    if (v != NewtonJudge::failed) { s->state_jumped = false; s->direct.newton_done(false); stats[k].ms_total = now_ms() - t0; }
    if (v != NewtonJudge::converged) { status[k] = judge[k].code; e->err[k] = judge[k].message; }
  };
  // the member's linear step by the serial code, in the ensemble's stream (ordered behind everything the batch queued)
  auto serial_step = [&](int k) {
    gmpnp_solver* s = e->m[k];
    hipStream_t keep = s->stream;
    s->stream = e->stream;
    const int rc = s->direct.use_direct() ? direct_step<DIM, NF>(s, o, stats[k], rn[k]) : krylov_step<DIM, NF>(s, o, stats[k], rn[k]);
    s->stream = keep;
    if (rc) { status[k] = rc; e->err[k] = g_err; live[k] = 0; }
    return rc;
  };
  struct Plan { int it; bool coarse_fresh, precond_was_valid, warm, has_upd; double rhs_norm; };
  std::vector<Plan> plan(n);
  std::vector<int32_t> act(n), batch, serial, sub, kry, fin, res;
  for (int k = 0; k < n; ++k) act[k] = k;
  e->act_slot = 0;
  { int rc = ens_upload_list(e, L_ACT, act); if (rc) return rc; }
  { int rc = ens3_residual<NF>(e, L_ACT, n); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) settle(k, true);
  const double q = 1.0 - o.relaxation_parameter;
  for (;;) {
    act.clear();
    for (int k = 0; k < n; ++k) if (live[k]) act.push_back(k);
    if (act.empty()) break;
    e->act_slot ^= 1;
    int rc = ens_upload_list(e, L_ACT, act); if (rc) return rc;
    // Jacobian of every live member (element records: left by the last residual evaluation)
    hipLaunchKernelGGL((k_jac_gather_ens<DIM, NF>), dim3(grid_for(s0->c.n_work * kWave, kVecBlock), (unsigned)act.size()), dim3(kVecBlock), 0,
                       e->stream, tab, ens_list(e, L_ACT));
    if (s0->c.n_robin > 0)
      hipLaunchKernelGGL(k_robin_add_ens, dim3(grid_for(s0->c.n_robin, 256), (unsigned)act.size()), dim3(256), 0, e->stream, tab, ens_list(e, L_ACT));
    HIP_TRY(hipGetLastError());
    batch.clear(); serial.clear(); res.clear();
    for (int k : act) {
      gmpnp_solver* s = e->m[k];
      s->jacobian_valid = true;
      Plan& p = plan[k];
      p = Plan{};
      p.it = stats[k].iterations;
      const double wa = predicted_start(s->cfg.warm_start, q, p.it).first;
      // not batched: the band LU, a right-hand side BiCGStab cannot start from, a predicted start k_warm_start has to form first
      if (s->direct.use_direct() || !std::isfinite(rn[k]) || !(rn[k] > 0.0) || (wa != 0.0 && !s->x0.ready(p.it, wa))) serial.push_back(k);
      else batch.push_back(k);
    }
    for (int k : serial) if (serial_step(k) == GMPNP_OK) res.push_back(k);
    if (!batch.empty()) {
      // preconditioner set-up (setup_preconditioner): node-block inverses and the column-scaled matrix of every member, the
      // coarse chain of those whose CoarseReuse asks for it
      const unsigned nb = (unsigned)batch.size();
      rc = ens_upload_list(e, L_BATCH, batch); if (rc) return rc;
      sub.clear();
      for (int k : batch) {
        gmpnp_solver* s = e->m[k];
        Plan& p = plan[k];
        p.precond_was_valid = s->precond_valid;
        p.coarse_fresh = s->coarse.fresh(false, s->cfg.coarse_lag, p.it, s->state_jumped);
        // (a handle without a valid preconditioner of this kind builds its coarse inverse whatever the rule says; the rule's own
        // answer is what CoarseReuse::solved hears, as in krylov_step)
        if (use_coarse && (p.coarse_fresh || !s->precond_valid || s->precond_mode != mode)) sub.push_back(k);
        s->precond_valid = true; s->precond_mode = mode;
        s->burst.expect(p.it);
      }
      hipLaunchKernelGGL((k_block_inverse_ens<NF>), dim3(grid_for(s0->t.nv, 4), nb), dim3(64), 0, e->stream, tab, ens_list(e, L_BATCH));
      hipLaunchKernelGGL((k_scale_columns_ens<NF>), dim3(grid_for(s0->c.n_work * kWave, kVecBlock), nb), dim3(kVecBlock), 0, e->stream, tab, ens_list(e, L_BATCH));
      if (!sub.empty()) {
        const unsigned nc = (unsigned)sub.size();
        const int32_t* lc = ens_list(e, L_COARSE);
        rc = ens_upload_list(e, L_COARSE, sub); if (rc) return rc;
        hipLaunchKernelGGL((k_coarse_rows_ens<NF>), dim3(s0->t.nslices, nc), dim3(64), 0, e->stream, tab, lc);
        hipLaunchKernelGGL((k_coarse_sum_ens<NF>), dim3(s0->t.nagg * s0->c.coarse_chunks, nc), dim3(kVecBlock), 0, e->stream, tab, lc);
        hipLaunchKernelGGL(k_coarse_reduce_ens, dim3(grid_for(s0->ncoarse * s0->ncoarse, kVecBlock), nc), dim3(kVecBlock), 0, e->stream, tab, lc);
        hipLaunchKernelGGL((k_coarse_invert_ens<NF>), dim3(nc), dim3(512), coarse_lds_bytes(s0->ncoarse, NF), e->stream, tab, lc);
      }
      HIP_TRY(hipGetLastError());
      // test of the predicted starts (kx, left by the previous update): one synchronisation for all of them
      sub.clear();
      for (int k : batch) {
        plan[k].rhs_norm = rn[k];
        if (predicted_start(e->m[k]->cfg.warm_start, q, plan[k].it).first != 0.0) sub.push_back(k);
      }
      if (!sub.empty()) {
        const unsigned nw = (unsigned)sub.size();
        rc = ens_upload_list(e, L_WARM, sub); if (rc) return rc;
        hipLaunchKernelGGL((k_spmv_plain_ens<NF>), dim3(s0->t.own_ntiles, nw), dim3(kKrylovThreads), 0, e->stream, tab, ens_list(e, L_WARM));
        hipLaunchKernelGGL(k_dots3_ens, dim3(s0->n_resblocks, nw), dim3(kVecBlock), 0, e->stream, tab, ens_list(e, L_WARM));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(e->stream));
        std::vector<int32_t> acc;
        for (int k : sub) {
          gmpnp_solver* s = e->m[k];
          if (accept_predicted_start(sum_partials(s, 0), sum_partials(s, 1), sum_partials(s, 2), &plan[k].rhs_norm)) { plan[k].warm = true; acc.push_back(k); }
        }
        if (!acc.empty()) {
          rc = ens_upload_list(e, L_START, acc); if (rc) return rc;
          hipLaunchKernelGGL(k_start_residual_ens, dim3(grid_for(s0->ndof, 256), (unsigned)acc.size()), dim3(256), 0, e->stream, tab, ens_list(e, L_START));
        }
      }
      // first pass of BiCGStab: all members start at k = 0 together
      const int cap = std::min(restart_every, (int)o.krylov_maximum_iterations);
      EnsIter3* hit = e->h_it3 + (size_t)e->act_slot * n;
      kry.clear(); serial.clear();
      int first = 1, B = 1;
      for (int k : batch) {
        gmpnp_solver* s = e->m[k];
        Plan& p = plan[k];
        const double tol = std::max(o.krylov_relative_tolerance * rn[k], o.krylov_absolute_tolerance);
        if (p.rhs_norm <= tol) { serial.push_back(k); continue; }   // nothing left to solve: the serial code's own ending
        const bool first_cold = !p.warm;
        const auto nab = predicted_start(s->cfg.warm_start, q, p.it + 1);
        p.has_upd = nab.first != 0.0;
        EnsIter3 rec{};
        rec.init = krylov_start(p.rhs_norm * p.rhs_norm, p.rhs_norm, first_cold ? o.krylov_relative_tolerance : 0.0,
                                first_cold ? o.krylov_absolute_tolerance : tol, cap);
        rec.upd = p.has_upd ? NewtonUpdate{s->u.p, s->kxp.p, o.relaxation_parameter, nab.first, nab.second} : NewtonUpdate{nullptr, nullptr, 0.0, 0.0, 0.0};
        rec.scale_dst = p.warm ? 1.0 : 0.0;
        std::memcpy(&hit[k], &rec, sizeof rec);
        B = std::max(B, s->cfg.burst_iters);
        kry.push_back(k);
      }
      for (int k : kry) first = std::max(first, e->m[k]->burst.first(use_coarse, e->m[k]->opts.krylov_batch, B, false));
      fin.clear();
      if (!kry.empty()) {
        const unsigned nk = (unsigned)kry.size();
        const int32_t* lk = ens_list(e, L_KRY);
        const EnsIter3* it3 = e->it3.p;
        rc = ens_upload_list(e, L_KRY, kry); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(e->it3.p, hit, (size_t)n * sizeof(EnsIter3), hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL((k_krylov_init_ens<NF>), dim3(s0->t.own_ntiles, nk), dim3(kVecBlock), 0, e->stream, tab, lk, it3);
        for (int k : kry) { volatile HostPoll* hp = e->m[k]->h_poll; hp->done = 0; hp->iters = 0; hp->rr = 0.0; }
        std::atomic_thread_fence(std::memory_order_seq_cst);
        int next_k = 0;
        const dim3 cg(std::max(1, s0->t.nagg), nk), tg(s0->t.own_ntiles, nk);
        auto burst = [&](int iters) {
          for (int it = 0; it < iters; ++it, ++next_k) {
            hipLaunchKernelGGL((k_coarse_a_ens<NF>), cg, dim3(kCoarseThreads), 0, e->stream, tab, lk, next_k);
            hipLaunchKernelGGL((k_bicg_a_ens<NF>), tg, dim3(kKrylovThreads), 0, e->stream, tab, lk, next_k);
            hipLaunchKernelGGL((k_coarse_b_ens<NF>), cg, dim3(kCoarseThreads), 0, e->stream, tab, lk, next_k);
            hipLaunchKernelGGL((k_bicg_b_ens<NF>), tg, dim3(kKrylovThreads), 0, e->stream, tab, lk, next_k);
          }
        };
        // bursts as in krylov(): the next burst is queued, then the host waits until every member is done or has finished the
        // iterations queued before it (the B kernels report into each member's pinned mirror)
        burst(first);
        int launched = first;
        for (;;) {
          const int target = launched;
          burst(B); launched += B;
          HIP_TRY(hipGetLastError());
          const double t_spin = now_ms();
          int spins = 0; bool all_done = false;
          for (;;) {
            bool reached = true; all_done = true;
            for (int k : kry) {
              volatile HostPoll* hp = e->m[k]->h_poll;
              if (!hp->done) { all_done = false; if (hp->iters < target) { reached = false; break; } }
            }
            if (reached) break;
            __builtin_ia32_pause();
            if ((++spins & 0xfff) == 0 && now_ms() - t_spin > 20000.0) {
              (void)hipStreamSynchronize(e->stream);
              return fail(GMPNP_ERR_HIP, "ensemble: the members' progress mirrors did not advance");
            }
          }
          if (all_done) break;
          if (launched > cap + 4 * B + first) { (void)hipStreamSynchronize(e->stream); return fail(GMPNP_ERR_HIP, "ensemble: BiCGStab ran past its iteration cap"); }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        for (int k : kry) {
          gmpnp_solver* s = e->m[k];
          Plan& p = plan[k];
          volatile HostPoll* hp = s->h_poll;
          const int done = hp->done, iters = hp->iters;
          if (done == 1 && iters > 0 && iters <= verify_above) {   // the normal end: short solves go unchecked
            s->burst.solve_done(use_coarse, iters, false);
            s->last_done = done;
            s->burst.record(p.it, iters);
            s->direct.krylov_converged(p.it);
            s->coarse.solved(p.coarse_fresh, iters);
            if (p.it < GMPNP_MAX_NEWTON_HISTORY) stats[k].krylov_per_iteration[p.it] = iters;
            stats[k].krylov_iterations += iters;
            s->x0.left(p.has_upd);
            fin.push_back(k);
          } else {
            serial.push_back(k);
          }
        }
      }
      if (!fin.empty()) {
        // dx = M^-1 y (+ the predicted start) with the Newton update and the next predicted start in the same launch
        const unsigned ne = (unsigned)fin.size();
        rc = ens_upload_list(e, L_END, fin); if (rc) return rc;
        if (use_coarse) hipLaunchKernelGGL((k_restrict_ens<NF>), dim3(s0->t.own_ntiles, ne), dim3(kVecBlock), 0, e->stream, tab, ens_list(e, L_END));
        hipLaunchKernelGGL((k_minv_apply_ens<NF>), dim3(s0->t.own_ntiles, ne), dim3(kKrylovThreads), 0, e->stream, tab, ens_list(e, L_END),
                           (const EnsIter3*)e->it3.p);
        sub.clear();
        for (int k : fin) { if (!plan[k].has_upd) sub.push_back(k); res.push_back(k); }
        if (!sub.empty()) {
          rc = ens_upload_list(e, L_AXPY, sub); if (rc) return rc;
          hipLaunchKernelGGL(k_axpy_u_ens, dim3(grid_for(s0->ndof, 256), (unsigned)sub.size()), dim3(256), 0, e->stream, tab, ens_list(e, L_AXPY),
                             -o.relaxation_parameter);
        }
        HIP_TRY(hipGetLastError());
      }
      // the unusual endings: the serial step from the member's own kb and Jacobian (kr was the work vector of the pass)
      for (int k : serial) {
        gmpnp_solver* s = e->m[k];
        s->precond_valid = plan[k].precond_was_valid;
        HIP_TRY(hipMemcpyAsync(s->kr.p, s->kb.p, (size_t)s->ndof * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
        if (serial_step(k) == GMPNP_OK) res.push_back(k);
      }
    }
    if (res.empty()) continue;
    std::sort(res.begin(), res.end());
    rc = ens_upload_list(e, L_RES, res); if (rc) return rc;
    rc = ens3_residual<NF>(e, L_RES, (int)res.size()); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));   // the residuals of all members
    for (int k : res) { stats[k].iterations++; settle(k, false); }
  }
  for (int k = 0; k < n; ++k)
    if (status[k] != GMPNP_OK) { g_err = "ensemble member " + std::to_string(k) + ": " + e->err[k]; return status[k]; }
  return GMPNP_OK;
}

}  // namespace

extern "C" {

int gmpnp_ensemble_create(int32_t n, gmpnp_solver* const* members, gmpnp_ensemble** out) {
  if (!members || !out) return fail(GMPNP_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (n < 1 || n > kEnsMaxMembers) return fail(GMPNP_ERR_INVALID, "ensemble size must be 1 ... 64");
  if (!members[0]) return fail(GMPNP_ERR_INVALID, "ensemble member 0: NULL handle");
  for (int k = 0; k < n; ++k) { int rc = ens_check_member(members[k], members[0], k); if (rc) return rc; }
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < k; ++j)
      if (members[j] == members[k]) return fail(GMPNP_ERR_INVALID, "a handle appears twice in the ensemble");
  std::unique_ptr<gmpnp_ensemble> e(new gmpnp_ensemble);
  e->m.assign(members, members + n);
  e->device = members[0]->opts.device_id; e->ndof = members[0]->ndof; e->nv = members[0]->t.nv;
  e->err.assign(n, std::string());
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamCreate(&e->stream));
  HIP_TRY(e->tab.alloc(n)); HIP_TRY(e->act.alloc((size_t)kEnsLists * kEnsMaxMembers)); HIP_TRY(e->ustage.alloc((size_t)n * e->ndof));
  HIP_TRY(hipHostMalloc((void**)&e->h_tab, (size_t)n * sizeof(EnsMember)));
  HIP_TRY(hipHostMalloc((void**)&e->h_act, (size_t)2 * kEnsLists * kEnsMaxMembers * sizeof(int32_t)));
  if (members[0]->dim == 3) {
    HIP_TRY(e->it3.alloc(n));
    HIP_TRY(hipHostMalloc((void**)&e->h_it3, (size_t)2 * n * sizeof(EnsIter3)));
    std::memset(e->h_it3, 0, (size_t)2 * n * sizeof(EnsIter3));
    // the coarse inverse keeps its whole matrix in LDS: opt in to > 64 KiB of dynamic LDS, as gmpnp_create does for the single handle's kernel
    HIP_TRY(hipFuncSetAttribute((const void*)k_coarse_invert_ens<9>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)coarse_lds_bytes(members[0]->ncoarse, 9)));
  }
  HIP_TRY(hipHostMalloc((void**)&e->h_u, (size_t)n * e->ndof * sizeof(double)));
  int rc = ens_upload_table(e.get()); if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(e->stream));
  *out = e.release();
  return GMPNP_OK;
}

void gmpnp_ensemble_destroy(gmpnp_ensemble* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  delete e;
}

int32_t gmpnp_ensemble_size(const gmpnp_ensemble* e) { return e ? (int32_t)e->m.size() : 0; }

const char* gmpnp_ensemble_member_error(const gmpnp_ensemble* e, int32_t k) {
  if (!e || k < 0 || k >= (int32_t)e->m.size()) return "";
  return e->err[k].c_str();
}

int gmpnp_ensemble_newton_solve(gmpnp_ensemble* e, const gmpnp_newton_options_t* o, gmpnp_newton_stats_t* stats, int32_t* status) {
  if (!e || !o || !stats || !status) return fail(GMPNP_ERR_INVALID, "NULL argument");
  if (o->maximum_iterations < 0 || o->krylov_maximum_iterations < 1) return fail(GMPNP_ERR_INVALID, "bad iteration limits");
  if (!step_fraction_valid(o->step_fraction)) return fail(GMPNP_ERR_INVALID, "step_fraction must be 0 (off) or lie in (0, 1)");
  const bool is3d = e->m[0]->dim == 3;
  if (is3d) {
    if (o->step_fraction != 0.0)
      return fail(GMPNP_ERR_INVALID, "step_fraction: the step limiter is not available in 3D ensembles (set it to 0)");
    if (o->linear_solver != GMPNP_LINEAR_BICGSTAB_TWOLEVEL && o->linear_solver != GMPNP_LINEAR_BICGSTAB_JACOBI)
      return fail(GMPNP_ERR_INVALID, "3D ensembles solve with GMPNP_LINEAR_BICGSTAB_TWOLEVEL or GMPNP_LINEAR_BICGSTAB_JACOBI");
  } else if (o->linear_solver != GMPNP_LINEAR_BLOCK_TRIDIAGONAL)
    return fail(GMPNP_ERR_INVALID, "ensembles solve with GMPNP_LINEAR_BLOCK_TRIDIAGONAL only");
  const int n = (int)e->m.size();
  for (int k = 0; k < n; ++k) { int rc = ens_check_member(e->m[k], e->m[0], k); if (rc) return rc; }
  HIP_TRY(hipSetDevice(e->device));
  if (is3d) return ens3_newton<9>(e, *o, stats, status);
  const double t0 = now_ms();
  { int rc = ens_drain_members(e); if (rc) return rc; }
  const double tau = o->step_fraction;
  if (tau != 0.0) for (gmpnp_solver* s : e->m) { int rc = step_prepare(s); if (rc) return rc; }   // before the table names the buffers
  // the member table is rebuilt for every solve: a gmpnp_set_* call may have re-allocated member storage since the last one
  { int rc = ens_upload_table(e); if (rc) return rc; }
  std::vector<char> live(n, 1);
  std::vector<NewtonJudge> judge; judge.reserve(n);   // one per member: the single handle's rule (gmpnp_host_rules.h)
  for (int k = 0; k < n; ++k) {
    stats[k] = fresh_newton_stats(); status[k] = GMPNP_OK; e->err[k].clear();
    judge.emplace_back(*o, stats[k], e->m[k]->cfg.strict_steric != 0);
    HIP_TRY(hipMemsetAsync(e->m[k]->status.p, 0, sizeof(int32_t), e->stream));
  }
  // member k's residual is in its pinned buffer: the verdict, mapped to status[k] / err[k] / live[k] (a member that fails keeps
  // its message and the others go on; a member that ends its solve ends as newton() does)
  auto settle = [&](int k, bool first) {
    gmpnp_solver* s = e->m[k];
    const double r = std::sqrt(sum_partials(s, 0));
    const NewtonJudge::Verdict v = first ? judge[k].first(r, *s->h_status) : judge[k].next(r, *s->h_status);
    if (v == NewtonJudge::go_on) return;
    live[k] = 0;
    if (v != NewtonJudge::failed) { s->state_jumped = false; stats[k].ms_total = now_ms() - t0; }
    if (v != NewtonJudge::converged) { status[k] = judge[k].code; e->err[k] = judge[k].message; }
  };
  std::vector<int32_t> act(n);
  for (int k = 0; k < n; ++k) act[k] = k;
  { int rc = ens_upload_active(e, act); if (rc) return rc; }
  { int rc = ens_residual(e, n); if (rc) return rc; }
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) settle(k, true);
  for (;;) {
    act.clear();
    for (int k = 0; k < n; ++k) if (live[k]) act.push_back(k);
    if (act.empty()) break;
    const int nact = (int)act.size();
    int rc = ens_upload_active(e, act); if (rc) return rc;
    rc = ens_update(e, nact, o->relaxation_parameter, tau); if (rc) return rc;
    rc = ens_residual(e, nact); if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));   // the one host synchronisation of the iteration
    for (int k : act) {
      e->m[k]->jacobian_valid = true;
      if (tau != 0.0) record_step(stats[k], stats[k].iterations, e->m[k]->limiter->h_report->alpha);
      stats[k].iterations++;
      settle(k, false);
    }
  }
  for (int k = 0; k < n; ++k)
    if (status[k] != GMPNP_OK) { g_err = "ensemble member " + std::to_string(k) + ": " + e->err[k]; return status[k]; }
  return GMPNP_OK;
}

int gmpnp_ensemble_assign_previous(gmpnp_ensemble* e) {
  if (!e) return fail(GMPNP_ERR_INVALID, "NULL handle");
  HIP_TRY(hipSetDevice(e->device));
  for (const gmpnp_solver* s : e->m)
    if (s->stepper && s->stepper->order == 2) return fail(GMPNP_ERR_INVALID, "gmpnp_ensemble_assign_previous: a member steps at order 2 (gmpnp_set_time_order): ensembles have no second-order time stepping");
  for (size_t k = 0; k < e->m.size(); ++k)
    if (stern_on(e->m[k]) || kinetics_on(e->m[k])) return ens_check_member(e->m[k], e->m[0], (int)k);   // (the Stern boundary condition or the surface kinetics were set after create)
  int rc = ens_drain_members(e); if (rc) return rc;
  // u / u_n of a handle are allocated once at create: the table of the last upload addresses them
  hipLaunchKernelGGL(k_ens_assign, dim3(grid_for(e->ndof, 256), (unsigned)e->m.size()), dim3(256), 0, e->stream, (const EnsMember*)e->tab.p, e->ndof);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(e->stream));   // blocking: a member call on the member's own stream sees u_n afterwards
  return GMPNP_OK;
}

int gmpnp_ensemble_get_state(gmpnp_ensemble* e, double* u_out) {
  if (!e || !u_out) return fail(GMPNP_ERR_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(e->device));
  for (size_t k = 0; k < e->m.size(); ++k)
    if (stern_on(e->m[k]) || kinetics_on(e->m[k])) return ens_check_member(e->m[k], e->m[0], (int)k);   // (the Stern boundary condition or the surface kinetics were set after create)
  int rc = ens_drain_members(e); if (rc) return rc;
  const int n = (int)e->m.size(), nf = e->m[0]->nf, nv = e->nv, ndof = e->ndof;
  hipLaunchKernelGGL(k_ens_gather_u, dim3(grid_for(ndof, 256), n), dim3(256), 0, e->stream, (const EnsMember*)e->tab.p, e->ustage.p, ndof);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(e->h_u, e->ustage.p, (size_t)n * ndof * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  for (int k = 0; k < n; ++k) {
    const int32_t* perm = e->m[k]->t.perm.data();
    const double* src = e->h_u + (size_t)k * ndof;
    double* dst = u_out + (size_t)k * ndof;
    for (int i = 0; i < nv; ++i) std::memcpy(&dst[(size_t)perm[i] * nf], &src[(size_t)i * nf], nf * sizeof(double));
  }
  return GMPNP_OK;
}

}  // extern "C"
